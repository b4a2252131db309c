#!/usr/bin/env python
"""om_sim_topk against om_sim_topk_async (DESIGN.md 4f "Stream-ordered search"): time per search at 1 / 64 / 128 / 6 980 queries, two
indexes on two streams, a graph replay, and the on-device redo's cost at 0 / 1 / 8 / 64 flagged queries.

    python tools/search_async_bench.py [--rows 8841823] [--redo-rows 1000000] [--runs 3] [--parent-lib PATH] [--out FILE.json]

Every figure is wall time around a device synchronisation, the median of `--reps` searches, reported per run; the entries are measured
interleaved (sync, async, parent, sync, ...) so that clock drift hits all alike.  --parent-lib: a libopenmatch_hip.so of another commit,
whose om_sim_topk runs over the same device buffers.  The redo leg uses an index of --redo-rows rows whose last 9 000 are copies of one
vector: a query along it ties 9 000 ways, more than a list holds, and is redone."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmatch_amd import native as N                      # noqa: E402
from openmatch_amd.index import FlatIPIndex                # noqa: E402

D_ = 768


def build_index(rows, dev, seed, tied=0):
    """the benchmark's index: anisotropic, CLS-like rows (mean + noise); `tied` copies of one vector at the end"""
    g = torch.Generator(device=dev).manual_seed(seed)
    shared = torch.randn(1, D_, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    idx = FlatIPIndex(D_, device=dev, precision="f16_rescore")
    idx._reserve(rows)
    for s in range(0, rows - tied, 1 << 20):
        n = min(1 << 20, rows - tied - s)
        idx.add(torch.randn(n, D_, device=dev, generator=g) * 0.05 + shared * 0.05)
    v = None
    if tied:
        v = torch.randn(1, D_, device=dev, generator=g) * 0.05 + shared * 0.05
        idx.add(v.expand(tied, D_).contiguous())
    q = torch.randn(6980, D_, device=dev, generator=g) * 0.05 + shared * 0.05
    return idx, q, v


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def parent_search(plib, idx, q, k, dev):
    nq = q.shape[0]
    nbytes = plib.om_sim_topk_workspace_bytes(nq, idx.dpad, k)
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    Dt = torch.empty(nq, k, dtype=torch.float32, device=dev)
    It = torch.empty(nq, k, dtype=torch.int64, device=dev)

    def run():
        rc = plib.om_sim_topk(N.SEARCH_F16_RESCORE, N.ptr(q), nq, N.ptr(idx._f32), N.ptr(idx._f16), N.ptr(idx._stats), idx.ntotal,
                              idx.dpad, k, 0, N.ptr(Dt), N.ptr(It), N.c_void_p(ws), nbytes, N.stream_ptr(dev))
        if rc:
            raise RuntimeError(plib.om_last_error().decode())
    return run, (Dt, It)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_841_823)
    ap.add_argument("--redo-rows", type=int, default=1_000_000)
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = a.topk
    plib = None
    if a.parent_lib:
        plib = C.CDLL(a.parent_lib)
        for name in ("om_sim_topk_workspace_bytes", "om_sim_topk", "om_last_error"):
            getattr(plib, name).restype, getattr(plib, name).argtypes = N._SIGNATURES[name]
    out = {"rows": a.rows, "d": D_, "k": k, "runs": a.runs, "reps": a.reps, "unit": "ms per search, median of reps, one figure per run"}

    idx, q_all, _ = build_index(a.rows, dev, 77)
    per = {}
    for nq in (1, 64, 128, 6980):
        q = q_all[:nq].contiguous()
        reps = a.reps if nq <= 128 else 2
        legs = {"sync": lambda: idx.search_device(q, k), "async": lambda: idx.search_device_async(q, k)}
        if plib is not None:
            legs["parent_sync"], _ = parent_search(plib, idx, q, k, dev)
        Ds, Is = idx.search_device(q, k)
        h = idx.search_device_async(q, k)
        info = h.info()
        res = {name: [] for name in legs}
        for _ in range(a.runs):
            for name, fn in legs.items():
                res[name].append(timed(fn, reps))
        res["same_bits"] = bool(torch.equal(h.D, Ds) and torch.equal(h.I, Is))
        res["async_info"] = info
        per["q%d" % nq] = res
        print(nq, res, flush=True)
    out["per_search_ms"] = per

    # a graph replay of the 64-query search
    q = q_all[:64].contiguous()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        idx.search_device_async(q, k)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        hg = idx.search_device_async(q, k)
    out["graph_replay_q64_ms"] = [timed(graph.replay, a.reps) for _ in range(a.runs)]
    out["graph_replay_same_bits"] = bool(torch.equal(hg.D, idx.search_device(q, k)[0]))
    print("graph", out["graph_replay_q64_ms"], flush=True)
    del graph, hg, idx
    torch.cuda.empty_cache()

    # two indexes (the two halves of the rows) on two streams against the same two searches on one stream
    half = a.rows // 2
    ia, qa, _ = build_index(half, dev, 78)
    ib, qb, _ = build_index(half, dev, 79)
    qa, qb = qa[:64].contiguous(), qb[:64].contiguous()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def one_stream():
        return ia.search_device_async(qa, k), ib.search_device_async(qb, k)

    def two_streams():
        with torch.cuda.stream(s1):
            x = ia.search_device_async(qa, k)
        with torch.cuda.stream(s2):
            y = ib.search_device_async(qb, k)
        return x, y

    def two_sync():
        ia.search_device(qa, k)
        ib.search_device(qb, k)
    out["two_indexes_q64_ms"] = {"rows_each": half, "sync_one_after_the_other": [], "async_one_stream": [], "async_two_streams": []}
    for _ in range(a.runs):
        out["two_indexes_q64_ms"]["sync_one_after_the_other"].append(timed(two_sync, a.reps))
        out["two_indexes_q64_ms"]["async_one_stream"].append(timed(one_stream, a.reps))
        out["two_indexes_q64_ms"]["async_two_streams"].append(timed(two_streams, a.reps))
    print("two", out["two_indexes_q64_ms"], flush=True)
    del ia, ib
    torch.cuda.empty_cache()

    # the redo: 64 queries of which m tie 9 000 ways
    ir, qr, v = build_index(a.redo_rows, dev, 80, tied=9000)
    redo = {"rows": a.redo_rows, "index_passes_per_redo": 7}
    base = None
    for m in (0, 1, 8, 64):
        q = qr[:64].clone()
        if m:
            q[:m] = v * torch.linspace(0.5, 1.5, m, device=dev)[:, None]
        h = ir.search_device_async(q, k)
        redone = h.info()["redone"]
        ms = [timed(lambda: ir.search_device_async(q, k), a.reps) for _ in range(a.runs)]
        if m == 0:
            base = statistics.median(ms)
            redo["sync_ms_m0"] = [timed(lambda: ir.search_device(q, k), a.reps) for _ in range(a.runs)]
        redo["m%d" % m] = {"redone": redone, "async_ms": ms, "redo_ms_per_index_pass": round((statistics.median(ms) - base) / 7, 4)}
        print("redo", m, redo["m%d" % m], flush=True)
    out["redo_q64"] = redo
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
