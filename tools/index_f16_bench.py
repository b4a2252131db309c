#!/usr/bin/env python
"""The float16-only index against the two-copy index (DESIGN.md 4f "Float16-only index"): resident bytes, add time and time per search
of FlatIPIndex(precision="f16") and FlatIPIndex(precision="f16_rescore") built from the same rows in one process.

    python tools/index_f16_bench.py [--rows 2000000] [--runs 3] [--reps 10] [--out FILE.json]

Memory: torch.cuda.max_memory_allocated after the build (one `reserve`, then adds of 2^17 float32 rows drawn on the device: the peak counts
one batch in flight -- 0.4 GB and the temporaries of drawing it, the same for both indexes), and the bytes of the index's own planes.  Search: k = 1000 at 1 / 64 / 128 / 1024 queries through
`search_device`, wall time around a device synchronisation, the median of --reps searches per run; the two precisions are measured
interleaved (f16, two-copy, f16, ...), --runs runs each, fastest and slowest reported.  Every cell also checks that the two indexes
return the same bits, which they do when the rows are float16 values (the default: the rows are rounded before either index sees them;
--raw-rows adds the float32 rows as drawn, and the two indexes then hold different values)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmatch_amd.index import FlatIPIndex                # noqa: E402

D_ = 768
BATCH = 1 << 17


def rows_of(n, dev, gen, shared, exact):
    """anisotropic, CLS-like rows (mean + noise), as tools/search_async_bench.py draws them"""
    x = torch.randn(n, D_, device=dev, generator=gen).mul_(0.05).add_(shared * 0.05)
    return x.half().float() if exact else x


def build(precision, rows, dev, exact):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    gen = torch.Generator(device=dev).manual_seed(77)
    shared = torch.randn(1, D_, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    idx = FlatIPIndex(D_, device=dev, precision=precision)
    idx.reserve(rows)
    add_ms = 0.0
    for s in range(0, rows, BATCH):
        x = rows_of(min(BATCH, rows - s), dev, gen, shared, exact)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.add(x)
        torch.cuda.synchronize()
        add_ms += (time.perf_counter() - t0) * 1e3
        del x
    planes = sum(t.numel() * t.element_size() for t in (idx._f32, idx._f16) if t is not None)
    return idx, {"max_memory_allocated_bytes": int(torch.cuda.max_memory_allocated(dev) - base), "plane_bytes": int(planes),
                 "bytes_per_element": round(planes / (idx.capacity * idx.dpad), 3), "add_ms_total": round(add_ms, 2),
                 "add_rows_per_s": round(rows / (add_ms / 1e3))}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--raw-rows", action="store_true", help="float32 rows as drawn: the two indexes then hold different values (no bit check)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, exact = a.topk, not a.raw_rows
    out = {"rows": a.rows, "d": D_, "k": k, "runs": a.runs, "reps": a.reps, "rows_are_float16_values": exact,
           "unit": "ms per search_device call, median of reps per run; fastest and slowest run"}
    for precision in ("f16", "f16_rescore"):      # untimed: the library's code object is loaded by the process's first launch
        warm = FlatIPIndex(D_, device=dev, precision=precision)
        warm.add(torch.randn(4096, D_, device=dev))
        warm.search_device(torch.randn(4, D_, device=dev), 10)
        del warm
    idx = {}
    for precision in ("f16", "f16_rescore"):
        idx[precision], out["build_" + precision] = build(precision, a.rows, dev, exact)
        print(precision, out["build_" + precision], flush=True)
    gen = torch.Generator(device=dev).manual_seed(78)
    shared = torch.randn(1, D_, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    q_all = torch.randn(1024, D_, device=dev, generator=gen) * 0.05 + shared * 0.05
    per = {}
    for nq in (1, 64, 128, 1024):
        q = q_all[:nq].contiguous()
        res, info = {p: [] for p in idx}, {}
        got = {}
        for p, ix in idx.items():
            D, I = ix.search_device(q, k)
            got[p], info[p] = (D.clone(), I.clone()), dict(ix.last_search_info)
        for _ in range(a.runs):
            for p, ix in idx.items():
                res[p].append(timed(lambda: ix.search_device(q, k), a.reps))
        cell = {p: {"fastest": min(v), "slowest": max(v), "runs": v, "info": info[p]} for p, v in res.items()}
        if exact:
            cell["same_bits"] = bool(torch.equal(got["f16"][0], got["f16_rescore"][0]) and torch.equal(got["f16"][1], got["f16_rescore"][1]))
        per["q%d" % nq] = cell
        print(nq, cell, flush=True)
    out["per_search_ms"] = per
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
