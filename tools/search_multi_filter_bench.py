#!/usr/bin/env python
"""Exact search with a filter per query against what the single-filter search offers (DESIGN.md 4f "A filter per query").

    python tools/search_multi_filter_bench.py [--rows 2000000] [--runs 3] [--reps 5] [--out profiles/search_multi_filter_bench.json]

One FlatIPIndex(precision="f16_rescore") of --rows x 768 anisotropic rows (as tools/search_filter_bench.py draws them); k = 100 and 1000.
  scan        64 and 1024 queries spread evenly over 1, 8 and 64 distinct uniform filters at p = 0.9 and 0.5:
              `search_device_filtered_multi_async` (one chain) against a loop of `search_device_filtered_async` per group of queries
              that share a filter -- the only thing the single-filter search offers -- and against the unfiltered search of the batch.
  candidates  64 and 1024 queries with 1000 candidate rows each: `search_device_candidates_async` against a loop of one-query searches
              through the 'gather' route, each under its own RowFilter built from the query's ids.  The loop is run over the first
              --loop-queries queries only (a RowFilter per query reads its counts back: the whole loop would take minutes) and its time
              is scaled to the batch ("loop_scaled": true); the results are compared on those queries.
  crossover   a shared sparse filter (1000 and p = 0.01 allowed rows) at 1, 2, 4, 8 and 16 queries: candidate lists (forced) against the
              'gather' route with its planes cached, and against the same route when every call gathers anew.
Wall time around a device synchronisation, the median of --reps searches per run, the versions alternated, --runs runs, fastest and
slowest reported.  Every cell compares the two results with torch.equal and records `redone`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from openmatch_amd.index import FlatIPIndex, RowFilter                              # noqa: E402
from search_filter_bench import D_, build                                           # noqa: E402  (the same index, drawn the same way)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, h


def timed(fn, reps):
    return round(statistics.median(once(fn)[0] for _ in range(reps)), 4)


def alternate(versions, runs, reps):
    """{name: fn} -> {name: {"fastest", "slowest", "runs"}}: per run every version once, in turn"""
    for fn in versions.values():
        once(fn)
    got = {name: [] for name in versions}
    for _ in range(runs):
        for name, fn in versions.items():
            got[name].append(timed(fn, reps))
    return {name: {"fastest": min(v), "slowest": max(v), "runs": v} for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-queries", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warm = FlatIPIndex(D_, device=dev, precision="f16_rescore")      # untimed: the library's code object is loaded by the first launch
    warm.add(torch.randn(8192, D_, device=dev))
    warm.search_device_filtered(torch.randn(4, D_, device=dev), 10, RowFilter(warm, torch.rand(8192, device=dev) < 0.5))
    del warm
    idx, shared = build(a.rows, dev)
    gen = torch.Generator(device=dev).manual_seed(78)
    q_all = torch.randn(1024, D_, device=dev, generator=gen) * 0.05 + shared * 0.05
    out = {"rows": a.rows, "d": D_, "precision": "f16_rescore", "runs": a.runs, "reps": a.reps, "loop_queries": a.loop_queries,
           "unit": "ms per batch (enqueue + device synchronisation), median of reps per run; fastest and slowest run",
           "scan": {}, "candidates": {}, "crossover": {}}

    def save():
        if a.out:                                                             # kept as far as the run got
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    # ---- scan: F distinct uniform filters, the queries dealt to them in turn
    for p in (0.9, 0.5):
        pool = [RowFilter(idx, torch.rand(a.rows, device=dev, generator=torch.Generator(device=dev).manual_seed(int(p * 1000) + 7 * f)) < p)
                for f in range(64)]
        for k in (100, 1000):
            for nq in (64, 1024):
                q = q_all[:nq].contiguous()
                for nf in (1, 8, 64):
                    filters = pool[:nf]
                    filter_of = [i % nf for i in range(nq)]
                    groups = [torch.tensor([i for i in range(nq) if i % nf == f], device=dev) for f in range(nf)]
                    qs = [q.index_select(0, g) for g in groups]

                    def multi():
                        return idx.search_device_filtered_multi_async(q, k, filters, filter_of=filter_of)

                    def loop():
                        return [idx.search_device_filtered_async(qs[f], k, filters[f]) for f in range(nf)]

                    def unfiltered():
                        return idx.search_device_async(q, k)
                    _, h = once(multi)
                    info = h.info()
                    _, hs = once(loop)
                    same = all(torch.equal(h.D.index_select(0, g), s.D) and torch.equal(h.I.index_select(0, g), s.I) for g, s in zip(groups, hs))
                    cell = {"parts": info["parts"], "redone": info["redone"], "redone_loop": sum(s.info()["redone"] for s in hs),
                            "rounds": info["rounds"], "equal": bool(same)}
                    del h, hs
                    cell.update(alternate({"multi": multi, "loop": loop, "unfiltered": unfiltered}, a.runs, a.reps))
                    cell["loop_over_multi"] = round(cell["loop"]["fastest"] / cell["multi"]["fastest"], 3)
                    cell["multi_over_unfiltered"] = round(cell["multi"]["fastest"] / cell["unfiltered"]["fastest"], 3)
                    out["scan"]["p%g/k%d/q%d/f%d" % (p, k, nq, nf)] = cell
                    print("scan", p, k, nq, nf, cell, flush=True)
                    save()
        del pool

    # ---- candidates: 1000 rows of its own per query
    cand_all = torch.stack([torch.randperm(a.rows, device=dev, generator=gen)[:1000] for _ in range(1024)])
    n_loop = a.loop_queries
    for k in (100, 1000):
        for nq in (64, 1024):
            q = q_all[:nq].contiguous()
            cand = cand_all[:nq].contiguous()

            def lists():
                return idx.search_device_candidates_async(q, k, cand)

            def loop():      # what the single-filter search offers: per query a RowFilter of its ids and a one-query 'gather' search
                return [idx.search_device_filtered_async(q[i:i + 1], k, RowFilter(idx, cand[i]), route="gather") for i in range(n_loop)]
            _, h = once(lists)
            _, hs = once(loop)
            same = all(torch.equal(h.D[i:i + 1], s.D) and torch.equal(h.I[i:i + 1], s.I) for i, s in enumerate(hs))
            cell = {"equal": bool(same), "redone": h.info()["redone"], "redone_loop": sum(s.info()["redone"] for s in hs), "loop_scaled": True}
            del h, hs
            t = alternate({"lists": lists, "loop": loop}, a.runs, a.reps)
            scale = nq / n_loop
            t["loop_of_%d_queries" % n_loop] = t.pop("loop")
            t["loop"] = {key: round(v * scale, 4) for key, v in t["loop_of_%d_queries" % n_loop].items() if key != "runs"}
            cell.update(t)
            cell["loop_over_lists"] = round(cell["loop"]["fastest"] / cell["lists"]["fastest"], 3)
            out["candidates"]["k%d/q%d" % (k, nq)] = cell
            print("candidates", k, nq, cell, flush=True)
            save()

    # ---- crossover: one sparse filter shared by 1 .. 16 queries, lists against gather
    sparse = {"c1000": RowFilter(idx, cand_all[0]),
              "p0.01": RowFilter(idx, torch.rand(a.rows, device=dev, generator=torch.Generator(device=dev).manual_seed(10)) < 0.01)}
    for name, rf in sparse.items():
        for k in (100, 1000):
            for nq in (1, 2, 4, 8, 16):
                q = q_all[:nq].contiguous()

                def lists():
                    return idx.search_device_filtered_multi_async(q, k, [rf] * nq, route="candidates")

                def gather():
                    return idx.search_device_filtered_async(q, k, rf, route="gather")

                def gather_anew():
                    rf._gathered = None
                    return idx.search_device_filtered_async(q, k, rf, route="gather")
                _, h = once(lists)
                _, g = once(gather)
                cell = {"n_allowed": rf.n_allowed, "equal": bool(torch.equal(h.D, g.D) and torch.equal(h.I, g.I)),
                        "redone": h.info()["redone"], "redone_gather": g.info()["redone"]}
                del h, g
                cell.update(alternate({"lists": lists, "gather_cached": gather, "gather_anew": gather_anew}, a.runs, a.reps))
                cell["gather_cached_over_lists"] = round(cell["gather_cached"]["fastest"] / cell["lists"]["fastest"], 3)
                cell["gather_anew_over_lists"] = round(cell["gather_anew"]["fastest"] / cell["lists"]["fastest"], 3)
                out["crossover"]["%s/k%d/q%d" % (name, k, nq)] = cell
                print("crossover", name, k, nq, cell, flush=True)
                save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
