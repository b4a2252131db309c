#!/usr/bin/env python
"""Filtered exact search against the unfiltered search of the same index (DESIGN.md 4f "Filtered search").

    python tools/search_filter_bench.py [--rows 2000000] [--runs 3] [--reps 5] [--out profiles/search_filter_bench.json]

One FlatIPIndex(precision="f16_rescore") of --rows x 768 anisotropic rows (as tools/index_f16_bench.py draws them); k = 100 and 1000;
1, 64 and 1024 queries.  Filters: all rows allowed, forced to the 'scan' route (what the drop launches cost on top of the unfiltered
chain), and uniform random filters passing p = 0.9, 0.5, 0.1 and 0.01 of the rows on the decided route and on both forced routes.
Every cell is measured interleaved with `search_device_async` on the same index in the same process -- the yardstick: wall time around
a device synchronisation, the median of --reps searches per run, --runs runs, fastest and slowest reported, and the ratio of the fastest
to the yardstick's fastest.  `redone`: queries the on-device redo recomputed (a forced scan of a filter sparser than the lists hold).
A cell whose first search takes longer than --slow-ms is reported from that one search ("single": true): those are the redo cells.
The 'gather' route's first call (which builds the planes of the allowed rows) is timed apart from its cached calls."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmatch_amd.index import FlatIPIndex, RowFilter, filter_route                # noqa: E402

D_ = 768
BATCH = 1 << 17


def build(rows, dev):
    gen = torch.Generator(device=dev).manual_seed(77)
    shared = torch.randn(1, D_, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    idx = FlatIPIndex(D_, device=dev, precision="f16_rescore")
    idx.reserve(rows)
    for s in range(0, rows, BATCH):
        idx.add(torch.randn(min(BATCH, rows - s), D_, device=dev, generator=gen).mul_(0.05).add_(shared * 0.05))
    return idx, shared


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, h


def timed(fn, reps):
    return round(statistics.median(once(fn)[0] for _ in range(reps)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=1500.0)
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
    filters = [("all", 1.0, RowFilter(idx, torch.ones(a.rows, dtype=torch.bool, device=dev)), ("scan",))]
    for p in (0.9, 0.5, 0.1, 0.01):
        mask = torch.rand(a.rows, device=dev, generator=torch.Generator(device=dev).manual_seed(int(p * 1000))) < p
        filters.append(("p%g" % p, p, RowFilter(idx, mask), (None, "scan", "gather")))
    out = {"rows": a.rows, "d": D_, "precision": "f16_rescore", "runs": a.runs, "reps": a.reps, "slow_ms": a.slow_ms,
           "unit": "ms per search (enqueue + device synchronisation), median of reps per run; fastest and slowest run",
           "n_allowed": {name: rf.n_allowed for name, _, rf, _ in filters}, "cells": {}}
    for k in (100, 1000):
        for nq in (1, 64, 1024):
            q = q_all[:nq].contiguous()
            base = lambda: idx.search_device_async(q, k)
            cells = {}
            for name, p, rf, routes in filters:
                for route in routes:
                    fn = lambda: idx.search_device_filtered_async(q, k, rf, route=route)
                    cell = {"route_decided": filter_route("f16_rescore", k, rf.first, rf.last, rf.n_allowed)}
                    if (route or cell["route_decided"]) == "gather":
                        rf._gathered = None                                   # the building call, apart
                        cell["gather_first_call_ms"] = round(once(fn)[0], 4)
                    first_ms, h = once(fn)
                    info = h.info()
                    cell.update(route=info["route"], redone=info["redone"], rounds=info["rounds"], max_list=info["max_list"])
                    del h
                    if first_ms > a.slow_ms:
                        cell.update(single=True, fastest=round(first_ms, 4), slowest=round(first_ms, 4), runs=[round(first_ms, 4)])
                        cell["unfiltered"] = [timed(base, a.reps)]
                    else:
                        once(fn)
                        runs, yard = [], []
                        for _ in range(a.runs):
                            yard.append(timed(base, a.reps))
                            runs.append(timed(fn, a.reps))
                        cell.update(fastest=min(runs), slowest=max(runs), runs=runs, unfiltered=yard)
                    cell["ratio_to_unfiltered"] = round(cell["fastest"] / min(cell["unfiltered"]), 3)
                    cells["%s/%s" % (name, route or "decided")] = cell
                    print(k, nq, name, route, cell, flush=True)
                rf._gathered = None                                           # (one filter's planes at a time)
            out["cells"]["k%d/q%d" % (k, nq)] = cells
            if a.out:                                                         # kept as far as the run got
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
