#!/usr/bin/env python
"""Exact search with an exclusion list per query against what served it before (DESIGN.md 4f "Exclusion lists").

    python tools/search_exclude_bench.py [--rows 2000000] [--runs 3] [--reps 5] [--out profiles/search_exclude_bench.json]

One FlatIPIndex(precision="f16_rescore") of --rows x 768 anisotropic rows (as tools/search_filter_bench.py draws them); k = 200 and 1000;
64 and 1024 queries; every query excludes its own E = 4, 64 and 1024 best hits (the case hard-negative mining has: the positives are at
the top of the ranking).  Per cell, in one process and in turn:
  exclude     `search_device_excluding_async` over the prepared table (int32 [Q, E] on the device);
  unfiltered  `search_device_async` of the same batch: the reference point -- the same pass over the index without any drop;
  bitmaps     `search_device_filtered_multi_async` with one `RowFilter(invert=True)` per query, built beforehand: the search alone is
              timed, what building the Q bitmaps cost is reported once as `bitmaps_build_ms`;
  overfetch   `search_device_async` for k + E, the result copied to the host, the excluded ids dropped and the rows cut to k there --
              only where k + E <= 2048.
Wall time around a device synchronisation, the median of --reps searches per run, the versions alternated, --runs runs, fastest and
slowest reported.  Every cell compares exclude with bitmaps (torch.equal) and, where there is one, with the over-fetched result, and
records `redone`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from openmatch_amd.index import FlatIPIndex, RowFilter, prepare_exclusions          # noqa: E402
from search_filter_bench import D_, build                                           # noqa: E402  (the same index, drawn the same way)
from search_multi_filter_bench import alternate, once                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warm = FlatIPIndex(D_, device=dev, precision="f16_rescore")      # untimed: the library's code object is loaded by the first launch
    warm.add(torch.randn(8192, D_, device=dev))
    warm.search_device_excluding(torch.randn(4, D_, device=dev), 10, [[1], [2], [3], []])
    del warm
    idx, shared = build(a.rows, dev)
    gen = torch.Generator(device=dev).manual_seed(78)
    q_all = torch.randn(1024, D_, device=dev, generator=gen) * 0.05 + shared * 0.05
    best = idx.search_device(q_all, 1024)[1]                         # every query's own 1024 best hits, best first
    out = {"rows": a.rows, "d": D_, "precision": "f16_rescore", "runs": a.runs, "reps": a.reps,
           "unit": "ms per batch (enqueue + device synchronisation), median of reps per run; fastest and slowest run", "cells": {}}

    def save():
        if a.out:                                                             # kept as far as the run got
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for n_excl in (4, 64, 1024):
        table_all = prepare_exclusions(best[:, :n_excl], a.rows)
        t0 = time.perf_counter()
        filters_all = [RowFilter(idx, best[i, :n_excl], invert=True) for i in range(1024)]
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        gone_host = best[:, :n_excl].cpu().numpy()
        for nq in (64, 1024):
            q = q_all[:nq].contiguous()
            table = table_all[:nq].contiguous()
            filters = filters_all[:nq]
            for k in (200, 1000):
                def exclude():
                    return idx.search_device_excluding_async(q, k, table)

                def unfiltered():
                    return idx.search_device_async(q, k)

                def bitmaps():
                    return idx.search_device_filtered_multi_async(q, k, filters)

                def overfetch():      # the workaround: k + E hits, the excluded dropped on the host, the rows cut to k
                    h = idx.search_device_async(q, k + n_excl)
                    D, I = h.D.cpu().numpy(), h.I.cpu().numpy()
                    keep = np.stack([~np.isin(I[i], gone_host[i]) for i in range(nq)])
                    order = np.argsort(~keep, axis=1, kind="stable")[:, :k]      # the kept hits first, in their order
                    return np.take_along_axis(D, order, 1), np.take_along_axis(I, order, 1)
                _, h = once(exclude)
                info = h.info()
                _, hb = once(bitmaps)
                cell = {"redone": info["redone"], "rounds": info["rounds"], "redone_bitmaps": hb.info()["redone"],
                        "equal_bitmaps": bool(torch.equal(h.D, hb.D) and torch.equal(h.I, hb.I)),
                        "bitmaps_build_ms_per_query": round(build_ms / 1024, 4), "bitmaps_bytes": int(nq * ((a.rows + 31) // 32) * 4),
                        "table_bytes": int(table.numel() * 4)}
                versions = {"exclude": exclude, "unfiltered": unfiltered, "bitmaps": bitmaps}
                if k + n_excl <= 2048:
                    Do, Io = overfetch()
                    cell["equal_overfetch"] = bool(np.array_equal(Do, h.D.cpu().numpy()) and np.array_equal(Io, h.I.cpu().numpy()))
                    versions["overfetch"] = overfetch
                del h, hb
                cell.update(alternate(versions, a.runs, a.reps))
                for name in versions:
                    if name != "unfiltered":
                        cell[name + "_over_unfiltered"] = round(cell[name]["fastest"] / cell["unfiltered"]["fastest"], 3)
                out["cells"]["e%d/q%d/k%d" % (n_excl, nq, k)] = cell
                print("cell", n_excl, nq, k, cell, flush=True)
                save()
        del filters_all, table_all
    print(json.dumps(out))


if __name__ == "__main__":
    main()
