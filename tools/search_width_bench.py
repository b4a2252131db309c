#!/usr/bin/env python
"""Small-batch exact top-k search across index widths: the float16 image is held at the headline's size (8 841 823 x 768
x 2 bytes = 13.6 GB) at every width, so a cell's time is one pass over the same number of bytes and index GB/s compares across columns.
Rows are generated on the device in chunks, clustered and normalised.  One JSON line per (d, queries) cell.
  python tools/search_width_bench.py [--dims 768 896 1024 1536 2048] [--queries 1 32 64 128] [--topk 1000] [--warmup 3] [--steps 20]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HEADLINE_ROWS, HEADLINE_D = 8841823, 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="*", default=[768, 896, 1024, 1536, 2048])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 32, 64, 128])
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--image-elems", type=int, default=HEADLINE_ROWS * HEADLINE_D, help="values of the float16 image at every width")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    from openmatch_amd.index import FlatIPIndex
    dev = torch.device("cuda:0")
    for d in a.dims:
        rows = a.image_elems // d
        g = torch.Generator(device=dev).manual_seed(77 + d)
        shared = torch.randn(1, d, device=dev, generator=g)
        # a shared component of the noise's own size (bench.py's index), then unit rows
        draw = lambda n: torch.nn.functional.normalize(shared + torch.randn(n, d, device=dev, generator=g), dim=1)
        index = FlatIPIndex(d, device=dev, precision="f16_rescore")
        index._reserve(rows)
        for s in range(0, rows, 1 << 19):
            index.add(draw(min(1 << 19, rows - s)))
        for nq in a.queries:
            q = draw(nq)
            for _ in range(a.warmup):
                index.search_device(q, a.topk)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.steps):
                index.search_device(q, a.topk)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.steps
            print(json.dumps({"tag": a.tag, "d": d, "rows": rows, "queries": nq, "topk": a.topk, "ms": round(ms, 4),
                              "index_GBps": round(rows * d * 2 / ms / 1e6, 1), "info": index.last_search_info}), flush=True)
        del index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
