#!/usr/bin/env python
"""Encode throughput of a MiniLM-L6-shaped bi-encoder (6 layers, hidden 384, 12 heads of 32, FFN 1 536: all-MiniLM-L6-v2,
e5-small-v2, bge-small-en-v1.5, gte-small), the shape the 32-wide-head attention kernels (attention_d32.hip) serve.  Random
weights; prints one JSON line: passages/s for B full-length L-token passages (padded) and for the same batch with ragged lengths
(U{8 .. L}), and ms per single 32-token query.

    python tools/small_encoder_bench.py [--batch 1024] [--len 128] [--dtype float16] [--iters 10]

Per-launch attention time (attention_d32_fwd_kernel rows of the stats file):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/small_encoder_bench.py --iters 3
    python tools/summarize_prof.py OUT        (or read OUT/**/*kernel_stats.csv: AverageNs per kernel name)
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS


def _timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--len", type=int, default=128)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from transformers import BertConfig, BertModel
    from openmatch.modeling import DRModelForInference
    dev = "cuda:0"
    torch.manual_seed(0)
    lm = BertModel(BertConfig(hidden_size=384, num_hidden_layers=6, num_attention_heads=12, intermediate_size=1536,
                              max_position_embeddings=512)).eval()
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True,
                                model_args=NS(encoder_only=False, dtype=a.dtype)).to(dev).eval()
    B, L = a.batch, a.len
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (B, L), generator=g).to(dev)
    full = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    lens = torch.randint(8, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long().to(dev)
    ragged = {"input_ids": ids * mask, "attention_mask": mask}
    q = {"input_ids": ids[:1, :32].contiguous(), "attention_mask": torch.ones_like(ids[:1, :32])}
    with torch.no_grad():
        t_full = _timed(lambda: model(passage=full), a.iters)
        t_rag = _timed(lambda: model(passage=ragged), a.iters)
        t_q = _timed(lambda: model(query=q), 10 * a.iters)
    print(json.dumps({"shape": "minilm-l6 (6 x 384, 12 heads of 32, ffn 1536)", "dtype": a.dtype, "batch": B, "len": L,
                      "padded": {"ms": round(t_full * 1e3, 2), "passages_per_s": round(B / t_full, 1)},
                      "ragged": {"tokens": int(lens.sum()), "ms": round(t_rag * 1e3, 2), "passages_per_s": round(B / t_rag, 1)},
                      "query_32_tokens_ms": round(t_q * 1e3, 3)}))


if __name__ == "__main__":
    main()
