#!/usr/bin/env python
"""Encode throughput of a ModernBERT-base-shaped bi-encoder (22 layers, hidden 768, 12 heads of 64, GeGLU FFN 1 152, a global
layer every third, window 128 elsewhere), random weights; prints one JSON line:
  * passages/s for B full-length L-token passages (--len 128 in float16 and bfloat16, and --long 512);
  * the fraction of the ~2.5 PFLOP/s dense 16-bit MFMA peak the GEMM FLOPs alone reach
    (2 (768 * 2304 + 768^2 + 768 * 2304 + 1152 * 768) = 10.03 MFLOP per token per layer, 220.6 MFLOP per token; bert-base 169.9);
  * with --attention-only, forwards of a 2-layer model (one global, one sliding layer) at 512 and 1 024 tokens in bfloat16, for the
    per-launch attention times of rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/modernbert_bench.py --attention-only
    (OUT/**/*kernel_stats.csv: attention_fwd16c_kernel = the global layer, attention_band16_kernel = the sliding one)

    python tools/modernbert_bench.py [--batch 1024] [--len 128] [--long 512] [--iters 5]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

FLOP_PER_TOKEN = 22 * 2 * (768 * 2304 + 768 * 768 + 768 * 2304 + 1152 * 768)
PEAK_16 = 2.5e15


def _timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _model(layers, dtype, layer_types=None):
    from transformers import ModernBertConfig, ModernBertModel
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(0)
    kw = dict(layer_types=layer_types) if layer_types else {}
    cfg = ModernBertConfig(hidden_size=768, num_hidden_layers=layers, num_attention_heads=12, intermediate_size=1152, vocab_size=50368,
                           max_position_embeddings=8192, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1,
                           sep_token_id=2, **kw)
    lm = ModernBertModel(cfg).eval()
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True,
                               model_args=NS(encoder_only=False, dtype=dtype)).to("cuda:0").eval()


def _batch(B, L):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 50000, (B, L), generator=g).to("cuda:0")
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--len", type=int, default=128)
    ap.add_argument("--long", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--attention-only", action="store_true", help="one global and one sliding layer at 512 and 1 024 tokens (for rocprofv3)")
    a = ap.parse_args()
    out = {"shape": "modernbert-base (22 x 768, 12 heads of 64, GeGLU 1152, window 128)"}
    with torch.no_grad():
        if a.attention_only:
            m = _model(2, "bfloat16", ["full_attention", "sliding_attention"])
            for L in (512, 1024):
                x = _batch(64 * 1024 // L, L)
                t = _timed(lambda: m(passage=x), a.iters)
                out[f"two_layer_{L}_ms"] = round(t * 1e3, 3)
            print(json.dumps(out))
            return
        for dtype in ("float16", "bfloat16"):
            m = _model(22, dtype)
            x = _batch(a.batch, a.len)
            t = _timed(lambda: m(passage=x), a.iters)
            tok = a.batch * a.len
            out[f"{dtype}_{a.len}"] = {"ms": round(t * 1e3, 2), "passages_per_s": round(a.batch / t, 1),
                                       "gemm_mfma_peak_fraction": round(FLOP_PER_TOKEN * tok / t / PEAK_16, 3)}
            if dtype == "float16":
                Bl = a.batch
                xl = _batch(Bl, a.long)
                tl = _timed(lambda: m(passage=xl), a.iters)
                out[f"{dtype}_{a.long}"] = {"batch": Bl, "ms": round(tl * 1e3, 2), "passages_per_s": round(Bl / tl, 1),
                                            "gemm_mfma_peak_fraction": round(FLOP_PER_TOKEN * Bl * a.long / tl / PEAK_16, 3)}
            del m
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
