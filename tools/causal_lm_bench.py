#!/usr/bin/env python
"""Encode throughput of decoder-only retrievers at two checkpoint shapes, random weights, bfloat16, `last` pooling + normalize, and
the per-layer time of the kernels the stack adds; prints one JSON line:
  * passages/s for full-length batches of 64 Ki tokens at 128 and 512 tokens --
      qwen2-0.5b   24 layers, hidden 896, 14 heads over 2 K / V heads, FFN 4 864, q / k / v biases
      llama-3.2-1b 16 layers, hidden 2 048, 32 heads over 8 K / V heads, FFN 8 192
  * us per launch (= per layer) at each shape and length, hipEvent-timed over --iters launches after a warm-up:
      causal      om_debug_attention_causal (the causal grouped kernel + the key-extent launch its hook makes; `extent` is that
                  launch alone, `causal_net` the difference)
      full        the existing bidirectional kernel (om_debug_attention_ex with kmax) on the same (B, L, heads): it needs MHA, so
                  its input carries the K / V heads repeated
      rope        om_debug_rope_gqa, in place

    python tools/causal_lm_bench.py [--tokens 65536] [--iters 20] [--kernels-only] [--encode-only]
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

DEV = "cuda:0"
SHAPES = {"qwen2-0.5b": dict(kind="qwen2", layers=24, hidden=896, heads=14, kv=2, ffn=4864, vocab=151936),
          "llama-3.2-1b": dict(kind="llama", layers=16, hidden=2048, heads=32, kv=8, ffn=8192, vocab=128256)}


def _timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _events_us(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _model(s):
    from transformers import LlamaConfig, LlamaModel, Qwen2Config, Qwen2Model
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(0)
    ccls, mcls = (LlamaConfig, LlamaModel) if s["kind"] == "llama" else (Qwen2Config, Qwen2Model)
    cfg = ccls(hidden_size=s["hidden"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"], num_key_value_heads=s["kv"],
               intermediate_size=s["ffn"], vocab_size=s["vocab"], max_position_embeddings=8192, pad_token_id=0)
    with torch.device(DEV):              # (initialised on the device: 1.2 G parameters take a while on the host)
        lm = mcls(cfg).eval()
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling="last", normalize=True,
                               model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV).eval()


def _batch(B, L, vocab):
    ids = torch.randint(3, vocab, (B, L), generator=torch.Generator().manual_seed(1)).to(DEV)
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def _kernels(s, B, L, iters):
    from openmatch_amd import native as N
    lib, st = N.lib(), N.stream_ptr()
    heads, kv, D = s["heads"], s["kv"], 64
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B * L, (heads + 2 * kv) * D, generator=g).to(torch.bfloat16).to(DEV)
    v = x.view(B * L, heads + 2 * kv, D)
    idx = torch.arange(heads, device=DEV) // (heads // kv)
    mha = torch.cat([v[:, :heads], v[:, heads:heads + kv][:, idx], v[:, heads + kv:][:, idx]], 1).reshape(B * L, 3 * heads * D).contiguous()
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    ctx = torch.empty(B * L, heads * D, dtype=torch.bfloat16, device=DEV)
    kmax = torch.empty(B, dtype=torch.int32, device=DEV)
    inv = (C.c_float * 32)(*[float(t) for t in 1.0 / (10000.0 ** (torch.arange(0, 64, 2).float() / 64))])
    run = lambda rc: N.check(rc)                                                                            # noqa: E731
    out = {}
    out["extent"] = _events_us(lambda: run(lib.om_debug_mask_extent(N.ptr(mask), B, L, N.ptr(kmax), st)), iters)
    out["causal"] = _events_us(lambda: run(lib.om_debug_attention_causal(N.OM_BF16, N.ptr(x), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, 0.125, st)),
                               iters)
    out["causal_net"] = out["causal"] - out["extent"]
    out["full"] = _events_us(lambda: run(lib.om_debug_attention_ex(N.OM_BF16, N.ptr(mha), N.ptr(ctx), N.ptr(mask), None, B, L, heads * D, heads,
                                                                   0.125, 0.0, 0, st, 0, N.ptr(kmax), None, 0)), iters)
    out["rope"] = _events_us(lambda: run(lib.om_debug_rope_gqa(N.OM_BF16, N.ptr(x), B * L, L, heads, kv, inv, 1.0, st)), iters)
    return {k: round(t, 1) for k, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--encode-only", action="store_true")
    a = ap.parse_args()
    out = {"dtype": "bfloat16", "tokens_per_batch": a.tokens}
    with torch.no_grad():
        for name, s in SHAPES.items():
            r = {}
            if not a.encode_only:
                for L in (128, 512, 1024):
                    r[f"kernel_us_per_layer_{L}"] = _kernels(s, a.tokens // L, L, a.iters)
            if not a.kernels_only:
                m = _model(s)
                for L in (128, 512):
                    B = a.tokens // L
                    x = _batch(B, L, s["vocab"])
                    t = _timed(lambda: m(passage=x), max(2, a.iters // 4))
                    r[f"encode_{L}"] = {"batch": B, "ms": round(t * 1e3, 2), "passages_per_s": round(B / t, 1)}
                del m
                torch.cuda.empty_cache()
            out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
