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

--ragged: the encode batches hold ragged right-padded rows instead of full-length ones (lengths ~ U{L/8 .. L}, as tools/train_bench.py
draws them) and each step is timed on its own; the result carries the median, fastest and slowest of --iters steps, the rows the
contractions ran on and B * L.  --packed (with --ragged): the batch also carries the host-side token counts, so the encoder takes
om_causal_encoder_forward_packed; without it the same batch runs the padded entry.  --dtype, --shapes and --lengths narrow a run.
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

DEV = "cuda:0"
SHAPES = {"qwen2-0.5b": dict(kind="qwen2", layers=24, hidden=896, heads=14, kv=2, ffn=4864, vocab=151936),
          "llama-3.2-1b": dict(kind="llama", layers=16, hidden=2048, heads=32, kv=8, ffn=8192, vocab=128256),
          "qwen3-embedding-0.6b": dict(kind="qwen3", layers=28, hidden=1024, heads=16, kv=8, head_dim=128, ffn=3072, vocab=151669)}


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


def _steps_ms(fn, iters):
    for _ in range(3):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


def _model(s, dtype="bfloat16"):
    from transformers import LlamaConfig, LlamaModel, Qwen2Config, Qwen2Model, Qwen3Config, Qwen3Model
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(0)
    ccls, mcls = {"llama": (LlamaConfig, LlamaModel), "qwen2": (Qwen2Config, Qwen2Model), "qwen3": (Qwen3Config, Qwen3Model)}[s["kind"]]
    extra = {"head_dim": s["head_dim"]} if "head_dim" in s else {}
    cfg = ccls(hidden_size=s["hidden"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"], num_key_value_heads=s["kv"],
               intermediate_size=s["ffn"], vocab_size=s["vocab"], max_position_embeddings=8192, pad_token_id=0, **extra)
    with torch.device(DEV):              # (initialised on the device: 1.2 G parameters take a while on the host)
        lm = mcls(cfg).eval()
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling="last", normalize=True,
                               model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()


def _batch(B, L, vocab):
    ids = torch.randint(3, vocab, (B, L), generator=torch.Generator().manual_seed(1)).to(DEV)
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def _ragged_batch(B, L, vocab, packed):
    from openmatch_amd.encoder import TOKEN_ROWS_KEY, token_rows_of
    ids = torch.randint(3, vocab, (B, L), generator=torch.Generator().manual_seed(1))
    lens = torch.randint(max(2, L // 8), L + 1, (B,), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    x = {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)}
    if packed:                           # the token counts a caller notes while the collator's batch is still on the host
        x[TOKEN_ROWS_KEY] = token_rows_of(mask)
    return x, int(lens.sum())


def _kernels_d128(s, B, L, iters):
    """The 128-wide causal kernel and the q / k norm + rotation pass alone, beside the 64-wide causal kernel on a case of equal FLOPs
    and bytes: twice the heads (and K / V heads) of half the width."""
    from openmatch_amd import native as N
    lib, st = N.lib(), N.stream_ptr()
    heads, kv, D = s["heads"], s["kv"], 128
    x = torch.randn(B * L, (heads + 2 * kv) * D, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    ctx = torch.empty(B * L, heads * D, dtype=torch.bfloat16, device=DEV)
    kmax = torch.empty(B, dtype=torch.int32, device=DEV)
    g = torch.ones(D, device=DEV)
    inv = (C.c_float * 64)(*[float(t) for t in 1.0 / (1000000.0 ** (torch.arange(0, D, 2).float() / D))])
    run = lambda rc: N.check(rc)                                                                            # noqa: E731
    out = {}
    out["extent"] = _events_us(lambda: run(lib.om_debug_mask_extent(N.ptr(mask), B, L, N.ptr(kmax), st)), iters)
    out["causal_d128"] = _events_us(lambda: run(lib.om_debug_attention_causal_hd(N.OM_BF16, N.ptr(x), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, 128,
                                                                                 128 ** -0.5, st)), iters) - out["extent"]
    out["causal_d64_equal_flops"] = _events_us(lambda: run(lib.om_debug_attention_causal_hd(N.OM_BF16, N.ptr(x), N.ptr(ctx), N.ptr(mask), B, L, 2 * heads,
                                                                                            2 * kv, 64, 0.125, st)), iters) - out["extent"]
    out["qknorm_rope"] = _events_us(lambda: run(lib.om_debug_qknorm_rope(N.OM_BF16, N.ptr(x), B * L, L, heads, kv, 128, N.ptr(g), N.ptr(g), 1e-6, inv,
                                                                         1.0, st)), iters)
    return {k: round(t, 1) for k, t in out.items()}


def _kernels(s, B, L, iters):
    if s.get("head_dim") == 128:
        return _kernels_d128(s, B, L, iters)
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
    ap.add_argument("--ragged", action="store_true", help="ragged right-padded encode batches, each step timed on its own")
    ap.add_argument("--packed", action="store_true", help="with --ragged: hand the host-side token counts over (the packed-rows entry)")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16", "float32"])
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated subset of " + ", ".join(SHAPES))
    ap.add_argument("--lengths", default="128,512", help="comma-separated encode lengths")
    a = ap.parse_args()
    if a.packed and not a.ragged:
        ap.error("--packed goes with --ragged")
    out = {"dtype": a.dtype, "tokens_per_batch": a.tokens}
    if a.ragged:
        out.update(ragged=True, packed=bool(a.packed))
    with torch.no_grad():
        for name in a.shapes.split(","):
            s = SHAPES[name]
            r = {}
            if not a.encode_only and not a.ragged:
                for L in (128, 512, 1024):
                    r[f"kernel_us_per_layer_{L}"] = _kernels(s, a.tokens // L, L, a.iters)
            if not a.kernels_only:
                from openmatch_amd import encoder as E
                m = _model(s, a.dtype)
                for L in (int(v) for v in a.lengths.split(",")):
                    B = a.tokens // L
                    if a.ragged:
                        x, tokens = _ragged_batch(B, L, s["vocab"], a.packed)
                        ms = _steps_ms(lambda: m(passage=x), a.iters)
                        med = ms[len(ms) // 2] if len(ms) % 2 else (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]) / 2
                        r[f"encode_{L}"] = {"batch": B, "tokens": tokens, "padded_rows": B * L, "rows": E.LAST_CALL["rows"],
                                            "packed_entry": E.LAST_CALL["packed"], "steps": len(ms), "ms_median": round(med, 2),
                                            "ms_min": round(ms[0], 2), "ms_max": round(ms[-1], 2), "passages_per_s": round(B / med * 1e3, 1)}
                        continue
                    x = _batch(B, L, s["vocab"])
                    t = _timed(lambda: m(passage=x), max(2, a.iters // 4))
                    r[f"encode_{L}"] = {"batch": B, "ms": round(t * 1e3, 2), "passages_per_s": round(B / t, 1)}
                del m
                torch.cuda.empty_cache()
            out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
