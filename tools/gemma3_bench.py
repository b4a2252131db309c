#!/usr/bin/env python
"""Encode throughput of EmbeddingGemma's shape (bidirectional Gemma3TextModel: 24 layers, hidden 768, 3 query heads over 1 K / V head of
256 columns, FFN 1 152, sliding and full layers 5 : 1, window 512 -> 256), random weights, float16, `mean` pooling + normalize, at
1 024 x 128 and 64 x 512 tokens, full-length batches; prints one JSON line:
  * passages/s and the step time of each batch shape (each step timed on its own, median reported);
  * the head_dim 256 attention kernel, hipEvent-timed alone through om_debug_attention_gqa_d256 (which also launches the small
    key-extent kernel) over --iters launches after a warm-up, full and banded, as us per layer and as the share of the step the
    attention of all layers accounts for (sliding layers x band us + full layers x full us over the step time);
  * the q / k norm + rotation pass and the norm-add row kernel the same way.

    python tools/gemma3_bench.py [--iters 20] [--dtype float16] [--layers 24]

--ragged: the batches hold ragged right-padded rows instead of full-length ones (lengths ~ U{L/8 .. L}, the draw of
tools/causal_lm_bench.py --ragged, the same batch in every run); the result carries the tokens, the rows the contractions ran on and
B * L beside the step times, and the attention kernels are timed on the ragged mask.  --packed (with --ragged): the batch also carries
the host-side token counts, so the encoder takes om_gemma3_encoder_forward_packed (the ceiling of its gain is B * L / rows, printed
as `row_ratio`), and the attention kernels are timed in their packed form (om_debug_attention_gqa_d256_packed over the packed
projection); without it the same batch runs the padded entry.  --batches narrows a run (e.g. 1024x128).
"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

from tools.causal_lm_bench import DEV, _batch, _events_us, _ragged_batch, _steps_ms

SHAPE = dict(layers=24, hidden=768, heads=3, kv=1, head_dim=256, ffn=1152, vocab=262144, sliding_window=512)
BATCHES = [(1024, 128), (64, 512)]


def _layer_types(n):
    return ["full_attention" if (i + 1) % 6 == 0 else "sliding_attention" for i in range(n)]


def _model(dtype, layers):
    from transformers import Gemma3TextConfig, Gemma3TextModel
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(0)
    cfg = Gemma3TextConfig(hidden_size=SHAPE["hidden"], num_hidden_layers=layers, num_attention_heads=SHAPE["heads"],
                           num_key_value_heads=SHAPE["kv"], head_dim=SHAPE["head_dim"], intermediate_size=SHAPE["ffn"], vocab_size=SHAPE["vocab"],
                           sliding_window=SHAPE["sliding_window"], layer_types=_layer_types(layers), use_bidirectional_attention=True,
                           max_position_embeddings=2048, pad_token_id=0)
    with torch.device(DEV):
        lm = Gemma3TextModel(cfg).eval()
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True, model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()


def _median(ms):
    return ms[len(ms) // 2] if len(ms) % 2 else (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]) / 2


def _kernels_us(dtype, B, L, iters, half_window, mask=None, packed=False):
    from openmatch_amd import native as N
    lib, st = N.lib(), N.stream_ptr()
    code = {"float16": N.OM_F16, "bfloat16": N.OM_BF16, "float32": N.OM_F32}[dtype]
    td = getattr(torch, dtype)
    heads, kv, D, H = SHAPE["heads"], SHAPE["kv"], SHAPE["head_dim"], SHAPE["hidden"]
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B * L, (heads + 2 * kv) * D, generator=g).to(td).to(DEV)
    ctx = torch.empty(B * L, heads * D, dtype=td, device=DEV)
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV) if mask is None else mask
    gn = torch.ones(D, device=DEV)
    inv = (C.c_float * 128)(*[float(t) for t in 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))])
    h = torch.randn(B * L, H, generator=g).to(td).to(DEV)
    x = torch.zeros(B * L, H, device=DEV)
    gh = torch.ones(H, device=DEV)
    scale = 256 ** -0.5

    if packed:      # the packed projection's rows are the padded one's up to each extent: the first `total` rows serve as they are
        kmax = torch.empty(B, dtype=torch.int32, device=DEV)
        N.check(lib.om_debug_mask_extent(N.ptr(mask), B, L, N.ptr(kmax), st))
        rows = (int(kmax.sum()) + 255) // 256 * 256
        cu, cls, row_map = (torch.empty(n, dtype=torch.int32, device=DEV) for n in (B + 2, B, rows))
        N.check(lib.om_debug_pack_rows(N.ptr(kmax), B, L, rows, N.ptr(cu), N.ptr(cls), N.ptr(row_map), st))
    M = rows if packed else B * L           # the rows the two row kernels run over in the step

    def attn(w):
        if packed:
            return lambda: N.check(lib.om_debug_attention_gqa_d256_packed(code, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), N.ptr(cu), B, L, heads, kv, scale,
                                                                          w, st))
        return lambda: N.check(lib.om_debug_attention_gqa_d256(code, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, scale, w, st))
    return {"attention_full": round(_events_us(attn(0), iters), 1),
            "attention_band": round(_events_us(attn(half_window), iters), 1),
            "band_is_full_attention": not 0 < half_window < L - 1,
            "qknorm_rope": round(_events_us(lambda: N.check(lib.om_debug_qknorm_rope_d256(code, N.ptr(qkv), M, L, heads, kv, N.ptr(gn), N.ptr(gn),
                                                                                          1e-6, inv, 1.0, st)), iters), 1),
            "rmsnorm_add": round(_events_us(lambda: N.check(lib.om_debug_rmsnorm_add(code, N.ptr(h), H, N.ptr(x), H, N.ptr(gh), M, H, 1e-6, st)),
                                            iters), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", default="float16", choices=["bfloat16", "float16", "float32"])
    ap.add_argument("--layers", type=int, default=SHAPE["layers"])
    ap.add_argument("--ragged", action="store_true", help="ragged right-padded batches, each step timed on its own")
    ap.add_argument("--packed", action="store_true", help="with --ragged: hand the host-side token counts over (the packed-rows entry)")
    ap.add_argument("--batches", default=",".join(f"{b}x{l}" for b, l in BATCHES), help="comma-separated BxL batch shapes")
    a = ap.parse_args()
    if a.packed and not a.ragged:
        ap.error("--packed goes with --ragged")
    from openmatch_amd import encoder as E
    types = _layer_types(a.layers)
    n_slide, n_full = types.count("sliding_attention"), types.count("full_attention")
    out = {"dtype": a.dtype, "shape": dict(SHAPE, layers=a.layers), "sliding_layers": n_slide, "full_layers": n_full}
    if a.ragged:
        out.update(ragged=True, packed=bool(a.packed))
    with torch.no_grad():
        m = _model(a.dtype, a.layers)
        half_window = m.lm_p.config.sliding_window - 1
        out["half_window"] = half_window
        for B, L in (tuple(int(v) for v in t.split("x")) for t in a.batches.split(",")):
            x, tokens = _ragged_batch(B, L, SHAPE["vocab"], a.packed) if a.ragged else (_batch(B, L, SHAPE["vocab"]), B * L)
            ms = _steps_ms(lambda: m(passage=x), a.iters)
            med = _median(ms)
            call = dict(E.LAST_CALL)
            us = _kernels_us(a.dtype, B, L, a.iters, half_window, x["attention_mask"] if a.ragged else None, call["packed"])
            attn_ms = (n_slide * us["attention_band"] + n_full * us["attention_full"]) * 1e-3
            out[f"{B}x{L}"] = {"batch": B, "length": L, "steps": len(ms), "ms_median": round(med, 2), "ms_min": round(ms[0], 2), "ms_max": round(ms[-1], 2),
                               "passages_per_s": round(B / med * 1e3, 1), "tokens_per_s": round(B * L / med * 1e3), "kernel_us_per_layer": us,
                               "attention_share_of_step": round(attn_ms / med, 4),
                               "qknorm_rope_share_of_step": round(a.layers * us["qknorm_rope"] * 1e-3 / med, 4),
                               "rmsnorm_add_share_of_step": round(2 * a.layers * us["rmsnorm_add"] * 1e-3 / med, 4)}
            if a.ragged:
                out[f"{B}x{L}"].update(tokens=tokens, padded_rows=B * L, rows=call["rows"], packed_entry=call["packed"],
                                       row_ratio=round(B * L / call["rows"], 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
