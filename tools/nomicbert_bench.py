#!/usr/bin/env python
"""Encode throughput of nomic-embed-text-v1.5 (NomicBertModel: 12 layers, hidden 768, 12 heads, FFN 3 072, rotary Q / K, SwiGLU) beside
bert-base at the same widths IN THE SAME RUN, random weights, float16, 128 tokens, `mean` pooling + normalize; prints one JSON line:
  * passages/s of each backbone, their ratio (nomic / bert), the rows the contractions ran on and whether the packed entry took the call;
  * the two elementwise launches NomicBERT adds to a BERT layer, hipEvent-timed alone through their hooks over --iters launches after
    a warm-up -- om_debug_rope (rows: om_debug_rope_rows) and om_debug_swiglu_rows -- as us per layer and as the share of the nomic
    step they account for (layers * us / step time).

    python tools/nomicbert_bench.py [--tokens 65536] [--iters 20] [--ragged [--packed]] [--dtype float16] [--length 128]

Without --ragged: full-length batches.  --ragged: ragged right-padded rows (lengths ~ U{L/8 .. L}, as tools/causal_lm_bench.py draws
them), each step timed on its own, median reported.  --packed (with --ragged): the batch also carries the host-side token counts, so the
encoder takes om_encoder_forward_packed.  --all: the three modes one after the other in one process (one JSON line, a key per mode).
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

from tools.causal_lm_bench import DEV, _events_us, _ragged_batch, _steps_ms, _batch

SHAPE = dict(layers=12, hidden=768, heads=12, ffn=3072, vocab=30528)


def _model(kind, dtype):
    from transformers import BertConfig, BertModel, NomicBertConfig, NomicBertModel
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(0)
    common = dict(hidden_size=SHAPE["hidden"], num_hidden_layers=SHAPE["layers"], num_attention_heads=SHAPE["heads"],
                  intermediate_size=SHAPE["ffn"], vocab_size=SHAPE["vocab"], pad_token_id=0)
    with torch.device(DEV):
        lm = (NomicBertModel(NomicBertConfig(max_position_embeddings=2048, **common)) if kind == "nomic"
              else BertModel(BertConfig(max_position_embeddings=512, **common), add_pooling_layer=False)).eval()
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True, model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()


def _median(ms):
    return ms[len(ms) // 2] if len(ms) % 2 else (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]) / 2


def _encode(kind, dtype, B, L, ragged, packed, iters):
    from openmatch_amd import encoder as E
    m = _model(kind, dtype)
    if ragged:
        x, tokens = _ragged_batch(B, L, SHAPE["vocab"], packed)
    else:
        x, tokens = _batch(B, L, SHAPE["vocab"]), B * L
    ms = _steps_ms(lambda: m(passage=x), iters)
    med = _median(ms)
    r = {"batch": B, "tokens": tokens, "padded_rows": B * L, "rows": E.LAST_CALL["rows"], "packed_entry": E.LAST_CALL["packed"], "steps": len(ms),
         "ms_median": round(med, 2), "ms_min": round(ms[0], 2), "ms_max": round(ms[-1], 2), "passages_per_s": round(B / med * 1e3, 1)}
    del m
    torch.cuda.empty_cache()
    return r


def _elementwise_us(dtype, rows, L, iters, mapped):
    """us per launch of the rotary pass over [rows, 3H] and of the SwiGLU pass [rows, 2F] -> [rows, F]"""
    from openmatch_amd import native as N
    lib, st = N.lib(), N.stream_ptr()
    code = {"float16": N.OM_F16, "bfloat16": N.OM_BF16, "float32": N.OM_F32}[dtype]
    td = getattr(torch, dtype)
    H, F = SHAPE["hidden"], SHAPE["ffn"]
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(rows, 3 * H, generator=g).to(td).to(DEV)
    ff = torch.randn(rows, 2 * F, generator=g).to(td).to(DEV)
    out = torch.empty(rows, F, dtype=td, device=DEV)
    row_map = torch.arange(rows, dtype=torch.int32, device=DEV)
    if mapped:
        rope = lambda: N.check(lib.om_debug_rope_rows(code, N.ptr(qkv), rows, L, H, 1000.0, N.ptr(row_map), st))      # noqa: E731
    else:
        rope = lambda: N.check(lib.om_debug_rope(code, N.ptr(qkv), rows, L, H, 1000.0, st))                            # noqa: E731
    return {"rope": round(_events_us(rope, iters), 1),
            "swiglu": round(_events_us(lambda: N.check(lib.om_debug_swiglu_rows(code, N.ptr(ff), N.ptr(out), rows, F, st)), iters), 1)}


def _mode(a, ragged, packed):
    B, L = a.tokens // a.length, a.length
    r = {"nomic-embed-text-v1.5": _encode("nomic", a.dtype, B, L, ragged, packed, a.iters),
         "bert-base": _encode("bert", a.dtype, B, L, ragged, packed, a.iters)}
    n, b = r["nomic-embed-text-v1.5"], r["bert-base"]
    r["ratio_nomic_over_bert"] = round(n["passages_per_s"] / b["passages_per_s"], 3)
    us = _elementwise_us(a.dtype, n["rows"], L, a.iters, n["packed_entry"])
    r["elementwise_us_per_layer"] = us
    r["elementwise_share_of_nomic_step"] = round(SHAPE["layers"] * (us["rope"] + us["swiglu"]) * 1e-3 / n["ms_median"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--dtype", default="float16", choices=["bfloat16", "float16", "float32"])
    ap.add_argument("--ragged", action="store_true", help="ragged right-padded encode batches, each step timed on its own")
    ap.add_argument("--packed", action="store_true", help="with --ragged: hand the host-side token counts over (the packed-rows entry)")
    ap.add_argument("--all", action="store_true", help="padded, --ragged and --ragged --packed in one process")
    a = ap.parse_args()
    if a.packed and not a.ragged:
        ap.error("--packed goes with --ragged")
    out = {"dtype": a.dtype, "tokens_per_batch": a.tokens, "length": a.length, "shape": SHAPE}
    with torch.no_grad():
        if a.all:
            out["padded"] = _mode(a, False, False)
            out["ragged"] = _mode(a, True, False)
            out["ragged_packed"] = _mode(a, True, True)
        else:
            out.update(ragged=bool(a.ragged), packed=bool(a.packed), **_mode(a, a.ragged, a.packed))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
