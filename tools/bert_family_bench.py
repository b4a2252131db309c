#!/usr/bin/env python
"""Encode throughput of the BERT-family backbones from ONE build, random weights, B full-length L-token passages in float16
(mean pooling + normalize through DRModelForInference, as tools/modernbert_bench.py measures): bert-base (12 x 768 / 12 / 3072),
DistilBERT-base (6 layers of the same), MPNet-base (bert-base's shape + one relative-position bias table for all layers) and,
as the yardstick for what a biased attention costs, a GTR-base-shaped T5 encoder (12 x 768 / 12 / 3072, ReLU, no gate).
Prints one JSON line: per backbone the median and the spread of the timed steps and passages/s, and the two ratios to read:
distilbert / bert (expected ~2: half the layers) and mpnet / bert beside t5 / bert (a gap of MPNet to bert-base beyond T5's
means the bias took a slow attention path: OM_ENCODER_DEBUG=1 names the path on stderr).

    python tools/bert_family_bench.py [--batch 1024] [--len 128] [--iters 9] [--dtype float16]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace as NS

SHAPE = dict(hidden=768, heads=12, ffn=3072, vocab=30522)


def _lm(kind):
    import transformers as T
    torch.manual_seed(0)
    s = SHAPE
    if kind == "bert":
        return T.BertModel(T.BertConfig(hidden_size=s["hidden"], num_attention_heads=s["heads"], intermediate_size=s["ffn"],
                                        num_hidden_layers=12, vocab_size=s["vocab"]), add_pooling_layer=False), False
    if kind == "distilbert":
        return T.DistilBertModel(T.DistilBertConfig(dim=s["hidden"], n_heads=s["heads"], hidden_dim=s["ffn"], n_layers=6,
                                                    vocab_size=s["vocab"])), False
    if kind == "mpnet":
        lm = T.MPNetModel(T.MPNetConfig(hidden_size=s["hidden"], num_attention_heads=s["heads"], intermediate_size=s["ffn"],
                                        num_hidden_layers=12, vocab_size=s["vocab"]))
        with torch.no_grad():
            lm.encoder.relative_attention_bias.weight.normal_(0.0, 1.0)
        return lm, False
    return T.T5EncoderModel(T.T5Config(d_model=s["hidden"], num_heads=s["heads"], d_kv=64, d_ff=s["ffn"], num_layers=12,
                                       vocab_size=32128, feed_forward_proj="relu")), True


def _steps(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--len", type=int, default=128)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--dtype", default="float16")
    a = ap.parse_args()
    from openmatch.modeling import DRModelForInference
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 30000, (a.batch, a.len), generator=g).to("cuda:0")
    x = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    out = {"batch": a.batch, "len": a.len, "dtype": a.dtype, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for kind in ("bert", "distilbert", "mpnet", "t5"):
            lm, enc_only = _lm(kind)
            m = DRModelForInference(lm_q=lm.eval(), lm_p=lm, pooling="mean", normalize=True,
                                    model_args=NS(encoder_only=enc_only, dtype=a.dtype)).to("cuda:0").eval()
            ts = _steps(lambda: m(passage=x), a.iters)
            med = statistics.median(ts)
            out[kind] = {"ms_median": round(med * 1e3, 3), "ms_min": round(min(ts) * 1e3, 3), "ms_max": round(max(ts) * 1e3, 3),
                         "passages_per_s": round(a.batch / med, 1)}
            del m, lm
    for k in ("distilbert", "mpnet", "t5"):
        out[f"{k}_over_bert"] = round(out[k]["passages_per_s"] / out["bert"]["passages_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
