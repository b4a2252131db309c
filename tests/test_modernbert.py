"""ModernBERT (ModernBertModel) encoded through the HIP path: pre-LayerNorm stack, rotary positions, sliding-window layers and the
GeGLU feed-forward (csrc/encoder.hip, csrc/attention_causal.hip, csrc/attention_band.hip), against the HF module built at test time (random init, perturbed
norms and embeddings, eager attention so its sliding-window mask is the explicit one), in fp32 on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS

DEV = "cuda:0"
SMALL = dict(hidden_size=256, num_attention_heads=4, intermediate_size=384)
BASE = dict(hidden_size=768, num_attention_heads=12, intermediate_size=1152)


def _cfg(shape=SMALL, layers=3, **kw):
    from transformers import ModernBertConfig
    layer_types = kw.pop("layer_types", None)
    cfg = ModernBertConfig(num_hidden_layers=layers, vocab_size=600, max_position_embeddings=1024, pad_token_id=0, bos_token_id=1,
                           eos_token_id=2, cls_token_id=1, sep_token_id=2, attn_implementation="eager", **shape, **kw)
    if layer_types is not None:       # (set afterwards: the config's rope validation refuses a list that lacks one of the two types)
        cfg.layer_types = layer_types
    return cfg


def _perturb(lm):
    """Trained-checkpoint-like norms, biases and embeddings, not the values of an init."""
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn_like(p))
            elif "embeddings" in name:
                p.add_(0.02 * torch.randn_like(p))
    return lm


def _mb(shape=SMALL, layers=3, seed=0, sharp=1.0, **kw):
    """sharp > 1 scales Wqkv: peaked attention, so that which keys a query sees (window, positions) moves the output far"""
    from transformers import ModernBertModel
    torch.manual_seed(seed)
    lm = _perturb(ModernBertModel(_cfg(shape, layers, **kw)).eval())
    if sharp != 1.0:
        with torch.no_grad():
            for layer in lm.layers:
                layer.attn.Wqkv.weight.mul_(sharp)
    return lm


def _ragged(rng, n, L, lo_len):
    ids = np.zeros((n, L), np.int64)
    mask = np.zeros((n, L), np.int64)
    for i in range(n):
        ln = L if i == 0 else int(rng.integers(min(lo_len, L), L + 1))        # one full-length row
        ids[i, :ln] = rng.integers(3, 600, ln)
        ids[i, 0] = 1
        mask[i, :ln] = 1
    return ids, mask


def _hf_reps(lm, ids, mask, pooling, head=None, normalize=False):
    with torch.no_grad():
        h = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state
        if pooling == "first":
            r = h[:, 0]
        else:
            m = torch.from_numpy(mask).unsqueeze(-1).float()
            r = (h * m).sum(1) / m.sum(1)
        if head is not None:
            r = head(r)
        if normalize:
            r = torch.nn.functional.normalize(r, dim=1)
    return r.double()


def _hip_reps(lm, ids, mask, pooling, dtype, head=None, normalize=False):
    from openmatch.modeling import DRModelForInference
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling=pooling, normalize=normalize, head_q=head, head_p=head,
                                model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        out = model.encode_passage(items)[1].double().cpu()
    lm.to("cpu")
    if head is not None:
        head.to("cpu")
    return out


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a, b, dim=1).min().item()


COS_BAR = {"float16": 5e-6, "bfloat16": 2e-4}        # tests/test_head_dim32.py: the same formats' bars against f32


# ------------------------------------------------------------------------------------------------------------- CPU
def test_arch_of_modernbert():
    from openmatch_amd.encoder import _arch_of
    assert _arch_of(_mb()) == "modernbert"


def test_config_translation_default_and_custom_layer_types():
    from openmatch_amd.encoder import modernbert_config_fields
    f = modernbert_config_fields(_cfg(layers=6))
    assert f == dict(rope_theta_global=160000.0, rope_theta_local=10000.0, half_window=64, sliding_layers=0b110110)
    f = modernbert_config_fields(_cfg(layers=4, local_attention=32, global_rope_theta=5000.0, local_rope_theta=400.0,
                                      layer_types=["sliding_attention", "full_attention", "full_attention", "sliding_attention"]))
    assert f == dict(rope_theta_global=5000.0, rope_theta_local=400.0, half_window=16, sliding_layers=0b1001)


def test_abi_version_and_config_fields():
    assert N.lib().om_abi_version() == 6 == N.ABI_VERSION
    fields = dict(N.OmEncoderConfig._fields_)
    assert fields["rope_theta_global"] is C.c_float and fields["rope_theta_local"] is C.c_float
    assert fields["half_window"] is C.c_int and fields["sliding_layers"] is C.c_uint64
    assert [n for n, _ in N.OmEncoderConfig._fields_][-4:] == ["rope_theta_global", "rope_theta_local", "half_window", "sliding_layers"]
    assert N.OmEncoderConfig.sliding_layers.offset == 88 and C.sizeof(N.OmEncoderConfig) == 96      # (include/openmatch_hip.h layout)
    assert [n for n, _ in N.OmEncoderWeights._fields_][-1] == "final_ln_b"
    assert N.ARCH_MODERNBERT == 2


def test_packed_rows_not_offered_for_modernbert():
    from openmatch_amd.encoder import _pack_modernbert  # noqa: F401  (host-only check below)
    cfg = N.OmEncoderConfig(arch=N.ARCH_MODERNBERT, dtype=N.OM_BF16, hidden=768, n_layers=22, n_heads=12, head_dim=64, ffn=1152,
                            vocab=600, act=N.ACT_GELU_ERF, ln_eps=1e-5, pooling=N.POOL_MEAN, rope_theta_global=160000.0,
                            rope_theta_local=10000.0, half_window=64, sliding_layers=0)
    assert N.lib().om_encoder_packed_supported(C.byref(cfg), 1, 64, 128, 4096) == 0


def test_refusals_on_the_host():
    from openmatch_amd.encoder import modernbert_config_fields
    with pytest.raises(NotImplementedError, match="attention_bias"):
        modernbert_config_fields(_cfg(attention_bias=True))
    with pytest.raises(NotImplementedError, match="mlp_bias"):
        modernbert_config_fields(_cfg(mlp_bias=True))
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        modernbert_config_fields(_cfg(dict(hidden_size=256, num_attention_heads=8, intermediate_size=384)))
    with pytest.raises(NotImplementedError, match="gelu"):
        modernbert_config_fields(_cfg(hidden_activation="relu"))


def test_training_is_refused_naming_modernbert():
    from openmatch_amd.train import encode_train
    lm = _mb()
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="ModernBERT training"):
        encode_train(lm, None, items, "first", False, N.OM_BF16, True)


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(24, 6), (128, 6), (200, 5), (320, 4), (512, 3), (1024, 2)])
def test_encode_matches_hf_small(L, n):
    """3 layers (global, sliding, sliding) at hidden 256, window 128: `first` pooling bare, `mean` pooling with a LinearHead and
    normalize; f32 within 1e-4 relative of HF fp32, 16-bit by cosine."""
    from openmatch.modeling import LinearHead
    lm = _mb(seed=L, norm_bias=L in (24, 320, 1024))
    torch.manual_seed(100 + L)
    head = LinearHead(256, 256)
    rng = np.random.default_rng(L)
    ids, mask = _ragged(rng, n, L, max(2, L // 3))
    for pooling, hd, norm in (("first", None, False), ("mean", head, True)):
        want = _hf_reps(lm, ids, mask, pooling, hd.linear if hd is not None else None, norm)
        for dtype in ("float32", "float16", "bfloat16"):
            got = _hip_reps(lm, ids, mask, pooling, dtype, hd, norm)
            rel, c = _rel(got, want), 1 - _cos(got, want)
            print(f"\n[modernbert small L={L} {pooling} {dtype}] max rel {rel:.2e}, 1 - cos {c:.2e}")
            assert torch.isfinite(got).all()
            if dtype == "float32":
                assert rel < 1e-4, rel
            else:
                assert c < COS_BAR[dtype], c


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(128, 4), (512, 2), (1024, 2)])
def test_encode_matches_hf_base_width(L, n):
    """ModernBERT-base width (768 / 12 heads / 1152), 4 layers (global, sliding, sliding, global), mean pooling."""
    lm = _mb(BASE, layers=4, seed=7 + L)
    rng = np.random.default_rng(L + 1)
    ids, mask = _ragged(rng, n, L, L // 4)
    want = _hf_reps(lm, ids, mask, "mean")
    for dtype in ("float32", "float16", "bfloat16"):
        got = _hip_reps(lm, ids, mask, "mean", dtype)
        rel, c = _rel(got, want), 1 - _cos(got, want)
        print(f"\n[modernbert base L={L} {dtype}] max rel {rel:.2e}, 1 - cos {c:.2e}")
        if dtype == "float32":
            assert rel < 1e-4, rel
        else:
            assert c < COS_BAR[dtype], c


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 512])
def test_band_exercised_every_layer_sliding(L):
    """local_attention = 32 (keys within 16 of the query) on every layer: the HIP result matches HF and is far from the same model
    with full attention, so a kernel that ignored the window would fail by far more than the tolerance."""
    kw = dict(local_attention=32, layer_types=["sliding_attention"] * 3)
    lm = _mb(seed=3, sharp=8.0, **kw)
    full = _mb(seed=3, local_attention=32, layer_types=["full_attention"] * 3,
               global_rope_theta=10000.0)                                   # the same weights, every layer global at the local theta
    full.load_state_dict(lm.state_dict())
    rng = np.random.default_rng(5)
    ids, mask = _ragged(rng, 3, L, L // 2)
    want = _hf_reps(lm, ids, mask, "mean")
    other = _hf_reps(full, ids, mask, "mean")
    assert _rel(other, want) > 0.1
    for dtype in ("float32", "float16", "bfloat16"):
        got = _hip_reps(lm, ids, mask, "mean", dtype)
        if dtype == "float32":
            assert _rel(got, want) < 1e-4, _rel(got, want)
        else:
            assert 1 - _cos(got, want) < COS_BAR[dtype]


@pytest.mark.gpu
def test_band_edges_are_inclusive_and_padding_inside_the_band():
    """Keys at exactly |q - k| = 16 count (HF's inclusive <=, both sides): the result of window 32 matches HF at 32 and not HF at
    30 or 34.  Rows end 5 .. 12 tokens before L, so padded keys fall inside the band of the last real queries."""
    L = 128
    ids, mask = _ragged(np.random.default_rng(9), 4, L, 2)
    for i, ln in enumerate((L, L - 5, L - 9, L - 12)):
        mask[i] = 0; mask[i, :ln] = 1
        ids[i, ln:] = 0
    refs = {}
    for la in (30, 32, 34):
        lm = _mb(seed=4, sharp=8.0, local_attention=la, layer_types=["sliding_attention"] * 2, layers=2)
        refs[la] = _hf_reps(lm, ids, mask, "mean")
        if la == 32:
            model32 = lm
    got = _hip_reps(model32, ids, mask, "mean", "float32")
    assert _rel(got, refs[32]) < 1e-4
    assert _rel(got, refs[30]) > 5e-3 and _rel(got, refs[34]) > 5e-3


@pytest.mark.gpu
def test_rope_thetas_per_layer_type():
    """Custom thetas on each layer type (global 5 000, local 400): matches HF, and HF with the two thetas swapped is far away."""
    kw = dict(local_attention=64)
    lm = _mb(seed=6, sharp=8.0, global_rope_theta=5000.0, local_rope_theta=400.0, **kw)
    swapped = _mb(seed=6, global_rope_theta=400.0, local_rope_theta=5000.0, **kw)
    swapped.load_state_dict(lm.state_dict())
    ids, mask = _ragged(np.random.default_rng(1), 3, 256, 100)
    want = _hf_reps(lm, ids, mask, "first")
    assert _rel(_hf_reps(swapped, ids, mask, "first"), want) > 0.1
    got = _hip_reps(lm, ids, mask, "first", "float32")
    assert _rel(got, want) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_padding_invariance(dtype):
    """The representations of a batch do not change, bit for bit, when 128 more pad columns are appended."""
    lm = _mb(seed=8, local_attention=32)
    ids, mask = _ragged(np.random.default_rng(2), 16, 128, 20)
    ids2 = np.concatenate([ids, np.zeros_like(ids)], 1)
    mask2 = np.concatenate([mask, np.zeros_like(mask)], 1)
    a = _hip_reps(lm, ids, mask, "mean", dtype)
    b = _hip_reps(lm, ids2, mask2, "mean", dtype)
    assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.gpu
def test_cross_encoder_over_modernbert():
    """RRModel over a ModernBertModel with LinearHead(256, 1): f32 scores within 1e-4 of HF fp32 + first pooling + head."""
    from openmatch.modeling import LinearHead, RRModel
    lm = _mb(seed=12)
    torch.manual_seed(13)
    head = LinearHead(256, 1)
    ids, mask = _ragged(np.random.default_rng(3), 8, 160, 40)
    want = _hf_reps(lm, ids, mask, "first", head.linear)
    model = RRModel(lm=lm, head=head, pooling="first", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with torch.no_grad():
        got = model.encode({"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)})
    assert got.shape == (8, 1)
    assert (got.double().cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


@pytest.mark.gpu
def test_retriever_end_to_end(tmp_path):
    """Corpus and queries encoded by the HIP ModernBERT, searched by Retriever: the top-10 ids are those of HF fp32 embeddings
    searched by the oracle's exact inner-product index."""
    import pickle
    from openmatch.modeling import DRModelForInference
    from openmatch.retriever import Retriever
    from oracle import flatip
    lm = _mb(seed=14)
    rng = np.random.default_rng(4)
    P_ids, P_mask = _ragged(rng, 96, 128, 30)
    Q_ids, Q_mask = _ragged(rng, 12, 32, 8)
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True,
                                model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with torch.no_grad():
        P = model.encode_passage({"input_ids": torch.from_numpy(P_ids).to(DEV), "attention_mask": torch.from_numpy(P_mask).to(DEV)})[1]
        Q = model.encode_query({"input_ids": torch.from_numpy(Q_ids).to(DEV), "attention_mask": torch.from_numpy(Q_mask).to(DEV)})[1]
    lm.to("cpu")
    Pw = _hf_reps(lm, P_ids, P_mask, "mean", None, True).float().numpy()
    Qw = _hf_reps(lm, Q_ids, Q_mask, "mean", None, True).float().numpy()
    doc_ids = [f"d{i}" for i in range(96)]
    qry_ids = [f"q{i}" for i in range(12)]
    with open(tmp_path / "embeddings.corpus.rank.0", "wb") as f:
        pickle.dump((P.cpu().numpy(), doc_ids), f, protocol=4)
    with open(tmp_path / "embeddings.query.rank.0", "wb") as f:
        pickle.dump((Q.cpu().numpy(), qry_ids), f, protocol=4)
    args = NS(device=DEV, output_dir=str(tmp_path), world_size=1, process_index=0, local_process_index=0, fp16=False)
    run = Retriever.from_embeddings(model, args).search(10)
    o = flatip.IndexFlatIP(Pw.shape[1]); o.add(Pw)
    _, I = o.search(Qw, 10)
    for qi, q in enumerate(qry_ids):
        assert list(run[q].keys()) == [doc_ids[j] for j in I[qi]], q


@pytest.mark.gpu
def test_refusals_on_the_device():
    """Training a ModernBERT DRModel raises naming ModernBERT; 1 025 tokens are refused."""
    from openmatch.modeling import DRModel
    lm = _mb(seed=15)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="first", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV)
    items = {"input_ids": torch.ones(2, 16, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(2, 16, dtype=torch.int64, device=DEV)}
    model.train()
    with pytest.raises(NotImplementedError, match="ModernBERT"):
        model.encode_passage(items)
    model.eval()
    long = {"input_ids": torch.ones(1, 1025, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(1, 1025, dtype=torch.int64, device=DEV)}
    with torch.no_grad(), pytest.raises(Exception, match="1024|1 024|length"):
        model.encode_passage(long)
