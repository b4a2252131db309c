"""Decoder-only retrievers (HF LlamaModel / Qwen2Model) encoded through the HIP path: pre-RMSNorm stack, rotary grouped-query CAUSAL
attention, SwiGLU, last-token pooling (csrc/encoder_causal.hip, csrc/attention_causal.hip), against the HF module built at test time
(random init, perturbed norms, biases and embeddings, eager attention), in fp32 on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS
from tests.test_modernbert import COS_BAR, _cos, _perturb, _ragged, _rel

DEV = "cuda:0"
SMALL = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=384)
QWEN05 = dict(hidden_size=896, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864)
LLAMA3 = {"rope_type": "llama3", "rope_theta": 10000.0, "factor": 8.0, "original_max_position_embeddings": 64, "low_freq_factor": 1.0,
          "high_freq_factor": 4.0}


def _cfg(kind="llama", shape=SMALL, layers=3, **kw):
    from transformers import LlamaConfig, Qwen2Config
    cls = LlamaConfig if kind == "llama" else Qwen2Config
    return cls(num_hidden_layers=layers, vocab_size=600, max_position_embeddings=1024, pad_token_id=0, bos_token_id=1, eos_token_id=2,
               attn_implementation="eager", **shape, **kw)


def _lm(kind="llama", shape=SMALL, layers=3, seed=0, sharp=1.0, **kw):
    """sharp > 1 scales the q / k weights: peaked attention, so that which keys a query sees moves the output far"""
    from transformers import LlamaModel, Qwen2Model
    torch.manual_seed(seed)
    lm = _perturb((LlamaModel if kind == "llama" else Qwen2Model)(_cfg(kind, shape, layers, **kw)).eval())
    with torch.no_grad():
        lm.embed_tokens.weight.add_(0.02 * torch.randn_like(lm.embed_tokens.weight))       # (_perturb's rule names "embeddings")
        if sharp != 1.0:
            for layer in lm.layers:
                layer.self_attn.q_proj.weight.mul_(sharp)
                layer.self_attn.k_proj.weight.mul_(sharp)
    return lm


def _left(ids, mask):
    """the same rows left-padded"""
    ids2, mask2 = np.zeros_like(ids), np.zeros_like(mask)
    L = ids.shape[1]
    for i in range(ids.shape[0]):
        n = int(mask[i].sum())
        ids2[i, L - n:] = ids[i, :n]
        mask2[i, L - n:] = 1
    return ids2, mask2


def _last_index(mask):
    m = torch.from_numpy(mask) != 0
    L = m.shape[1]
    return L - 1 - m.flip(1).to(torch.int8).argmax(1)


def _hf_hidden(lm, ids, mask):
    with torch.no_grad():
        return lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state


def _pool(h, mask, pooling, head=None, normalize=False):
    with torch.no_grad():
        if pooling == "last":
            r = h[torch.arange(h.shape[0]), _last_index(mask)]
        elif pooling == "first":
            r = h[:, 0]
        else:
            m = torch.from_numpy(mask).unsqueeze(-1).float()
            r = (h * m).sum(1) / m.sum(1)
        if head is not None:
            r = head(r)
        if normalize:
            r = torch.nn.functional.normalize(r, dim=1)
    return r.double()


def _hf_reps(lm, ids, mask, pooling, head=None, normalize=False):
    return _pool(_hf_hidden(lm, ids, mask), mask, pooling, head, normalize)


def _model(lm, pooling, dtype, head=None, normalize=False):
    from openmatch.modeling import DRModelForInference
    return DRModelForInference(lm_q=lm, lm_p=lm, pooling=pooling, normalize=normalize, head_q=head, head_p=head,
                               model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()


def _hip(lm, ids, mask, pooling, dtype, head=None, normalize=False, hidden=False):
    model = _model(lm, pooling, dtype, head, normalize)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        h, r = model.encode_passage(items)
    lm.to("cpu")
    if head is not None:
        head.to("cpu")
    return (h.cpu(), r.double().cpu()) if hidden else r.double().cpu()


def _autocast_deviation(lm, ids, mask, pooling, head, normalize, dtype, want):
    """1 - cos of HF's OWN torch.autocast run of the same model and inputs against its fp32 run (the reference's `--fp16` path)"""
    lm.to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=getattr(torch, dtype)):
        h = lm(input_ids=torch.from_numpy(ids).to(DEV), attention_mask=torch.from_numpy(mask).to(DEV)).last_hidden_state.float().cpu()
    lm.to("cpu")
    return 1 - _cos(_pool(h, mask, pooling, head, normalize), want)


def _check(got, want, dtype, tag, oracle=None):
    """float32: max relative error < 1e-4.  16-bit: 1 - cos below COS_BAR; where that bar is not met the gate is 1.0 x the deviation of
    HF's own autocast run of the same model and inputs from its fp32 run -- oracle = (lm, ids, mask, pooling,
    head linear, normalize) -- and both figures are printed."""
    rel, c = _rel(got, want), 1 - _cos(got, want)
    print(f"\n[{tag} {dtype}] max rel {rel:.2e}, 1 - cos {c:.2e}")
    assert torch.isfinite(got).all()
    if dtype == "float32":
        assert rel < 1e-4, rel
    elif c >= COS_BAR[dtype] and oracle is not None:
        ref = _autocast_deviation(*oracle, dtype, want)
        print(f"[{tag} {dtype}] above the bar {COS_BAR[dtype]:.0e}: HF autocast against its own fp32 run 1 - cos {ref:.2e}")
        assert c <= ref, (c, ref)
    else:
        assert c < COS_BAR[dtype], c


# ------------------------------------------------------------------------------------------------------------- CPU
def test_arch_dispatch():
    from transformers import GPT2Config, GPT2Model, MistralConfig, MistralModel
    from openmatch_amd.encoder import _arch_of
    assert _arch_of(_lm("llama", layers=1)) == "causal" and _arch_of(_lm("qwen2", layers=1)) == "causal"
    mistral = MistralModel(MistralConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=128,
                                         num_hidden_layers=1, vocab_size=100))
    with pytest.raises(NotImplementedError, match="MistralModel"):
        _arch_of(mistral)
    with pytest.raises(NotImplementedError, match="GPT2Model"):
        _arch_of(GPT2Model(GPT2Config(n_embd=64, n_layer=1, n_head=2, vocab_size=100)))


@pytest.mark.parametrize("rope", [None, {"rope_type": "linear", "rope_theta": 10000.0, "factor": 4.0}, LLAMA3])
def test_config_translation(rope):
    from openmatch_amd.encoder import causal_config, causal_config_fields
    lm = _lm("llama", layers=2, **({"rope_parameters": rope} if rope else {}))
    f = causal_config_fields(lm.config, lm)
    assert f["n_kv_heads"] == 2 and f["n_heads"] == 4 and f["hidden"] == 256 and f["ffn"] == 384 and f["head_dim"] == 64
    assert f["arch"] == N.ARCH_CAUSAL and f["act"] == N.ACT_SILU and f["ln_eps"] == lm.config.rms_norm_eps
    assert torch.equal(torch.tensor(f["inv_freq"], dtype=torch.float32), lm.rotary_emb.inv_freq.float())
    assert f["rope_attention_scaling"] == float(lm.rotary_emb.attention_scaling) == 1.0
    if rope is not None:
        default = causal_config_fields((d := _lm("llama", layers=2)).config, d)
        assert f["inv_freq"] != default["inv_freq"]
        if rope["rope_type"] == "linear":
            assert np.allclose(np.array(f["inv_freq"]) * 4.0, default["inv_freq"], rtol=1e-6)
    cc = causal_config(dict(dtype=N.OM_F16, head_in=0, head_out=0, **f), N.POOL_LAST, True)
    assert cc.n_kv_heads == 2 and cc.base.pooling == 3 and cc.base.normalize == 1 and cc.base.dtype == N.OM_F16
    assert list(cc.inv_freq) == [np.float32(v) for v in f["inv_freq"]]
    q = _lm("qwen2", layers=1)
    assert causal_config_fields(q.config, q)["n_kv_heads"] == 2
    lm.rotary_emb.attention_scaling = 1.25                       # what a scaled rope type would leave there
    assert causal_config_fields(lm.config, lm)["rope_attention_scaling"] == 1.25


def test_refusals_on_the_host():
    from openmatch_amd.encoder import causal_config_fields

    def fields(kind="llama", **kw):
        lm = _lm(kind, layers=1, **kw)
        return causal_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="LlamaModel.*head_dim 64"):
        fields(shape=dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=384))
    with pytest.raises(NotImplementedError, match="LlamaModel.*mlp_bias"):
        fields(mlp_bias=True)
    with pytest.raises(NotImplementedError, match="Qwen2Model.*use_sliding_window"):
        fields("qwen2", use_sliding_window=True, sliding_window=64, max_window_layers=0)
    for kind in ("dynamic", "yarn", "longrope"):
        lm = _lm("llama", layers=1)
        lm.config.rope_parameters = {"rope_type": kind, "rope_theta": 10000.0, "factor": 2.0}
        with pytest.raises(NotImplementedError, match=f"LlamaModel.*{kind}"):
            causal_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="silu"):
        fields(hidden_act="gelu")


def test_training_is_refused_naming_the_family():
    from openmatch_amd.train import encode_train
    lm = _lm("llama", layers=1)
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="Llama / Qwen2 training"):
        encode_train(lm, None, items, "last", False, N.OM_BF16, True)


def test_pooling_last_is_for_causal_backbones_only():
    from transformers import BertModel
    from openmatch_amd.encoder import check_pooling, hip_encode
    from tests.helpers import tiny_bert_config
    bert = BertModel(tiny_bert_config())
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="pooling='last'.*Llama / Qwen2.*BertModel"):
        hip_encode(bert, items, "last", None, False, N.OM_F32)
    with pytest.raises(ValueError, match="Unknown pooling type: max"):
        hip_encode(bert, items, "max", None, False, N.OM_F32)
    with pytest.raises(ValueError, match="Unknown pooling type: max"):
        check_pooling(_lm("llama", layers=1), "max")
    check_pooling(_lm("llama", layers=1), "last")


def test_abi_is_unchanged_and_the_causal_struct_embeds_the_config():
    lib = N.lib()
    assert lib.om_abi_version() == 6 == N.ABI_VERSION
    assert C.sizeof(N.OmEncoderConfig) == 96
    assert N.OmCausalConfig.base.offset == 0 and N.OmCausalConfig.n_kv_heads.offset == 96
    assert N.OmCausalConfig.rope_attention_scaling.offset == 100 and N.OmCausalConfig.inv_freq.offset == 104
    assert C.sizeof(N.OmCausalConfig) == 232
    assert N.POOL_LAST == 3 and N.ARCH_CAUSAL == 3
    # argument checks happen on the host, before any launch
    f = dict(arch=N.ARCH_CAUSAL, dtype=N.OM_BF16, hidden=256, n_layers=1, n_heads=4, head_dim=64, ffn=384, vocab=600, act=N.ACT_SILU,
             ln_eps=1e-6, pooling=N.POOL_LAST)
    cc = N.OmCausalConfig(base=N.OmEncoderConfig(**f), n_kv_heads=2, rope_attention_scaling=1.0, inv_freq=(C.c_float * 32)(*([0.5] * 32)))
    assert lib.om_causal_encoder_workspace_bytes(C.byref(cc), 4, 128) >= 512 * (256 * 3 + 512 + 2 * 384) * 2
    w = N.OmEncoderWeights()

    def refused(cfg, L=8):
        return lib.om_causal_encoder_forward(C.byref(cfg), C.byref(w), 16, 16, 1, L, None, 16, 256, 1 << 30, None)
    assert refused(cc, 1025) != 0 and b"1024" in lib.om_last_error()
    cc.n_kv_heads = 3
    assert refused(cc) != 0 and b"divide" in lib.om_last_error()
    cc.n_kv_heads = 2
    cc.base.head_dim = 128
    assert refused(cc) != 0 and b"head_dim 64" in lib.om_last_error()
    cc.base.head_dim = 64
    cc.base.arch = N.ARCH_BERT
    assert refused(cc) != 0 and b"OM_ARCH_CAUSAL" in lib.om_last_error()
    # the existing entry keeps refusing what it does not know
    bad = N.OmEncoderConfig(**f)
    assert lib.om_encoder_forward(C.byref(bad), C.byref(w), 16, 16, None, 1, 8, None, 16, 256, 1 << 30, None) != 0


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(24, 6), (128, 6), (200, 5), (320, 4), (512, 3), (1024, 2)])
def test_encode_matches_hf_small(L, n):
    """3 layers at hidden 256, 4 heads over 2 K / V heads: `last` pooling bare, `mean` pooling with a LinearHead and normalize, on a
    ragged right-padded batch and on the same rows left-padded; f32 within 1e-4 relative of HF fp32, 16-bit by cosine."""
    from openmatch.modeling import LinearHead
    lm = _lm("llama" if L in (24, 200, 512) else "qwen2", seed=L, **({"attention_bias": True} if L == 200 else {}))
    torch.manual_seed(100 + L)
    head = LinearHead(256, 256)
    ids, mask = _ragged(np.random.default_rng(L), n, L, max(2, L // 3))
    for side, (i_, m_) in (("right", (ids, mask)), ("left", _left(ids, mask))):
        for pooling, hd, norm in (("last", None, False), ("mean", head, True)):
            want = _hf_reps(lm, i_, m_, pooling, hd.linear if hd is not None else None, norm)
            for dtype in ("float32", "float16", "bfloat16"):
                _check(_hip(lm, i_, m_, pooling, dtype, hd, norm), want, dtype, f"causal small L={L} {side} {pooling}",
                       (lm, i_, m_, pooling, hd.linear if hd is not None else None, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(128, 4), (512, 2)])
def test_encode_matches_hf_qwen2_half_b_width(L, n):
    """Qwen2-0.5B width (896 / 14 heads / 2 K / V heads / 4864), 2 layers, with its q / k / v biases"""
    lm = _lm("qwen2", QWEN05, layers=2, seed=7 + L)
    ids, mask = _ragged(np.random.default_rng(L + 1), n, L, L // 4)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in ("float32", "float16", "bfloat16"):
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, f"qwen2-0.5B width L={L}", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_mha_gqa_mqa(n_kv):
    lm = _lm("llama", dict(SMALL, num_key_value_heads=n_kv), seed=20 + n_kv, sharp=4.0)
    ids, mask = _ragged(np.random.default_rng(n_kv), 5, 200, 60)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in ("float32", "float16", "bfloat16"):
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, f"n_kv={n_kv}", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
def test_causality_bit_for_bit():
    """Replacing every token after position t leaves the hidden states at positions <= t bit-identical; the `last` representation
    follows the last token."""
    lm = _lm("llama", seed=31)
    L = 320
    rng = np.random.default_rng(31)
    ids = rng.integers(3, 600, (3, L)).astype(np.int64)
    mask = np.ones_like(ids)
    for dtype in ("float32", "float16", "bfloat16"):
        h0, r0 = _hip(lm, ids, mask, "last", dtype, hidden=True)
        for t in (1, 63, 64, 127, 300):
            ids2 = ids.copy()
            ids2[:, t + 1:] = rng.integers(3, 600, (3, L - t - 1))
            ids2[:, L - 1] = (ids[:, L - 1] - 3 + 1) % 597 + 3          # the last token certainly changes
            h1, r1 = _hip(lm, ids2, mask, "last", dtype, hidden=True)
            bits = torch.int32 if dtype == "float32" else torch.int16
            assert torch.equal(h0[:, :t + 1].contiguous().view(bits), h1[:, :t + 1].contiguous().view(bits)), (dtype, t)
            assert not torch.equal(h0[:, t + 1:], h1[:, t + 1:])
            assert (r0 - r1).abs().max().item() > 1e-3


def _bidirectional_reps(lm, ids, mask):
    """The same weights with the triangle taken out of the eager mask: attention restated over (key unmasked) alone"""
    import transformers.models.llama.modeling_llama as M
    orig = M.eager_attention_forward

    def full(module, query, key, value, attention_mask, scaling, dropout=0.0, **kw):
        keym = (_bidirectional_reps.mask != 0)[:, None, None, :].expand(-1, 1, query.shape[2], -1)
        add = torch.zeros(keym.shape, dtype=query.dtype).masked_fill(~keym, torch.finfo(query.dtype).min)
        return orig(module, query, key, value, add, scaling, dropout, **kw)
    _bidirectional_reps.mask = torch.from_numpy(mask)
    M.eager_attention_forward = full
    try:
        return _hf_reps(lm, ids, mask, "mean")
    finally:
        M.eager_attention_forward = orig


@pytest.mark.gpu
def test_not_bidirectional():
    lm = _lm("llama", seed=41, sharp=6.0)
    ids, mask = _ragged(np.random.default_rng(41), 3, 200, 100)
    want = _hf_reps(lm, ids, mask, "mean")
    other = _bidirectional_reps(lm, ids, mask)
    assert _rel(other, want) > 0.1, _rel(other, want)
    got = _hip(lm, ids, mask, "mean", "float32")
    assert _rel(got, want) < 1e-4, _rel(got, want)


@pytest.mark.gpu
def test_llama3_rope():
    lm = _lm("llama", seed=51, sharp=6.0, rope_parameters=LLAMA3)
    plain = _lm("llama", seed=51)
    plain.load_state_dict(lm.state_dict())
    ids, mask = _ragged(np.random.default_rng(51), 3, 512, 300)
    want = _hf_reps(lm, ids, mask, "last")
    assert _rel(_hf_reps(plain, ids, mask, "last"), want) > 0.05
    for dtype in ("float32", "float16", "bfloat16"):
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, "llama3 rope L=512", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
def test_last_token_pooling_and_padding_invariance():
    """`last` = HF hidden states at the last non-zero mask index, right- and left-padded; 128 pad columns appended on the right change
    nothing bit for bit in any format, prepended on the left nothing beyond float32 rounding (the rotary phases shift together)."""
    lm = _lm("qwen2", seed=61)
    ids, mask = _ragged(np.random.default_rng(61), 16, 128, 20)
    for i_, m_ in ((ids, mask), _left(ids, mask)):
        h = _hf_hidden(lm, i_, m_)
        want = h[torch.arange(16), _last_index(m_)].double()
        assert _rel(_hip(lm, i_, m_, "last", "float32"), want) < 1e-4
    pad = np.zeros_like(ids)
    right = (np.concatenate([ids, pad], 1), np.concatenate([mask, pad], 1))
    left = (np.concatenate([pad, ids], 1), np.concatenate([pad, mask], 1))
    for dtype in ("float32", "float16", "bfloat16"):
        a = _hip(lm, ids, mask, "last", dtype)
        b = _hip(lm, *right, "last", dtype)
        assert torch.equal(a, b), (dtype, (a - b).abs().max().item())
    a = _hip(lm, ids, mask, "last", "float32")
    assert _rel(_hip(lm, *left, "last", "float32"), a) < 1e-4


@pytest.mark.gpu
def test_cross_encoder_over_qwen2():
    from openmatch.modeling import LinearHead, RRModel
    lm = _lm("qwen2", seed=71)
    torch.manual_seed(72)
    head = LinearHead(256, 1)
    ids, mask = _ragged(np.random.default_rng(7), 8, 160, 40)
    want = _hf_reps(lm, ids, mask, "last", head.linear)
    model = RRModel(lm=lm, head=head, pooling="last", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with torch.no_grad():
        got = model.encode({"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)})
    assert got.shape == (8, 1)
    assert (got.double().cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


@pytest.mark.gpu
def test_retriever_end_to_end(tmp_path):
    """Corpus and queries encoded by the HIP Llama, searched by Retriever: the top-10 ids are those of HF fp32 embeddings searched by
    the oracle's exact inner-product index."""
    import pickle
    from openmatch.retriever import Retriever
    from oracle import flatip
    lm = _lm("llama", seed=81)
    rng = np.random.default_rng(8)
    P_ids, P_mask = _ragged(rng, 96, 128, 30)
    Q_ids, Q_mask = _ragged(rng, 12, 32, 8)
    model = _model(lm, "last", "float32", normalize=True)
    with torch.no_grad():
        P = model.encode_passage({"input_ids": torch.from_numpy(P_ids).to(DEV), "attention_mask": torch.from_numpy(P_mask).to(DEV)})[1]
        Q = model.encode_query({"input_ids": torch.from_numpy(Q_ids).to(DEV), "attention_mask": torch.from_numpy(Q_mask).to(DEV)})[1]
    lm.to("cpu")
    Pw = _hf_reps(lm, P_ids, P_mask, "last", None, True).float().numpy()
    Qw = _hf_reps(lm, Q_ids, Q_mask, "last", None, True).float().numpy()
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
    """Training raises naming the family; 1 025 tokens are refused; the next valid call succeeds."""
    from openmatch.modeling import DRModel
    lm = _lm("llama", seed=91)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="last", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV)
    items = {"input_ids": torch.ones(2, 16, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(2, 16, dtype=torch.int64, device=DEV)}
    model.train()
    with pytest.raises(NotImplementedError, match="Llama / Qwen2 training"):
        model.encode_passage(items)
    model.eval()
    long = {"input_ids": torch.ones(1, 1025, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(1, 1025, dtype=torch.int64, device=DEV)}
    with torch.no_grad(), pytest.raises(Exception, match="1024|1 024|length"):
        model.encode_passage(long)
    with torch.no_grad():
        reps = model.encode_passage(items)[1]
    assert reps.shape == (2, 256) and torch.isfinite(reps).all()
