"""NomicBERT (HF NomicBertModel: nomic-embed-text-v1 / v1.5) on the host: dispatch, config translation, refusals, the plan of its
forward (csrc/encoder_plan.h through om_debug_encoder_plan: the four BERT loops under OM_ARCH_NOMICBERT), workspace sizes and the
packed weights.  No GPU."""
import ctypes as C

import pytest
import torch

from openmatch_amd import native as N
from tests.test_modernbert import _perturb

F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
FUSED, PENDING, FEW32, PLAIN = (N.ENC_PATH[k] for k in ("bert_fused", "bert_pending_ln", "bert_few32", "bert_plain"))
FEW, TWO = 1 << 8, 1 << 9
SMALL = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512)
ODD = dict(hidden_size=192, num_attention_heads=3, intermediate_size=320)


def _cfg(shape=SMALL, layers=3, **kw):
    from transformers import NomicBertConfig
    return NomicBertConfig(num_hidden_layers=layers, vocab_size=600, max_position_embeddings=1024, pad_token_id=0,
                           attn_implementation="eager", **shape, **kw)


def _nomic(shape=SMALL, layers=3, seed=0, **kw):
    from transformers import NomicBertModel
    torch.manual_seed(seed)
    return _perturb(NomicBertModel(_cfg(shape, layers, **kw)).eval())


def _c(dtype, hidden=256, n_heads=4, ffn=512, **kw):
    return N.OmEncoderConfig(**dict(dict(arch=N.ARCH_NOMICBERT, dtype=dtype, hidden=hidden, n_layers=3, n_heads=n_heads, head_dim=64, ffn=ffn,
                                         vocab=600, max_pos=1024, type_vocab=2, act=N.ACT_SILU, ln_eps=1e-12, pooling=N.POOL_FIRST,
                                         rope_theta_global=1000.0), **kw))


def _plan(cfg, B, L, packed=0, hidden=0):
    return N.lib().om_debug_encoder_plan(C.byref(cfg), 0, 0, B, L, packed, hidden)


# ------------------------------------------------------------------------------------------------------------- dispatch
def test_arch_of_nomicbert():
    from transformers import NomicBertForMaskedLM
    from openmatch_amd.encoder import _PACKERS, _arch_of
    assert _arch_of(_nomic(layers=1)) == "nomicbert" and "nomicbert" in _PACKERS
    with pytest.raises(NotImplementedError, match="NomicBERT.*got NomicBertForMaskedLM"):
        _arch_of(NomicBertForMaskedLM(_cfg(layers=1)))


def test_config_translation():
    from openmatch_amd.encoder import nomicbert_config_fields
    lm = _nomic(layers=2)
    f = nomicbert_config_fields(lm.config, lm)
    assert f == dict(arch=N.ARCH_NOMICBERT, hidden=256, n_layers=2, n_heads=4, head_dim=64, ffn=512, vocab=600, max_pos=1024, type_vocab=2,
                     act=N.ACT_SILU, ln_eps=lm.config.layer_norm_eps, rel_buckets=0, rel_max_dist=0, rope_theta_global=1000.0)
    assert N.ARCH_NOMICBERT == 4
    # the frequencies the device derives from the theta are the module's own: 1 / theta ** (2 i / 64) in f32
    want = 1.0 / (torch.tensor(1000.0) ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64))
    assert torch.equal(lm.rotary_emb.inv_freq.float(), want)
    other = _nomic(layers=1, rope_parameters={"rope_type": "default", "rope_theta": 12345.0})
    assert nomicbert_config_fields(other.config, other)["rope_theta_global"] == 12345.0
    # every field is one of the struct's, and the struct keeps its size: OM_ABI_VERSION does not change
    cfg = N.OmEncoderConfig(dtype=F16, pooling=N.POOL_MEAN, normalize=1, head_in=0, head_out=0, **f)
    assert cfg.rope_theta_global == 1000.0 and cfg.rope_theta_local == 0.0 and cfg.half_window == 0 and cfg.sliding_layers == 0
    assert C.sizeof(N.OmEncoderConfig) == 96 and N.lib().om_abi_version() == 6 == N.ABI_VERSION


def test_refusals_on_the_host():
    from openmatch_amd.encoder import check_pooling, nomicbert_config_fields

    def fields(shape=SMALL, **kw):
        lm = _nomic(shape, layers=1, **kw)
        return nomicbert_config_fields(lm.config, lm)
    lm = _nomic(layers=1)
    lm.config.rope_parameters = {"rope_type": "linear", "rope_theta": 1000.0, "factor": 2.0}
    with pytest.raises(NotImplementedError, match="NomicBertModel.*rope type 'linear'"):
        nomicbert_config_fields(lm.config, lm)
    lm = _nomic(layers=1)
    lm.rotary_emb.attention_scaling = 1.25                       # what a scaled rope type would leave there
    with pytest.raises(NotImplementedError, match="NomicBertModel.*attention_scaling must be 1"):
        nomicbert_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="NomicBertModel.*head_dim 64"):
        fields(dict(hidden_size=256, num_attention_heads=8, intermediate_size=512))
    with pytest.raises(NotImplementedError, match="NomicBertModel.*head_dim 64"):
        fields(dict(hidden_size=256, num_attention_heads=2, intermediate_size=512, head_dim=64))      # head_dim * heads != hidden
    with pytest.raises(NotImplementedError, match="NomicBertModel.*hidden_act must be 'silu'.*'gelu'"):
        fields(hidden_act="gelu")
    with pytest.raises(NotImplementedError, match="NomicBertModel.*multiples of 64"):
        fields(dict(hidden_size=256, num_attention_heads=4, intermediate_size=544))
    with pytest.raises(NotImplementedError, match="NomicBertModel.*at most 2048"):
        fields(dict(hidden_size=2112, num_attention_heads=33, intermediate_size=128))
    with pytest.raises(NotImplementedError, match="pooling='last'.*NomicBertModel"):
        check_pooling(_nomic(layers=1), "last")


def test_training_is_refused_naming_the_family():
    from openmatch_amd.train import encode_train
    lm = _nomic(layers=1)
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="NomicBERT training"):
        encode_train(lm, None, items, "mean", False, N.OM_BF16, True)


def test_host_rules_for_batches():
    """token_type_ids pass through as for BERT; a left-padded batch is legal (no position table: HF's arange); float16 stays float16"""
    from openmatch_amd.encoder import check_position_layout, inference_code, token_types_of
    lm = _nomic(layers=1)
    tti = torch.ones(2, 8, dtype=torch.int64)
    assert token_types_of(lm, {"token_type_ids": tti}) is tti
    ids = torch.tensor([[0, 0, 0, 5, 6, 7]])
    check_position_layout(lm, ids, (ids != 0).long())
    assert inference_code(lm, F16, 128) == F16 and inference_code(lm, BF16, 128) == BF16


# ------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name,cfg,B,L,kw,want", [
    ("query_f16", _c(F16), 1, 16, {}, PENDING | FEW),                    # 16 rows <= 64: LayerNorms pending in the few-rows contractions
    ("query_bf16", _c(BF16), 1, 16, {}, PENDING | FEW),
    ("few_f16", _c(F16), 5, 24, {}, FEW32 | FEW),                        # 64 < 120 rows <= 1 024
    ("few_bf16", _c(BF16), 5, 24, {}, FEW32 | FEW),
    ("fused_f16", _c(F16), 16, 128, {}, FUSED | TWO),                    # 2 048 rows; 3H, 2F, H multiples of 256; SiLU is rule 7a's exception
    ("fused_bf16", _c(BF16), 16, 128, {}, FUSED | TWO),
    ("fused_long", _c(F16), 8, 320, {}, FUSED | TWO),
    ("fused_1024", _c(BF16), 2, 1024, {}, FUSED | TWO),
    ("f32_query", _c(F32), 1, 16, {}, PLAIN),
    ("f32_few", _c(F32), 5, 24, {}, PLAIN),
    ("f32_batch", _c(F32), 16, 128, {}, PLAIN),
    ("f32_long", _c(F32), 2, 1024, {}, PLAIN),
    ("odd_f16", _c(F16, 192, 3, 320), 16, 128, {}, PLAIN),               # hidden 192, 2F = 640: no multiples of 256
    ("odd_bf16", _c(BF16, 192, 3, 320), 16, 128, {}, PLAIN),
    ("packed_f16", _c(F16), 16, 128, dict(packed=1024), FUSED | TWO),
    ("packed_bf16", _c(BF16), 16, 128, dict(packed=1024), FUSED | TWO),
    ("nomic_embed_width", _c(F16, 768, 12, 3072), 16, 128, {}, FUSED | TWO),
], ids=lambda v: v if isinstance(v, str) else "")
def test_plan(name, cfg, B, L, kw, want):
    assert _plan(cfg, B, L, **kw) == want, N.lib().om_last_error()


def test_plan_refusals():
    lib = N.lib()
    assert _plan(_c(F16, 192, 3, 320), 16, 128, packed=1024) == -1 and b"packed rows need the fused 16-bit path" in lib.om_last_error()
    assert _plan(_c(F32), 16, 128, packed=1024) == -1 and b"packed rows: 16-bit inference" in lib.om_last_error()
    assert _plan(_c(F16), 16, 128, packed=1024, hidden=1) == -1 and b"representations only" in lib.om_last_error()
    assert _plan(_c(F16, 256, 8, 512, head_dim=32), 16, 128) == -1 and b"NomicBERT" in lib.om_last_error() and b"head_dim 64" in lib.om_last_error()
    assert _plan(_c(F16, act=N.ACT_GELU_ERF), 16, 128) == -1 and b"NomicBERT" in lib.om_last_error() and b"silu" in lib.om_last_error()
    assert _plan(_c(F16, rope_theta_global=0.0), 16, 128) == -1 and b"theta" in lib.om_last_error()
    assert _plan(_c(F16, rel_buckets=32, rel_max_dist=128), 16, 128) == -1 and b"rel_buckets" in lib.om_last_error()
    assert _plan(_c(F16), 1, 1025) == -1 and b"[1,1024]" in lib.om_last_error()
    assert _plan(_c(F16, max_pos=64), 2, 65) == -1 and b"max_pos" in lib.om_last_error()


def test_bert_keeps_its_rule_7a():
    """the exception is the new architecture's alone: a BERT configuration whose activation is not erf-GELU still runs unfused"""
    bert = dict(arch=N.ARCH_BERT, hidden=256, n_layers=3, n_heads=4, head_dim=64, ffn=1024, vocab=600, max_pos=512, type_vocab=2, ln_eps=1e-12,
                pooling=N.POOL_FIRST)
    assert _plan(N.OmEncoderConfig(dtype=F16, act=N.ACT_GELU_ERF, **bert), 16, 128) == FUSED | TWO
    assert _plan(N.OmEncoderConfig(dtype=BF16, act=N.ACT_RELU, **bert), 16, 128) == PLAIN


def test_workspace_bytes_and_packed_supported():
    lib = N.lib()
    for dt, es in ((F32, 4), (F16, 2), (BF16, 2)):
        c = _c(dt)
        # at least x, y, x1, ctx [M, H], qkv [M, 3H], ff [M, 2F] and the SwiGLU output [M, F]
        assert lib.om_encoder_workspace_bytes(C.byref(c), 16, 128) >= 2048 * (4 * 256 + 3 * 256 + 2 * 512 + 512) * es
    c = _c(F16)
    assert lib.om_encoder_workspace_bytes_packed(C.byref(c), 16, 128, 1024) >= 1024 * (7 * 256 + 3 * 512) * 2
    assert lib.om_encoder_workspace_bytes_packed(C.byref(c), 16, 128, 1024) < lib.om_encoder_workspace_bytes(C.byref(c), 16, 128)
    # the [gate; up] contraction is what sizes ff: twice BERT's at the same widths
    b = _c(F16, arch=N.ARCH_BERT, act=N.ACT_GELU_ERF, rope_theta_global=0.0)
    assert lib.om_encoder_workspace_bytes(C.byref(c), 16, 128) - lib.om_encoder_workspace_bytes(C.byref(b), 16, 128) >= 2048 * 2 * 512 * 2
    assert lib.om_encoder_packed_supported(C.byref(c), 0, 16, 128, 1024) == 1
    assert lib.om_encoder_packed_supported(C.byref(_c(BF16)), 0, 16, 128, 1024) == 1
    assert lib.om_encoder_packed_supported(C.byref(_c(F32)), 0, 16, 128, 1024) == 0
    assert lib.om_encoder_packed_supported(C.byref(_c(F16, 192, 3, 320)), 0, 16, 128, 1024) == 0
    assert lib.om_encoder_packed_supported(C.byref(c), 0, 8, 128, 512) == 0              # 1 024 padded rows: the few-rows kernels
    # the fold buffer holds the 2F-row feed-forward slot
    assert lib.om_encoder_fold_bytes(C.byref(c)) >= 3 * (3 * 256 * 256 + 2 * 512 * 256) * 2
    assert lib.om_encoder_fold_bytes(C.byref(_c(F32))) == 0


def test_host_packed_rows_rule(monkeypatch):
    from openmatch_amd.encoder import packed_rows_apply
    c = _c(F16, pooling=N.POOL_MEAN)
    assert packed_rows_apply(c, 16, 128, 1024, False, "mean") is True
    assert packed_rows_apply(c, 16, 128, 1024, True, "mean") is False                   # hidden states wanted
    assert packed_rows_apply(c, 16, 128, 2048, False, "mean") is False                  # no tile saved
    assert packed_rows_apply(_c(F32), 16, 128, 1024, False, "mean") is False
    monkeypatch.setenv("OM_ENCODER_PACKED", "0")
    assert packed_rows_apply(c, 16, 128, 1024, False, "mean") is False


# ------------------------------------------------------------------------------------------------------------- packing
def test_packed_weight_shapes():
    """_pack_nomicbert on the CPU (a device is only a place to copy to): ffn1_w is [2F, H] = [gate_proj; up_proj], qkv_w [3H, H] =
    [q; k; v], no bias pointer is set, ln1 / ln2 are post_attention_layernorm / post_mlp_layernorm"""
    from openmatch_amd.encoder import _pack_nomicbert
    lm = _nomic(layers=2)
    pk = _pack_nomicbert(lm, F32, "cpu")
    by_ptr = {t.data_ptr(): t for t in pk.keep}
    assert pk.cfg["arch"] == N.ARCH_NOMICBERT and pk.cfg["dtype"] == F32 and pk.cfg["rope_theta_global"] == 1000.0
    assert pk.weights.pos_emb is None and pk.weights.rel_bias is None and pk.weights.final_ln_g is None
    assert torch.equal(by_ptr[pk.weights.word_emb], lm.embeddings.word_embeddings.weight)
    assert torch.equal(by_ptr[pk.weights.type_emb], lm.embeddings.token_type_embeddings.weight)
    assert torch.equal(by_ptr[pk.weights.emb_ln_g], lm.embeddings.LayerNorm.weight)
    assert torch.equal(by_ptr[pk.weights.emb_ln_b], lm.embeddings.LayerNorm.bias)
    for i, layer in enumerate(lm.layers):
        lw = pk.layers[i]
        assert lw.qkv_b is None and lw.o_b is None and lw.ffn1_b is None and lw.ffn2_b is None and lw.ffn1g_w is None
        ffn1 = by_ptr[lw.ffn1_w]
        assert ffn1.shape == (2 * 512, 256)
        assert torch.equal(ffn1[:512], layer.mlp.gate_proj.weight) and torch.equal(ffn1[512:], layer.mlp.up_proj.weight)
        qkv = by_ptr[lw.qkv_w]
        assert qkv.shape == (3 * 256, 256)
        sa = layer.self_attn
        assert torch.equal(qkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight], 0))
        assert torch.equal(by_ptr[lw.ffn2_w], layer.mlp.down_proj.weight) and by_ptr[lw.ffn2_w].shape == (256, 512)
        assert torch.equal(by_ptr[lw.o_w], sa.o_proj.weight)
        assert torch.equal(by_ptr[lw.ln1_g], layer.post_attention_layernorm.weight)
        assert torch.equal(by_ptr[lw.ln1_b], layer.post_attention_layernorm.bias)
        assert torch.equal(by_ptr[lw.ln2_g], layer.post_mlp_layernorm.weight)
        assert torch.equal(by_ptr[lw.ln2_b], layer.post_mlp_layernorm.bias)
    pk16 = _pack_nomicbert(lm, BF16, "cpu")
    assert {t.data_ptr(): t for t in pk16.keep}[pk16.layers[0].ffn1_w].dtype == torch.bfloat16


def test_symbols_resolve():
    lib = N.lib()
    for name in ("om_debug_swiglu_rows", "om_debug_rope_rows", "om_debug_embed"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None
    # argument checks happen on the host, before any launch
    assert lib.om_debug_swiglu_rows(F16, None, 256, 4, 64, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(F16, 256, None, 4, 64, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(F16, 256, 512, 4, 96, None) != 0 and b"multiple of 64" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(7, 256, 512, 4, 64, None) != 0 and b"dtype" in lib.om_last_error()
    assert lib.om_debug_rope_rows(F16, 256, 4, 16, 128, 1000.0, None, None) != 0 and b"null" in lib.om_last_error()
