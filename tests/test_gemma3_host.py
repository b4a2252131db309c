"""EmbeddingGemma on the host (no GPU): a bidirectional HF Gemma3TextModel built at test time is dispatched, translated into an
OmGemma3Config and packed as csrc/encoder_gemma3.hip expects it -- every norm weight as 1 + w, the embedding table scaled by
float32(sqrt(hidden)) -- and everything the stack does not serve is refused by name, on the host and through the C entry."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N

TINY = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=192)
TYPES3 = ["sliding_attention", "sliding_attention", "full_attention"]


def gemma_cfg(shape=TINY, layer_types=TYPES3, window=8, **kw):
    from transformers import Gemma3TextConfig
    kw.setdefault("use_bidirectional_attention", True)
    kw.setdefault("query_pre_attn_scalar", 256)
    return Gemma3TextConfig(num_hidden_layers=len(layer_types), layer_types=list(layer_types), sliding_window=window, vocab_size=600,
                            max_position_embeddings=1024, pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager",
                            **shape, **kw)


def gemma_lm(shape=TINY, layer_types=TYPES3, window=8, seed=0, **kw):
    """Random weights with trained-checkpoint-like norm weights: Gemma initialises them to ZERO (an effective weight of 1), which would
    hide a missing `1 +`.  (Scaling q_proj / k_proj does not sharpen the attention here: q_norm / k_norm undo it.  The spread of the
    scores is set by the norm weights and query_pre_attn_scalar.)"""
    from transformers import Gemma3TextModel
    torch.manual_seed(seed)
    lm = Gemma3TextModel(gemma_cfg(shape, layer_types, window, **kw)).eval()
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.copy_(0.3 * torch.randn_like(p))
        lm.embed_tokens.weight.add_(0.02 * torch.randn_like(lm.embed_tokens.weight))
    return lm


def test_dispatch_and_refusals_by_name():
    from transformers import Gemma3ForCausalLM, GPT2Config, GPT2Model
    from openmatch_amd.encoder import _arch_of, check_pooling
    lm = gemma_lm()
    assert _arch_of(lm) == "gemma3"
    with pytest.raises(NotImplementedError, match="Gemma3ForCausalLM"):
        _arch_of(Gemma3ForCausalLM(gemma_cfg(layer_types=TYPES3[:1])))

    class Gemma3Model(torch.nn.Module):          # (the multimodal wrapper needs a vision tower: its NAME is what is refused)
        pass
    with pytest.raises(NotImplementedError, match="Gemma3Model.*Gemma3TextModel"):
        _arch_of(Gemma3Model())
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*GPT2Model"):
        _arch_of(GPT2Model(GPT2Config(n_embd=64, n_layer=1, n_head=2, vocab_size=100)))
    check_pooling(lm, "first")
    check_pooling(lm, "mean")
    check_pooling(lm, None)
    with pytest.raises(NotImplementedError, match="pooling='last'.*Gemma3TextModel"):
        check_pooling(lm, "last")


@pytest.mark.parametrize("window,half", [(512, 256), (8, 4)])
def test_config_translation(window, half):
    from openmatch_amd.encoder import gemma3_config, gemma3_config_fields
    types = ["sliding_attention", "full_attention", "sliding_attention", "sliding_attention", "full_attention"]
    lm = gemma_lm(layer_types=types, window=window, query_pre_attn_scalar=200)
    assert lm.config.sliding_window == window // 2 + 1          # the config has halved it already
    f = gemma3_config_fields(lm.config, lm)
    assert f["half_window"] == lm.config.sliding_window - 1 == half
    assert f["sliding_layers"] == 0b01101 and [bool(f["sliding_layers"] >> i & 1) for i in range(5)] == [t == "sliding_attention" for t in types]
    rot = lm.rotary_emb
    assert torch.equal(torch.tensor(f["full_inv_freq"], dtype=torch.float32), rot.full_attention_inv_freq.float())
    assert torch.equal(torch.tensor(f["sliding_inv_freq"], dtype=torch.float32), rot.sliding_attention_inv_freq.float())
    assert f["full_inv_freq"] != f["sliding_inv_freq"] and len(f["full_inv_freq"]) == 128
    assert f["full_scaling"] == float(rot.full_attention_attention_scaling) and f["sliding_scaling"] == float(rot.sliding_attention_attention_scaling)
    assert f["attn_scale"] == 200 ** -0.5 != 256 ** -0.5
    assert f["arch"] == N.ARCH_GEMMA3 == 5 and f["act"] == N.ACT_GELU_TANH and f["head_dim"] == 256 and f["n_kv_heads"] == 1
    assert f["hidden"] == 128 and f["ffn"] == 192 and f["n_heads"] == 2 and f["ln_eps"] == lm.config.rms_norm_eps
    gc = gemma3_config(dict(dtype=N.OM_F16, head_in=0, head_out=0, **f), N.POOL_MEAN, True)
    assert gc.half_window == half and gc.sliding_layers == 0b01101 and gc.bidirectional == 1 and gc.attn_logit_softcapping == 0.0
    assert gc.attn_scale == np.float32(200 ** -0.5) and gc.base.n_kv_heads == 1 and gc.base.base.pooling == N.POOL_MEAN
    assert list(gc.full_inv_freq) == [np.float32(v) for v in f["full_inv_freq"]]
    assert list(gc.sliding_inv_freq) == [np.float32(v) for v in f["sliding_inv_freq"]]
    # a linear rope on one layer type: the module's own buffer, whatever the rule
    lin = gemma_lm(layer_types=types, window=window, rope_parameters={
        "full_attention": {"rope_type": "linear", "rope_theta": 1000000.0, "factor": 8.0},
        "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}})
    fl = gemma3_config_fields(lin.config, lin)
    assert np.allclose(np.array(fl["full_inv_freq"]) * 8.0, f["full_inv_freq"], rtol=1e-6) and fl["sliding_inv_freq"] == f["sliding_inv_freq"]
    # deepcopy keeps the window; a round trip through to_dict() and the constructor halves it again
    assert copy.deepcopy(lm).config.sliding_window == lm.config.sliding_window


def test_refusals_on_the_host():
    from openmatch_amd.encoder import gemma3_config_fields

    def fields(**kw):
        shape = kw.pop("shape", TINY)
        lm = gemma_lm(shape, layer_types=TYPES3[1:], **kw)
        return gemma3_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*head_dim 128"):
        fields(shape=dict(TINY, head_dim=128))
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*use_bidirectional_attention"):
        fields(use_bidirectional_attention=False)
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*at most 2048"):
        fields(shape=dict(TINY, hidden_size=2112))
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*multiples of 64"):
        fields(shape=dict(TINY, intermediate_size=200))
    with pytest.raises(NotImplementedError, match=r"Gemma3TextModel.*num_key_value_heads \(2\) must divide"):
        fields(shape=dict(TINY, hidden_size=192, num_attention_heads=3, num_key_value_heads=2))
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*gelu_pytorch_tanh"):
        fields(hidden_activation="silu")
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*attention_bias"):
        fields(attention_bias=True)
    with pytest.raises(NotImplementedError, match="Gemma3TextModel.*attn_logit_softcapping"):
        fields(attn_logit_softcapping=50.0)
    for kind in ("dynamic", "yarn"):
        lm = gemma_lm(layer_types=TYPES3[1:])
        lm.config.rope_parameters["full_attention"] = {"rope_type": kind, "rope_theta": 10000.0, "factor": 2.0}
        with pytest.raises(NotImplementedError, match=f"Gemma3TextModel.*{kind}"):
            gemma3_config_fields(lm.config, lm)


def test_training_is_refused_naming_the_family():
    from openmatch_amd.train import encode_train
    lm = gemma_lm(layer_types=TYPES3[1:])
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="Gemma3 training"):
        encode_train(lm, None, items, "mean", False, N.OM_BF16, True)


def test_packing_adds_one_to_every_norm_and_scales_the_table():
    """On the CPU device: _Packed.dev copies to whatever device it is given"""
    from openmatch_amd.encoder import _pack_gemma3
    lm = gemma_lm()
    pk = _pack_gemma3(lm, N.OM_F32, torch.device("cpu"))
    by_ptr = {t.data_ptr(): t for t in pk.keep}
    cfg = lm.config

    def at(ptr):
        return by_ptr[ptr]
    assert len(pk.norms) == len(pk.layers) == 3
    for i, layer in enumerate(lm.layers):
        pairs = [(pk.layers[i].ln1_g, layer.input_layernorm), (pk.layers[i].ln2_g, layer.pre_feedforward_layernorm),
                 (pk.norms[i].q_norm_g, layer.self_attn.q_norm), (pk.norms[i].k_norm_g, layer.self_attn.k_norm),
                 (pk.norms[i].post_attention_norm_g, layer.post_attention_layernorm),
                 (pk.norms[i].post_feedforward_norm_g, layer.post_feedforward_layernorm)]
        for ptr, mod in pairs:
            w = mod.weight.detach()
            assert w.abs().max() > 0.1                       # perturbed: a zero weight would not tell g = 1 + w from g = 1
            assert torch.equal(at(ptr), 1.0 + w.float())     # HF: 1.0 + self.weight.float()
        sa = layer.self_attn
        assert torch.equal(at(pk.layers[i].qkv_w), torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight], 0).detach())
        assert at(pk.layers[i].qkv_w).shape == (4 * 256, 128) and at(pk.layers[i].o_w).shape == (128, 512)
        assert torch.equal(at(pk.layers[i].ffn1_w), layer.mlp.gate_proj.weight.detach())
        assert torch.equal(at(pk.layers[i].ffn1g_w), layer.mlp.up_proj.weight.detach())
        assert torch.equal(at(pk.layers[i].ffn2_w), layer.mlp.down_proj.weight.detach())
        assert not pk.layers[i].qkv_b and not pk.layers[i].o_b
    assert torch.equal(at(pk.weights.final_ln_g), 1.0 + lm.norm.weight.detach().float())
    table = at(pk.weights.word_emb)
    assert torch.equal(table, lm.embed_tokens.weight.detach() * torch.tensor(cfg.hidden_size ** 0.5, dtype=torch.float32))
    ids = torch.tensor([[5, 17, 599]])
    with torch.no_grad():
        assert torch.equal(table[ids], lm.embed_tokens(ids))          # HF's own scaled lookup, bit for bit
    assert pk.cfg["arch"] == N.ARCH_GEMMA3 and pk.cfg["half_window"] == 4 and pk.cfg["sliding_layers"] == 0b011


def _c_config(**over):
    f = dict(arch=N.ARCH_GEMMA3, dtype=N.OM_BF16, hidden=768, n_layers=3, n_heads=3, head_dim=256, ffn=1152, vocab=600, act=N.ACT_GELU_TANH,
             ln_eps=1e-6, pooling=N.POOL_MEAN)
    own = dict(n_kv_heads=1, attn_scale=0.0625, half_window=256, sliding_layers=0b011, full_scaling=1.0, sliding_scaling=1.0,
               attn_logit_softcapping=0.0, bidirectional=1)
    for k, v in over.items():
        (own if k in own else f)[k] = v
    inner = N.OmCausalConfig(base=N.OmEncoderConfig(**f), n_kv_heads=own.pop("n_kv_heads"), rope_attention_scaling=1.0)
    return N.OmGemma3Config(base=inner, full_inv_freq=(C.c_float * 128)(*([0.5] * 128)), sliding_inv_freq=(C.c_float * 128)(*([0.25] * 128)), **own)


def test_abi_is_unchanged_and_the_gemma3_struct_embeds_the_config():
    lib = N.lib()
    assert lib.om_abi_version() == 6 == N.ABI_VERSION
    assert C.sizeof(N.OmEncoderConfig) == 96 and C.sizeof(N.OmCausalConfig) == 232 and C.sizeof(N.OmCausalConfig2) == 496
    G = N.OmGemma3Config
    assert G.base.offset == 0 and G.attn_scale.offset == 232 and G.half_window.offset == 236 and G.sliding_layers.offset == 240
    assert G.full_scaling.offset == 248 and G.sliding_scaling.offset == 252 and G.attn_logit_softcapping.offset == 256
    assert G.bidirectional.offset == 260 and G.full_inv_freq.offset == 264 and G.sliding_inv_freq.offset == 776 and C.sizeof(G) == 1288
    assert C.sizeof(N.OmGemma3Norms) == 32 and N.OmGemma3Norms.post_feedforward_norm_g.offset == 24
    assert N.ARCH_GEMMA3 == 5
    # workspace: x f32 | y | qkv | ctx | ff | ff2 in the compute format over the row count (whole 256-row tiles from 512 rows on) + the small ones
    B, L = 4, 200
    rows = 1024
    floor = rows * (768 * 4 + (768 + 5 * 256 + 3 * 256 + 2 * 1152) * 2) + B * L * 768 * 4
    got = lib.om_gemma3_encoder_workspace_bytes(C.byref(_c_config()), B, L)
    assert floor <= got <= floor + 16 * 256 + 2 * B * 768 * 4
    f32 = lib.om_gemma3_encoder_workspace_bytes(C.byref(_c_config(dtype=N.OM_F32, pooling=N.POOL_FIRST)), B, L)
    assert f32 >= B * L * (768 * 4 + (768 + 5 * 256 + 3 * 256 + 2 * 1152) * 4)
    assert lib.om_gemma3_encoder_workspace_bytes(C.byref(_c_config(head_dim=128)), B, L) == 0


def test_every_refusal_comes_back_through_the_c_entry():
    lib = N.lib()
    layers = (N.OmLayerWeights * 3)()
    norms = (N.OmGemma3Norms * 3)()
    for i in range(3):
        for name in ("qkv_w", "o_w", "ln1_g", "ln2_g", "ffn1_w", "ffn1g_w", "ffn2_w"):
            setattr(layers[i], name, 256)
        for name, _ in N.OmGemma3Norms._fields_:
            setattr(norms[i], name, 256)
    w = N.OmEncoderWeights(word_emb=256, final_ln_g=256, layers_host=C.cast(layers, C.POINTER(N.OmLayerWeights)))

    def refused(cfg, L=8, norms_=norms):
        rc = lib.om_gemma3_encoder_forward(C.byref(cfg), C.byref(w), norms_, 16, 16, 1, L, None, 16, 256, 1 << 40, None)
        return lib.om_last_error() if rc != 0 else None
    for over, text in ((dict(head_dim=128), b"head_dim 256"), (dict(head_dim=64), b"head_dim 256"),
                       (dict(hidden=2112), b"at most 2048"), (dict(hidden=800), b"multiples of 64"), (dict(ffn=1100), b"multiples of 64"),
                       (dict(n_heads=3, n_kv_heads=2), b"divide"), (dict(act=N.ACT_SILU), b"gelu_pytorch_tanh"),
                       (dict(act=N.ACT_GELU_ERF), b"gelu_pytorch_tanh"), (dict(attn_logit_softcapping=50.0), b"attn_logit_softcapping"),
                       (dict(bidirectional=0), b"use_bidirectional_attention"), (dict(arch=N.ARCH_CAUSAL), b"OM_ARCH_GEMMA3"),
                       (dict(pooling=N.POOL_LAST), b"last"), (dict(attn_scale=0.0), b"attn_scale"), (dict(n_layers=65), b"64 layers"),
                       (dict(half_window=0), b"half_window"), (dict(sliding_layers=0b1000), b"past n_layers")):
        msg = refused(_c_config(**over))
        assert msg is not None and text in msg, (over, msg)
    msg = refused(_c_config(), L=1025)
    assert msg is not None and b"1024" in msg and b"Gemma3" in msg
    layers[1].qkv_b = 256
    msg = refused(_c_config())
    assert msg is not None and b"attention_bias" in msg
    layers[1].qkv_b = None
    norms[2].k_norm_g = None
    msg = refused(_c_config())
    assert msg is not None and b"k_norm_g" in msg
    norms[2].k_norm_g = 256
    msg = refused(_c_config(), norms_=None)
    assert msg is not None and b"norm weights" in msg
    # the other entries keep refusing the new arch code
    bad = N.OmEncoderConfig(arch=N.ARCH_GEMMA3, dtype=N.OM_BF16, hidden=768, n_layers=1, n_heads=12, head_dim=64, ffn=3072, vocab=600,
                            act=N.ACT_GELU_TANH, ln_eps=1e-6, pooling=N.POOL_MEAN)
    assert lib.om_encoder_forward(C.byref(bad), C.byref(w), 16, 16, None, 1, 8, None, 16, 256, 1 << 30, None) != 0
    # the debug hooks check their arguments on the host
    inv = (C.c_float * 128)(*([0.5] * 128))
    assert lib.om_debug_attention_gqa_d256(N.OM_F32, 256, 256, 256, 1, 1025, 3, 1, 0.0625, 0, None) != 0 and b"1024" in lib.om_last_error()
    assert lib.om_debug_attention_gqa_d256(N.OM_F32, 256, 256, 256, 1, 8, 3, 2, 0.0625, 0, None) != 0 and b"divide" in lib.om_last_error()
    assert lib.om_debug_attention_gqa_d256(7, 256, 256, 256, 1, 8, 3, 1, 0.0625, 0, None) != 0 and b"dtype" in lib.om_last_error()
    assert lib.om_debug_qknorm_rope_d256(N.OM_F32, 256, 8, 1025, 3, 1, 256, 256, 1e-6, inv, 1.0, None) != 0
    assert lib.om_debug_qknorm_rope_d256(N.OM_F32, 256, 8, 8, 3, 1, None, 256, 1e-6, inv, 1.0, None) != 0
    assert lib.om_debug_qknorm_rope(N.OM_F32, 256, 8, 8, 3, 1, 256, 256, 256, 1e-6, inv, 1.0, None) != 0 and b"Gemma3" in lib.om_last_error()
    assert lib.om_debug_rmsnorm_add(N.OM_F32, 256, 2052, 256, 2052, 256, 4, 2052, 1e-6, None) != 0 and b"2048" in lib.om_last_error()
