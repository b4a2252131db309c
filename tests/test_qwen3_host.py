"""Qwen3 embedders (HF Qwen3Model) on the host: dispatch, the config translation (head_dim 128, an attention width that is not the
hidden size, 64 rotary frequencies, the q / k norm flag), the refusals by name, and the om_causal2_* entries' argument checks, all
before anything touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.test_causal_lm import LLAMA3
from tests.test_modernbert import _perturb

TINY = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384)
EMB06 = dict(hidden_size=1024, num_attention_heads=16, num_key_value_heads=8, head_dim=128, intermediate_size=3072)


def _cfg3(shape=TINY, layers=3, **kw):
    from transformers import Qwen3Config
    return Qwen3Config(num_hidden_layers=layers, vocab_size=600, max_position_embeddings=1024, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                       attn_implementation="eager", **{**shape, **kw})


def _lm3(shape=TINY, layers=3, seed=0, sharp=1.0, **kw):
    """tests/test_causal_lm.py::_lm for Qwen3Model: _perturb moves every norm weight, q_norm / k_norm included, away from 1"""
    from transformers import Qwen3Model
    torch.manual_seed(seed)
    lm = _perturb(Qwen3Model(_cfg3(shape, layers, **kw)).eval())
    with torch.no_grad():
        lm.embed_tokens.weight.add_(0.02 * torch.randn_like(lm.embed_tokens.weight))
        if sharp != 1.0:
            for layer in lm.layers:
                layer.self_attn.q_proj.weight.mul_(sharp)
                layer.self_attn.k_proj.weight.mul_(sharp)
    return lm


def test_arch_dispatch():
    from transformers import Qwen3ForCausalLM
    from openmatch_amd.encoder import _arch_of
    assert _arch_of(_lm3(layers=1)) == "causal"
    with pytest.raises(NotImplementedError, match="Qwen3ForCausalLM"):
        _arch_of(Qwen3ForCausalLM(_cfg3(layers=1)))


@pytest.mark.parametrize("rope", [None, {"rope_type": "linear", "rope_theta": 10000.0, "factor": 4.0}, LLAMA3])
def test_config_translation(rope):
    from openmatch_amd.encoder import causal2_config, qwen3_config_fields
    lm = _lm3(layers=2, **({"rope_parameters": rope} if rope else {}))
    f = qwen3_config_fields(lm.config, lm)
    assert f["head_dim"] == 128 and f["n_heads"] == 4 and f["n_kv_heads"] == 2 and f["hidden"] == 256 and f["ffn"] == 384
    assert f["n_heads"] * f["head_dim"] == 512 != f["hidden"]
    assert f["arch"] == N.ARCH_CAUSAL and f["act"] == N.ACT_SILU and f["ln_eps"] == lm.config.rms_norm_eps and f["qk_norm"] == 1
    assert len(f["inv_freq"]) == 64
    assert torch.equal(torch.tensor(f["inv_freq"], dtype=torch.float32), lm.rotary_emb.inv_freq.float())
    assert f["rope_attention_scaling"] == float(lm.rotary_emb.attention_scaling) == 1.0
    if rope is not None:
        default = qwen3_config_fields((d := _lm3(layers=2)).config, d)
        assert f["inv_freq"] != default["inv_freq"]
    cc = causal2_config(dict(dtype=N.OM_F16, head_in=0, head_out=0, **f), N.POOL_LAST, True)
    assert cc.qk_norm == 1 and cc.base.n_kv_heads == 2 and cc.base.base.head_dim == 128 and cc.base.base.pooling == 3
    assert cc.base.base.normalize == 1 and cc.base.base.dtype == N.OM_F16 and cc.base.base.ln_eps == np.float32(lm.config.rms_norm_eps)
    assert list(cc.inv_freq) == [np.float32(v) for v in f["inv_freq"]]
    # the same model with heads of 64 columns: 32 frequencies, carried by the embedded struct
    lm64 = _lm3(dict(TINY, head_dim=64), layers=2, **({"rope_parameters": rope} if rope else {}))
    f64 = qwen3_config_fields(lm64.config, lm64)
    assert f64["head_dim"] == 64 and len(f64["inv_freq"]) == 32 and f64["qk_norm"] == 1
    assert torch.equal(torch.tensor(f64["inv_freq"], dtype=torch.float32), lm64.rotary_emb.inv_freq.float())
    c64 = causal2_config(dict(dtype=N.OM_F32, head_in=0, head_out=0, **f64), N.POOL_MEAN, False)
    assert list(c64.base.inv_freq) == [np.float32(v) for v in f64["inv_freq"]] and c64.base.base.head_dim == 64


def test_refusals_on_the_host():
    from openmatch_amd.encoder import qwen3_config_fields

    def fields(shape=TINY, **kw):
        lm = _lm3(shape, layers=1, **kw)
        return qwen3_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="Qwen3Model.*head_dim 96"):
        fields(dict(TINY, head_dim=96))
    with pytest.raises(NotImplementedError, match="Qwen3Model.*use_sliding_window"):
        fields(use_sliding_window=True, sliding_window=64, max_window_layers=0)
    with pytest.raises(NotImplementedError, match="Qwen3Model.*2048"):
        fields(dict(hidden_size=2560, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=128))
    lm = _lm3(layers=1)
    lm.config.rope_parameters = {"rope_type": "yarn", "rope_theta": 10000.0, "factor": 2.0}
    with pytest.raises(NotImplementedError, match="Qwen3Model.*yarn"):
        qwen3_config_fields(lm.config, lm)
    with pytest.raises(NotImplementedError, match="Qwen3Model.*silu"):
        fields(hidden_act="gelu")
    lm = _lm3(layers=2)
    lm.config.layer_types = ["full_attention", "sliding_attention"]
    with pytest.raises(NotImplementedError, match="Qwen3Model.*full_attention"):
        qwen3_config_fields(lm.config, lm)


def test_training_is_refused_naming_the_family():
    from openmatch_amd.train import encode_train
    items = {"input_ids": torch.ones(2, 8, dtype=torch.int64), "attention_mask": torch.ones(2, 8, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="Qwen3 training"):
        encode_train(_lm3(layers=1), None, items, "last", False, N.OM_BF16, True)


def test_pooling_last_is_served():
    from openmatch_amd.encoder import check_pooling
    check_pooling(_lm3(layers=1), "last")


def _cfg2(dtype=N.OM_BF16, head_dim=128, hidden=256, n_kv=2, pooling=N.POOL_LAST):
    f = dict(arch=N.ARCH_CAUSAL, dtype=dtype, hidden=hidden, n_layers=1, n_heads=4, head_dim=head_dim, ffn=384, vocab=600, act=N.ACT_SILU,
             ln_eps=1e-6, pooling=pooling)
    inner = N.OmCausalConfig(base=N.OmEncoderConfig(**f), n_kv_heads=n_kv, rope_attention_scaling=1.0, inv_freq=(C.c_float * 32)(*([0.5] * 32)))
    return N.OmCausalConfig2(base=inner, qk_norm=1, reserved=0, inv_freq=(C.c_float * 64)(*([0.5] * 64)))


def test_abi_is_unchanged_and_the_new_struct_embeds_the_causal_config():
    lib = N.lib()
    assert lib.om_abi_version() == 6 == N.ABI_VERSION
    assert C.sizeof(N.OmEncoderConfig) == 96 and C.sizeof(N.OmCausalConfig) == 232 and N.OmCausalConfig.inv_freq.offset == 104
    assert N.OmCausalConfig2.base.offset == 0 and N.OmCausalConfig2.qk_norm.offset == 232 and N.OmCausalConfig2.inv_freq.offset == 240
    assert C.sizeof(N.OmCausalConfig2) == 240 + 64 * 4
    assert C.sizeof(N.OmCausalQkNorm) == 16
    cc = _cfg2()
    # x f32 + y + qkv (1024 columns) + ctx (512 columns) + two ffn buffers, 512 rows of 16-bit elements
    assert lib.om_causal2_encoder_workspace_bytes(C.byref(cc), 4, 128) >= 512 * (256 * 4 + (256 + 1024 + 512 + 2 * 384) * 2)
    w = N.OmEncoderWeights()
    qkn = (N.OmCausalQkNorm * 1)()

    def refused(cfg, L=8):
        return lib.om_causal2_encoder_forward(C.byref(cfg), C.byref(w), qkn, 16, 16, 1, L, None, 16, 256, 1 << 30, None)
    assert refused(cc, 1025) != 0 and b"1024" in lib.om_last_error()
    assert refused(_cfg2(n_kv=3)) != 0 and b"divide" in lib.om_last_error()
    assert refused(_cfg2(head_dim=96)) != 0 and b"head_dim must be 64 or 128" in lib.om_last_error()
    assert refused(_cfg2(hidden=2560)) != 0 and b"2048" in lib.om_last_error()
    assert lib.om_causal2_encoder_workspace_bytes(C.byref(_cfg2(hidden=2560)), 4, 128) == 0
    bad = _cfg2()
    bad.base.base.arch = N.ARCH_BERT
    assert refused(bad) != 0 and b"OM_ARCH_CAUSAL" in lib.om_last_error()

    def refused_packed(cfg, rows, B=16, L=128):
        return lib.om_causal2_encoder_forward_packed(C.byref(cfg), C.byref(w), qkn, 16, 16, B, L, rows, 16, 256, 1 << 30, None)
    assert refused_packed(cc, 1000) != 0 and b"multiple of 256" in lib.om_last_error()
    assert refused_packed(cc, 256) != 0 and b"512" in lib.om_last_error()
    assert lib.om_causal2_encoder_packed_supported(C.byref(cc), 16, 128, 1000) == 0
    assert lib.om_causal2_encoder_packed_supported(C.byref(cc), 16, 128, 1024) == 1
    assert lib.om_causal2_encoder_packed_supported(C.byref(_cfg2(head_dim=64)), 16, 128, 1024) == 1
    assert lib.om_causal2_encoder_packed_supported(C.byref(_cfg2(hidden=2560)), 16, 128, 1024) == 0
    assert lib.om_causal2_encoder_packed_supported(C.byref(cc), 1, 1025, 1024) == 0
    # the older entry still answers head_dim 128 as it did
    old = N.OmCausalConfig(base=cc.base.base, n_kv_heads=2, rope_attention_scaling=1.0, inv_freq=(C.c_float * 32)(*([0.5] * 32)))
    assert lib.om_causal_encoder_forward(C.byref(old), C.byref(w), 16, 16, 1, 8, None, 16, 256, 1 << 30, None) != 0
    assert b"head_dim 64" in lib.om_last_error()


# (dtype, pooling, B, L, packed_rows or 0, bytes) for _cfg2's shape: what the library built from the commit BEFORE csrc/prenorm_stack.h
# answered -- under 512 rows, 600 and 800 rows (16-bit: whole 256-row tiles), and packed
WORKSPACE_BYTES = ((N.OM_BF16, N.POOL_LAST, 3, 40, 0, 741120), (N.OM_F16, N.POOL_FIRST, 5, 120, 0, 4724480), (N.OM_F32, N.POOL_MEAN, 5, 120, 0, 7378688),
                   (N.OM_BF16, N.POOL_MEAN, 4, 200, 0, 7115520), (N.OM_F16, N.POOL_LAST, 16, 128, 1024, 6313216),
                   (N.OM_BF16, N.POOL_MEAN, 4, 1024, 1280, 9185536), (N.OM_F32, N.POOL_FIRST, 16, 128, 1536, 17325312))


def test_workspace_bytes_are_what_they_were():
    lib = N.lib()
    for dtype, pooling, B, L, rows, want in WORKSPACE_BYTES:
        cc = _cfg2(dtype=dtype, pooling=pooling)
        got = lib.om_causal2_encoder_workspace_bytes_packed(C.byref(cc), B, L, rows) if rows else lib.om_causal2_encoder_workspace_bytes(C.byref(cc), B, L)
        assert got == want, (dtype, pooling, B, L, rows)


def test_a_null_qk_norm_weight_is_refused_before_the_first_launch():
    """k_norm_g of layer 2 of 3 is null: the refusal comes back on a machine without a GPU, so nothing was launched for layers 0 and 1
    (fake non-null pointers, no stream: the call shape of tests/test_gemma3_host.py::test_every_refusal_comes_back_through_the_c_entry)"""
    lib = N.lib()
    layers = (N.OmLayerWeights * 3)()
    qkn = (N.OmCausalQkNorm * 3)()
    for i in range(3):
        for name in ("qkv_w", "o_w", "ln1_g", "ln2_g", "ffn1_w", "ffn1g_w", "ffn2_w"):
            setattr(layers[i], name, 256)
        qkn[i].q_norm_g = qkn[i].k_norm_g = 256
    qkn[2].k_norm_g = None
    w = N.OmEncoderWeights(word_emb=256, final_ln_g=256, layers_host=C.cast(layers, C.POINTER(N.OmLayerWeights)))
    cc = _cfg2()
    cc.base.base.n_layers = 3
    assert lib.om_causal2_encoder_forward(C.byref(cc), C.byref(w), qkn, 16, 16, 1, 8, None, 16, 256, 1 << 40, None) != 0
    assert b"Qwen3 layers with qk_norm need q_norm_g and k_norm_g" in lib.om_last_error()
    layers[0].ffn2_w = None                # the pointers of every layer, likewise
    assert lib.om_causal2_encoder_forward(C.byref(cc), C.byref(w), qkn, 16, 16, 1, 8, None, 16, 256, 1 << 40, None) != 0
    assert b"Qwen3 layers need qkv_w, o_w" in lib.om_last_error()
