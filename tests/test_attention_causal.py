"""The kernels of the decoder-only stack alone (csrc/attention_causal.hip): causal grouped-query attention against a float64
restatement on the stored inputs, under the per-element bound tests/test_attention_kernels.py derives for the key-chunked family
(its error_bound, unchanged: the causal kernels are that family's bodies), and the grouped rotary pass against HF's own
apply_rotary_pos_emb."""
import ctypes as C
import math

import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import (BITS_DT, DEV, F16, F32, BF16, NAME, TORCH_DT, attention_reference, bits, error_bound, new_ctx,
                                          rows_of, untouched, violations)

D = 64
SCALE = 0.125
LENGTHS = [1, 31, 128, 129, 200, 320, 512, 1000, 1024]
GROUPS = [(4, 4), (4, 2), (4, 1), (9, 3)]


def grouped_inputs(dtype, B, L, heads, kv, seed):
    """[B * L, (heads + 2 kv) * 64]: q and k so that the scaled scores spread by about 2, V of O(1), distinct per key AND per K / V head"""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(2.0 / (SCALE * math.sqrt(D)))
    x = torch.randn(B, L, heads + 2 * kv, D, generator=g)
    x[:, :, :heads + kv] *= a
    x[:, :, heads + kv:] += (torch.arange(L).float() % 7 - 3.0)[None, :, None, None] * 0.5
    x[:, :, heads + kv:] += torch.arange(kv).float()[None, None, :, None]
    return x.reshape(B * L, (heads + 2 * kv) * D).to(TORCH_DT[dtype]).to(DEV)


def as_mha(qkv, B, L, heads, kv, head_map):
    """The grouped projection as the [B * L, 3 H] layout of attention_reference, query head h reading K / V head head_map(h)"""
    x = qkv.view(B, L, heads + 2 * kv, D)
    idx = torch.tensor([head_map(h) for h in range(heads)], device=qkv.device)
    q, k, v = x[:, :, :heads], x[:, :, heads:heads + kv][:, :, idx], x[:, :, heads + kv:][:, :, idx]
    return torch.stack([q, k, v], 2).reshape(B * L, 3 * heads * D)


def causal_visibility(mask):
    """visible[b, q, k]: k <= q and unmasked; contract[b, q]: the query is unmasked itself and sees a key.  A query outside the
    contract is given every key so that the reference stays finite; its row is only asserted finite."""
    B, L = mask.shape
    m = mask != 0
    i = torch.arange(L, device=mask.device)
    vis = m[:, None, :] & (i[None, :] <= i[:, None])[None]
    contract = vis.any(-1) & m
    vis = vis | ~vis.any(-1)[:, :, None]
    return vis, contract


def padding_masks(B, L):
    """row 0 full, then right-padded rows, then left-padded ones; the last row has exactly its first min(5, L - 1) tokens masked"""
    mask = torch.ones(B, L, dtype=torch.int64)
    g = torch.Generator().manual_seed(L)
    for b in range(1, B):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        if b % 2:
            mask[b, n:] = 0
        else:
            mask[b, :L - n] = 0
    mask[B - 1] = 1
    mask[B - 1, :min(5, L - 1)] = 0
    return mask


def launch(dtype, qkv, ctx, mask, B, L, heads, kv):
    rc = N.lib().om_debug_attention_causal(dtype, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, SCALE, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run_case(dtype, B, L, heads, kv, mask, head_map=None, seed=0):
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=77 + 13 * L + heads + kv + seed)
    mask = mask.to(DEV)
    qkv0 = qkv.clone()
    ctx = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, ctx, mask, B, L, heads, kv) == 0, N.lib().om_last_error()
    assert torch.equal(bits(qkv, dtype), bits(qkv0, dtype))
    assert untouched(ctx[B * L:], dtype), "rows after ctx were written"
    group = heads // kv
    vis, contract = causal_visibility(mask)
    ref, mag, smax, vabs = attention_reference(as_mha(qkv, B, L, heads, kv, head_map or (lambda h: h // group)), mask, None, B, L, heads, D,
                                               SCALE, vis=vis)
    bound = error_bound(ref, mag, smax, vabs, L, D, dtype)
    got = ctx[:B * L].view(B, L, heads * D)
    return got, ref, bound, contract


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", GROUPS)
@pytest.mark.parametrize("L", LENGTHS)
def test_causal_attention_against_float64(L, heads, kv, dtype):
    B = 5 if L <= 512 else 4
    got, ref, bound, contract = run_case(dtype, B, L, heads, kv, padding_masks(B, L))
    ratio = ((got.double() - ref).abs() / bound)[rows_of(contract, heads * D)]
    print(f"causal {NAME[dtype]} L={L} heads={heads} kv={kv}: max err/bound {ratio.max().item():.3f}, compared rows "
          f"{contract.float().mean().item():.2f}")
    bad = violations(got, ref, bound, contract)
    assert not bad.any(), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), ratio.max().item())
    assert torch.isfinite(got.double()).all()              # masked-query rows included (the first rows under left padding)
    assert contract.float().mean() > 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", [(4, 2), (9, 3)])
def test_group_mapping_is_h_div_group(heads, kv, dtype):
    """Query head h reads K / V head h // group (HF repeat_kv), and that is far from h % n_kv"""
    B, L = 3, 200
    mask = torch.ones(B, L, dtype=torch.int64)
    got, ref, bound, contract = run_case(dtype, B, L, heads, kv, mask)
    assert not violations(got, ref, bound, contract).any()
    _, wrong, _, _ = run_case(dtype, B, L, heads, kv, mask, head_map=lambda h: h % kv)
    rel = ((got.double() - wrong).abs().max() / wrong.abs().max()).item()
    assert rel > 0.1, rel


@pytest.mark.gpu
def test_future_keys_do_not_reach_a_query():
    """Rewriting K and V of every key after position t leaves ctx of the queries up to t bit-identical"""
    B, L, heads, kv = 2, 320, 4, 2
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    for dtype in (F32, BF16, F16):
        qkv = grouped_inputs(dtype, B, L, heads, kv, seed=5)
        ctx = new_ctx(B * L, heads * D, dtype)
        assert launch(dtype, qkv, ctx, mask, B, L, heads, kv) == 0
        for t in (0, 63, 127, 128, 300):
            q2 = qkv.clone().view(B, L, -1)
            q2[:, t + 1:, heads * D:] = grouped_inputs(dtype, B, L, heads, kv, seed=6 + t).view(B, L, -1)[:, t + 1:, heads * D:]
            ctx2 = new_ctx(B * L, heads * D, dtype)
            assert launch(dtype, q2.view(B * L, -1), ctx2, mask, B, L, heads, kv) == 0
            a, b = ctx[:B * L].view(B, L, -1), ctx2[:B * L].view(B, L, -1)
            assert torch.equal(bits(a[:, :t + 1].contiguous(), dtype), bits(b[:, :t + 1].contiguous(), dtype)), (NAME[dtype], t)
            assert not torch.equal(bits(a[:, t + 1:].contiguous(), dtype), bits(b[:, t + 1:].contiguous(), dtype))


def _hf_rotary(rope_parameters, L):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    cfg = LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=384, num_hidden_layers=1,
                      vocab_size=600, max_position_embeddings=1024, rope_parameters=rope_parameters)
    rot = LlamaRotaryEmbedding(cfg)
    cos, sin = rot(torch.zeros(1, dtype=torch.float32), torch.arange(L)[None])
    return rot, cos, sin


ROPES = {"default": {"rope_type": "default", "rope_theta": 10000.0},
         "linear": {"rope_type": "linear", "rope_theta": 10000.0, "factor": 4.0},
         "llama3": {"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "original_max_position_embeddings": 64,
                    "low_freq_factor": 1.0, "high_freq_factor": 4.0}}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(ROPES))
def test_rope_gqa_matches_hf(kind):
    """float32: q and k heads match apply_rotary_pos_emb to 1e-6, the v heads are untouched bit for bit; position = row % L"""
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    B, L, heads, kv = 3, 257, 4, 2
    rot, cos, sin = _hf_rotary(ROPES[kind], L)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, L, heads + 2 * kv, D, generator=g)
    q, k = x[:, :, :heads].transpose(1, 2), x[:, :, heads:heads + kv].transpose(1, 2)      # [B, heads, L, D]
    wq, wk = apply_rotary_pos_emb(q, k, cos, sin)
    dev = x.reshape(B * L, -1).to(DEV).contiguous()
    inv = (C.c_float * 32)(*[float(v) for v in rot.inv_freq])
    N.check(N.lib().om_debug_rope_gqa(F32, N.ptr(dev), B * L, L, heads, kv, inv, float(rot.attention_scaling), N.stream_ptr()))
    torch.cuda.synchronize()
    got = dev.cpu().view(B, L, heads + 2 * kv, D)
    eq = (got[:, :, :heads] - wq.transpose(1, 2)).abs().max().item()
    ek = (got[:, :, heads:heads + kv] - wk.transpose(1, 2)).abs().max().item()
    print(f"rope {kind}: max |dq| {eq:.2e}, max |dk| {ek:.2e}")
    assert eq < 1e-6 * max(1.0, x.abs().max().item()) and ek < 1e-6 * max(1.0, x.abs().max().item())
    assert torch.equal(got[:, :, heads + kv:].contiguous().view(torch.int32), x[:, :, heads + kv:].contiguous().view(torch.int32))
    if kind != "default":
        dq, _ = apply_rotary_pos_emb(q, k, *_hf_rotary(ROPES["default"], L)[1:])
        assert (dq - wq).abs().max().item() > 0.1


@pytest.mark.gpu
def test_rope_gqa_16bit_rounds_once_and_refuses_bad_arguments():
    B, L, heads, kv = 2, 96, 4, 1
    rot, cos, sin = _hf_rotary(ROPES["default"], L)
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    inv = (C.c_float * 32)(*[float(v) for v in rot.inv_freq])
    for dtype in (BF16, F16):
        x = torch.randn(B, L, heads + 2 * kv, D, generator=torch.Generator().manual_seed(3)).to(TORCH_DT[dtype])
        wq, _ = apply_rotary_pos_emb(x[:, :, :heads].transpose(1, 2).float(), x[:, :, heads:heads + kv].transpose(1, 2).float(), cos, sin)
        dev = x.reshape(B * L, -1).to(DEV).contiguous()
        N.check(N.lib().om_debug_rope_gqa(dtype, N.ptr(dev), B * L, L, heads, kv, inv, 1.0, N.stream_ptr()))
        torch.cuda.synchronize()
        got = dev.cpu().view(B, L, heads + 2 * kv, D)[:, :, :heads].float()
        want = wq.transpose(1, 2).to(TORCH_DT[dtype]).float()
        ulp = 2.0 ** (-7 if dtype == BF16 else -10)
        assert ((got - want).abs() <= ulp * want.abs() + 1e-6).all()      # one rounding of an f32 value that differs by an ulp of f32 at most
    lib = N.lib()
    x = torch.zeros(8, 6 * D, device=DEV)
    assert lib.om_debug_rope_gqa(F32, N.ptr(x), 8, 1025, 4, 1, inv, 1.0, N.stream_ptr()) != 0
    assert lib.om_debug_rope_gqa(F32, N.ptr(x), 8, 8, 4, 3, inv, 1.0, N.stream_ptr()) != 0 and b"divide" in lib.om_last_error()
    ctx = torch.zeros(8, 4 * D, device=DEV)
    m = torch.ones(1, 8, dtype=torch.int64, device=DEV)
    assert lib.om_debug_attention_causal(F32, N.ptr(x), N.ptr(ctx), N.ptr(m), 1, 8, 4, 3, SCALE, N.stream_ptr()) != 0
    assert lib.om_debug_attention_causal(F32, N.ptr(x), N.ptr(ctx), N.ptr(m), 1, 1025, 4, 1, SCALE, N.stream_ptr()) != 0
