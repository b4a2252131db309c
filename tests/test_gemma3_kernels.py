"""The kernels EmbeddingGemma adds, alone: bidirectional grouped-query attention over heads of 256 columns, full and banded
(csrc/attention_d256.hip, csrc/attn_chunked_wide.h), against the float64 restatement of tests/test_attention_kernels.py under its
per-element bound with D = 256; the q / k RMSNorm + rotary pass at D = 256 in Gemma3's form against HF's own Gemma3RMSNorm and
apply_rotary_pos_emb; and the norm of a sublayer output added into the f32 residual stream against float64 under ln_fwd_bound."""
import ctypes as C
import math

import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import (BF16, DEV, F16, F32, NAME, TORCH_DT, U_ACC, attention_reference, bits, error_bound, new_ctx, rows_of,
                                          untouched, violations, visibility)
from tests.test_row_kernels import ln_forward, ln_fwd_bound

D = 256
SCALE = 256 ** -0.5
DTYPES = [F32, BF16, F16]
LENGTHS = [1, 31, 33, 64, 65, 128, 129, 257, 640]       # a wave edge, the 64-key chunk edge, the 128-query block edge, 3 and 10 chunks
GROUPS = [(3, 1), (4, 1), (4, 2), (2, 2)]
BAND = [(300, 1), (300, 63), (300, 64), (300, 65), (300, 127), (300, 128), (640, 256), (1024, 256), (129, 64)]


def grouped_inputs(dtype, B, L, heads, kv, seed, scale=SCALE):
    """tests/test_qwen3_kernels.py::grouped_inputs with 256 columns per head: [B * L, (heads + 2 kv) * 256], q and k so that the scaled
    scores spread by about 2, V of O(1), distinct per key AND per K / V head"""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(2.0 / (scale * math.sqrt(D)))
    x = torch.randn(B, L, heads + 2 * kv, D, generator=g)
    x[:, :, :heads + kv] *= a
    x[:, :, heads + kv:] += (torch.arange(L).float() % 7 - 3.0)[None, :, None, None] * 0.5
    x[:, :, heads + kv:] += torch.arange(kv).float()[None, None, :, None]
    return x.reshape(B * L, (heads + 2 * kv) * D).to(TORCH_DT[dtype]).to(DEV)


def as_mha(qkv, B, L, heads, kv, head_map):
    """the grouped projection regrouped as the fused [q | k | v] of `heads` heads that attention_reference takes"""
    x = qkv.view(B, L, heads + 2 * kv, D)
    idx = torch.tensor([head_map(h) for h in range(heads)], device=qkv.device)
    q, k, v = x[:, :, :heads], x[:, :, heads:heads + kv][:, :, idx], x[:, :, heads + kv:][:, :, idx]
    return torch.stack([q, k, v], 2).reshape(B * L, 3 * heads * D)


def four_masks(L):
    """full, right-padded, left-padded, holes"""
    mask = torch.zeros(4, L, dtype=torch.int64)
    mask[0] = 1
    mask[1, :max(1, (6 * L) // 10)] = 1
    mask[2, (3 * L) // 10:] = 1
    mask[3, ::3] = 1
    return mask


def launch(dtype, qkv, ctx, mask, B, L, heads, kv, w=0, scale=SCALE):
    rc = N.lib().om_debug_attention_gqa_d256(dtype, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, scale, w, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


_REF = {}       # the float64 reference of a case, computed once and left unchanged


def run_case(dtype, L, heads, kv, w=0, head_map=None, tag="", scale=SCALE, mask=None):
    mask = (four_masks(L) if mask is None else mask).to(DEV)
    B = mask.shape[0]
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=91 + 13 * L + heads + kv, scale=scale)
    qkv0 = qkv.clone()
    ctx = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, ctx, mask, B, L, heads, kv, w, scale) == 0, N.lib().om_last_error()
    assert torch.equal(bits(qkv, dtype), bits(qkv0, dtype)), "the input projection was written"
    assert untouched(ctx[B * L:], dtype), "rows after ctx were written"
    group = heads // kv
    key = (B, L, heads, kv, dtype, w, tag, scale)
    if key not in _REF:
        vis, contract = visibility(mask, w)
        ref, mag, smax, vabs = attention_reference(as_mha(qkv, B, L, heads, kv, head_map or (lambda h: h // group)), mask, None, B, L, heads, D,
                                                   scale, w=w, vis=vis)
        _REF[key] = (ref, error_bound(ref, mag, smax, vabs, L, D, dtype), contract)
    ref, bound, contract = _REF[key]
    return ctx[:B * L].view(B, L, heads * D), ref, bound, contract


def assert_case(got, ref, bound, contract, heads, tag):
    ratio = ((got.double() - ref).abs() / bound)[rows_of(contract, heads * D)]
    print(f"{tag}: max err/bound {ratio.max().item():.3f}, rows under contract {contract.float().mean().item():.2f}")
    bad = violations(got, ref, bound, contract)
    assert not bad.any(), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), ratio.max().item())
    assert torch.isfinite(got.double()).all()              # rows without a contract included
    assert contract.float().mean() >= 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L", LENGTHS)
def test_full_attention_d256_against_float64(L, dtype):
    got, ref, bound, contract = run_case(dtype, L, 3, 1)
    assert_case(got, ref, bound, contract, 3, f"d256 full {NAME[dtype]} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_full_attention_d256_at_1024_tokens(dtype):
    got, ref, bound, contract = run_case(dtype, 1024, 3, 1)
    assert_case(got, ref, bound, contract, 3, f"d256 full {NAME[dtype]} L=1024")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", GROUPS)
@pytest.mark.parametrize("L,w", [(129, 0), (257, 100)])
def test_groups_d256_against_float64(L, w, heads, kv, dtype):
    got, ref, bound, contract = run_case(dtype, L, heads, kv, w)
    assert_case(got, ref, bound, contract, heads, f"d256 {NAME[dtype]} L={L} w={w} heads={heads} kv={kv}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L,w", BAND)
def test_band_d256_against_float64(L, w, dtype):
    got, ref, bound, contract = run_case(dtype, L, 3, 1, w)
    assert_case(got, ref, bound, contract, 3, f"d256 band {NAME[dtype]} L={L} w={w}")
    # the controls on the device's own output: the neighbouring windows and another scale are rejected by the same bound
    for tag, kw in (("w+1", dict(w=w + 1)), ("w-1", dict(w=w - 1)), ("scale", dict(w=w, scale=SCALE * 1.05))):
        if kw["w"] < 1:
            continue
        mask = four_masks(L).to(DEV)
        vis, _ = visibility(mask, kw["w"])
        qkv = grouped_inputs(dtype, 4, L, 3, 1, seed=91 + 13 * L + 4)
        other, _, _, _ = attention_reference(as_mha(qkv, 4, L, 3, 1, lambda h: 0), mask, None, 4, L, 3, D, kw.get("scale", SCALE), w=kw["w"], vis=vis)
        assert violations(got, other, bound, contract).any(), f"the bound admits the control {tag}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_widest_windows_d256(dtype):
    """w = L - 2 is the last band (one pair of tokens hidden from each other): against float64.  w >= L - 1 reaches every key: full
    attention's kernel and its bits."""
    L = 200
    got, ref, bound, contract = run_case(dtype, L, 3, 1, L - 2)
    assert_case(got, ref, bound, contract, 3, f"d256 band {NAME[dtype]} L={L} w=L-2")
    full, _, _, _ = run_case(dtype, L, 3, 1, 0)
    assert not torch.equal(bits(got.contiguous(), dtype), bits(full.contiguous(), dtype))
    for w in (L - 1, L, 5000, -3):
        same, _, _, _ = run_case(dtype, L, 3, 1, w)
        assert torch.equal(bits(same.contiguous(), dtype), bits(full.contiguous(), dtype)), w


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", [(4, 2), (6, 3)])
def test_group_mapping_is_h_div_group(heads, kv, dtype):
    """Query head h reads K / V head h // group (HF repeat_kv), and that is far from h % n_kv"""
    L = 200
    mask = torch.ones(3, L, dtype=torch.int64)
    got, ref, bound, contract = run_case(dtype, L, heads, kv, mask=mask, tag="ones")
    assert not violations(got, ref, bound, contract).any()
    _, wrong, _, _ = run_case(dtype, L, heads, kv, head_map=lambda h: h % kv, tag="wrong map", mask=mask)
    rel = ((got.double() - wrong).abs().max() / wrong.abs().max()).item()
    assert rel > 0.1, rel


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L,w", [(300, 63), (300, 64), (640, 256)])
def test_keys_outside_the_band_do_not_reach_a_query(L, w, dtype):
    """Rewriting K and V of every key with |q - k| > w leaves ctx of query q bit-identical and changes other queries"""
    B, heads, kv = 2, 3, 1
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=5)
    ctx = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, ctx, mask, B, L, heads, kv, w) == 0
    other = grouped_inputs(dtype, B, L, heads, kv, seed=6).view(B, L, -1)
    for q in (0, 63, 64, 127, 128, L // 2, L - 1):
        q2 = qkv.clone().view(B, L, -1)
        far = (torch.arange(L, device=DEV) - q).abs() > w
        assert far.any()
        q2[:, far, heads * D:] = other[:, far, heads * D:]
        ctx2 = new_ctx(B * L, heads * D, dtype)
        assert launch(dtype, q2.view(B * L, -1), ctx2, mask, B, L, heads, kv, w) == 0
        a, b = ctx[:B * L].view(B, L, -1), ctx2[:B * L].view(B, L, -1)
        assert torch.equal(bits(a[:, q].contiguous(), dtype), bits(b[:, q].contiguous(), dtype)), (NAME[dtype], q)
        assert not torch.equal(bits(a.contiguous(), dtype), bits(b.contiguous(), dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_a_fully_masked_sequence_stays_finite_and_uniform(dtype):
    L = 150
    mask = torch.ones(2, L, dtype=torch.int64)
    mask[1] = 0
    for w in (0, 20):
        got, ref, bound, contract = run_case(dtype, L, 3, 1, w, mask=mask, tag="masked row")
        assert torch.isfinite(got.double()).all()
        assert not violations(got, ref, bound, contract).any()


# ------------------------------------------------------------------------------------------------ q / k norm + rotary positions
ROPES = {"sliding": {"rope_type": "default", "rope_theta": 10000.0}, "full": {"rope_type": "default", "rope_theta": 1000000.0}}


def _hf_rotary(kind, L):
    from transformers import Gemma3TextConfig
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RotaryEmbedding
    cfg = Gemma3TextConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=D, intermediate_size=192, num_hidden_layers=2,
                           layer_types=["sliding_attention", "full_attention"], vocab_size=600, max_position_embeddings=1024,
                           rope_parameters={"sliding_attention": ROPES["sliding"], "full_attention": ROPES["full"]})
    rot = Gemma3RotaryEmbedding(cfg)
    layer_type = f"{kind}_attention"
    cos, sin = rot(torch.zeros(1, dtype=torch.float32), torch.arange(L)[None], layer_type)
    inv = getattr(rot, f"{layer_type}_inv_freq")
    return (C.c_float * 128)(*[float(v) for v in inv]), float(getattr(rot, f"{layer_type}_attention_scaling")), cos, sin


def _hf_norm_rope(x, heads, kv, wq, wk, eps, cos, sin):
    """Gemma3Attention.forward's q_norm / k_norm + apply_rotary_pos_emb on [B, L, heads + 2 kv, 256] in f32; wq / wk are the module's
    own weights w (the kernel receives 1 + w)"""
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm, apply_rotary_pos_emb
    nq, nk = Gemma3RMSNorm(D, eps), Gemma3RMSNorm(D, eps)
    with torch.no_grad():
        nq.weight.copy_(wq)
        nk.weight.copy_(wk)
        q, k = nq(x[:, :, :heads]), nk(x[:, :, heads:heads + kv])
        rq, rk = apply_rotary_pos_emb(q.transpose(1, 2), k.transpose(1, 2), cos, sin)
    return rq.transpose(1, 2), rk.transpose(1, 2)


def _run_qknorm(dtype, x, L, heads, kv, wq, wk, eps, inv, scaling):
    dev = x.reshape(x.shape[0] * L, -1).to(DEV).contiguous()
    dq, dk = (1.0 + wq).to(DEV), (1.0 + wk).to(DEV)             # g = 1 + w in f32, as the host packs it (held until the launch has run)
    N.check(N.lib().om_debug_qknorm_rope_d256(dtype, N.ptr(dev), dev.shape[0], L, heads, kv, N.ptr(dq), N.ptr(dk), eps, inv, scaling, N.stream_ptr()))
    torch.cuda.synchronize()
    return dev.cpu().view(x.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 200, 1024])
@pytest.mark.parametrize("kind", ["sliding", "full"])
def test_qknorm_rope_d256_matches_hf_f32(kind, L):
    """float32: the q and k heads match Gemma3RMSNorm + apply_rotary_pos_emb within 1e-6 * max(1, |x|max), the bar of
    test_qwen3_kernels.py at D = 128; the v heads are untouched bit for bit; position = row % L; both thetas"""
    B, heads, kv, eps = 2, 3, 1, 1e-6
    inv, scaling, cos, sin = _hf_rotary(kind, L)
    g = torch.Generator().manual_seed(11 + L)
    x = torch.randn(B, L, heads + 2 * kv, D, generator=g) * 1.7
    wq, wk = 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    want_q, want_k = _hf_norm_rope(x, heads, kv, wq, wk, eps, cos, sin)
    got = _run_qknorm(F32, x, L, heads, kv, wq, wk, eps, inv, scaling)
    eq = (got[:, :, :heads] - want_q).abs().max().item()
    ek = (got[:, :, heads:heads + kv] - want_k).abs().max().item()
    bar = 1e-6 * max(1.0, x.abs().max().item())
    print(f"qknorm+rope d256 f32 {kind} L={L}: max |dq| {eq:.2e}, max |dk| {ek:.2e}, bar {bar:.2e}")
    assert eq < bar and ek < bar
    assert torch.equal(got[:, :, heads + kv:].contiguous().view(torch.int32), x[:, :, heads + kv:].contiguous().view(torch.int32))
    zero_q, _ = _hf_norm_rope(x, heads, kv, torch.zeros(D), torch.zeros(D), eps, cos, sin)      # a weight taken as g = w, or dropped
    assert (zero_q - want_q).abs().max().item() > 0.1
    if L > 1:
        _, _, cos2, sin2 = _hf_rotary("full" if kind == "sliding" else "sliding", L)
        assert (_hf_norm_rope(x, heads, kv, wq, wk, eps, cos2, sin2)[0] - want_q).abs().max().item() > 0.1      # the other theta


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_qknorm_rope_d256_16bit_is_the_f32_computation_rounded_once(dtype):
    """16-bit, against HF's f32 computation on the stored inputs rounded ONCE: Gemma3RMSNorm keeps the normalised value in f32 through
    the weight multiply, so there is no rounding between the two (the Qwen3 form has one).  Every element meets the bar
    test_qwen3_kernels.py uses, |got - want16| <= ulp (|y cos| + |rotate_half(y) sin| + |want16|) + 1e-6.  And EQUAL bits are asserted
    on every element the format pins: two correct f32 evaluations differ by at most (D + 16) u in the normalised value (the sum of D
    squares in any order, the eps add, rsqrt, one product: test_qwen3_kernels.pinned_by_the_formats), the weight multiply adds u, the
    rotation 8 u of its products' magnitude (the cos / sin table, two products, one sum), so |w - w'| <= (D + 25) u mag; an element
    whose f32 result rounds alike from that whole interval is the same 16-bit number in both.  At D = 256 the interval is
    2 x 281 u = 3.4e-5 of mag against a spacing of 2^-11 .. 2^-10 (f16) or 2^-8 .. 2^-7 (bf16) of the result, so about 5 % (f16) or
    0.6 % (bf16) of the elements are undecided where mag is the result's own magnitude, more where the two products cancel; the share
    of pinned elements is asserted to be more than half so that the equality says something, and printed.  A kernel that rounds the
    normalised value before the weight multiply moves the f32 result by up to half a 16-bit ulp on every element and fails the
    equality on about three pinned elements in ten (test_qwen3_kernels.py states the same figure for the converse change)."""
    B, L, heads, kv, eps = 2, 96, 3, 1, 1e-6
    dt = TORCH_DT[dtype]
    u = 2.0 ** -24
    inv, scaling, cos, sin = _hf_rotary("sliding", L)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, L, heads + 2 * kv, D, generator=g) * 1.7).to(dt)
    wq, wk = 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    want_q, want_k = _hf_norm_rope(x.float(), heads, kv, wq, wk, eps, cos, sin)
    plain_q, plain_k = _hf_norm_rope(x.float(), heads, kv, wq, wk, eps, torch.ones_like(cos), torch.zeros_like(sin))
    got = _run_qknorm(dtype, x, L, heads, kv, wq, wk, eps, inv, scaling)
    ulp = 2.0 ** (-7 if dtype == BF16 else -10)
    for name, g_, w_, y in (("q", got[:, :, :heads], want_q, plain_q), ("k", got[:, :, heads:heads + kv], want_k, plain_k)):
        w16 = w_.to(dt).float()
        c, sn = cos[0][None, :, None, :], sin[0][None, :, None, :]
        mag = (y * c).abs() + (torch.cat([y[..., D // 2:], y[..., :D // 2]], -1) * sn).abs()
        pinned = (w_ + (D + 25) * u * mag).to(dt) == (w_ - (D + 25) * u * mag).to(dt)
        err = (g_.float() - w16).abs()
        equal = err == 0
        print(f"qknorm+rope d256 {NAME[dtype]} {name}: pinned {pinned.float().mean().item():.5f}, equal to HF rounded once "
              f"{equal.float().mean().item():.5f} of all and {equal[pinned].float().mean().item():.5f} of the pinned elements; "
              f"max err / bar {(err / (ulp * (mag + w16.abs()) + 1e-6)).max().item():.3f}")
        assert pinned.float().mean().item() > 0.5
        assert equal[pinned].all(), (int((~equal & pinned).sum()), torch.nonzero(~equal & pinned)[:5].tolist())
        assert (err <= ulp * (mag + w16.abs()) + 1e-6).all()
    assert torch.equal(bits(got[:, :, heads + kv:].contiguous(), dtype), bits(x[:, :, heads + kv:].contiguous(), dtype))


# ------------------------------------------------------------------------------------------------ norm of a sublayer output + add
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("M", [1, 5, 17])
@pytest.mark.parametrize("H", [64, 640, 768, 1152, 2048])
def test_rmsnorm_add_against_float64(H, M, dtype):
    """x[f32] += (h rsqrt(mean(h^2) + eps)) g on the stored values: the norm under ln_fwd_bound with an f32 output (the sum is not
    rounded to the 16-bit format), plus the one rounding of the f32 add, u |x + y|.  Rows after M and the columns of the pitch past H
    keep their bits; h is not written."""
    eps, pad = 1e-6, 4
    gen = torch.Generator().manual_seed(H + M)
    h = (torch.randn(M + 2, H + pad, generator=gen) * 3.0).to(TORCH_DT[dtype]).to(DEV)
    x = torch.randn(M + 2, H + pad, generator=gen).to(DEV)
    gw = (1.0 + 0.3 * torch.randn(H, generator=gen)).to(DEV)
    h0, x0 = h.clone(), x.clone()
    N.check(N.lib().om_debug_rmsnorm_add(dtype, N.ptr(h), H + pad, N.ptr(x), H + pad, N.ptr(gw), M, H, eps, N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(h, dtype), bits(h0, dtype))
    assert torch.equal(x[M:].view(torch.int32), x0[M:].view(torch.int32)) and torch.equal(x[:, H:].contiguous().view(torch.int32), x0[:, H:].contiguous().view(torch.int32))
    R = ln_forward(h0[:M, :H].double(), gw.double(), None, eps, True)
    want = x0[:M, :H].double() + R.y
    bound = ln_fwd_bound(R, H, F32) + U_ACC * want.abs()
    err = (x[:M, :H].double() - want).abs()
    print(f"rmsnorm-add {NAME[dtype]} H={H} M={M}: max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    # the controls: the norm without its weight, and the norm rounded to the input's magnitude of a missing add
    assert not ((x0[:M, :H].double() + R.xhat - want).abs() <= bound).all()
    assert not ((R.y - want).abs() <= bound).all()
