"""The kernels a Qwen3 embedder adds, alone (csrc/attention_causal128.hip, csrc/attn_chunked_wide.h): causal grouped-query attention over
heads of 128 columns against the float64 restatement of tests/test_attention_kernels.py under its per-element bound (error_bound takes
D), padded and packed, and the q / k RMSNorm + rotary pass against HF's own Qwen3RMSNorm and apply_rotary_pos_emb."""
import ctypes as C
import math

import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_causal import ROPES, causal_visibility, padding_masks
from tests.test_attention_kernels import (BF16, DEV, F16, F32, NAME, TORCH_DT, attention_reference, bits, error_bound, mask_extent, new_ctx,
                                          pack_rows, rows_of, untouched, violations)

D = 128
SCALE = 128 ** -0.5
LENGTHS = [1, 31, 33, 128, 129, 257, 640]       # a wave edge, a chunk edge, diagonal + full chunks, 5 chunks
GROUPS = [(4, 4), (4, 2), (4, 1), (6, 3)]


def grouped_inputs(dtype, B, L, heads, kv, seed):
    """tests/test_attention_causal.py::grouped_inputs with 128 columns per head: [B * L, (heads + 2 kv) * 128], q and k so that the
    scaled scores spread by about 2, V of O(1), distinct per key AND per K / V head"""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(2.0 / (SCALE * math.sqrt(D)))
    x = torch.randn(B, L, heads + 2 * kv, D, generator=g)
    x[:, :, :heads + kv] *= a
    x[:, :, heads + kv:] += (torch.arange(L).float() % 7 - 3.0)[None, :, None, None] * 0.5
    x[:, :, heads + kv:] += torch.arange(kv).float()[None, None, :, None]
    return x.reshape(B * L, (heads + 2 * kv) * D).to(TORCH_DT[dtype]).to(DEV)


def as_mha(qkv, B, L, heads, kv, head_map):
    x = qkv.view(B, L, heads + 2 * kv, D)
    idx = torch.tensor([head_map(h) for h in range(heads)], device=qkv.device)
    q, k, v = x[:, :, :heads], x[:, :, heads:heads + kv][:, :, idx], x[:, :, heads + kv:][:, :, idx]
    return torch.stack([q, k, v], 2).reshape(B * L, 3 * heads * D)


def launch(dtype, qkv, ctx, mask, B, L, heads, kv):
    rc = N.lib().om_debug_attention_causal_hd(dtype, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), B, L, heads, kv, D, SCALE, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


_REF = {}       # (B, L, heads, kv, dtype, map) -> the float64 reference of a case, computed once


def run_case(dtype, B, L, heads, kv, mask, head_map=None, seed=0, tag="group"):
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=77 + 13 * L + heads + kv + seed)
    mask = mask.to(DEV)
    qkv0 = qkv.clone()
    ctx = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, ctx, mask, B, L, heads, kv) == 0, N.lib().om_last_error()
    assert torch.equal(bits(qkv, dtype), bits(qkv0, dtype))
    assert untouched(ctx[B * L:], dtype), "rows after ctx were written"
    group = heads // kv
    key = (B, L, heads, kv, dtype, tag, seed)
    if key not in _REF:
        vis, contract = causal_visibility(mask)
        ref, mag, smax, vabs = attention_reference(as_mha(qkv, B, L, heads, kv, head_map or (lambda h: h // group)), mask, None, B, L, heads, D,
                                                   SCALE, vis=vis)
        _REF[key] = (ref, error_bound(ref, mag, smax, vabs, L, D, dtype), contract)
    ref, bound, contract = _REF[key]
    return ctx[:B * L].view(B, L, heads * D), ref, bound, contract


def _assert_case(got, ref, bound, contract, heads, tag):
    ratio = ((got.double() - ref).abs() / bound)[rows_of(contract, heads * D)]
    print(f"{tag}: max err/bound {ratio.max().item():.3f}, compared rows {contract.float().mean().item():.2f}")
    bad = violations(got, ref, bound, contract)
    assert not bad.any(), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), ratio.max().item())
    assert torch.isfinite(got.double()).all()              # masked-query rows included (the first rows under left padding)
    assert contract.float().mean() > 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", GROUPS)
@pytest.mark.parametrize("L", LENGTHS)
def test_causal_attention_d128_against_float64(L, heads, kv, dtype):
    """four rows: full, right-padded, left-padded, and one whose leading tokens alone are masked"""
    B = 4
    got, ref, bound, contract = run_case(dtype, B, L, heads, kv, padding_masks(B, L), tag="lengths")
    _assert_case(got, ref, bound, contract, heads, f"causal d128 {NAME[dtype]} L={L} heads={heads} kv={kv}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_causal_attention_d128_at_1024_tokens(dtype):
    got, ref, bound, contract = run_case(dtype, 2, 1024, 4, 2, padding_masks(2, 1024), tag="1024")
    _assert_case(got, ref, bound, contract, 4, f"causal d128 {NAME[dtype]} L=1024")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", [(4, 2), (6, 3)])
def test_group_mapping_is_h_div_group(heads, kv, dtype):
    """Query head h reads K / V head h // group (HF repeat_kv), and that is far from h % n_kv"""
    B, L = 3, 200
    mask = torch.ones(B, L, dtype=torch.int64)
    got, ref, bound, contract = run_case(dtype, B, L, heads, kv, mask)
    assert not violations(got, ref, bound, contract).any()
    _, wrong, _, _ = run_case(dtype, B, L, heads, kv, mask, head_map=lambda h: h % kv, tag="wrong map")
    rel = ((got.double() - wrong).abs().max() / wrong.abs().max()).item()
    assert rel > 0.1, rel


@pytest.mark.gpu
def test_future_keys_do_not_reach_a_query():
    """Rewriting K and V of every key after position t leaves ctx of the queries up to t bit-identical"""
    B, L, heads, kv = 2, 257, 4, 2
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    for dtype in (F32, BF16, F16):
        qkv = grouped_inputs(dtype, B, L, heads, kv, seed=5)
        ctx = new_ctx(B * L, heads * D, dtype)
        assert launch(dtype, qkv, ctx, mask, B, L, heads, kv) == 0
        for t in (0, 127, 128, 200):
            q2 = qkv.clone().view(B, L, -1)
            q2[:, t + 1:, heads * D:] = grouped_inputs(dtype, B, L, heads, kv, seed=6 + t).view(B, L, -1)[:, t + 1:, heads * D:]
            ctx2 = new_ctx(B * L, heads * D, dtype)
            assert launch(dtype, q2.view(B * L, -1), ctx2, mask, B, L, heads, kv) == 0
            a, b = ctx[:B * L].view(B, L, -1), ctx2[:B * L].view(B, L, -1)
            assert torch.equal(bits(a[:, :t + 1].contiguous(), dtype), bits(b[:, :t + 1].contiguous(), dtype)), (NAME[dtype], t)
            assert not torch.equal(bits(a[:, t + 1:].contiguous(), dtype), bits(b[:, t + 1:].contiguous(), dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("B,L", [(16, 128), (4, 640)])
def test_packed_attention_is_the_padded_kernel_row_for_row(B, L, dtype):
    """Ragged right-padded batches: every packed row carries the bits of its padded row; rows of the packed ctx at and beyond the
    token count keep the sentinel."""
    heads, kv = 4, 2
    g = torch.Generator().manual_seed(B + L)
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        mask[b, :L if b == 0 else int(torch.randint(1, L + 1, (1,), generator=g))] = 1
    mask = mask.to(DEV)
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=3 + L)
    padded = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, padded, mask, B, L, heads, kv) == 0
    kmax = mask_extent(mask)
    total = int(kmax.sum())
    assert total == int(mask.sum())
    rows = total + 7
    cu, _, row_map = pack_rows(kmax, L, rows)
    src = row_map[:total].long()
    qp = torch.zeros(rows, qkv.shape[1], dtype=TORCH_DT[dtype], device=DEV)
    qp[:total] = qkv[src]
    qp0 = qp.clone()
    ctx = new_ctx(rows, heads * D, dtype)
    rc = N.lib().om_debug_attention_causal_hd_packed(dtype, N.ptr(qp), N.ptr(ctx), N.ptr(mask), N.ptr(cu), B, L, heads, kv, D, SCALE, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, N.lib().om_last_error()
    assert torch.equal(bits(qp, dtype), bits(qp0, dtype))
    assert torch.equal(bits(ctx[:total].contiguous(), dtype), bits(padded[:B * L][src].contiguous(), dtype))
    assert untouched(ctx[total:], dtype), "rows at and beyond the token count were written"


# ------------------------------------------------------------------------------------------------ q / k norm + rotary positions
def _hf_rotary(rope_parameters, L, head_dim):
    from transformers import Qwen3Config
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    cfg = Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=head_dim, intermediate_size=384,
                      num_hidden_layers=1, vocab_size=600, max_position_embeddings=1024, rope_parameters=rope_parameters)
    rot = Qwen3RotaryEmbedding(cfg)
    cos, sin = rot(torch.zeros(1, dtype=torch.float32), torch.arange(L)[None])
    return rot, cos, sin


def _hf_norm_rope(x, heads, kv, hd, wq, wk, eps, cos, sin, norm_dtype=None):
    """Qwen3Attention.forward's q_norm / k_norm + apply_rotary_pos_emb on [B, L, heads + 2 kv, hd]; norm_dtype: the 16-bit format the
    normalised value is cast back to (Qwen3RMSNorm's .to(input_dtype)) before the f32 weight multiply, as under autocast"""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb
    q, k = x[:, :, :heads], x[:, :, heads:heads + kv]
    if wq is not None:
        nq, nk = Qwen3RMSNorm(hd, eps), Qwen3RMSNorm(hd, eps)
        with torch.no_grad():
            nq.weight.copy_(wq)
            nk.weight.copy_(wk)
            if norm_dtype is None:
                q, k = nq(q), nk(k)
            else:
                q, k = nq(q.to(norm_dtype)).float(), nk(k.to(norm_dtype)).float()      # f32 weight * 16-bit value -> f32
    with torch.no_grad():
        rq, rk = apply_rotary_pos_emb(q.transpose(1, 2), k.transpose(1, 2), cos, sin)
    return rq.transpose(1, 2), rk.transpose(1, 2)


def _inv(rot, hd):
    return (C.c_float * (hd // 2))(*[float(v) for v in rot.inv_freq])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 200, 1024])
@pytest.mark.parametrize("kind", ["default", "llama3"])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "rope only"])
@pytest.mark.parametrize("hd", [128, 64])
def test_qknorm_rope_matches_hf_f32(hd, norm, kind, L):
    """float32: the q and k heads match Qwen3RMSNorm + apply_rotary_pos_emb within 1e-6 * max(1, |x|max), the bar of
    test_rope_gqa_matches_hf; the v heads are untouched bit for bit; position = row % L"""
    B, heads, kv, eps = 2, 4, 2, 1e-6
    rot, cos, sin = _hf_rotary(ROPES[kind], L, hd)
    g = torch.Generator().manual_seed(11 + L + hd)
    x = torch.randn(B, L, heads + 2 * kv, hd, generator=g) * 1.7
    wq, wk = (1.0 + 0.3 * torch.randn(hd, generator=g), 1.0 + 0.3 * torch.randn(hd, generator=g)) if norm else (None, None)
    want_q, want_k = _hf_norm_rope(x, heads, kv, hd, wq, wk, eps, cos, sin)
    dev = x.reshape(B * L, -1).to(DEV).contiguous()
    dq, dk = (wq.to(DEV), wk.to(DEV)) if norm else (None, None)
    N.check(N.lib().om_debug_qknorm_rope(F32, N.ptr(dev), B * L, L, heads, kv, hd, N.ptr(dq), N.ptr(dk), eps, _inv(rot, hd),
                                         float(rot.attention_scaling), N.stream_ptr()))
    torch.cuda.synchronize()
    got = dev.cpu().view(B, L, heads + 2 * kv, hd)
    eq = (got[:, :, :heads] - want_q).abs().max().item()
    ek = (got[:, :, heads:heads + kv] - want_k).abs().max().item()
    bar = 1e-6 * max(1.0, x.abs().max().item())
    print(f"qknorm+rope f32 hd={hd} norm={norm} {kind} L={L}: max |dq| {eq:.2e}, max |dk| {ek:.2e}, bar {bar:.2e}")
    assert eq < bar and ek < bar
    assert torch.equal(got[:, :, heads + kv:].contiguous().view(torch.int32), x[:, :, heads + kv:].contiguous().view(torch.int32))
    if norm:
        plain_q, _ = _hf_norm_rope(x, heads, kv, hd, None, None, eps, cos, sin)
        assert (plain_q - want_q).abs().max().item() > 0.1


def _rounds_alike(v, rel, dt):
    """the elements of the f32 tensor v that round to ONE value of the format dt from anywhere within rel * |v| of v (rounding is
    monotone: the two ends agree, so everything between them does)"""
    return (v * (1.0 + rel)).to(dt) == (v * (1.0 - rel)).to(dt)


def pinned_by_the_formats(x, want, mag, hd, eps, dt):
    """The elements of the rotated heads whose 16-bit value the number formats alone determine, whatever the order of the f32 sums.
    HF's result has two roundings to the 16-bit format, and an f32 value that precedes one can differ between two correct
    implementations:
      * the normalised value n = x * rsqrt(mean(x^2) + eps).  The sum of D squares, each rounded (u = 2^-24), added in ANY order is
        within D u of the exact sum, relatively: two orders differ by at most 2 D u, + u each for the eps sum; rsqrt halves that and
        adds its own error (taken as 4 u a side: sqrt and divide, or a library rsqrt); the product x * r rounds once a side:
        |n - n'| <= (D + 1 + 8 + 2) u |n|, taken as (D + 16) u.  An n that rounds alike from that whole interval is the SAME 16-bit
        number in both, and then y = g * n is the same f32 number.
      * the f32 result w = y cos + rotate_half(y) sin before the store.  With equal y the one difference left is the cos / sin table
        (libm's f32 cos against a rounded double cos: 2 u relative a side); each product then differs by at most 4 u of itself with
        its rounding, the sum by 2 u more: |w - w'| <= 6 u mag, mag = |y cos| + |rotate_half(y) sin|, taken as 8 u mag.
    An element is pinned when its own n and its rotation partner's n round alike and w rounds alike from w +- 8 u mag.
    x: the stored heads as f32 [.., hd]; want: HF's f32 result; returns (pinned, the share of elements whose n rounds alike)."""
    u = 2.0 ** -24
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)          # Qwen3RMSNorm.forward up to its cast
    n_alike = _rounds_alike(n, (hd + 16) * u, dt)
    pair = n_alike & torch.roll(n_alike, hd // 2, -1)
    w_alike = (want + 8 * u * mag).to(dt) == (want - 8 * u * mag).to(dt)
    return pair & w_alike, n_alike.float().mean().item()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", [128, 64])
def test_qknorm_rope_16bit_is_the_f32_computation_rounded_once(hd, dtype):
    """16-bit, against HF's f32 computation on the stored inputs (the normalised value cast back to the storage format before the
    f32 weight multiply, as Qwen3RMSNorm does) rounded once.  Which of "equal" and "within 1 ulp" holds: EQUAL, bit for bit, on
    every element that the formats pin (pinned_by_the_formats: neither the cast of the normalised value nor the final rounding sits
    within the f32 reduction's own error of a tie) -- asserted, and the share of pinned elements is asserted to be at least 0.9,
    which follows from the formats: the cast of n is undecided on a share of at most 2 (D + 16) u / 2^-11 = 3.5 % of the elements in
    f16 at D = 128 (the interval's width over the smallest spacing of the format; bf16: 0.44 %), an element needs its partner's n
    too (7 %), and the final rounding is undecided on about 16 u mag / (2^-11 |w|) < 1 %.  A kernel that drops the cast of n, or rounds
    y as well, moves the f32 result by a fraction of a 16-bit ulp on EVERY element, and about three in ten of the pinned ones then
    store another number (a CPU restatement of the kernel with either change: 0.69-0.70 of the pinned elements equal).  Fused
    products in the rotation move the f32 result by half an f32 ulp, inside the allowance for the cos / sin table: the f32 test
    above is the one that bounds them.
    The elements that are not pinned are not all within 1 ulp of the RESULT, and cannot be: an n on the other side of a tie moves
    y = n g by one 16-bit ulp of y, hence the result by up to ulp * (|y cos| + |rotate_half(y) sin|), an ulp at the magnitude of the
    PRODUCTS, which exceeds the result's where they cancel; rounding either f32 result adds half an ulp of the result.  Their bar is
    |got - want16| <= ulp * (|y cos| + |rotate_half(y) sin| + |want16|) + 1e-6 (the last term for denormal-sized results).
    Measured on an MI355X: MEASURED_FIGURES"""
    B, L, heads, kv, eps = 2, 96, 4, 1, 1e-6
    dt = TORCH_DT[dtype]
    rot, cos, sin = _hf_rotary(ROPES["default"], L, hd)
    g = torch.Generator().manual_seed(3 + hd)
    x = (torch.randn(B, L, heads + 2 * kv, hd, generator=g) * 1.7).to(dt)
    wq, wk = 1.0 + 0.3 * torch.randn(hd, generator=g), 1.0 + 0.3 * torch.randn(hd, generator=g)
    want_q, want_k = _hf_norm_rope(x.float(), heads, kv, hd, wq, wk, eps, cos, sin, norm_dtype=dt)
    dev = x.reshape(B * L, -1).to(DEV).contiguous()
    dq, dk = wq.to(DEV), wk.to(DEV)                         # (held until the launch has run)
    N.check(N.lib().om_debug_qknorm_rope(dtype, N.ptr(dev), B * L, L, heads, kv, hd, N.ptr(dq), N.ptr(dk), eps, _inv(rot, hd), 1.0,
                                         N.stream_ptr()))
    torch.cuda.synchronize()
    got = dev.cpu().view(B, L, heads + 2 * kv, hd)
    ulp = 2.0 ** (-7 if dtype == BF16 else -10)
    # y = the normed, weighted heads before the rotation (HF's own, through a rotation by zero): the magnitude of the two products
    plain_q, plain_k = _hf_norm_rope(x.float(), heads, kv, hd, wq, wk, eps, torch.ones_like(cos), torch.zeros_like(sin), norm_dtype=dt)
    xf = x.float()
    for name, g_, w_, y, x_ in (("q", got[:, :, :heads], want_q, plain_q, xf[:, :, :heads]),
                                ("k", got[:, :, heads:heads + kv], want_k, plain_k, xf[:, :, heads:heads + kv])):
        w16 = w_.to(dt).float()
        c, sn = cos[0][None, :, None, :], sin[0][None, :, None, :]
        mag = (y * c).abs() + (torch.cat([y[..., hd // 2:], y[..., :hd // 2]], -1) * sn).abs()
        pinned, n_alike = pinned_by_the_formats(x_, w_, mag, hd, eps, dt)
        err = (g_.float() - w16).abs()
        equal = err == 0
        print(f"qknorm+rope {NAME[dtype]} hd={hd} {name}: pinned {pinned.float().mean().item():.5f} (n rounds alike {n_alike:.5f}), equal to HF "
              f"rounded once {equal.float().mean().item():.5f} of all and {equal[pinned].float().mean().item():.5f} of the pinned elements, "
              f"within 1 ulp of the result {(err <= ulp * w16.abs() + 1e-6).float().mean().item():.5f}; "
              f"max err / bar {(err / (ulp * (mag + w16.abs()) + 1e-6)).max().item():.3f}")
        assert pinned.float().mean().item() >= 0.9
        assert equal[pinned].all(), (int((~equal & pinned).sum()), torch.nonzero(~equal & pinned)[:5].tolist())
        assert (err <= ulp * (mag + w16.abs()) + 1e-6).all()
    assert torch.equal(bits(got[:, :, heads + kv:].contiguous(), dtype), bits(x[:, :, heads + kv:].contiguous(), dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", [128, 64])
def test_qknorm_rope_rows_form_is_the_plain_form_row_for_row(hd, dtype):
    """packed rows: row t takes the position row_map[t] % L and equals the plain pass's row row_map[t]; rows with row_map < 0 are left
    alone"""
    B, L, heads, kv, eps = 5, 200, 4, 2, 1e-6
    rot, _, _ = _hf_rotary(ROPES["llama3"], L, hd)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(B * L, (heads + 2 * kv) * hd, generator=g) * 1.7).to(TORCH_DT[dtype]).to(DEV)
    wq, wk = (1.0 + 0.3 * torch.randn(hd, generator=g)).to(DEV), (1.0 + 0.3 * torch.randn(hd, generator=g)).to(DEV)
    mask = padding_masks(B, L)
    mask[B - 1] = 1
    mask[B - 1, 150:] = 0
    mask[2] = 1
    mask[2, 77:] = 0
    kmax = mask_extent(mask.to(DEV))
    total = int(kmax.sum())
    rows = total + 9
    _, _, row_map = pack_rows(kmax, L, rows)
    assert (row_map[total:] < 0).all()
    plain = x.clone()
    N.check(N.lib().om_debug_qknorm_rope(dtype, N.ptr(plain), B * L, L, heads, kv, hd, N.ptr(wq), N.ptr(wk), eps, _inv(rot, hd), 1.0, N.stream_ptr()))
    packed = torch.zeros(rows, x.shape[1], dtype=x.dtype, device=DEV)
    packed[:total] = x[row_map[:total].long()]
    packed[total:] = 3.0
    N.check(N.lib().om_debug_qknorm_rope_rows(dtype, N.ptr(packed), rows, L, heads, kv, hd, N.ptr(wq), N.ptr(wk), eps, _inv(rot, hd), 1.0,
                                              N.ptr(row_map), N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(packed[:total].contiguous(), dtype), bits(plain[row_map[:total].long()].contiguous(), dtype))
    assert (packed[total:] == 3.0).all()
    assert not torch.equal(plain, x)


@pytest.mark.gpu
def test_hooks_refuse_bad_arguments():
    lib = N.lib()
    inv = (C.c_float * 64)(*([0.5] * 64))
    x = torch.zeros(8, 6 * D, device=DEV)
    ctx = torch.zeros(8, 4 * D, device=DEV)
    m = torch.ones(1, 8, dtype=torch.int64, device=DEV)
    assert lib.om_debug_qknorm_rope(F32, N.ptr(x), 8, 1025, 4, 1, D, None, None, 1e-6, inv, 1.0, N.stream_ptr()) != 0
    assert lib.om_debug_qknorm_rope(F32, N.ptr(x), 8, 8, 4, 3, D, None, None, 1e-6, inv, 1.0, N.stream_ptr()) != 0 and b"divide" in lib.om_last_error()
    assert lib.om_debug_qknorm_rope(F32, N.ptr(x), 8, 8, 4, 1, 96, None, None, 1e-6, inv, 1.0, N.stream_ptr()) != 0 and b"64 or 128" in lib.om_last_error()
    assert lib.om_debug_attention_causal_hd(F32, N.ptr(x), N.ptr(ctx), N.ptr(m), 1, 8, 4, 3, D, SCALE, N.stream_ptr()) != 0
    assert lib.om_debug_attention_causal_hd(F32, N.ptr(x), N.ptr(ctx), N.ptr(m), 1, 1025, 4, 1, D, SCALE, N.stream_ptr()) != 0
    assert lib.om_debug_attention_causal_hd(F32, N.ptr(x), N.ptr(ctx), N.ptr(m), 1, 8, 4, 1, 96, SCALE, N.stream_ptr()) != 0
