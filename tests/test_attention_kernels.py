"""The attention forward kernel by kernel (csrc/attention.hip, attention_d32.hip, attention_band.hip) against a float64
reference of  ctx = (keep o softmax(scale Q K^T + bias + mask)) keep_scale V  on the exact stored (rounded) inputs, element by
element, within a bound derived from the arithmetic (error_bound below).  The one constant of the bound that is not derived
is EXP_REL, the relative error of the exp path, measured on the MI355X (see beside the constant).

Every GPU case names the kernel family and key-tile count it must reach and asserts them through om_debug_attention_last();
every case carries negative controls on the reference side (the last unmasked key dropped, the bias rolled by one key column,
w +- 1, seed + 1, scale (1 + 2^-5)) that the bound must reject; qkv, mask and bias must come back bit-unchanged and so must
sentinel rows after ctx's last row.

Contracts the kernels share, as this file pins them:
  * a padded key has probability exactly 0 whenever its sequence has an unmasked key (finfo.min added in the f32 and 32-wide
    kernels, -1e30 in the log2 domain in the 16-bit 64-wide ones: the same result);
  * a sequence WITHOUT any unmasked key is uniform over all its L keys (and kmax[b] = L for it);
  * band: key k is visible from q iff |q - k| <= w and k is unmasked.  A band query whose window holds no unmasked key has no
    contract (the kernels average what they visited): such rows, computed from the mask and w alone, are only required to be
    finite; every band case still compares at least half of its query rows, every other case all of them;
  * dropout is keyed on the mask's row pitch Lm (attn_common.h), so a packed and a padded call draw the same mask;
  * packed rows (cu): the rows that exist carry the bits of the padded call; rows of ctx past cu[B] are NOT written;
  * rope: position = row % L for any M (M need not be a multiple of L); the V columns are not touched.
Left open on purpose: 0 x NaN.  A key with probability exactly 0 (padded, out of band) that sits in a visited tile multiplies
its V row by 0.0 in the matrix core, so a NaN there spreads to that tile's queries, while a skipped tile (kmax, band) does not
read it.  The NaN case below therefore uses an unmasked key under full attention, where every query of that (sequence, head)
sees it and no other (sequence, head) may.

family -> GPU cases (test_lengths ids are [route-dtype-L]; routes: OM_OPT_ATTENTION_FAST 1 = default, 0 = fast0, 2 = chunk16, 6 = long16)
  GENERIC      f32: test_lengths[default-f32-*] (L <= 256), test_masks[f32-64-*], test_bias_dropout[generic-f32-*]
               bf16: test_lengths[fast0-bf16-*] (L <= 256, every KT), test_masks_switched[fast0-bf16-*], test_bias_dropout[generic-bf16-*]
  FWD16        test_lengths[default-bf16|f16-*] (L <= 256), test_masks[*16-64-nokmax], test_bias_dropout[fwd16-*], test_reverse
  FWD16_KMAX4  test_masks[bf16|f16-64-kmax], test_packed_rows[*-128-fwd16_kmax4-nodrop], test_reverse[bf16-64-128-*]
  FWD16C       test_lengths[default-*16-*] (L > 256), test_lengths[chunk16-*] (every L), test_masks_switched[chunk16-*],
               test_bias_dropout[fwd16c-*], test_packed_rows[*-384-fwd16c-*]
  LONG         f32: test_lengths[default-f32-*] (L > 256), test_bias_dropout[long-f32-*]
               16-bit: test_lengths[long16-*] (every L), test_lengths[fast0-bf16-*] (L > 256), test_masks_switched[long16-*],
               test_bias_dropout[long-bf16|f16-*], test_packed_rows[*-long-*]
  D32          test_lengths_d32, test_masks[*-32-*], test_bias_dropout[d32-*], test_packed_rows[*-d32-*], test_reverse[*-32-*]
  BAND16       test_band[bf16|f16-*]
  BAND32       test_band[f32-*]

Every expectation above comes from a table or a small function of this file (ROUTES, masks_expect, BD / bd_expect, REVERSE, PACKED,
SWITCHES, BAND, REFUSALS) that the CPU tests walk as well: test_forward_plan_names_what_the_gpu_cases_assert asks the planner
(csrc/attn_plan.h, through om_debug_attention_plan, no GPU) for every case and expects the family, tile count or refusal the GPU case
asserts, so the two cannot drift.  kt_of is this file's own statement of the tile rule.

The attention backward kernels are run, family by family against a float64 reference, in tests/test_attention_bwd_kernels.py, which
imports this file's shared pieces; their planner is walked here against BWD_TABLE (test_backward_plan_matches_the_table), and
the training tests of tests/test_gpu_parity.py assert through om_debug_attention_bwd_last() which of them each arm reached.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from openmatch_amd import native as N

DEV = "cuda:0"
F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
BITS_DT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
DTYPES = [F32, BF16, F16]
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}        # half an ulp, relative
FLOOR = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -24}     # subnormal spacing
U_ACC = 2.0 ** -24
# Relative error of one exp / exp2 evaluation as the kernels make it (expf in f32; __expf and v_exp_f32 in 16 bits), argument
# rounding excluded (that is the score term of the bound).  MEASURED, the only fitted constant: two-key sequences with V = [1, 0]
# so that ctx is the probability, score gaps 0 .. 16, the float32 kernels (GENERIC, LONG, D32, BAND32) against float64 on an
# MI355X, 2026-10-16: largest observed relative error of a probability 1.552e-7 (2.60 x 2^-24, the same in all four kernels);
# the constant is twice that, and test_exp_constant_still_holds repeats the measurement.  (In the 16-bit kernels the error of the
# exponential sits four orders of magnitude below the rounding of the probabilities to the storage type and cannot be resolved
# through their output.)
EXP_MEASURED = 1.56e-7
EXP_REL = 2 * EXP_MEASURED
FAM = N.ATTN_FAMILY
SENTINEL = {F32: 0x5A5A5A5A, BF16: 0x5A5A, F16: 0x5A5A}
LENGTHS = [1, 31, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257, 384, 511, 512, 1000, 1024]
SCALES = [0.125, 1.0 / math.sqrt(32.0), 0.1137]
DROP_ODD = 1000.5 / 65536.0          # p 2^16 = 1000.5: the threshold rounds (to 1001)


def kt_of(L):
    return 1 if L <= 32 else 2 if L <= 64 else 4 if L <= 128 else 6 if L <= 192 else 8


# ---------------------------------------------------------------------------------------------------------------
# dropout mask, reference, bound (pure torch / numpy: the CPU tests below check them on an emulated kernel)
# ---------------------------------------------------------------------------------------------------------------
def drop_threshold(p):
    """DropCfg (csrc/kernels.h): p resolved to 2^-16 in f32 arithmetic; (thresh, keep_scale as float64 of the same ratio)."""
    if not p > 0:
        return 0, 1.0
    t = int(np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5))
    t = min(t, 65535)
    return t, 65536.0 / (65536 - t)


def hash64(seed, idx):
    """om_hash64 (csrc/kernels.h) on numpy uint64 (wrapping)."""
    m = np.uint64(0xD6E8FEB86659FD93)
    s32 = np.uint64(32)
    with np.errstate(over="ignore"):
        x = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
        x = x ^ (x >> s32)
        x = x * m
        x = x ^ (x >> s32)
        x = x * m
        x = x ^ (x >> s32)
    return x


def drop_keep(seed, B, heads, Lm, p, b0=0):
    """keep[b, h, q, key] (bool) from the formula of csrc/attn_common.h: one hash per four keys,
    index ((b heads + h) Lm + q) ((Lm + 3) >> 2) + (key >> 2), field key & 3 kept iff >= thresh.  Lm: the mask's row pitch."""
    thresh, _ = drop_threshold(p)
    b = np.arange(b0, b0 + B, dtype=np.uint64).reshape(B, 1, 1, 1)
    h = np.arange(heads, dtype=np.uint64).reshape(1, heads, 1, 1)
    q = np.arange(Lm, dtype=np.uint64).reshape(1, 1, Lm, 1)
    key = np.arange(Lm, dtype=np.uint64).reshape(1, 1, 1, Lm)
    with np.errstate(over="ignore"):
        idx = ((b * np.uint64(heads) + h) * np.uint64(Lm) + q) * np.uint64((Lm + 3) >> 2) + (key >> np.uint64(2))
    bits = hash64(seed, idx)
    field = (bits >> (np.uint64(16) * (key & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.from_numpy(field >= np.uint64(thresh))


def visibility(mask, w=0):
    """visible[b, q, k] (bool) and contract[b, q]: padded keys excluded; a sequence without any unmasked key sees all its
    keys (uniformly: attention_reference); band: |q - k| <= w and unmasked -- a band query whose window holds no unmasked key has no contract (and, so that the
    reference stays finite, is given every key).  Computed from the mask and w alone."""
    B, L = mask.shape
    m = mask != 0
    vis = m[:, None, :].expand(B, L, L).clone()
    contract = torch.ones(B, L, dtype=torch.bool, device=mask.device)
    if w > 0 and w < L - 1:
        i = torch.arange(L, device=mask.device)
        vis &= ((i[:, None] - i[None, :]).abs() <= w)[None]
        contract = vis.any(-1)
        vis |= ~contract[:, :, None]
    else:
        vis |= ~m.any(-1)[:, None, None]
    return vis, contract


def split_qkv(qkv, B, L, heads, D):
    x = qkv.double().view(B, L, 3, heads, D).permute(2, 0, 3, 1, 4)      # [3, B, heads, L, D]
    return x[0], x[1], x[2]


def attention_reference(qkv, mask, bias, B, L, heads, D, scale, keep=None, keep_scale=1.0, w=0, vis=None):
    """float64 on the stored values.  Returns (ctx [B, L, heads * D], mag [B, L, heads, 1] = sum_k pd_k |v_k| per d -> [.., D],
    smag [B, L, heads] = max_k (scale sum_d |q_d| |k_d| + |bias|) over the visible keys, vabs = keep_scale sum_visible |v|)."""
    q, k, v = split_qkv(qkv, B, L, heads, D)
    if vis is None:
        vis, _ = visibility(mask, w)
    s = scale * (q @ k.transpose(-1, -2))
    smag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    if bias is not None:
        s = s + bias.double()[None]
        smag = smag + bias.double().abs()[None]
    vb = vis[:, None]
    s = s.masked_fill(~vb, -math.inf)
    if not 0 < w < L - 1:                                    # no unmasked key: the mask term absorbs every score -> uniform
        s = s.masked_fill(~(mask != 0).any(-1)[:, None, None, None], 0.0)
    p = torch.softmax(s, -1)
    pd = p if keep is None else p * keep.to(p.device) * keep_scale
    ctx = pd @ v
    mag = pd @ v.abs()
    smax = smag.masked_fill(~vb, 0.0).amax(-1)
    vabs = keep_scale * (vb.double().expand(B, heads, L, L) @ v.abs())
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, heads * t.shape[-1])
    return back(ctx), back(mag), smax.permute(0, 2, 1), back(vabs)


def error_bound(ctx, mag, smax, vabs, L, D, dtype):
    """Per-element bound on |kernel - float64 reference|, with A = sum_k pd_k |v_k| (mag):
      * output rounding: u_out |ctx|;
      * scores: f32 accumulation over D products, the scale (and log2 e) multiply, the bias add and the subtraction of the
        maximum, each one rounding of a value no larger than 2 smax -> ds = (D + 8) 2^-24 . 2 smax per score; to first order a
        score error ds moves a probability by at most a factor exp(2 ds) (numerator and normaliser) -> expm1(2 ds) A;
      * the exponential: EXP_REL on each term and on the normaliser -> 2 EXP_REL A;
      * PV: f32 accumulation over the L keys and one rescale per 128-key chunk -> (L + 16) 2^-24 A;
      * 16-bit kernels: every probability is rounded to the storage type before the PV MFMA, u16 sum_k p_k |v_k| = u16 A.  This
        is the same figure whether the kernel normalises before the rounding (GENERIC in bf16) or after it (FWD16, FWD16C, D32,
        BAND16, LONG: they round exp(s - max) <= 1 and divide by the f32 sum of the unrounded terms), because the rounding is
        relative.  In float16 a term below 2^-14 is rounded on the subnormal grid instead, 2^-25 absolute against a
        normaliser >= 1: 2^-25 keep_scale sum_visible |v_k|;
      * the keep scale is an f32 (2^-24, inside the PV term's slack of 16), and a subnormal floor of the output format."""
    u = U_OUT[dtype]
    ds = (D + 8) * U_ACC * 2.0 * smax                                           # [B, L, heads]
    ds = ds[..., None].expand(*ds.shape, D).reshape(ctx.shape)
    rel = torch.expm1(2.0 * ds) + 2.0 * EXP_REL + (L + 16) * U_ACC
    extra = torch.zeros_like(ctx)
    if dtype != F32:
        rel = rel + u
        if dtype == F16:
            extra = 2.0 ** -25 * vabs
    return u * ctx.abs() + (1 + u) * (rel * mag + extra) + FLOOR[dtype]


def rows_of(contract, width):
    return contract[:, :, None].expand(*contract.shape, width)


def violations(got, ref, bound, contract):
    """Elements under contract farther than `bound` from the reference or not finite; rows without a contract must be finite."""
    got = got.double()
    c = rows_of(contract, got.shape[-1])
    fin = torch.isfinite(got)
    return (c & ~(fin & ((got - ref).abs() <= bound))) | (~c & ~fin)


def make_inputs(dtype, B, L, heads, D, scale, seed, bias=False, device="cpu"):
    """Q, K so that the scaled scores spread by about 2; V of O(1) and distinct per key; bias of O(1), not symmetric, per head."""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(2.0 / (scale * math.sqrt(D)))
    x = torch.randn(B, L, 3, heads, D, generator=g)
    x[:, :, :2] *= a
    x[:, :, 2] += (torch.arange(L).float() % 7 - 3.0)[None, :, None, None] * 0.5
    qkv = x.reshape(B * L, 3 * heads * D).to(TORCH_DT[dtype]).to(device)
    pb = torch.randn(heads, L, L, generator=g).to(device) if bias else None
    return qkv, pb


MASKS11 = (128, 97, 64, 33, 32, 31, 16, 1)


def masks_eleven(L=128):
    """The patterns of test_attention_skips_masked_key_tiles_exactly (tests/test_gpu_parity.py)."""
    mask = torch.zeros(12, L, dtype=torch.long)
    for b, n in enumerate(MASKS11):
        mask[b, :n] = 1
    mask[8, :20] = 1; mask[8, 120] = 1
    mask[9, ::3] = 1
    mask[10, 40:50] = 1
    return mask


def mixed_mask(B, L):
    """row 0 full, row 1 a prefix of about 0.6 L, row 2 holes (every third key), further rows prefixes."""
    mask = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        if b % 3 == 0:
            mask[b] = 1
        elif b % 3 == 1:
            mask[b, :max(1, (6 * L) // 10)] = 1
        else:
            mask[b, ::3] = 1
    return mask


def controls(qkv, mask, bias, B, L, heads, D, scale, keep_args, w, ref, bound, contract):
    """The negative controls on the reference side; returns the names of those the bound FAILED to reject (must be empty).
    `last_key` needs a sequence with two unmasked keys or more and must be rejected inside EVERY sequence it altered (each has its
    own kmax boundary); the others must be rejected somewhere.  `bias_roll` needs a bias, `w+-1` a band, `seed+1` dropout."""
    ctl = {}
    keep, ks = (None, 1.0) if keep_args is None else (drop_keep(*keep_args), drop_threshold(keep_args[4])[1])
    R = lambda **kw: attention_reference(qkv, kw.pop("mask", mask), kw.pop("bias", bias), B, L, heads, D, kw.pop("scale", scale),
                                         kw.pop("keep", keep), ks, kw.pop("w", w))[0]
    m2, altered = mask.clone(), []
    for b in range(B):
        nz = torch.nonzero(mask[b]).flatten()
        if nz.numel() >= 2:
            m2[b, nz[-1]] = 0
            altered.append(b)
    last_key = R(mask=m2) if altered else None
    if bias is not None and L > 1:
        ctl["bias_roll"] = R(bias=torch.roll(bias, 1, dims=-1))
    if 0 < w < L - 1:
        ctl["w+1"] = R(w=w + 1)
        if w > 1:
            ctl["w-1"] = R(w=w - 1)
    if keep_args is not None:
        s, *rest = keep_args
        ctl["seed+1"] = R(keep=drop_keep(s + 1, *rest))
    if L > 1:
        ctl["scale"] = R(scale=scale * (1 + 2.0 ** -5))
    c = rows_of(contract, ref.shape[-1])
    missed = [n for n, x in ctl.items() if not bool(((x - ref).abs() > bound)[c].any())]
    if altered:
        hit = (((last_key - ref).abs() > bound) & c).flatten(1).any(-1)
        missed += [f"last_key[b={b}]" for b in altered if not bool(hit[b])]
    return missed


# ---------------------------------------------------------------------------------------------------------------
# CPU: the bound admits an honest kernel and rejects the controls; the Python dropout mask is the C one
# ---------------------------------------------------------------------------------------------------------------
def emulate_kernel(qkv, mask, bias, B, L, heads, D, scale, dtype, keep=None, keep_scale=1.0, w=0, chunk=128, norm_first=False):
    """A kernel of the shape of the ones under test, in torch: f32 scores, online softmax over key chunks with the rescale,
    probabilities rounded to the storage type before the f32 PV product, output rounded to the storage type.
    norm_first: the whole row at once, probabilities normalised BEFORE the rounding (attention_kernel)."""
    x = qkv.float().view(B, L, 3, heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32)
    if bias is not None:
        s = s + bias[None]
    s = s + torch.where(mask != 0, 0.0, -1e30).float()[:, None, None, :]          # added in f32: absorbs the score
    if 0 < w < L - 1:
        i = torch.arange(L)
        s = torch.where(((i[:, None] - i[None, :]).abs() <= w)[None, None], s, s.clamp(max=-1e30))
    r16 = (lambda t: t) if dtype == F32 else (lambda t: t.to(TORCH_DT[dtype]).float())
    kp = torch.ones_like(s) if keep is None else keep.float()
    if norm_first:
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = r16(e / e.sum(-1, keepdim=True) * kp * np.float32(keep_scale)) @ v
    else:
        m = torch.full(s.shape[:-1] + (1,), -math.inf)
        l = torch.zeros_like(m)
        o = torch.zeros(s.shape[:-1] + (D,))
        for c in range(0, L, chunk):
            sc = s[..., c:c + chunk]
            mn = torch.maximum(m, sc.amax(-1, keepdim=True))
            al = torch.exp(m - mn)
            e = torch.exp(sc - mn)
            l = l * al + e.sum(-1, keepdim=True)
            o = o * al + r16(e * kp[..., c:c + chunk]) @ v[..., c:c + chunk, :]
            m = mn
        o = o * (np.float32(keep_scale) / l)
    return o.permute(0, 2, 1, 3).reshape(B, L, heads * D).to(TORCH_DT[dtype])


CPU_CASES = [(L, D, bias, p, w) for L, D in ((77, 64), (300, 64), (130, 32))
             for bias in (False, True) for p in (0.0, 0.1) for w in (0,)] + [(300, 64, False, 0.0, 1), (300, 64, False, 0.0, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L,D,bias,p,w", CPU_CASES)
def test_bound_admits_emulated_kernel_and_rejects_controls(dtype, L, D, bias, p, w):
    B, heads, scale, seed = 4, 2, SCALES[(L + D) % 3], 1234
    qkv, pb = make_inputs(dtype, B, L, heads, D, scale, seed=L + D, bias=bias)
    mask = mixed_mask(B, L)
    mask[3] = 0                                              # a sequence without any unmasked key
    keep_args = (seed, B, heads, L, p) if p > 0 else None
    keep, ks = (drop_keep(*keep_args), drop_threshold(p)[1]) if p > 0 else (None, 1.0)
    _, contract = visibility(mask, w)
    ref, mag, smax, vabs = attention_reference(qkv, mask, pb, B, L, heads, D, scale, keep, ks, w)
    bound = error_bound(ref, mag, smax, vabs, L, D, dtype)
    for norm_first in (False, True):
        got = emulate_kernel(qkv, mask, pb, B, L, heads, D, scale, dtype, keep, ks, w, norm_first=norm_first).view(B, L, -1)
        bad = violations(got, ref, bound, contract)
        assert not bad.any(), (NAME[dtype], norm_first, int(bad.sum()))
    assert contract.float().mean() >= 0.5
    missed = controls(qkv, mask, pb, B, L, heads, D, scale, keep_args, w, ref, bound, contract)
    assert not missed, missed


def test_python_dropout_mask_equals_the_c_one():
    lib = N.lib()
    rng = np.random.default_rng(0)
    n = 0
    for (B, heads, Lm, p, seed) in ((3, 5, 128, 0.1, 7), (2, 3, 131, 0.5, 2 ** 63 + 12345), (2, 2, 257, DROP_ODD, 99), (4, 3, 6, 0.3, 1)):
        keep = drop_keep(seed, B, heads, Lm, p).numpy()
        for _ in range(1200):
            b, h, q, k = (int(rng.integers(B)), int(rng.integers(heads)), int(rng.integers(Lm)), int(rng.integers(Lm)))
            got = lib.om_debug_attn_drop_keep(seed, b, h, heads, Lm, q, k, p)
            assert got == int(keep[b, h, q, k]), (B, heads, Lm, p, b, h, q, k)
            n += 1
        # keyed on the PITCH: a sequence of 100 rows inside a mask of pitch Lm draws the mask of pitch Lm, not of pitch 100
        assert lib.om_debug_attn_drop_keep(seed, 1, 1, heads, Lm, 3, 5, p) == int(keep[1, 1, 3, 5])
        pk = 1 - drop_threshold(p)[0] / 65536.0                 # the kept fraction, within five standard deviations of its mean
        assert abs(keep.mean() - pk) < 5 * math.sqrt(pk * (1 - pk) / keep.size)
    assert n >= 4000
    assert drop_threshold(DROP_ODD)[0] == 1001 and drop_threshold(0.5) == (32768, 2.0) and drop_threshold(0.0) == (0, 1.0)
    other = drop_keep(7, 3, 5, 127, 0.1).numpy()
    assert not np.array_equal(other[:, :, :100, :100], drop_keep(7, 3, 5, 128, 0.1).numpy()[:, :, :100, :100])


def test_hooks_are_bound():
    lib = N.lib()
    for name in ("om_debug_attention_ex", "om_debug_rope", "om_debug_mask_extent", "om_debug_pack_rows", "om_debug_attention_last",
                 "om_debug_attn_drop_keep", "om_debug_attention", "om_debug_attention_plan", "om_debug_attention_bwd_plan",
                 "om_debug_attention_bwd_last"):
        assert name in N.exported_symbols() and hasattr(lib, name)
    assert lib.om_debug_attention_ex(BF16, None, None, None, None, 1, 8, 64, 1, 0.125, 0.0, 0, None, 0, None, None, 0) != 0
    assert b"null" in lib.om_last_error()
    assert lib.om_debug_attention_last() == 0                         # a call that launches nothing reads 0
    assert lib.om_debug_mask_extent(1, 1, 0, 1, None) != 0 and b"mask extent: L must be at least 1" in lib.om_last_error()
    assert lib.om_debug_pack_rows(1, 1, 8, 0, 1, 1, 1, None) != 0 and b"packed rows: rows must be at least 1" in lib.om_last_error()
    assert lib.om_abi_version() == 6
    assert sorted(FAM.values()) == list(range(1, 9))


def test_visibility_rules():
    mask = torch.tensor([[1, 1, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1]])
    vis, c = visibility(mask)
    assert c.all() and vis[1].all() and vis[0, :, :3].all() and not vis[0, :, 3:].any()
    vis, c = visibility(mask, 2)
    assert c[0].tolist() == [True] * 5 + [False] * 3 and not c[1].any()
    assert c[2].tolist() == [True, True, True, False, False, True, True, True]
    assert vis[2, 5].tolist() == [False] * 7 + [True] and vis[0, 4].tolist() == [False, False, True] + [False] * 5
    assert visibility(mask, 7)[1].all() and visibility(mask, 6)[1][0].all()


# ---------------------------------------------------------------------------------------------------------------
# CPU: the planners (csrc/attn_plan.h) through their host-only hooks, on the tables the GPU cases below take their expectations from
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def option(opt, value):
    lib = N.lib()
    old = lib.om_debug_option_value(opt)
    assert lib.om_debug_option(opt, value) == 0
    try:
        yield
    finally:
        lib.om_debug_option(opt, old)
        assert lib.om_debug_option_value(opt) == old


FAM_NAME = {v: k for k, v in FAM.items()}
BWD_FAM_NAME = {v: k for k, v in N.ATTN_BWD_FAMILY.items()}


def planned(dtype, B, L, heads, D, bias=False, p=0.0, kmax=False, cu=False, w=0):
    """What the forward entry would launch: (family name, kt), None for an empty batch, the error text for a refusal."""
    rc = N.lib().om_debug_attention_plan(dtype, B, L, heads * D, heads, int(bias), p, int(kmax), int(cu), w)
    return N.lib().om_last_error() if rc < 0 else None if rc == 0 else (FAM_NAME[rc & 0xFF], rc >> 8)


def test_forward_plan_names_what_the_gpu_cases_assert():
    n = 0
    for route, dtype in ROUTE_CASES:                                         # test_lengths, test_masks_switched
        fast, _, fam = ROUTES[route]
        with option(N.OPT_ATTENTION_FAST, fast):
            for L in LENGTHS:
                B, heads = shape_for(L)
                assert planned(dtype, B, L, heads, 64) == fam(dtype, L), (route, NAME[dtype], L)
                n += 1
            if (route, dtype) in ROUTE_CASES[3:]:
                for use_kmax in (False, True):
                    assert planned(dtype, 12, 128, 5, 64, kmax=use_kmax) == fam(dtype, 128), (route, NAME[dtype], use_kmax)
                    n += 1
    for dtype in DTYPES:
        for L in LENGTHS:                                                    # test_lengths_d32
            B, heads = shape_for(L)
            assert planned(dtype, B, L, heads, 32, kmax=L % 2 == 0) == ("d32", kt_of(L)), (NAME[dtype], L)
            n += 1
        for D in (64, 32):                                                   # test_masks
            for use_kmax in (False, True):
                assert planned(dtype, 12, 128, 5, D, kmax=use_kmax) == masks_expect(dtype, D, use_kmax), (NAME[dtype], D, use_kmax)
                n += 1
        for L, w in BAND:                                                    # test_band, and the window that reaches every key
            for use_kmax in (False, True):
                B, heads = shape_for(L)
                assert planned(dtype, B, L, heads, 64, kmax=use_kmax, w=w) == band_expect(dtype), (NAME[dtype], L, w)
                n += 1
        assert planned(dtype, 3, 300, 5, 64, kmax=True, w=299) == widest_window_expect(dtype)
        n += 1
    for family, dtype, L, D in BD:                                           # test_bias_dropout
        for bias in (False, True):
            for drop in (False, True):
                _, p, fast, kt, refused = bd_expect(family, dtype, L, D, drop)
                with option(N.OPT_ATTENTION_FAST, 1 if refused else fast):
                    got = planned(dtype, 3, L, 5, D, bias=bias, p=p)
                assert (DROP_REFUSAL in got) if refused else got == (family, kt), (family, NAME[dtype], L, bias, drop, got)
                n += 1
    for dtype, L, D in DROP_REFUSALS:                                        # test_dropout_refusals
        assert DROP_REFUSAL in planned(dtype, 1, L, 2, D, p=0.1), (NAME[dtype], L, D)
        n += 1
    for dtype, D, L, bias, p, family, kt in REVERSE:                         # test_reverse_is_bit_identical
        assert planned(dtype, 3, L, 5, D, bias=bias, p=p, kmax=True) == (family, kt), (NAME[dtype], D, L)
        n += 1
    for dtype, D, L, family, p, fast in PACKED:                              # test_packed_rows: the padded call, then the packed one
        with option(N.OPT_ATTENTION_FAST, fast):
            for cu in (False, True):
                assert planned(dtype, 6, L, 5, D, p=p, kmax=True, cu=cu) == (family, packed_kt(family, L)), (NAME[dtype], D, L, family, cu)
                n += 1
    assert PACKED_REFUSAL in planned(F32, 1, 8, 1, 64, cu=True)              # test_packed_rows_refused_in_f32
    for fast, L, family, kt in SWITCHES:                                     # test_switches
        with option(N.OPT_ATTENTION_FAST, fast):
            assert planned(BF16, 3, L, 5, 64) == (family, kt), (fast, L)
            n += 1
    for dtype, D, L, fast, family, kt in NONFINITE:
        with option(N.OPT_ATTENTION_FAST, fast):
            assert planned(dtype, 3, L, 5, D) == (family, kt), (NAME[dtype], D, L, fast)
            n += 1
    assert n == 392, n                                                       # every table case above was walked
    # refusals and the empty batch, by rule 1 of the planner
    assert planned(BF16, 0, 128, 5, 64) is None and planned(F32, -1, 5000, 5, 48) is None
    assert b"dtype must be OM_F32, OM_BF16 or OM_F16" in planned(7, 1, 128, 5, 64)
    assert b"head_dim must be 32 or 64" in planned(BF16, 1, 128, 5, 48)
    assert b"banded attention: head_dim must be 64" in planned(BF16, 1, 128, 5, 32, w=5)
    assert b"banded attention: no position bias, dropout, packed rows" in planned(BF16, 1, 128, 5, 64, bias=True, w=5)
    assert b"sequence length must be in [1,1024]" in planned(F16, 1, 1025, 5, 64) and b"sequence length must be in [1,1024]" in planned(F16, 1, 0, 5, 32)
    assert b"batch too large for one launch" in planned(F16, 2 ** 31, 8, 1, 64)
    with option(N.OPT_ATTENTION_FAST, 0):
        assert PACKED_REFUSAL in planned(BF16, 1, 8, 1, 64, cu=True)         # 64-wide bfloat16 without bit 0 has no 16-bit kernel
        assert planned(BF16, 1, 8, 1, 32, cu=True) == ("d32", 1) and planned(F16, 1, 8, 1, 64, cu=True) == ("fwd16", 1)


# The backward planner's outcome at every length of LENGTHS, one letter each:
#   b transposing-read kernel (bwd16)   g generic kernel   l tile-at-a-time pair (long)   d the 32-wide-heads kernel
#   X 32-wide heads stop at 256 tokens  P packed rows are 16-bit only  F float32 stops at 192 tokens  S beyond 256 tokens 16 bits only
#   T the tile-at-a-time pair stops at 512 tokens  C ... and does not read cu (the one refusal that used to be a silently dropped argument)
# keyed by (head width, 16-bit format?, packed rows?) and then by OM_OPT_ATTENTION_FAST; a position bias (with its gradient buffer)
# changes none of them.  LENGTHS:  1 31 32 33 64 65 128 | 129 192 | 193 256 | 257 384 511 512 | 1000 1024
BWD_TABLE = {
    (32, True, False): {f: "ddddddddddd" "XXXXXX" for f in range(4)},
    (32, True, True): {f: "ddddddddddd" "XXXXXX" for f in range(4)},
    (32, False, False): {f: "ddddddddddd" "XXXXXX" for f in range(4)},
    (32, False, True): {f: "PPPPPPPPPPP" "XXXXXX" for f in range(4)},
    (64, False, False): {f: "ggggggg" "gg" "FF" "SSSS" "TT" for f in range(4)},
    (64, False, True): {f: "PPPPPPP" "PP" "PP" "SSSS" "TT" for f in range(4)},
    (64, True, False): {0: "ggggggg" "gg" "gg" "llll" "TT", 1: "bbbbbbb" "gg" "ll" "llll" "TT",
                        2: "lllllll" "ll" "ll" "llll" "TT", 3: "lllllll" "ll" "ll" "llll" "TT"},
    (64, True, True): {0: "ggggggg" "gg" "gg" "CCCC" "TT", 1: "bbbbbbb" "gg" "gg" "CCCC" "TT",
                       2: "bbbbbbb" "gg" "gg" "CCCC" "TT", 3: "bbbbbbb" "gg" "gg" "CCCC" "TT"},
}
BWD_LETTER = {"b": "bwd16", "g": "generic", "l": "long", "d": "d32",
              "X": b"training with head_dim 32 supports sequence lengths up to 256", "P": b"packed rows: attention backward for 16-bit formats",
              "F": b"float32 training supports sequence lengths up to 192 (16-bit formats: 256)", "S": b"attention backward beyond 256 tokens: 16-bit formats",
              "T": b"attention backward (tile-at-a-time form): up to 512 tokens", "C": b"attention backward (tile-at-a-time form): no packed rows"}


def planned_bwd(dtype, B, L, heads, D, bias=False, drel=None, packed=False):
    rc = N.lib().om_debug_attention_bwd_plan(dtype, B, L, heads * D, heads, int(bias), int(bias if drel is None else drel), int(packed), int(packed))
    return N.lib().om_last_error() if rc < 0 else None if rc == 0 else (BWD_FAM_NAME[rc & 0xFF], rc >> 8)


def test_backward_plan_matches_the_table():
    n = 0
    for fast in range(4):
        with option(N.OPT_ATTENTION_FAST, fast):
            for dtype in DTYPES:
                for D in (32, 64):
                    for packed in (False, True):
                        row = BWD_TABLE[(D, dtype != F32, packed)][fast]
                        assert len(row) == len(LENGTHS)
                        for L, letter in zip(LENGTHS, row):
                            for bias in (False, True):
                                got, want = planned_bwd(dtype, 4, L, 3, D, bias=bias, packed=packed), BWD_LETTER[letter]
                                ok = (want in got) if isinstance(want, bytes) else got == (want, 4 if want == "long" else kt_of(L))
                                assert isinstance(got, type(want) if isinstance(want, bytes) else tuple) and ok, (fast, NAME[dtype], D, packed, L, bias, got)
                                n += 1
    assert n == 4 * 3 * 2 * 2 * len(LENGTHS) * 2
    assert planned_bwd(BF16, 0, 128, 3, 64) is None
    assert b"head_dim must be 32 or 64" in planned_bwd(BF16, 1, 128, 3, 48)
    assert b"a position bias needs its gradient buffer" in planned_bwd(BF16, 1, 128, 3, 32, bias=True, drel=False)
    assert planned_bwd(BF16, 1, 128, 3, 64, bias=True, drel=False) == ("generic", 4)       # 64-wide: the generic kernel adds the bias and skips its gradient


def test_plan_hooks_leave_the_last_launch_words_alone():
    lib = N.lib()
    assert lib.om_debug_attention_ex(BF16, None, None, None, None, 1, 8, 64, 1, 0.125, 0.0, 0, None, 0, None, None, 0) != 0      # refused: last = 0
    before = (lib.om_debug_attention_last(), lib.om_debug_attention_bwd_last())
    assert planned(BF16, 3, 128, 5, 64) == ("fwd16", 4) and planned_bwd(BF16, 3, 128, 5, 64) == ("bwd16", 4)
    assert b"sequence length" in planned(BF16, 3, 2000, 5, 64)
    assert (lib.om_debug_attention_last(), lib.om_debug_attention_bwd_last()) == before and before[0] == 0


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def bits(t, dtype):
    return t.view(BITS_DT[dtype])


def launch(dtype, qkv, ctx, mask, bias, B, L, H, heads, scale, p=0.0, seed=0, reverse=0, kmax=None, cu=None, w=0):
    rc = N.lib().om_debug_attention_ex(dtype, N.ptr(qkv), N.ptr(ctx), N.ptr(mask), N.ptr(bias), B, L, H, heads, scale, p, seed,
                                       N.stream_ptr(), reverse, N.ptr(kmax), N.ptr(cu), w)
    torch.cuda.synchronize()
    return rc


def mask_extent(mask):
    B, L = mask.shape
    kmax = torch.full((B,), -7, dtype=torch.int32, device=mask.device)
    N.check(N.lib().om_debug_mask_extent(N.ptr(mask), B, L, N.ptr(kmax), N.stream_ptr()))
    torch.cuda.synchronize()
    return kmax


def pack_rows(kmax, L, rows):
    B = kmax.numel()
    cu = torch.full((B + 2,), -7, dtype=torch.int32, device=kmax.device)
    cls = torch.full((B,), -7, dtype=torch.int32, device=kmax.device)
    row_map = torch.full((rows,), -7, dtype=torch.int32, device=kmax.device)
    N.check(N.lib().om_debug_pack_rows(N.ptr(kmax), B, L, rows, N.ptr(cu), N.ptr(cls), N.ptr(row_map), N.stream_ptr()))
    torch.cuda.synchronize()
    return cu, cls, row_map


GUARD = 3


def new_ctx(rows, H, dtype):
    return torch.full((rows + GUARD, H), SENTINEL[dtype], dtype=BITS_DT[dtype], device=DEV).view(TORCH_DT[dtype])


def untouched(t, dtype):
    """every element still holds the sentinel"""
    return bool((bits(t, dtype) == bits(new_ctx(1, 1, dtype), dtype)[0, 0]).all())


def run_case(dtype, B, L, heads, D, scale, mask, family, kt, bias=False, p=0.0, seed=0, use_kmax=False, w=0, reverse=0, tag=0):
    """One launch against the reference: family, bound, controls, guard memory.  Returns ctx [B * L, H]."""
    H = heads * D
    qkv, pb = make_inputs(dtype, B, L, heads, D, scale, seed=1000 + 13 * L + D + tag, bias=bias, device=DEV)
    mask = mask.to(DEV)
    qkv0, mask0, pb0 = qkv.clone(), mask.clone(), None if pb is None else pb.clone()
    kmax = mask_extent(mask) if use_kmax else None
    ctx = new_ctx(B * L, H, dtype)
    rc = launch(dtype, qkv, ctx, mask, pb, B, L, H, heads, scale, p, seed, reverse, kmax, None, w)
    assert rc == 0, N.lib().om_last_error()
    last = N.lib().om_debug_attention_last()
    assert (last & 0xFF, last >> 8) == (FAM[family], kt), (family, kt, last & 0xFF, last >> 8)
    # guard memory
    assert torch.equal(bits(qkv, dtype), bits(qkv0, dtype)) and torch.equal(mask, mask0)
    assert pb is None or torch.equal(pb.view(torch.int32), pb0.view(torch.int32))
    assert untouched(ctx[B * L:], dtype), "rows after ctx were written"
    keep_args = (seed, B, heads, L, p) if p > 0 else None
    keep, ks = (drop_keep(*keep_args).to(DEV), drop_threshold(p)[1]) if p > 0 else (None, 1.0)
    _, contract = visibility(mask, w)
    ref, mag, smax, vabs = attention_reference(qkv, mask, pb, B, L, heads, D, scale, keep, ks, w)
    bound = error_bound(ref, mag, smax, vabs, L, D, dtype)
    got = ctx[:B * L].view(B, L, H)
    bad = violations(got, ref, bound, contract)
    ratio = ((got.double() - ref).abs() / bound)[rows_of(contract, H)]
    print(f"attn {family}/{kt} {NAME[dtype]} B={B} L={L} heads={heads} D={D} scale={scale:.4f} bias={bias} p={p:.4f} kmax={use_kmax} w={w}: "
          f"max err/bound {ratio.max().item():.3f}, compared rows {contract.float().mean().item():.2f}")
    assert not bad.any(), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), ratio.max().item())
    assert contract.float().mean() >= (0.5 if 0 < w < L - 1 else 1.0)
    missed = controls(qkv, mask, pb, B, L, heads, D, scale, keep_args, w, ref, bound, contract)
    assert not missed, missed
    return ctx[:B * L]


def shape_for(L):
    return (3, 5) if L <= 512 else (2, 3)


# how a 64-wide case is routed: name -> (OM_OPT_ATTENTION_FAST, dtypes, (family, kt) of a length).  `default` is the shipped value 1.
def _fam_default(dtype, L):
    if dtype == F32:
        return ("generic", kt_of(L)) if L <= 256 else ("long", 4)
    return ("fwd16", kt_of(L)) if L <= 256 else ("fwd16c", 4)


ROUTES = {
    "default": (1, DTYPES, _fam_default),
    "fast0": (0, [BF16], lambda dtype, L: ("generic", kt_of(L)) if L <= 256 else ("long", 4)),      # attention_kernel<bf16_t>, then LONG
    "chunk16": (2, [BF16, F16], lambda dtype, L: ("fwd16c", 4)),                                     # bit 1: FWD16C at every length
    "long16": (6, [BF16, F16], lambda dtype, L: ("long", 4)),                                        # bits 1 + 2: LONG at every length
}
ROUTE_CASES = [(r, d) for r, (_, dts, _) in ROUTES.items() for d in dts]
ROUTE_IDS = [f"{r}-{NAME[d]}" for r, d in ROUTE_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("route,dtype", ROUTE_CASES, ids=ROUTE_IDS)
def test_lengths(route, dtype, L):
    """Every 64-wide family x every dtype it serves at every length edge (no kmax).  default: GENERIC / LONG in f32, FWD16 / FWD16C in
    16 bits; fast0: attention_kernel<bf16_t> (every KT) and LONG in bf16; chunk16 / long16: FWD16C and LONG in both 16-bit formats
    from 1 token to 1 024 (tail chunks, up to eight rescales)."""
    fast, _, fam = ROUTES[route]
    B, heads = shape_for(L)
    family, kt = fam(dtype, L)
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, B, L, heads, 64, SCALES[LENGTHS.index(L) % 3], mixed_mask(B, L), family, kt, tag=fast)


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_lengths_d32(dtype, L):
    B, heads = shape_for(L)
    run_case(dtype, B, L, heads, 32, SCALES[(LENGTHS.index(L) + 1) % 3], mixed_mask(B, L), "d32", kt_of(L), use_kmax=L % 2 == 0)


def masks_expect(dtype, D, use_kmax):
    """(family, kt) of a test_masks case: 128 tokens at the shipped switch."""
    if D == 32:
        return "d32", 4
    if dtype == F32:
        return "generic", 4
    return ("fwd16_kmax4" if use_kmax else "fwd16"), 4


@pytest.mark.gpu
@pytest.mark.parametrize("use_kmax", [False, True], ids=["nokmax", "kmax"])
@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_masks(dtype, D, use_kmax):
    """The eleven mask patterns (and a sequence without any key: uniform over all L), with kmax and without."""
    run_case(dtype, 12, 128, 5, D, 0.125 if D == 64 else SCALES[1], masks_eleven(), *masks_expect(dtype, D, use_kmax), use_kmax=use_kmax)


@pytest.mark.gpu
@pytest.mark.parametrize("use_kmax", [False, True], ids=["nokmax", "kmax"])
@pytest.mark.parametrize("route,dtype", ROUTE_CASES[3:], ids=ROUTE_IDS[3:])
def test_masks_switched(route, dtype, use_kmax):
    """The same eleven patterns on the 64-wide kernels behind OM_OPT_ATTENTION_FAST: attention_kernel<bf16_t>, FWD16C and LONG in 16 bits."""
    fast, _, fam = ROUTES[route]
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, 12, 128, 5, 64, 0.125, masks_eleven(), *fam(dtype, 128), use_kmax=use_kmax, tag=fast)


@pytest.mark.gpu
def test_mask_extent_and_pack_rows_exact():
    mask = masks_eleven().to(DEV)
    B, L = mask.shape
    kmax = mask_extent(mask)
    want = [int(torch.nonzero(mask[b]).max()) + 1 if mask[b].any() else L for b in range(B)]
    assert want == [128, 97, 64, 33, 32, 31, 16, 1, 121, 127, 50, 128] and kmax.tolist() == want
    total = sum(want)
    for rows in (total + 5, total, 300, 1):
        cu, cls, row_map = pack_rows(kmax, L, rows)
        run, e_cu, e_cls, e_map = 0, [], [], [-1] * rows
        for b in range(B):
            e_cu.append(min(run, rows)); e_cls.append(run if run < rows else rows - 1)
            for k in range(want[b]):
                if run + k < rows:
                    e_map[run + k] = b * L + k
            run += want[b]
        e_cu += [min(total, rows), total]                     # cu[B] clamped to `rows`, cu[B + 1] the true count
        assert cu.tolist() == e_cu and cls.tolist() == e_cls and row_map.tolist() == e_map, rows


BD = [("fwd16", BF16, 100, 64), ("fwd16", F16, 100, 64), ("fwd16", F16, 200, 64), ("fwd16c", BF16, 300, 64), ("fwd16c", F16, 512, 64),
      ("d32", F32, 100, 32), ("d32", BF16, 100, 32), ("d32", F16, 300, 32), ("generic", F32, 100, 64), ("generic", BF16, 100, 64),
      ("long", F32, 300, 64), ("long", BF16, 300, 64), ("long", F16, 300, 64)]


DROP_REFUSAL = b"attention with dropout: up to 512 tokens in the 16-bit formats (float32: 256)"
PACKED_REFUSAL = b"packed rows: the 16-bit attention kernels"


def bd_expect(family, dtype, L, D, drop):
    """(index in BD, dropout rate, OM_OPT_ATTENTION_FAST, kt, refused) of a test_bias_dropout case."""
    i = BD.index((family, dtype, L, D))
    p = (0.1, 0.5, DROP_ODD)[i % 3] if drop else 0.0
    fast = 0 if (family == "generic" and dtype == BF16) else 4 if (family == "long" and dtype != F32) else 1
    kt = kt_of(L) if family in ("fwd16", "generic", "d32") else 4
    return i, p, fast, kt, family == "long" and dtype == F32 and drop


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("family,dtype,L,D", BD, ids=[f"{f}-{NAME[d]}-{L}" for f, d, L, _ in BD])
def test_bias_dropout(family, dtype, L, D, bias, drop):
    B, heads = 3, 5
    i, p, fast, kt, refused = bd_expect(family, dtype, L, D, drop)
    mask = mixed_mask(B, L).to(DEV)
    if refused:                                             # float32 dropout stops at 256 tokens
        qkv, pb = make_inputs(dtype, B, L, heads, D, 0.125, seed=1, bias=bias, device=DEV)
        ctx = new_ctx(B * L, heads * D, dtype)
        assert launch(dtype, qkv, ctx, mask, pb, B, L, heads * D, heads, 0.125, p, 5) != 0
        assert DROP_REFUSAL in N.lib().om_last_error()
        assert N.lib().om_debug_attention_last() == 0
        assert untouched(ctx, dtype)
        return
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, B, L, heads, D, SCALES[i % 3], mask, family, kt, bias=bias, p=p, seed=0xC0FFEE + i, tag=i)


DROP_REFUSALS = [(BF16, 600, 64), (F16, 513, 64), (F32, 257, 32), (BF16, 1024, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,L,D", DROP_REFUSALS)
def test_dropout_refusals(dtype, L, D):
    B, heads = 1, 2
    qkv, _ = make_inputs(dtype, B, L, heads, D, 0.125, seed=2, device=DEV)
    mask = torch.ones(B, L, dtype=torch.long, device=DEV)
    ctx = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, ctx, mask, None, B, L, heads * D, heads, 0.125, 0.1, 5) != 0
    assert DROP_REFUSAL in N.lib().om_last_error()
    assert N.lib().om_debug_attention_last() == 0
    assert untouched(ctx, dtype)


REVERSE = [(BF16, 64, 128, False, 0.0, "fwd16_kmax4", 4), (F16, 64, 200, False, 0.0, "fwd16", 8), (BF16, 32, 128, False, 0.0, "d32", 4),
           (F32, 32, 100, False, 0.0, "d32", 4), (BF16, 64, 100, True, 0.0, "fwd16", 4), (F16, 64, 100, False, 0.1, "fwd16", 4),
           (F16, 64, 64, True, 0.5, "fwd16", 2), (BF16, 32, 100, True, 0.1, "d32", 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,L,bias,p,family,kt", REVERSE,
                         ids=[f"{NAME[d]}-{D}-{L}-{'bias' if b else 'nobias'}-{'drop' if p else 'nodrop'}" for d, D, L, b, p, _, _ in REVERSE])
def test_reverse_is_bit_identical(dtype, D, L, bias, p, family, kt):
    """reverse = 1 (the kernels that walk the batch rows last to first) gives the bits of reverse = 0, in the bias and dropout
    bodies too."""
    B, heads, H = 3, 5, 5 * D
    qkv, pb = make_inputs(dtype, B, L, heads, D, 0.125, seed=3, bias=bias, device=DEV)
    mask = mixed_mask(B, L).to(DEV)
    kmax = mask_extent(mask)
    out = []
    for rev in (0, 1):
        ctx = new_ctx(B * L, H, dtype)
        assert launch(dtype, qkv, ctx, mask, pb, B, L, H, heads, 0.125, p=p, seed=77, reverse=rev, kmax=kmax) == 0
        last = N.lib().om_debug_attention_last()
        assert (last & 0xFF, last >> 8) == (FAM[family], kt), (last & 0xFF, last >> 8)
        out.append(bits(ctx, dtype).clone())
    assert torch.equal(out[0], out[1])
    assert not bool((out[0][:B * L] == bits(new_ctx(1, 1, dtype), dtype)[0, 0]).all(-1).any())


PACKED = [(BF16, 64, 128, "fwd16_kmax4", 0.0, 1), (F16, 64, 128, "fwd16_kmax4", 0.0, 1), (BF16, 64, 200, "fwd16", 0.0, 1),
          (BF16, 64, 384, "fwd16c", 0.0, 1), (F16, 64, 384, "fwd16c", 0.0, 1), (F16, 32, 128, "d32", 0.0, 1), (BF16, 32, 384, "d32", 0.0, 1),
          (BF16, 64, 128, "fwd16", 0.1, 1), (F16, 64, 384, "fwd16c", 0.5, 1), (BF16, 32, 128, "d32", 0.1, 1),
          (BF16, 64, 384, "long", 0.0, 4), (F16, 64, 384, "long", 0.5, 4), (F16, 64, 128, "long", 0.0, 6), (BF16, 64, 1000, "long", 0.0, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,L,family,p,fast", PACKED, ids=[f"{NAME[d]}-{D}-{L}-{f}-{'drop' if p else 'nodrop'}" for d, D, L, f, p, _ in PACKED])
def test_packed_rows(dtype, D, L, family, p, fast):
    with option(N.OPT_ATTENTION_FAST, fast):
        _packed_rows(dtype, D, L, family, p)


def packed_kt(family, L):
    return 4 if family in ("fwd16c", "long") else kt_of(L)


def _packed_rows(dtype, D, L, family, p):
    """cu: the rows that exist carry the bits of the padded call (which itself meets the bound), at 256 tokens or fewer and
    beyond, with dropout too (the hash is keyed on the mask's pitch, not on the sequence's own length).  Rows of the packed ctx
    past cu[B] (the pad rows up to `rows`) are NOT written: the kernels return for an empty sequence and store only rows below
    their sequence's length, so the sentinel must survive there."""
    B, heads, H = 6, 5, 5 * D
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate((L, 1, L // 2 + 1, 33, 0, 97)):
        mask[b, :n] = 1
    mask[4, 0] = 1; mask[4, 5] = 1                         # holes inside a packed sequence: rows 0 .. 5 exist
    kt = packed_kt(family, L)
    padded = run_case(dtype, B, L, heads, D, 0.125, mask, family, kt, use_kmax=True, tag=77, p=p, seed=4242)
    qkv, _ = make_inputs(dtype, B, L, heads, D, 0.125, seed=1000 + 13 * L + D + 77, device=DEV)
    mask = mask.to(DEV)
    kmax = mask_extent(mask)
    rows = int(kmax.sum()) + 7
    cu, cls, row_map = pack_rows(kmax, L, rows)
    total = int(cu[B])
    src = row_map[:total].long()
    qp = torch.zeros(rows, 3 * H, dtype=TORCH_DT[dtype], device=DEV)
    qp[:total] = qkv[src]
    ctx = new_ctx(rows, H, dtype)
    assert launch(dtype, qp, ctx, mask, None, B, L, H, heads, 0.125, p=p, seed=4242, kmax=kmax, cu=cu) == 0
    last = N.lib().om_debug_attention_last()
    assert (last & 0xFF, last >> 8) == (FAM[family], kt)
    assert torch.equal(bits(ctx, dtype)[:total], bits(padded, dtype)[src])
    assert untouched(ctx[total:], dtype)


@pytest.mark.gpu
def test_packed_rows_refused_in_f32():
    qkv, _ = make_inputs(F32, 1, 8, 1, 64, 0.125, seed=1, device=DEV)
    mask = torch.ones(1, 8, dtype=torch.long, device=DEV)
    cu = torch.tensor([0, 8, 8], dtype=torch.int32, device=DEV)
    assert launch(F32, qkv, new_ctx(8, 64, F32), mask, None, 1, 8, 64, 1, 0.125, cu=cu) != 0
    assert PACKED_REFUSAL in N.lib().om_last_error()


SWITCHES = [(0, 100, "generic", 4), (1, 100, "fwd16", 4), (2, 100, "fwd16c", 4), (4, 300, "long", 4),
            (6, 100, "long", 4), (0, 300, "long", 4), (1, 300, "fwd16c", 4), (0, 256, "generic", 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("fast,L,family,kt", SWITCHES)
def test_switches(fast, L, family, kt):
    """OM_OPT_ATTENTION_FAST 0 / 1 / bit 1 / bit 2 in bf16 reach the family the header names; the old value comes back."""
    before = N.lib().om_debug_option_value(N.OPT_ATTENTION_FAST)
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(BF16, 3, L, 5, 64, 0.125, mixed_mask(3, L), family, kt, tag=fast)
    assert N.lib().om_debug_option_value(N.OPT_ATTENTION_FAST) == before


BAND = [(300, 1), (300, 63), (300, 64), (300, 65), (300, 127), (300, 128), (300, 298), (129, 64), (257, 127), (1000, 64), (1024, 128), (385, 2)]


def band_expect(dtype):
    return ("band32" if dtype == F32 else "band16"), 4


def widest_window_expect(dtype):
    """w = L - 1 at 300 tokens reaches every key: full attention at the shipped switch"""
    return ("long" if dtype == F32 else "fwd16c"), 4


@pytest.mark.gpu
@pytest.mark.parametrize("use_kmax", [False, True], ids=["nokmax", "kmax"])
@pytest.mark.parametrize("L,w", BAND)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_band(dtype, L, w, use_kmax):
    """Both band kernels: w around the 64 / 128 edges, L across 128-query blocks, w = L - 2 (still banded), kmax clipping."""
    B, heads = (3, 5) if L <= 512 else (2, 3)
    mask = mixed_mask(B, L)
    mask[1, :] = 0; mask[1, :max(1, (7 * L) // 10)] = 1        # a prefix: kmax clips inside the band of the last query blocks
    run_case(dtype, B, L, heads, 64, 0.125 if w != 65 else SCALES[2], mask, *band_expect(dtype), use_kmax=use_kmax, w=w)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_band_widest_window_is_full_attention(dtype):
    L = 300
    run_case(dtype, 3, L, 5, 64, 0.125, mixed_mask(3, L), *widest_window_expect(dtype), w=L - 1, use_kmax=True)


def rope_table(theta, L):
    """The f32 table recipe of csrc/attention_causal.hip (omk_rope), written out again: inv_freq_i = 1 / f32(theta ** (2 i / 64)),
    angle = f32(inv_freq_i * pos), cos / sin of that f32 angle rounded to f32."""
    i = np.arange(32)
    e = (2 * i).astype(np.float32) / np.float32(64.0)
    inv = np.float32(1.0) / np.power(np.float64(np.float32(theta)), e.astype(np.float64)).astype(np.float32)
    ang = (inv[None, :] * np.arange(L, dtype=np.float32)[:, None]).astype(np.float32)
    return (torch.from_numpy(np.cos(ang.astype(np.float64)).astype(np.float32)).double(),
            torch.from_numpy(np.sin(ang.astype(np.float64)).astype(np.float32)).double())


@pytest.mark.gpu
@pytest.mark.parametrize("M,L", [(5, 1), (2 * 1024, 1024), (2 * 37 + 3, 37)])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_rope(dtype, M, L):
    """q' = q cos + rotate_half(q) sin over pairs (i, i + 32), position = row % L -- also when M is not a multiple of L (the
    code defines it so: pinned).  Two thetas in one process (the table cache); V bit-unchanged; rows after M untouched."""
    heads, H = 3, 192
    g = torch.Generator().manual_seed(M + L)
    x0 = torch.randn(M + GUARD, 3 * H, generator=g).to(TORCH_DT[dtype]).to(DEV)
    for theta in (10000.0, 160000.0, 10000.0):
        x = x0.clone()
        N.check(N.lib().om_debug_rope(dtype, N.ptr(x), M, L, H, theta, N.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(bits(x, dtype)[:, 2 * H:], bits(x0, dtype)[:, 2 * H:]) and torch.equal(bits(x, dtype)[M:], bits(x0, dtype)[M:])
        cos, sin = (t.to(DEV) for t in rope_table(theta, L))
        pos = torch.arange(M, device=DEV) % L
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]                       # [M, 1, 32]
        v = x0[:M, :2 * H].double().view(M, 2 * heads, 64)
        a, b = v[..., :32], v[..., 32:]
        ref = torch.cat([a * c - b * s, b * c + a * s], -1)
        mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
        bound = U_OUT[dtype] * ref.abs() + 3 * U_ACC * mag + FLOOR[dtype]       # two products and a sum in f32, one output rounding
        got = x[:M, :2 * H].double().view(M, 2 * heads, 64)
        assert bool(((got - ref).abs() <= bound).all()), ((got - ref).abs() / bound).max().item()
        if L > 1:                                                               # controls: the other theta, positions off by one
            c2, s2 = (t.to(DEV)[pos][:, None, :] for t in rope_table(170000.0 - theta, L))
            assert bool(((torch.cat([a * c2 - b * s2, b * c2 + a * s2], -1) - ref).abs() > bound).any())
            pr = (pos + 1) % L
            assert bool(((torch.cat([a * cos[pr][:, None] - b * sin[pr][:, None], b * cos[pr][:, None] + a * sin[pr][:, None]], -1) - ref).abs() > bound).any())
    assert N.lib().om_debug_rope(dtype, N.ptr(x), M, 1025, H, 10000.0, N.stream_ptr()) != 0
    assert b"rotary positions: sequence length must be in [1,1024]" in N.lib().om_last_error()


NONFINITE = [(F32, 64, 100, 1, "generic", 4), (BF16, 64, 100, 1, "fwd16", 4), (F16, 64, 300, 1, "fwd16c", 4), (F32, 64, 300, 1, "long", 4),
             (BF16, 32, 100, 1, "d32", 4), (F32, 32, 300, 1, "d32", 8), (BF16, 64, 100, 0, "generic", 4), (F16, 64, 300, 4, "long", 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,L,fast,family,kt", NONFINITE, ids=[f"{f}-{NAME[d]}-{D}-{L}" for d, D, L, _, f, _ in NONFINITE])
def test_non_finite_inputs_stay_where_they_belong(dtype, D, L, fast, family, kt):
    """A NaN in the V row of one unmasked key reaches every query of that (sequence, head) -- each sees the key with non-zero
    probability -- and no other.  An infinite Q row (every score of that query is +-inf) poisons that query alone: the other
    queries of the same (sequence, head), which share its workgroup, its key tiles and its wave, keep the bits of the clean run."""
    B, heads, H = 3, 5, 5 * D
    qkv, _ = make_inputs(dtype, B, L, heads, D, 0.125, seed=9, device=DEV)
    mask = torch.ones(B, L, dtype=torch.long, device=DEV)
    b, h, j = 1, 3, L // 2
    with option(N.OPT_ATTENTION_FAST, fast):
        clean = new_ctx(B * L, H, dtype)
        assert launch(dtype, qkv, clean, mask, None, B, L, H, heads, 0.125) == 0
        last = N.lib().om_debug_attention_last()
        assert (last & 0xFF, last >> 8) == (FAM[family], kt), (last & 0xFF, last >> 8)
        assert torch.isfinite(clean[:B * L].float()).all()
        for col0, val in ((2 * H, math.nan), (0, math.inf)):
            x = qkv.clone()
            x[b * L + j, col0 + h * D: col0 + (h + 1) * D] = val
            ctx = new_ctx(B * L, H, dtype)
            assert launch(dtype, x, ctx, mask, None, B, L, H, heads, 0.125) == 0
            assert N.lib().om_debug_attention_last() == last
            hit = torch.zeros(B, L, heads, D, dtype=torch.bool, device=DEV)
            if math.isnan(val):
                hit[b, :, h] = True                  # every query of the (sequence, head)
            else:
                hit[b, j, h] = True                  # the one query
            hit = hit.view(B * L, H)
            assert torch.equal(bits(ctx, dtype)[:B * L][~hit], bits(clean, dtype)[:B * L][~hit])
            assert not torch.isfinite(ctx[:B * L].float()[hit]).any()
            if math.isnan(val):
                assert torch.isnan(ctx[:B * L].float()[hit]).all()


@pytest.mark.gpu
def test_exp_constant_still_holds():
    """Re-measures EXP_MEASURED the way it was obtained: two-key sequences with V = [1, 0] (ctx is the probability of key 0), exact
    scores (q . k = g, scale 1/8) with gaps up to 16 either way, the four float32 kernels against float64.  Prints the largest
    relative error and asserts it has not grown past the recorded figure (a compiler or library change that moves it shows here,
    not as a vague failure of the bound)."""
    worst = {}
    for name, D, L, B, w, fam in (("generic", 64, 2, 2048, 0, ("generic", 1)), ("d32", 32, 2, 2048, 0, ("d32", 1)), ("long", 64, 257, 16, 0, ("long", 4)),
                                  ("d32 chunked", 32, 300, 16, 0, ("d32", 8)), ("band32", 64, 130, 1024, 1, ("band32", 4))):
        g = torch.Generator().manual_seed(L + D)
        gaps = ((torch.rand(B, L, generator=g) * 256 - 128) * 8).round() / 8
        x = torch.zeros(B, L, 3, D)
        x[:, :, 0, 0] = gaps                                   # q = (g, 0, ...)
        x[:, 0, 1, 0] = 1.0                                    # k_0 = (1, 0, ...), k_1 = 0: scores (g / 8, 0)
        x[:, 0, 2, :] = 1.0                                    # v_0 = 1, v_1 = 0
        qkv = x.reshape(B * L, 3 * D).to(DEV)
        mask = torch.zeros(B, L, dtype=torch.long, device=DEV)
        mask[:, :2] = 1
        ctx = new_ctx(B * L, D, F32)
        assert launch(F32, qkv, ctx, mask, None, B, L, D, 1, 0.125, w=w) == 0
        last = N.lib().om_debug_attention_last()
        assert (last & 0xFF, last >> 8) == (FAM[fam[0]], fam[1])
        nq = L if w == 0 else 2                                # band, w = 1: queries 0 and 1 see exactly keys 0 and 1
        p0 = torch.sigmoid(gaps.double().to(DEV) * 0.125)[:, :nq, None]
        rel = (ctx[:B * L].double().view(B, L, D)[:, :nq] - p0).abs() / p0
        worst[name] = rel.max().item()
    print("exp path, largest relative error of a probability:", {k: f"{v:.4e}" for k, v in worst.items()})
    assert max(worst.values()) <= EXP_MEASURED, worst
