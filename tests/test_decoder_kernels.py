"""The T5 decoder position (csrc/decoder.hip) kernel by kernel and as a whole train step.  Each of its six kernels is called alone through
an om_debug_dec_* hook (pointers, dtype and ranges checked, every argument forwarded to the launcher that om_t5_decoder_step and the
train pair call) and compared with a float64 -- or bit-exact -- statement of what it computes, on the exact stored (rounded) inputs,
element by element, no element excluded, sentinel guards behind every written tensor.  The train forward / backward pair is compared
with torch float64 autograd of a plain-torch decoder position that is fed the kernels' OWN dropout masks, computed in Python.

References
    cross forward   per (b, h), d = 64, NO 1/sqrt(d):  s_l = q_h . K_h[l] + (mask[b, l] ? 0 : -3.4028235e38),  p = softmax_l(s),
                    pd_l = keep_l p_l keep_scale,  ctx = sum_l pd_l V_h[l],  keep_l = dropout_keep(seed, (b heads + h) L + l) through
                    keep_of.  In f32 the additive constant absorbs the score, so a masked key scores exactly -3.4028235e38: its
                    probability is exactly 0 whenever the row has an unmasked key, and a row WITHOUT one is uniform over all L keys
                    (Hugging Face's convention); its scores still carry their gradient (p = 1 / L in ds below).
    cross backward  the kernel's header comment:  dV[l] = pd_l dctx,  dpd_l = dctx . V[l],  dp = keep keep_scale dpd,
                    ds_l = p_l (dp_l - sum_j p_j dp_j),  dK[l] = ds_l q,  dq = sum_l ds_l K[l].
                    test_reference_is_the_autograd_of_the_forward checks them against torch float64 autograd of the forward reference.
    final           out = x rsqrt(mean(x^2) + eps) g in f32
    head drop       v[b, h, :] keep_scale as ONE f32 product rounded once to the storage type, or +0; one draw per (b, h), key b heads + h
    start, cast     the f32 value rounded once to nearest even (cast: +-inf, values past the float16 range, float16 subnormals too)
    dec_site        seed + 0x9E3779B97F4A7C15 (16 layer + site + 1) + 0x5DEECE66D mod 2^64; om_debug_dec_site pins the Python port

Bounds (u = 2^-24, U / FLOOR the half ulp and the subnormal spacing of the storage type; every kernel computes in f32 whatever the
storage type, so only the ONE output rounding depends on it):
    score     a 64-term fmaf chain: 65 u sum_d |q_d k_d|; the subtraction of the maximum rounds a value below 2 smax:
              ds = 67 u smax, smax the largest sum_d |q_d k_d| over the row's unmasked keys.  A probability moves by at most
              expm1(2 ds) (numerator and normaliser), plus the exponential twice (2 EXP_REL), the normaliser's sum (L + 3) u in any
              order, and the reciprocal, the keep-scale and the final product (3 u):  eP, relative.
    ctx       sum_l pd_l V[l] as a ceil(L / 4) + 3 term sum per lane (four row groups of fmaf chains, three additions):
              (eP + (ceil(L / 4) + 3) u) sum_l pd_l |V_l|, then U |ctx| + FLOOR.
    dpd, dp   a 64-term chain and the keep scale: eD = 66 u of A_l = keep keep_scale sum_d |dctx_d V_ld|.
    dot       an L-term sum in any order of p_l dp_l: E_dot = (eP + eD + (L + 4) u) sum_l p_l A_l.
    ds        p (dp - dot): (eP + 2 u) |ds_l| + p_l (eD A_l + E_dot) =: E_ds -- the cancellation enters as an absolute term.
    dK, dV    one product each: E_ds |q_d| + u |dK|;  (eP + 2 u) |dV|;  then U and FLOOR.
    dq        sum_l ds_l K[l], ceil(L / 4) + 3 terms per lane: sum_l E_ds |K_ld| + (ceil(L / 4) + 3) u sum_l |ds_l K_ld|, then U, FLOOR.
    final     (RSQRT_REL + (H + 3) u + 3 u) |out|: rsqrtf, the H-term sum of squares, three products.
EXP_REL is the attention file's constant (measured on other kernels).  The measurement was repeated through om_debug_dec_cross in
float32 (two keys, V rows [1, 0, ...] and [0, ...], score gaps 0 .. 16 either way, so that ctx[0] is the probability): see DEC_EXP_MEASURED
below; test_exp_constant_holds_for_dec_cross asserts it stays within EXP_MEASURED x 1.001.  No bound is fitted to a 16-bit kernel.

kernel -> cases
    dec_cross_kernel       test_cross_lengths, test_cross_masks, test_cross_dropout, test_cross_deterministic,
                           test_cross_controls_on_device, test_exp_constant_holds_for_dec_cross; the train-step tests
    dec_cross_bwd_kernel   the same five cross cases (forward and backward share inputs, seed and reference); the train-step tests
    dec_final_kernel       test_final; om_t5_decoder_step in test_train_step_matches_float64_autograd and test_step_serves_an_ungated_gelu_stack
    dec_head_drop_kernel   test_head_drop_is_the_port; the train-step tests with p > 0
    dec_start_kernel       test_start;  dec_cast_kernel: test_cast; both in test_train_step_16bit
    dec_site               test_dec_site_port_equals_the_library (CPU)
    the three entry points test_entry_point_refusals

Negative controls (test_bound_admits_emulated_kernel_and_rejects_controls, CPU: the float64 reference with one thing wrong against
the true reference and its bound; an emulation of both kernels in float32 in the kernels' order -- fmaf chains, wave partials, four
row groups -- must pass).  Worst |error| / bound of each control over dq, dK, dV and ctx, at the CPU case where it is smallest
(f32 / bf16), recorded 2026-10-20:
    bwd_seed+1             the backward draws its mask from seed + 1                        3.6e36 / 3.6e36 (a zero row against FLOOR)
    key_l_alone            the dropout key is l, without the block offset (b heads + h) L   1.1e4  / 3.8e3
    no_keep_scale          dp = keep dpd, without the keep scale                            204    / 3.8
    drop_pd_only           the mask on pd but not on dp                                     1.6e3  / 9.3e2
    renorm_after_drop      pd renormalised to sum 1 after the dropout                       129    / 3.8
    no_mask                the attention mask ignored                                       2.7e38 / 2.7e38
    swap_kv                the K and V halves of kv exchanged                               1.4e7  / 4.1e5
    scaled                 scores times 1 / sqrt(64)                                        2.3e6  / 6.8e4
    keys_ge_256_dropped    only the first 256 keys (one key per thread)                     7.0e3  / 2.5e2
    h_is_block_div_heads   h = block / heads instead of block % heads                       7.7e7  / 2.3e6
    masked_row_nan         a row without an unmasked key uniform over zero keys: NaN         inf    / inf
    minus_zero_rows        dK / dV of a masked key stored as -0: p_l = +0 times a negative (dp - dot) or q_d.  A bit comparison, no
                           ratio: this is what dec_cross_bwd_kernel did before this file existed.  test_cross_masks[f32] and
                           test_cross_masks[bf16] fail on it ('dK of a masked key is not +0'; float16 happened to store +0); the
                           kernel now adds +0 to both products before the store.
The GPU cases repeat 'seed + 1' and 'no keep scale' on the device's own output (test_cross_controls_on_device: 4.3e3 / 125 / 827
bounds away in f32 / bf16 / f16 for the missing keep scale at p = 0.5).
One sign of zero is NOT pinned: dec_head_drop_kernel in float16 returns +0 for a kept -0 (bfloat16 and float32 return -0, the f32
product); the inputs of test_head_drop_is_the_port hold no -0.

The whole step (test_train_step_*): a float64 decoder position in plain torch (RMSNorm, v / o self-attention over the one position,
cross-attention, ReLU or gated gelu_new feed-forward) that takes the seven dropout masks as inputs: dec_site(seed, layer, site) and
keep_of with the keys the code uses -- element b N + n for the omk_dropout and GEMM-epilogue sites (0 start, 3 cross output, 4
feed-forward output, 5 feed-forward inner, 6 self-attention output, (n_layers, 1) the final output), b heads + h for the head drop
(site 1), (b heads + h) L + l for the cross probabilities (site 2).  float32 tolerances are the project's own for this path
(test_t5_encoder_decoder_training_matches_hf_autograd): out within 1e-4 max(1, |out|max), every gradient relative L2 < 2e-3 or
max error < 1e-7.  16-bit limits are those of test_t5_decoder_position_over_long_passages_matches_hf: whole-gradient relative L2
< 1e-1 (bf16), < 1e-2 (f16) with every f16 tensor < 5e-2.  Measured on an MI355X, 2026-10-20:
    float32   out max error 2.3e-6 .. 4.5e-6 (|out|max 2.9 .. 5.3); worst gradient relative L2 2.9e-6 .. 3.8e-6 (L0.ca_q_w, L0.ca_ln_g)
    bfloat16  out cosine 0.999972; whole-gradient relative L2 1.65e-2; worst tensor 2.34e-2 (L1.ca_q_w)
    float16   out cosine 1.000000; whole-gradient relative L2 2.05e-3; worst tensor 2.98e-3 (L1.ca_q_w)
The limits are not tightened to these figures.  om_t5_decoder_step against the train forward at p = 0 in float32: bit-identical,
ReLU and gated (the fused gelu_new x gate epilogue and the final RMSNorm of the step give the bits of the train path's separate
kernels at these shapes); the test asserts equal bits.
om_t5_decoder_step does NOT make dec_check's gated / ffn1g_w check: with act = tanh-GELU and ffn1g_w NULL it serves an UNGATED
gelu_new stack (x += Wo gelu_new(Wi n)); training refuses that combination.  test_step_serves_an_ungated_gelu_stack pins it as it is.
"""
import ctypes as C
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import DROP_ODD, EXP_MEASURED, EXP_REL, drop_threshold
from tests.test_gemm_epilogues import assert_within, guards_ok, sync
from tests.test_gemm_kernels import BF16, DEV, F16, F32, FLOOR, NAME, SENTINEL, TORCH_DT, U_ACC, U_OUT, Buf, _bits
from tests.test_row_kernels import FAKE, RSQRT_REL, keep_of

# EXP_REL (2 x EXP_MEASURED of tests/test_attention_kernels.py) re-measured through om_debug_dec_cross in float32 on an MI355X,
# 2026-10-20: largest relative error of a probability 1.3248e-7 (2.22 x 2^-24), below EXP_MEASURED = 1.56e-7, so the attention
# file's constant is used as it is; test_exp_constant_holds_for_dec_cross repeats the measurement.
DEC_EXP_MEASURED = 1.33e-7

u = U_ACC
ALL_DT = [F32, BF16, F16]
GUARD = 3                    # sentinel rows behind every written tensor
GUARD_F = 7.5
D = 64
MASK64 = (1 << 64) - 1
NEG = torch.finfo(torch.float32).min       # the f32 that -3.4028235e38f is
EPS = 1e-6


def stream():
    return N.stream_ptr(torch.device(DEV))


def dec_site(seed, layer, site):
    """dec_site of csrc/decoder.hip (uint64 wrap-around)"""
    return (seed + 0x9E3779B97F4A7C15 * (16 * layer + site + 1) + 0x5DEECE66D) & MASK64


# ---------------------------------------------------------------------------------------------------------------
# cross attention: reference, bound, emulation, controls (pure torch, device-agnostic)
# ---------------------------------------------------------------------------------------------------------------
def cross_keep(seed, B, heads, L, p, offset=True):
    """(keep [B, heads, L] bool, keep scale as the kernel's f32): key (b heads + h) L + l; offset False is the control 'l alone'"""
    if drop_threshold(p)[0] == 0:
        return torch.ones(B, heads, L, dtype=torch.bool), 1.0
    blk = torch.arange(B * heads, dtype=torch.int64)[:, None]
    keys = (blk * L if offset else blk * 0) + torch.arange(L, dtype=torch.int64)[None, :]
    keep, scale = keep_of(seed, keys, p)
    return keep.view(B, heads, L), float(scale)


def split_heads(q, kv, dctx, B, L, heads, dt=torch.float64):
    qh = q.to(dt).reshape(B, heads, D)
    kvv = kv.to(dt).reshape(B, L, 2, heads, D)
    K, V = kvv[:, :, 0].permute(0, 2, 1, 3), kvv[:, :, 1].permute(0, 2, 1, 3)        # [B, heads, L, D]
    return qh, K, V, dctx.to(dt).reshape(B, heads, D)


CONTROLS = ("bwd_seed+1", "key_l_alone", "no_keep_scale", "drop_pd_only", "renorm_after_drop", "no_mask", "swap_kv", "scaled",
            "keys_ge_256_dropped", "h_is_block_div_heads", "masked_row_nan")


def cross_reference(q, kv, mask, dctx, B, L, heads, keep=None, ks=1.0, ctl=None, keep_bwd=None):
    """float64 on the stored values: ctx [B, heads, D], dq, dK / dV [B, heads, L, D] and the magnitudes cross_bounds needs.  keep: the
    forward's mask, keep_bwd: the backward's (None: the same).  ctl names a wrong kernel (CONTROLS)."""
    qh, K, V, dO = split_heads(q, kv, dctx, B, L, heads)
    if ctl == "swap_kv":
        K, V = V, K
    dev = qh.device
    s = torch.einsum("bhd,bhld->bhl", qh, K)
    smag = torch.einsum("bhd,bhld->bhl", qh.abs(), K.abs())
    if ctl == "scaled":
        s = s / 8.0
    m = (mask.to(dev) != 0)[:, None, :].expand(B, heads, L)
    if ctl == "no_mask":
        m = torch.ones_like(m)
    anyk = m.any(-1, keepdim=True)
    s = torch.where(anyk, s.masked_fill(~m, -math.inf), torch.zeros_like(s))          # no unmasked key: uniform over all L
    if ctl == "keys_ge_256_dropped":
        s = s.clone()
        s[..., 256:] = -math.inf
    P = torch.softmax(s, -1)
    if ctl == "masked_row_nan":
        P = torch.where(anyk, P, torch.full_like(P, math.nan))
    kf = torch.ones_like(P) if keep is None else keep.to(dev).double()
    kb = kf if keep_bwd is None else keep_bwd.to(dev).double()
    Pd = P * kf * ks
    if ctl == "renorm_after_drop":
        Pd = P * kf / (P * kf).sum(-1, keepdim=True)
    ctx = torch.einsum("bhl,bhld->bhd", Pd, V)
    Pdb = P * kb * ks
    Mdp = kb if ctl == "no_keep_scale" else torch.ones_like(P) if ctl == "drop_pd_only" else kb * ks
    dP = Mdp * torch.einsum("bhd,bhld->bhl", dO, V)
    A = kb * ks * torch.einsum("bhd,bhld->bhl", dO.abs(), V.abs())
    dot = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - dot)
    R = NS(ctx=ctx, dq=torch.einsum("bhl,bhld->bhd", dS, K), dK=dS[..., None] * qh[:, :, None, :], dV=Pdb[..., None] * dO[:, :, None, :],
           P=P, Pd=Pd, dS=dS, A=A, Ga=(P * A).sum(-1, keepdim=True), q=qh, K=K, V=V, dO=dO,
           smax=(smag * (m & anyk)).amax(-1, keepdim=True), AV=torch.einsum("bhl,bhld->bhd", Pd, V.abs()))
    if ctl == "h_is_block_div_heads":                 # block (b, h) computes head (b heads + h) / heads = b (folded into range)
        pick = (torch.arange(B, device=dev) % heads)[:, None].expand(B, heads)
        bi = torch.arange(B, device=dev)[:, None].expand(B, heads)
        R.ctx, R.dq, R.dK, R.dV = R.ctx[bi, pick], R.dq[bi, pick], R.dK[bi, pick], R.dV[bi, pick]
    return R


def cross_bounds(R, L, dtype):
    """(ctx, dq, dK, dV) bounds of the docstring"""
    U, fl = U_OUT[dtype], FLOOR[dtype]
    eP = torch.expm1(2.0 * 67 * u * R.smax) + 2 * EXP_REL + (L + 3) * u + 3 * u                  # [B, heads, 1]
    nacc = ((L + 3) // 4 + 3) * u
    eD = 66 * u
    Edot = (eP + eD + (L + 4) * u) * R.Ga
    Eds = (eP + 2 * u) * R.dS.abs() + R.P * (eD * R.A + Edot)
    out = lambda v, raw: U * v.abs() + (1 + U) * raw + fl
    return (out(R.ctx, (eP + nacc) * R.AV),
            out(R.dq, torch.einsum("bhl,bhld->bhd", Eds, R.K.abs()) + nacc * torch.einsum("bhl,bhld->bhd", R.dS.abs(), R.K.abs())),
            out(R.dK, Eds[..., None] * R.q.abs()[:, :, None, :] + u * R.dK.abs()),
            out(R.dV, (eP[..., None] + 2 * u) * R.dV.abs()))


def _fma(x, y, acc):
    """fmaf on float32 tensors: the product of two floats is exact in float64"""
    return (x.double() * y.double() + acc.double()).float()


def _block_sum(x):
    """x [B, heads, L] f32: per-thread partial over l = tid + 256 j, a wave sum over 64 lanes, (w0 + w1) + (w2 + w3)"""
    B, heads, L = x.shape
    pad = torch.zeros(B, heads, 1024, dtype=torch.float32)
    pad[..., :L] = x
    t = pad.view(B, heads, 4, 4, 64)                                  # [j, wave, lane]
    per = t[:, :, 0]
    for j in range(1, 4):
        per = per + t[:, :, j]
    w = per.sum(-1)
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3]))[..., None]


def _group_sum(w, X):
    """sum_l w[l] X[l] as the kernels form it: four row groups l = grp + 4 i, an fmaf chain each, (g0 + g1) + (g2 + g3)"""
    B, heads, L, _ = X.shape
    n4 = (L + 3) // 4
    wp = torch.zeros(B, heads, n4 * 4, dtype=torch.float32)
    Xp = torch.zeros(B, heads, n4 * 4, D, dtype=torch.float32)
    wp[..., :L], Xp[:, :, :L] = w, X
    wp, Xp = wp.view(B, heads, n4, 4), Xp.view(B, heads, n4, 4, D)
    acc = torch.zeros(B, heads, 4, D, dtype=torch.float32)
    for i in range(n4):
        acc = _fma(wp[:, :, i, :, None], Xp[:, :, i], acc)
    return (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])


def emulate_cross(q, kv, mask, dctx, B, L, heads, dtype, keep, ks):
    """Both cross kernels in float32 in their own order, outputs rounded once to the storage type (returned as float64)"""
    f32 = torch.float32
    qh, K, V, dO = split_heads(q, kv, dctx, B, L, heads, f32)
    a, dd = torch.zeros(B, heads, L, dtype=f32), torch.zeros(B, heads, L, dtype=f32)
    for d in range(D):
        a = _fma(qh[:, :, None, d], K[..., d], a)
        dd = _fma(dO[:, :, None, d], V[..., d], dd)
    sc = a + torch.where(mask != 0, 0.0, NEG).to(f32)[:, None, :]
    e = torch.exp(sc - sc.amax(-1, keepdim=True))
    inv = 1.0 / _block_sum(e)
    kf = keep.to(f32)
    ks32 = torch.tensor(ks, dtype=f32)
    rnd = lambda t: t.to(TORCH_DT[dtype]).double()
    ctx = _group_sum(kf * (e * ks32), V) * inv
    pl = e * inv
    pd, dp = kf * (pl * ks32), kf * (dd * ks32)
    dot = _block_sum(pl * dp)
    ds = pl * (dp - dot)
    return rnd(ctx), rnd(_group_sum(ds, K)), rnd(ds[..., None] * qh[:, :, None, :]), rnd(pd[..., None] * dO[:, :, None, :])


def cross_inputs(dtype, B, L, heads, seed, qscale=0.3, device="cpu"):
    """q, kv, dctx in the storage type: scores of a few units either way (no 1/sqrt(d) comes later), gradients over five binades"""
    g = torch.Generator().manual_seed(seed)
    H = heads * D
    q = torch.randn(B, H, generator=g) * qscale
    kv = torch.randn(B * L, 2 * H, generator=g)
    dctx = torch.randn(B, H, generator=g) * (2.0 ** ((torch.arange(H) % 5).float() - 2.0))[None, :]
    td = TORCH_DT[dtype]
    return q.to(td).to(device), kv.to(td).to(device), dctx.to(td).to(device)


def ragged_mask(B, L, seed=0):
    """row 0 keeps a single key (the middle one), the others a prefix of at least one key, the last row everything"""
    g = torch.Generator().manual_seed(1000 + L + seed)
    mask = torch.zeros(B, L, dtype=torch.int64)
    mask[0, L // 2] = 1
    for b in range(1, B):
        n = L if b == B - 1 else int(torch.randint(1, L + 1, (1,), generator=g))
        mask[b, :n] = 1
    return mask


def control_outputs(c, name):
    """(ctx, dq, dK, dV) of the named wrong kernel in float64, or None where the control is an identity at this case"""
    ref = lambda **kw: cross_reference(c.q, c.kv, c.mask, c.dctx, c.B, c.L, c.heads, kw.pop("keep", c.keep), c.ks, **kw)
    dropping = c.thresh > 0
    if name == "bwd_seed+1":
        x = ref(keep_bwd=cross_keep(c.seed + 1, c.B, c.heads, c.L, c.p)[0]) if dropping else None
    elif name == "key_l_alone":
        k2 = cross_keep(c.seed, c.B, c.heads, c.L, c.p, offset=False)[0]
        x = ref(keep=k2) if dropping else None
    elif name in ("no_keep_scale", "drop_pd_only", "renorm_after_drop"):
        x = ref(ctl=name) if dropping else None
    elif name == "no_mask":
        x = ref(ctl=name) if bool((c.mask == 0).any()) else None
    elif name == "keys_ge_256_dropped":
        x = ref(ctl=name) if c.L > 256 else None
    elif name == "h_is_block_div_heads":
        x = ref(ctl=name) if c.heads > 1 and c.B > 1 else None
    elif name == "masked_row_nan":
        x = ref(ctl=name) if bool((c.mask == 0).all(-1).any()) else None
    else:
        x = ref(ctl=name)
    return None if x is None else (x.ctx, x.dq, x.dK, x.dV)


def worst_ratio(got, c):
    """largest |got - reference| / bound over ctx, dq, dK, dV; anything non-finite counts as infinitely far"""
    worst = 0.0
    for g, r, b in zip(got, (c.R.ctx, c.R.dq, c.R.dK, c.R.dV), c.bounds):
        ratio = (g.double() - r).abs() / b
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
        worst = max(worst, float(ratio.max()))
    return worst


def prepare(dtype, B, L, heads, mask, p=0.0, seed=0, tag=0, qscale=0.3, device="cpu"):
    c = NS(dtype=dtype, B=B, L=L, heads=heads, H=heads * D, p=p, seed=seed, mask=mask.to(device), thresh=drop_threshold(p)[0])
    c.q, c.kv, c.dctx = cross_inputs(dtype, B, L, heads, 7000 + 13 * L + heads + tag, qscale, device)
    c.keep, c.ks = cross_keep(seed, B, heads, L, p)
    c.R = cross_reference(c.q, c.kv, c.mask, c.dctx, B, L, heads, c.keep, c.ks)
    c.bounds = cross_bounds(c.R, L, dtype)
    return c


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("p", [0.0, 0.3], ids=["nodrop", "drop"])
def test_reference_is_the_autograd_of_the_forward(p, ragged):
    """dq, dK, dV of cross_reference against torch float64 autograd of the forward written out independently.  The row without an
    unmasked key enters as s - stop_gradient(s): value 0 (uniform), gradient passed on -- what a kernel whose f32 mask constant
    absorbs the score computes."""
    B, L, heads = 3, 37, 2
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, heads * D, generator=g, dtype=torch.float64).requires_grad_()
    kv = torch.randn(B * L, 2 * heads * D, generator=g, dtype=torch.float64).requires_grad_()
    dctx = torch.randn(B, heads * D, generator=g, dtype=torch.float64)
    mask = ragged_mask(B, L) if ragged else torch.ones(B, L, dtype=torch.int64)
    if ragged:
        mask[1] = 0
    keep, ks = cross_keep(11, B, heads, L, p)
    qh, K, V, _ = split_heads(q, kv, dctx, B, L, heads)
    s = (qh[:, :, None, :] * K).sum(-1)
    m = (mask != 0)[:, None, :]
    s = torch.where(m.any(-1, keepdim=True), s, s - s.detach()).masked_fill(~m & m.any(-1, keepdim=True), -math.inf)
    pd = torch.softmax(s, -1) * keep.double() * ks
    ctx = (pd[..., None] * V).sum(2)
    (ctx.reshape(B, -1) * dctx).sum().backward()
    R = cross_reference(q.detach(), kv.detach(), mask, dctx, B, L, heads, keep, ks)
    assert torch.allclose(R.ctx, ctx.detach(), rtol=0, atol=1e-13)
    gq, gK, gV, _ = split_heads(q.grad, kv.grad, dctx, B, L, heads)
    for got, want in ((R.dq, gq), (R.dK, gK), (R.dV, gV)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12), (got - want).abs().max().item()
    if ragged:
        padded = ((mask == 0) & (mask != 0).any(-1, keepdim=True))[:, None, :, None].expand_as(R.dK)
        assert bool((R.dK[padded] == 0).all()) and bool((R.dV[padded] == 0).all()) and bool((R.dK[1] != 0).all())
        if not p:                                     # the fully masked row: the plain mean of V
            assert torch.allclose(R.ctx[1], R.V[1].mean(1), rtol=0, atol=1e-13)


CPU_CASES = [(3, 70, 2, 0.1, "ragged"), (3, 300, 2, DROP_ODD, "full_row_masked"), (2, 257, 3, 0.5, "ragged"), (3, 5, 2, 0.5, "ragged")]
CONTROL_RATIOS = {}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
def test_bound_admits_emulated_kernel_and_rejects_controls(dtype):
    """the emulated kernels pass; every control is rejected at every case where it is not an identity, and every control is live at
    one case at least.  pytest -s prints the table of the docstring."""
    seen = {}
    for B, L, heads, p, kind in CPU_CASES:
        mask = ragged_mask(B, L)
        if kind == "full_row_masked":
            mask[1] = 0
        c = prepare(dtype, B, L, heads, mask, p, seed=0x1234 + L, tag=1)
        em = worst_ratio(emulate_cross(c.q, c.kv, c.mask, c.dctx, B, L, heads, dtype, c.keep, c.ks), c)
        print(f"emulated {NAME[dtype]} B{B} L{L} heads{heads} p{p:.4f}: worst error / bound {em:.3f}")
        assert em <= 1.0, (B, L, heads, p, em)
        for name in CONTROLS:
            out = control_outputs(c, name)
            if out is None:
                continue
            r = worst_ratio(out, c)
            seen[name] = min(seen.get(name, math.inf), r)
            assert r > 1.0, (name, B, L, heads, p, r)
    assert sorted(seen) == sorted(CONTROLS), sorted(set(CONTROLS) - set(seen))
    CONTROL_RATIOS[dtype] = seen
    for name in CONTROLS:
        print(f"control {name:24s} {NAME[dtype]}: {seen[name]:.3g}")


def test_dec_site_port_equals_the_library():
    lib = N.lib()
    for seed in (0, 1, 1 << 63, MASK64):
        for layer in range(25):
            for site in range(7):
                assert lib.om_debug_dec_site(seed, layer, site) == dec_site(seed, layer, site), (seed, layer, site)
    assert dec_site(MASK64, 0, 0) < MASK64            # wrapped


HOOKS = ["om_debug_dec_cross", "om_debug_dec_cross_bwd", "om_debug_dec_final", "om_debug_dec_head_drop", "om_debug_dec_start",
         "om_debug_dec_cast", "om_debug_dec_site"]


def test_hooks_are_bound_and_check_arguments():
    """every refusal comes before any launch and reads no pointer (made-up addresses)"""
    lib = N.lib()
    for name in HOOKS:
        assert name in N.exported_symbols() and hasattr(lib, name)
    p, z, s = C.c_void_p(FAKE), C.c_void_p(0), C.c_void_p(0)
    err = lib.om_last_error
    cross = lambda dt=F32, q=p, kv=p, m=p, o=p, L=8, H=128, heads=2, dp=0.0: lib.om_debug_dec_cross(dt, q, kv, m, o, 2, L, H, heads, dp, 1, s)
    bwd = lambda dt=F32, q=p, kv=p, m=p, d=p, dq=p, dkv=p, L=8, H=128, heads=2, dp=0.0: \
        lib.om_debug_dec_cross_bwd(dt, q, kv, m, d, dq, dkv, 2, L, H, heads, dp, 1, s)
    for fn, name, ptrs in ((cross, b"om_debug_dec_cross", ("q", "kv", "m", "o")), (bwd, b"om_debug_dec_cross_bwd", ("q", "kv", "m", "d", "dq", "dkv"))):
        for k in ptrs:
            assert fn(**{k: z}) != 0 and b"null argument" in err() and name in err(), k
        assert fn(dt=7) != 0 and b"dtype must be" in err()
        for L in (0, -1, 1025):
            assert fn(L=L) != 0 and b"sequence length must be in [1,1024]" in err(), L
        for H, heads in ((128, 3), (64, 2), (96, 1), (128, 0)):
            assert fn(H=H, heads=heads) != 0 and b"H must be heads * 64" in err(), (H, heads)
        for dp in (1.0, -0.1, 1.5, math.nan):
            assert fn(dp=dp) != 0 and b"drop_p must be in [0, 1)" in err(), dp
    assert lib.om_debug_dec_cross(F32, p, p, p, p, 0, 8, 128, 2, 0.0, 1, s) == 0                       # no rows: no launch
    assert lib.om_debug_dec_cross_bwd(F32, p, p, p, p, p, p, 0, 8, 128, 2, 0.0, 1, s) == 0
    for args in ((z, p, p), (p, z, p), (p, p, z)):
        assert lib.om_debug_dec_final(F32, *args, 2, 64, EPS, s) != 0 and b"om_debug_dec_final: null argument" in err()
    assert lib.om_debug_dec_final(9, p, p, p, 2, 64, EPS, s) != 0 and b"dtype must be" in err()
    assert lib.om_debug_dec_final(F32, p, p, p, 2, 0, EPS, s) != 0 and b"H must be at least 1" in err()
    assert lib.om_debug_dec_final(F32, p, p, p, 0, 64, EPS, s) == 0
    assert lib.om_debug_dec_head_drop(F32, z, 2, 64, 0.1, 1, s) != 0 and b"om_debug_dec_head_drop: null argument" in err()
    assert lib.om_debug_dec_head_drop(-1, p, 2, 64, 0.1, 1, s) != 0 and b"dtype must be" in err()
    for H in (0, 32, 96):
        assert lib.om_debug_dec_head_drop(F32, p, 2, H, 0.1, 1, s) != 0 and b"H must be heads * 64" in err()
    for dp in (1.0, -0.5):
        assert lib.om_debug_dec_head_drop(F32, p, 2, 64, dp, 1, s) != 0 and b"drop_p must be in [0, 1)" in err()
    assert lib.om_debug_dec_head_drop(F32, p, 0, 64, 0.1, 1, s) == 0
    for args in ((z, p), (p, z)):
        assert lib.om_debug_dec_start(F32, *args, 2, 64, s) != 0 and b"om_debug_dec_start: null argument" in err()
        assert lib.om_debug_dec_cast(F32, *args, 16, s) != 0 and b"om_debug_dec_cast: null argument" in err()
    assert lib.om_debug_dec_start(3, p, p, 2, 64, s) != 0 and b"dtype must be" in err()
    assert lib.om_debug_dec_start(F32, p, p, 2, 0, s) != 0 and b"H must be at least 1" in err()
    assert lib.om_debug_dec_cast(3, p, p, 16, s) != 0 and b"dtype must be" in err()
    assert lib.om_debug_dec_start(F32, p, p, 0, 64, s) == 0 and lib.om_debug_dec_cast(F32, p, p, 0, s) == 0


# ---------------------------------------------------------------------------------------------------------------
# GPU: the cross kernels
# ---------------------------------------------------------------------------------------------------------------
def run_cross(c, p=None, seed=None, seed_bwd=None, label=""):
    """both kernels on the inputs of c: (ctx, dq, dK, dV) as [B, heads, (L,) D] views of guarded buffers; guards and inputs checked"""
    lib = N.lib()
    p = c.p if p is None else p
    seed = c.seed if seed is None else seed
    B, L, H, heads, dt = c.B, c.L, c.H, c.heads, c.dtype
    ctx, dq, dkv = Buf(dt, B, H, H, post=GUARD), Buf(dt, B, H, H, post=GUARD), Buf(dt, B * L, 2 * H, 2 * H, post=GUARD)
    snaps = [b.snapshot() for b in (ctx, dq, dkv)]
    ins = [t.clone() for t in (c.q, c.kv, c.dctx, c.mask)]
    with torch.cuda.device(DEV):
        rc = lib.om_debug_dec_cross(dt, N.ptr(c.q), N.ptr(c.kv), N.ptr(c.mask), ctx.ptr(), B, L, H, heads, p, seed, stream())
        rc2 = lib.om_debug_dec_cross_bwd(dt, N.ptr(c.q), N.ptr(c.kv), N.ptr(c.mask), N.ptr(c.dctx), dq.ptr(), dkv.ptr(), B, L, H, heads, p,
                                         seed if seed_bwd is None else seed_bwd, stream())
    sync()
    assert rc == 0 and rc2 == 0, lib.om_last_error()
    guards_ok(label, (ctx, snaps[0]), (dq, snaps[1]), (dkv, snaps[2]))
    for a, b in zip((c.q, c.kv, c.dctx, c.mask), ins):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{label}: input modified"
    sent = SENTINEL[dt] - (1 << 32 if dt == F32 and SENTINEL[dt] >= 1 << 31 else 0)
    for name, b in (("ctx", ctx), ("dq", dq), ("dkv", dkv)):
        assert not bool((_bits(b.window) == sent).any()), f"{label}: {name} keeps a sentinel inside (an element was not written)"
    kvv = dkv.window.view(B, L, 2, heads, D)
    return ctx.window.view(B, heads, D), dq.window.view(B, heads, D), kvv[:, :, 0].permute(0, 2, 1, 3), kvv[:, :, 1].permute(0, 2, 1, 3)


def hold(c, got, label):
    for name, g, r, b in zip(("ctx", "dq", "dK", "dV"), got, (c.R.ctx, c.R.dq, c.R.dK, c.R.dV), c.bounds):
        assert_within(f"{label} {name}", g, r, b, c.dtype)


LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cross_lengths(dtype, L):
    """B = 2, heads = 3 (odd on purpose: b and h of a block must come apart the right way), ragged masks, p = 0"""
    c = prepare(dtype, 2, L, 3, ragged_mask(2, L), device=DEV)
    label = f"dec_cross/{NAME[dtype]}/L{L}"
    got = run_cross(c, label=label)
    hold(c, got, label)
    if L >= 2:                                        # row 0 keeps one key: ctx is that V row, every other dkv row of it is zero
        assert torch.equal(_bits(got[0][0].contiguous()), _bits(c.kv.view(2, L, 2, 3, D)[0, L // 2, 1].contiguous()))


def mask_cases(L):
    full = torch.ones(L, dtype=torch.int64)
    holes = full.clone()
    holes[L // 3:L // 3 + 17] = 0
    holes[L - 9:L - 2] = 0
    last = torch.zeros(L, dtype=torch.int64)
    last[L - 1] = 1
    none = torch.zeros(L, dtype=torch.int64)
    return torch.stack([full, holes, last, none, holes.flip(0)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cross_masks(dtype):
    """L = 130, heads = 2: all kept, holes, only the last key, one fully masked row beside normal ones"""
    L, heads = 130, 2
    mask = mask_cases(L)
    B = mask.shape[0]
    c = prepare(dtype, B, L, heads, mask, tag=2, device=DEV)
    label = f"dec_cross masks/{NAME[dtype]}"
    ctx, dq, dK, dV = got = run_cross(c, label=label)            # run_cross: guards (nothing past B L rows), no sentinel inside
    hold(c, got, label)
    m = c.mask != 0
    padded = (~m & m.any(-1, keepdim=True))[:, None, :, None].expand(B, heads, L, D)
    assert bool(padded.any())
    for name, t in (("dK", dK), ("dV", dV)):
        assert bool((_bits(t.contiguous())[padded] == 0).all()), f"{label}: {name} of a masked key is not +0"
    # the fully masked row: the plain mean of V (f32 sum of L terms and the division: (L + 4) u, one output rounding), gradients non-zero
    V = c.R.V[3]
    mean = V.mean(1)
    bound = U_OUT[dtype] * mean.abs() + (1 + U_OUT[dtype]) * (L + 4) * u * V.abs().mean(1) + FLOOR[dtype]
    assert_within(f"{label} mean of V", ctx[3], mean, bound, dtype)
    assert bool((dK[3].double().abs().amax(-1) > 0).all()) and bool((dV[3].double().abs().amax(-1) > 0).all())


DROP_P = [0.1, DROP_ODD, 0.5]
DROP_L = [5, 65, 257, 1023]


@pytest.mark.gpu
@pytest.mark.parametrize("L", DROP_L)
@pytest.mark.parametrize("p", DROP_P, ids=lambda p: f"p{p:.4f}")
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cross_dropout(dtype, p, L):
    """heads = 2, B = 3, L % 4 != 0: a hash group of four keys straddles two (b, h) blocks.  Forward and backward share the seed and
    are both held to the bound; the exactly-zero dV rows among the unmasked keys are the ported mask's dropped set."""
    B, heads, seed = 3, 2, 0xC0FFEE00 + L
    mask = ragged_mask(B, L, seed=1)
    mask[0] = 1
    c = prepare(dtype, B, L, heads, mask, p, seed, tag=3, qscale=0.1, device=DEV)
    assert L % 4 != 0
    label = f"dec_cross drop/{NAME[dtype]}/p{p:.4f}/L{L}"
    ctx, dq, dK, dV = got = run_cross(c, label=label)
    hold(c, got, label)
    m = (c.mask != 0)[:, None, :].expand(B, heads, L)
    zero_rows = (dV.double().abs().amax(-1) == 0)
    dropped = ~c.keep.to(DEV)
    assert bool((c.R.dV.abs().amax(-1)[m & ~dropped] > 4 * FLOOR[dtype]).all())           # the inputs: a kept row cannot round to zero
    assert torch.equal(zero_rows & m, dropped & m), f"{label}: the zero dV rows are not the port's dropped keys"
    assert L == 5 or (bool(dropped.any()) and bool((~dropped).any()))
    if p == 0.1:                                      # p 2^16 < 0.5: threshold 0, the p = 0 arithmetic
        tiny = run_cross(c, p=2.0 ** -18, label=label + " tiny p")
        none = run_cross(c, p=0.0, label=label + " p 0")
        assert drop_threshold(2.0 ** -18)[0] == 0
        for a, b in zip(tiny, none):
            assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{label}: p = 2^-18 differs from p = 0"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cross_deterministic(dtype):
    c = prepare(dtype, 3, 300, 2, ragged_mask(3, 300), 0.1, seed=77, tag=4, device=DEV)
    a = run_cross(c, label="first")
    b = run_cross(c, label="second")
    for x, y in zip(a, b):
        assert torch.equal(_bits(x.contiguous()), _bits(y.contiguous()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cross_controls_on_device(dtype):
    """the device's own output is far from the controls' references: a backward under seed + 1 (run that way on the device, too)
    and a dp without the keep scale"""
    B, L, heads, p, seed = 3, 257, 2, 0.5, 4242
    c = prepare(dtype, B, L, heads, ragged_mask(B, L), p, seed, tag=5, qscale=0.1, device=DEV)
    got = run_cross(c, label="controls")
    hold(c, got, "controls")
    for name in ("bwd_seed+1", "no_keep_scale"):
        ctl = control_outputs(c, name)
        far = max(float(((g.double() - r).abs() / b).max()) for g, r, b in zip(got, ctl, c.bounds))
        print(f"device output against control {name}: {far:.3g} bounds away")
        assert far > 1.0, name
    wrong = run_cross(c, seed_bwd=seed + 1, label="bwd seed + 1")
    assert worst_ratio(wrong, c) > 1.0
    Rw = cross_reference(c.q, c.kv, c.mask, c.dctx, B, L, heads, c.keep, c.ks, keep_bwd=cross_keep(seed + 1, B, heads, L, p)[0])
    for g, r, b in zip(wrong, (Rw.ctx, Rw.dq, Rw.dK, Rw.dV), cross_bounds(Rw, L, dtype)):
        assert bool(((g.double() - r).abs() <= b).all())


def measure_exp():
    """two keys, V rows [1, 0, ...] and [0, ...]: ctx[0] is the probability of key 0; exact scores q . k = gap, gaps -16 .. 16"""
    B = 4096
    gaps = (torch.arange(B, dtype=torch.float64) / (B - 1) * 32 - 16) * 8
    gaps = (gaps.round() / 8).float()
    q = torch.zeros(B, D)
    q[:, 0] = gaps
    kv = torch.zeros(B, 2, 2, D)
    kv[:, 0, 0, 0] = 1.0                              # k_0 = (1, 0, ...), k_1 = 0: scores (gap, 0)
    kv[:, 0, 1, 0] = 1.0                              # v_0 = (1, 0, ...), v_1 = 0
    q, kv = q.to(DEV), kv.reshape(B * 2, 2 * D).to(DEV)
    mask = torch.ones(B, 2, dtype=torch.int64, device=DEV)
    ctx = Buf(F32, B, D, D, post=GUARD)
    with torch.cuda.device(DEV):
        rc = N.lib().om_debug_dec_cross(F32, N.ptr(q), N.ptr(kv), N.ptr(mask), ctx.ptr(), B, 2, D, 1, 0.0, 0, stream())
    sync()
    assert rc == 0, N.lib().om_last_error()
    p0 = torch.sigmoid(gaps.double().to(DEV))
    return float(((ctx.window[:, 0].double() - p0).abs() / p0).max())


@pytest.mark.gpu
def test_exp_constant_holds_for_dec_cross():
    worst = measure_exp()
    print(f"dec_cross exp path, largest relative error of a probability: {worst:.4e} ({worst / u:.2f} u); recorded {DEC_EXP_MEASURED:.2e}")
    assert worst <= EXP_MEASURED * 1.001, worst


# ---------------------------------------------------------------------------------------------------------------
# GPU: final norm, head drop, start, cast
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_final(dtype, B):
    lib = N.lib()
    for H in (64, 128, 192, 320, 768, 1024):
        g = torch.Generator().manual_seed(H + B)
        x = torch.randn(B, H, generator=g)
        x[0] *= 2.0 ** -10                            # mean square about 2^-20
        if B > 1:
            x[1] *= 2.0 ** 10                         # about 2^20 (float16: |x| stays below 65504)
            x[2, 1:] = 0.0                            # one element carries the row
        x = x.to(TORCH_DT[dtype]).to(DEV)
        gain = (1.0 + 0.3 * torch.randn(H, generator=g)).to(DEV)
        out = Buf(F32, B, H, H, post=GUARD)
        snap, keep = out.snapshot(), (x.clone(), gain.clone())
        with torch.cuda.device(DEV):
            rc = lib.om_debug_dec_final(dtype, N.ptr(x), N.ptr(gain), out.ptr(), B, H, EPS, stream())
        sync()
        label = f"dec_final/{NAME[dtype]}/B{B}/H{H}"
        assert rc == 0, lib.om_last_error()
        guards_ok(label, (out, snap))
        assert torch.equal(_bits(x), _bits(keep[0])) and torch.equal(gain, keep[1])
        xd = x.double()
        ref = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + float(np.float32(EPS))) * gain.double()
        assert_within(label, out.window, ref, (RSQRT_REL + (H + 3) * u + 3 * u) * ref.abs() + FLOOR[F32], F32)
        ctl = xd * torch.rsqrt((xd * xd).sum(-1, keepdim=True) / (H - 1) + EPS) * gain.double()          # control: a wrong divisor
        assert bool(((ctl - ref).abs() > (RSQRT_REL + (H + 6) * u) * ref.abs() + FLOOR[F32]).any())


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1, 0.99999])
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_head_drop_is_the_port(dtype, p):
    """in place; B H = 4032 is not a multiple of 256; one draw per (b, h) covers all 64 lanes"""
    lib = N.lib()
    B, heads, seed = 21, 3, 0xDEADBEEFCAFEF00D
    H = heads * D
    x = (torch.randn(B, H, generator=torch.Generator().manual_seed(3)) * 0.01 + 0.02).to(TORCH_DT[dtype])      # x 65536 stays finite in float16
    x[0, 0], x[0, 1] = 0.0, -0.25                    # (no -0: in float16 the device returns +0 for it, see the docstring)
    v = Buf(dtype, B, H, H, post=GUARD, fill=x.to(DEV))
    snap = v.snapshot()
    with torch.cuda.device(DEV):
        rc = lib.om_debug_dec_head_drop(dtype, v.ptr(), B, H, p, seed, stream())
    sync()
    assert rc == 0, lib.om_last_error()
    guards_ok(f"head_drop p{p}", (v, snap))
    keep, scale = keep_of(seed, torch.arange(B * heads, dtype=torch.int64), p)
    keep = keep.view(B, heads, 1).expand(B, heads, D).reshape(B, H)
    want = torch.where(keep, x.float() * torch.tensor(scale), torch.zeros(())).to(TORCH_DT[dtype])
    assert torch.equal(_bits(v.window.cpu().contiguous()), _bits(want)), p
    if p == 0.0:
        assert torch.equal(_bits(want), _bits(x))
    else:
        assert bool((~keep).any()) and (p > 0.9 or bool(keep.any()))


WRAP = 8192 * 256 + 3
START_SHAPES = [(1, 1), (5, 51), (4, 64), (1, 257), (WRAP // 5, 5)]            # B H = 1, 255, 256, 257, 8192 * 256 + 3


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_start(dtype):
    lib = N.lib()
    assert [b * h for b, h in START_SHAPES] == [1, 255, 256, 257, WRAP]
    for B, H in START_SHAPES:
        emb = (torch.randn(H, generator=torch.Generator().manual_seed(H)) * 3).to(DEV)
        emb[0] = -0.0
        x = torch.full((B * H + 8,), GUARD_F, dtype=TORCH_DT[dtype], device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.om_debug_dec_start(dtype, N.ptr(emb), N.ptr(x), B, H, stream())
        sync()
        assert rc == 0, lib.om_last_error()
        assert bool((x[B * H:] == GUARD_F).all()), (B, H)
        want = emb.to(TORCH_DT[dtype])[None, :].expand(B, H).contiguous()
        assert torch.equal(_bits(x[:B * H].view(B, H)), _bits(want)), (B, H)


def cast_values(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * torch.exp2(torch.randint(-30, 20, (n,), generator=torch.Generator().manual_seed(n + 1)).float())
    special = torch.tensor([math.inf, -math.inf, 65504.0, 65519.9, 65520.0, 70000.0, -1e30, 3.3e38, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26,
                            -2.0 ** -20, 0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12])
    if n >= 255:
        x[3:3 + special.numel()] = special
    else:
        x[0] = math.inf
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DT, ids=lambda d: NAME[d])
def test_cast(dtype):
    """the f32 value rounded once to nearest even; 8192 * 256 + 3 elements: the grid-stride loop wraps"""
    lib = N.lib()
    for n in (1, 255, 256, 257, WRAP):
        x = cast_values(n).to(DEV)
        y = torch.full((n + 8,), GUARD_F, dtype=TORCH_DT[dtype], device=DEV)
        keep = x.clone()
        with torch.cuda.device(DEV):
            rc = lib.om_debug_dec_cast(dtype, N.ptr(x), N.ptr(y), n, stream())
        sync()
        assert rc == 0, lib.om_last_error()
        assert bool((y[n:] == GUARD_F).all()) and torch.equal(_bits(x), _bits(keep)), n
        want = x.cpu().to(TORCH_DT[dtype])
        assert torch.equal(_bits(y[:n].cpu()), _bits(want)), (n, (_bits(y[:n].cpu()) != _bits(want)).nonzero()[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------
# the whole step: a float64 decoder position in plain torch, fed the kernels' own masks
# ---------------------------------------------------------------------------------------------------------------
MATS = ("sa_v_w", "sa_o_w", "ca_q_w", "ca_kv_w", "ca_o_w", "ffn1_w", "ffn1g_w", "ffn2_w")
GAINS = ("sa_ln_g", "ca_ln_g", "ffn_ln_g")
RELU, GATED, UNGATED_GELU = 0, 1, 2


def gelu_new64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def make_weights(nl, H, F, kind, seed):
    """f32 tensors on the CPU: matrices [out, in] at T5's initial scales, RMSNorm gains 1 + 0.3 randn"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    W = {"start_emb": r(H), "final_ln_g": 1.0 + 0.3 * r(H), "layers": []}
    for _ in range(nl):
        lw = {"sa_v_w": r(H, H) * H ** -0.5, "sa_o_w": r(H, H) * H ** -0.5, "ca_q_w": r(H, H) * (H * D) ** -0.5 * 4,
              "ca_kv_w": r(2 * H, H) * H ** -0.5, "ca_o_w": r(H, H) * H ** -0.5, "ffn1_w": r(F, H) * H ** -0.5,
              "ffn2_w": r(H, F) * F ** -0.5}
        if kind == GATED:
            lw["ffn1g_w"] = r(F, H) * H ** -0.5
        for n in GAINS:
            lw[n] = 1.0 + 0.3 * r(H)
        W["layers"].append(lw)
    return W


def step_masks(seed, p, nl, B, H, F, heads, L):
    """the seven sites' multipliers keep keep_scale (float64), keyed as the code keys them; None at p = 0"""
    if not p > 0:
        return None
    def elem(s, n):
        keep, sc = keep_of(s, torch.arange(B * n, dtype=torch.int64).view(B, n), p)
        return keep.double() * float(sc)
    M = {"start": elem(dec_site(seed, 0, 0), H), "final": elem(dec_site(seed, nl, 1), H), "layers": []}
    for l in range(nl):
        hk, sc = keep_of(dec_site(seed, l, 1), torch.arange(B * heads, dtype=torch.int64).view(B, heads), p)
        ck, cs = cross_keep(dec_site(seed, l, 2), B, heads, L, p)
        M["layers"].append({"head": (hk.double() * float(sc))[:, :, None].expand(B, heads, D).reshape(B, H), "cross": ck.double() * cs,
                            "ca_out": elem(dec_site(seed, l, 3), H), "ffn_out": elem(dec_site(seed, l, 4), H),
                            "ffn_in": elem(dec_site(seed, l, 5), F), "sa_out": elem(dec_site(seed, l, 6), H)})
    return M


def rms64(x, g, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * g


def decoder_reference(W, E, mask, M, kind, heads, eps=EPS):
    """out [B, H] of the decoder position in float64 (differentiable): W's tensors and E [B, L, H] are float64 leaves"""
    B, L, H = E.shape
    one = lambda name, l=None: 1.0 if M is None else (M[name] if l is None else M["layers"][l][name])
    x = W["start_emb"][None, :].expand(B, H) * one("start")
    m = (mask != 0)[:, None, :]
    for l, lw in enumerate(W["layers"]):
        v = (rms64(x, lw["sa_ln_g"], eps) @ lw["sa_v_w"].t()) * one("head", l)
        x = x + (v @ lw["sa_o_w"].t()) * one("sa_out", l)
        q = (rms64(x, lw["ca_ln_g"], eps) @ lw["ca_q_w"].t()).view(B, heads, D)
        kv = (E @ lw["ca_kv_w"].t()).view(B, L, 2, heads, D)
        K, V = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)
        s = (q[:, :, None, :] * K).sum(-1).masked_fill(~m, -math.inf)
        pd = torch.softmax(s, -1) * one("cross", l)
        ctx = (pd[..., None] * V).sum(2).reshape(B, H)
        x = x + (ctx @ lw["ca_o_w"].t()) * one("ca_out", l)
        n = rms64(x, lw["ffn_ln_g"], eps)
        f = n @ lw["ffn1_w"].t()
        a = torch.relu(f) if kind == RELU else gelu_new64(f) * (n @ lw["ffn1g_w"].t()) if kind == GATED else gelu_new64(f)
        x = x + ((a * one("ffn_in", l)) @ lw["ffn2_w"].t()) * one("ffn_out", l)
    return rms64(x, W["final_ln_g"], eps) * one("final")


def aligned(nbytes, slack=0):
    """(owner, 256-byte aligned address) of nbytes of device memory filled with 0x5A, `slack` guard bytes behind"""
    buf = torch.full((int(nbytes) + 256 + slack,), 0x5A, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256
    return buf, buf.data_ptr() + off, off


class DeviceDecoder:
    """OmT5DecoderWeights / OmT5DecoderGrads over device tensors, as encoder._pack_t5_decoder and train._T5EncDecTrain build them"""

    def __init__(self, W, dtype, H, F, heads, kind, head_dim=D):
        td = TORCH_DT[dtype]
        nl = len(W["layers"])
        act = N.ACT_RELU if kind == RELU else N.ACT_GELU_TANH
        self.cfg = N.OmEncoderConfig(arch=N.ARCH_T5, dtype=dtype, hidden=H, n_layers=nl, n_heads=heads, head_dim=head_dim, ffn=F, vocab=600,
                                     max_pos=0, type_vocab=0, act=act, ln_eps=EPS, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_NONE,
                                     head_in=0, head_out=0, normalize=0)
        self.nl, self.H, self.F, self.dtype = nl, H, F, dtype
        self.dev = {"start_emb": W["start_emb"].to(DEV), "final_ln_g": W["final_ln_g"].to(DEV), "layers": []}
        self.grad = {"start_emb": torch.zeros(H, device=DEV), "final_ln_g": torch.zeros(H, device=DEV), "layers": []}
        self.layers = (N.OmT5DecoderLayer * nl)()
        self.glayers = (N.OmT5DecoderLayerGrads * nl)()
        for l, lw in enumerate(W["layers"]):
            d, g = {}, {}
            for name in MATS + GAINS:
                if name in lw:
                    d[name] = lw[name].to(td if name in MATS else torch.float32).to(DEV).contiguous()
                    setattr(self.layers[l], name, d[name].data_ptr())
                shape = lw[name].shape if name in lw else (F, H)
                g[name] = torch.zeros(*shape, device=DEV)          # ffn1g_w's buffer exists even when it is not gated: it must stay zero
                setattr(self.glayers[l], name, g[name].data_ptr())
            self.dev["layers"].append(d)
            self.grad["layers"].append(g)
        self.w = N.OmT5DecoderWeights(start_emb=self.dev["start_emb"].data_ptr(), final_ln_g=self.dev["final_ln_g"].data_ptr(),
                                      layers_host=C.cast(self.layers, C.POINTER(N.OmT5DecoderLayer)), n_layers=nl)
        self.g = N.OmT5DecoderGrads(start_emb=self.grad["start_emb"].data_ptr(), final_ln_g=self.grad["final_ln_g"].data_ptr(),
                                    layers_host=C.cast(self.glayers, C.POINTER(N.OmT5DecoderLayerGrads)))

    def sizes(self, B, L):
        lib = N.lib()
        return (lib.om_t5_decoder_tape_bytes(C.byref(self.cfg), self.nl, B, L), lib.om_t5_decoder_train_workspace_bytes(C.byref(self.cfg), self.nl, B, L),
                lib.om_t5_decoder_workspace_bytes(C.byref(self.cfg), B, L))

    def forward(self, E, mask, p, seed):
        """(rc, out [B, H] f32); keeps the tape for backward"""
        B, L, H = E.shape
        nt, nw, _ = self.sizes(B, L)
        self.tape, self.ws = aligned(nt, 256), aligned(nw, 256)
        self.nt, self.nw = nt, nw
        out = Buf(F32, B, H, H, post=GUARD)
        snap = out.snapshot()
        with torch.cuda.device(DEV):
            rc = N.lib().om_t5_decoder_train_forward(C.byref(self.cfg), C.byref(self.w), N.ptr(E), N.ptr(mask), B, L, p, seed, C.c_void_p(self.tape[1]),
                                                     nt, out.ptr(), C.c_void_p(self.ws[1]), nw, stream())
        sync()
        guards_ok("train forward out", (out, snap))
        self.guards("forward")
        return rc, out.window

    def guards(self, what):
        for name, (buf, _, off), n in (("tape", self.tape, self.nt), ("workspace", self.ws, self.nw)):
            assert bool((buf[off + n:] == 0x5A).all()) and bool((buf[:off] == 0x5A).all()), f"{what}: written outside the {name}"

    def backward(self, E, mask, p, seed, d_out):
        B, L, H = E.shape
        dE = Buf(self.dtype, B * L, H, H, post=GUARD)
        snap = dE.snapshot()
        with torch.cuda.device(DEV):
            rc = N.lib().om_t5_decoder_train_backward(C.byref(self.cfg), C.byref(self.w), N.ptr(E), N.ptr(mask), B, L, p, seed, C.c_void_p(self.tape[1]),
                                                      N.ptr(d_out), C.byref(self.g), dE.ptr(), C.c_void_p(self.ws[1]), self.nw, stream())
        sync()
        guards_ok("train backward d_enc_hidden", (dE, snap))
        self.guards("backward")
        return rc, dE.window.view(B, L, H)

    def step(self, E, mask):
        B, L, H = E.shape
        n = self.sizes(B, L)[2]
        buf, ptr, off = aligned(n, 256)
        out = Buf(F32, B, H, H, post=GUARD)
        snap = out.snapshot()
        with torch.cuda.device(DEV):
            rc = N.lib().om_t5_decoder_step(C.byref(self.cfg), C.byref(self.w), N.ptr(E), N.ptr(mask), B, L, out.ptr(), C.c_void_p(ptr), n, stream())
        sync()
        guards_ok("decoder step out", (out, snap))
        assert bool((buf[off + n:] == 0x5A).all()) and bool((buf[:off] == 0x5A).all()), "step: written outside the workspace"
        return rc, out.window


def reference_step(W, E, mask, dtype, kind, heads, p, seed, d_out):
    """float64 autograd on the values the device holds (matrices, start row and E rounded to the storage type):
    (out, {name: gradient}) with names 'start_emb', 'final_ln_g', 'd_enc', 'L<l>.<name>'"""
    td = TORCH_DT[dtype]
    leaf = lambda t, rounded: (t.to(td) if rounded else t).double().requires_grad_()
    B, L, H = E.shape
    F = W["layers"][0]["ffn1_w"].shape[0]
    W64 = {"start_emb": leaf(W["start_emb"], True), "final_ln_g": leaf(W["final_ln_g"], False),
           "layers": [{n: leaf(t, n in MATS) for n, t in lw.items()} for lw in W["layers"]]}
    E64 = leaf(E.cpu(), True)
    out = decoder_reference(W64, E64, mask.cpu(), step_masks(seed, p, len(W["layers"]), B, H, F, heads, L), kind, heads)
    (out * d_out.cpu().double()).sum().backward()
    grads = {"start_emb": W64["start_emb"].grad, "final_ln_g": W64["final_ln_g"].grad, "d_enc": E64.grad}
    for l, lw in enumerate(W64["layers"]):
        for n, t in lw.items():
            grads[f"L{l}.{n}"] = t.grad
    return out.detach(), grads


def device_grads(dd, dE):
    got = {"start_emb": dd.grad["start_emb"], "final_ln_g": dd.grad["final_ln_g"], "d_enc": dE}
    for l, g in enumerate(dd.grad["layers"]):
        for n, t in g.items():
            got[f"L{l}.{n}"] = t
    return {k: v.detach().double().cpu() for k, v in got.items()}


def step_case(dtype, kind, p, L, seed=0x5EED, B=3, H=128, F=256, nl=2):
    heads = H // D
    W = make_weights(nl, H, F, kind, 31 + kind)
    g = torch.Generator().manual_seed(L + kind)
    E = torch.randn(B, L, H, generator=g).to(TORCH_DT[dtype]).to(DEV)
    mask = ragged_mask(B, L, seed=2)
    mask[0, :L // 3] = 1                              # a few keys in the first row, not one: its gradient is not all in one V row
    d_out = torch.randn(B, H, generator=g).to(DEV)
    dd = DeviceDecoder(W, dtype, H, F, heads, kind)
    return NS(W=W, E=E, mask=mask.to(DEV), d_out=d_out, dd=dd, heads=heads, B=B, L=L, H=H, F=F, nl=nl, kind=kind, p=p, seed=seed, dtype=dtype)


def rel_l2(got, want):
    return float((got - want).norm() / (want.norm() + 1e-300))


STEP_CASES = [(RELU, 0.0, 70), (RELU, 0.1, 70), (GATED, 0.0, 70), (GATED, 0.1, 70), (GATED, 0.1, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,p,L", STEP_CASES, ids=[f"{'gated' if k else 'relu'}-p{p}-L{L}" for k, p, L in STEP_CASES])
def test_train_step_matches_float64_autograd(kind, p, L):
    """float32: out and every gradient against float64 autograd under the kernels' own masks; ffn1g_w's buffer stays zero when not
    gated; a second backward doubles the weight gradients (they add) and leaves d_enc_hidden as it was (it is written); at p = 0
    om_t5_decoder_step against the train forward"""
    c = step_case(F32, kind, p, L)
    lib = N.lib()
    want_out, want = reference_step(c.W, c.E, c.mask, F32, kind, c.heads, p, c.seed, c.d_out)
    rc, out = c.dd.forward(c.E, c.mask, p, c.seed)
    assert rc == 0, lib.om_last_error()
    err = float((out.double().cpu() - want_out).abs().max())
    print(f"train forward out: max error {err:.3e} (|out|max {float(want_out.abs().max()):.3f})")
    assert err < 1e-4 * max(1.0, float(want_out.abs().max())), err
    if p > 0:
        assert bool((out == 0).any()) and bool(((want_out == 0) == (out.cpu() == 0)).all())           # the final dropout's own zeros
    rc, dE = c.dd.backward(c.E, c.mask, p, c.seed, c.d_out)
    assert rc == 0, lib.om_last_error()
    got = device_grads(c.dd, dE)
    worst = ("", 0.0)
    for name, g in got.items():
        if name not in want:
            assert name.endswith("ffn1g_w") and kind != GATED and float(g.abs().max()) == 0.0, name
            continue
        rel, amax = rel_l2(g, want[name]), float((g - want[name]).abs().max())
        worst = max(worst, (name, rel), key=lambda t: t[1])
        assert rel < 2e-3 or amax < 1e-7, (name, rel, amax)
    assert set(want) <= set(got)
    print(f"train backward: worst gradient relative L2 {worst[1]:.3e} ({worst[0]})")
    first = {k: v.clone() for k, v in got.items()}
    rc, dE2 = c.dd.backward(c.E, c.mask, p, c.seed, c.d_out)
    assert rc == 0, lib.om_last_error()
    again = device_grads(c.dd, dE2)
    assert torch.equal(again["d_enc"], first["d_enc"]), "d_enc_hidden is written, not added to"
    for name, g in again.items():
        if name != "d_enc" and name in want:
            assert rel_l2(g, 2.0 * first[name]) < 1e-5, name
    if p == 0:
        rc, step = c.dd.step(c.E, c.mask)
        assert rc == 0, lib.om_last_error()
        same = torch.equal(step, out)
        diff = float((step.double() - out.double()).abs().max())
        print(f"om_t5_decoder_step against the train forward: {'bit-identical' if same else f'max difference {diff:.3e}'}")
        assert float((step.double().cpu() - want_out).abs().max()) < 1e-4 * max(1.0, float(want_out.abs().max()))
        assert same, diff


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_train_step_16bit(dtype):
    """gated, p = 0.1, L = 70; the reference runs on the rounded weights and inputs; limits: see the docstring"""
    c = step_case(dtype, GATED, 0.1, 70)
    lib = N.lib()
    want_out, want = reference_step(c.W, c.E, c.mask, dtype, GATED, c.heads, c.p, c.seed, c.d_out)
    rc, out = c.dd.forward(c.E, c.mask, c.p, c.seed)
    assert rc == 0, lib.om_last_error()
    rc, dE = c.dd.backward(c.E, c.mask, c.p, c.seed, c.d_out)
    assert rc == 0, lib.om_last_error()
    got = device_grads(c.dd, dE)
    assert set(want) == set(got)
    names = sorted(want)
    per = {n: rel_l2(got[n], want[n]) for n in names}
    whole = rel_l2(torch.cat([got[n].flatten() for n in names]), torch.cat([want[n].flatten() for n in names]))
    worst = max(per.items(), key=lambda t: t[1])
    cos = float(torch.nn.functional.cosine_similarity(out.double().cpu(), want_out, dim=1).min())
    print(f"16-bit train step {NAME[dtype]}: out cosine {cos:.6f}, whole-gradient relative L2 {whole:.3e}, worst tensor {worst[1]:.3e} ({worst[0]})")
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(g).all()) for g in got.values())
    assert whole < (1e-2 if dtype == F16 else 1e-1), whole
    if dtype == F16:
        assert worst[1] < 5e-2, worst


@pytest.mark.gpu
def test_step_serves_an_ungated_gelu_stack():
    """act = tanh-GELU with ffn1g_w NULL: om_t5_decoder_step runs x += Wo gelu_new(Wi n) (training refuses the combination, see
    test_entry_point_refusals); pinned against the float64 reference of that stack"""
    c = step_case(F32, UNGATED_GELU, 0.0, 70)
    want_out, _ = reference_step(c.W, c.E, c.mask, F32, UNGATED_GELU, c.heads, 0.0, 0, c.d_out)
    rc, out = c.dd.step(c.E, c.mask)
    assert rc == 0, N.lib().om_last_error()
    err = float((out.double().cpu() - want_out).abs().max())
    print(f"ungated gelu_new step: max error {err:.3e}")
    assert err < 1e-4 * max(1.0, float(want_out.abs().max())), err
    relu_ref, _ = reference_step(c.W, c.E, c.mask, F32, RELU, c.heads, 0.0, 0, c.d_out)
    assert float((relu_ref - want_out).abs().max()) > 1e-2                         # control: the ReLU stack is something else


@pytest.mark.gpu
def test_entry_point_refusals():
    """om_t5_decoder_step, om_t5_decoder_train_forward and om_t5_decoder_train_backward refuse, by message, before the first kernel
    that could go wrong.  Every call gets REAL buffers of the right size, so a check that failed to refuse would still run in bounds."""
    lib = N.lib()
    B, L, H, F = 2, 16, 128, 256
    err = lib.om_last_error

    def calls(dd, Lc=L, p=0.0, ws_shift=0, short=None):
        """the three entry points on buffers sized for max(L, Lc); short: 'ws' or 'tape' passes a size one byte below the need"""
        Lb = max(L, min(Lc, 1100))
        E = torch.zeros(B, Lb, H, dtype=TORCH_DT[dd.dtype], device=DEV)
        mask = torch.ones(B, Lb, dtype=torch.int64, device=DEV)
        big = NS(cfg=N.OmEncoderConfig.from_buffer_copy(dd.cfg))
        big.cfg.head_dim, big.cfg.n_heads = D, H // D
        need = lambda f, *a: max(f(C.byref(big.cfg), *a, B, Lb), 4096)
        nt, nw, ns = need(lib.om_t5_decoder_tape_bytes, dd.nl), need(lib.om_t5_decoder_train_workspace_bytes, dd.nl), need(lib.om_t5_decoder_workspace_bytes)
        tape, ws, sws = aligned(nt, 512), aligned(nw, 512), aligned(ns, 512)
        out, d_out, dE = torch.zeros(B, H, device=DEV), torch.zeros(B, H, device=DEV), torch.zeros(B, Lb, H, dtype=TORCH_DT[dd.dtype], device=DEV)
        exact = lambda f, *a: f(C.byref(dd.cfg), *a, B, Lc)
        st = exact(lib.om_t5_decoder_workspace_bytes) - 1 if short == "ws" else ns
        tt = exact(lib.om_t5_decoder_tape_bytes, dd.nl) - 1 if short == "tape" else nt
        wt = exact(lib.om_t5_decoder_train_workspace_bytes, dd.nl) - 1 if short == "ws" else nw
        res = []
        with torch.cuda.device(DEV):
            rc = lib.om_t5_decoder_step(C.byref(dd.cfg), C.byref(dd.w), N.ptr(E), N.ptr(mask), B, Lc, N.ptr(out), C.c_void_p(sws[1] + ws_shift), st, stream())
            res.append((rc, err()))
            rc = lib.om_t5_decoder_train_forward(C.byref(dd.cfg), C.byref(dd.w), N.ptr(E), N.ptr(mask), B, Lc, p, 1, C.c_void_p(tape[1]), tt, N.ptr(out),
                                                 C.c_void_p(ws[1] + ws_shift), wt, stream())
            res.append((rc, err()))
            rc = lib.om_t5_decoder_train_backward(C.byref(dd.cfg), C.byref(dd.w), N.ptr(E), N.ptr(mask), B, Lc, p, 1, C.c_void_p(tape[1]), N.ptr(d_out),
                                                  C.byref(dd.g), N.ptr(dE), C.c_void_p(ws[1] + ws_shift), wt, stream())
            res.append((rc, err()))
        sync()
        return res

    def refused(res, text, which=(0, 1, 2)):
        for i in which:
            assert res[i][0] != 0 and text in res[i][1], (i, text, res[i])

    new = lambda kind=RELU, **kw: DeviceDecoder(make_weights(2, H, F, kind, 3), F32, H, F, H // D, kind, **kw)
    ok = calls(new())
    assert [r[0] for r in ok] == [0, 0, 0], ok
    refused(calls(new(), Lc=1025), b"sequence length must be in [1,1024]")
    dd = new(head_dim=32)
    dd.cfg.n_heads = 4
    refused(calls(dd), b"head_dim must be 64")
    dd = new()
    dd.cfg.act = N.ACT_GELU_ERF
    refused(calls(dd), b"T5 decoder supports relu and gated gelu_new")
    refused(calls(new(), ws_shift=8), b"must be 256-byte aligned")
    res = calls(new(), short="ws")
    refused(res, b"workspace too small", (0, 2))
    refused(res, b"tape or workspace too small", (1,))
    res = calls(new(), short="tape")
    refused(res, b"tape or workspace too small", (1,))
    assert res[0][0] == 0 and res[2][0] == 0                                   # the step has no tape; the backward is not told its size
    res = calls(new(), p=1.0)
    refused(res, b"dropout must be in [0, 1)", (1, 2))
    assert res[0][0] == 0                                                      # the step takes no dropout
    dd = new()
    dd.layers[1].ca_o_w = None
    refused(calls(dd), b"incomplete decoder layer weights")
    # gated <-> ffn1g_w: training refuses both mismatches; the step runs whichever form the pointer says
    dd = new(GATED)
    dd.layers[0].ffn1g_w = None
    res = calls(dd)
    refused(res, b"the gated feed-forward (and only it) needs ffn1g_w", (1, 2))
    assert res[0][0] == 0
    dd = new(RELU)
    dd.layers[0].ffn1g_w = dd.dev["layers"][0]["ffn1_w"].data_ptr()
    refused(calls(dd), b"the gated feed-forward (and only it) needs ffn1g_w", (1, 2))
