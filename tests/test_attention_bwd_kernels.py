"""The attention backward kernel by kernel (csrc/attention_bwd16.hip, train_kernels.hip: attention_bwd_kernel and the
attention_bwd_long_a / _b pair, attention_d32.hip: attention_d32_bwd_kernel) against a float64 reference on the exact stored (rounded)
qkv, dctx and pos_bias, element by element, within a bound derived from the arithmetic (bwd_error_bound below).  The one constant of the
bound that is not derived is the forward file's EXP_REL, reused.  The kernels are called alone through om_debug_attention_bwd_ex, which
forwards every argument to the one backward entry; attn_plan_bwd chooses the family, and every GPU case asserts through
om_debug_attention_bwd_last() the (family, key tiles) it must reach.

The reference (bwd_reference), per (sequence, head), with keep the forward's dropout mask and dO = dctx:
    P = softmax(scale Q K^T + bias + mask)      Pd = keep o P keep_scale          dPd = dO V^T       dP = keep keep_scale o dPd
    delta = rowsum(P o dP)                      dS = P o (dP - delta)
    dQ = scale dS K        dK = scale dS^T Q        dV = Pd^T dO        drel[h][k - q + Lm - 1] += sum_b dS[b, h, q, k]
test_reference_is_the_autograd_of_the_forward checks these formulas against torch.autograd of the float64 forward.

Contracts the kernels share, as this file pins them:
  * visibility is the forward's: a padded key has probability exactly 0 whenever its sequence has an unmasked key, so its dK and dV
    rows are exactly +-0 (every family writes them); a sequence WITHOUT any unmasked key is uniform over all its L keys, and its
    gradients are those of the uniform P (dS = P o (dP - delta) with P = 1 / L);
  * padded QUERY rows are rows like any other: they get a dQ and contribute to dK, dV and drel;
  * drel ACCUMULATES into what the buffer holds (f32 atomics, so its bits depend on the order; dqkv is bit-reproducible);
  * a position bias comes with its gradient buffer: without it 32-wide heads are refused, and 64-wide heads run GENERIC, which adds
    the bias and skips its gradient;
  * dropout is keyed on the mask's row pitch Lm, so a packed and a padded call draw the same mask, and it is the forward's mask:
    LONG takes delta as dO . O from the forward's stored output, which only equals rowsum(P o dP) under the same (p, seed);
  * LONG needs ctx and stats (refused without); no other family reads or writes them;
  * packed rows (cu): the rows that exist carry the bits of the padded call whose dctx is zero beyond each sequence's extent (a padded
    query row with a non-zero dO would add to dK / dV, and a packed call has no such row); rows of dqkv from cu[B] on are NOT written
    (train.hip zeroes them with omk_zero_rows_from); a sequence of length 0 writes nothing.
Left open on purpose, as in the forward file: 0 x NaN.  The NaN case uses an unmasked query under full attention.

family -> GPU cases (test_lengths ids are [route-dtype-L]; routes: OM_OPT_ATTENTION_FAST 1 = default, 0 = fast0, 2 = long_all)
  BWD16     bf16, f16: test_lengths[default-bf16|f16-L<=128], test_masks[bwd16-*], test_bias_dropout[bwd16-*], test_packed_rows[bwd16-*],
            test_non_finite_dctx_stays_where_it_belongs[bwd16-*], test_deterministic[bwd16-*]
  GENERIC   f32: test_lengths[default-f32-*], test_masks[generic-f32], test_bias_dropout[generic-f32-*]   (no packed rows in f32: "P")
            bf16, f16: test_lengths[fast0-*] (every KT), test_lengths[default-*16-129|192], test_masks[generic-bf16|f16], test_bias_dropout[generic-bf16|f16-*],
            test_packed_rows[generic-*] (L = 200 by default, L = 128 under fast0, bias + drel once), test_bias_without_gradient_buffer
  LONG      bf16, f16: test_lengths[default-*16-L>=193], test_lengths[long_all-*], test_masks[long-*], test_bias_dropout[long-*],
            test_long_pairs_with_the_forward_kernel, test_long_needs_ctx_and_stats   (no packed rows: "C")
  D32       f32, bf16, f16: test_lengths_d32, test_masks[d32-*], test_bias_dropout[d32-*], test_packed_rows[d32-*] (16-bit), test_non_finite_dctx_stays_where_it_belongs[d32-*],
            test_deterministic[d32-*]   (test_non_finite_... and test_deterministic run GENERIC and LONG too)
Every expectation comes from a table of this file (ROUTES, MASKS, BD, PACKED, NONFINITE) that test_backward_plan_names_what_the_gpu_cases_assert
walks through om_debug_attention_bwd_plan without a GPU.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import (BF16, BWD_LETTER, BWD_TABLE, DEV, DROP_ODD, DTYPES, EXP_REL, F16, F32, FLOOR, LENGTHS, NAME,
                                          SCALES, TORCH_DT, U_ACC, U_OUT, attention_reference, bits, drop_keep, drop_threshold,
                                          error_bound, kt_of, make_inputs, mask_extent, masks_eleven, mixed_mask, new_ctx, option, pack_rows,
                                          planned_bwd, split_qkv, untouched, visibility)
from tests.test_attention_kernels import launch as launch_fwd

BFAM = N.ATTN_BWD_FAMILY
DREL_FILL = 0.25           # drel is pre-filled: the kernels accumulate
DREL_GUARD = 7.5           # floats after drel's last


# ---------------------------------------------------------------------------------------------------------------
# reference, bound, controls (pure torch: the CPU tests below check them on an emulated kernel)
# ---------------------------------------------------------------------------------------------------------------
def make_dctx(dtype, B, L, H, seed, device="cpu"):
    """O(1) gradients whose row magnitudes spread over five binades (2^-2 .. 2^2 by query row)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, H, generator=g) * (2.0 ** ((torch.arange(L) % 5).float() - 2.0))[None, :, None]
    return x.reshape(B * L, H).to(TORCH_DT[dtype]).to(device)


def rel_bins(x, L):
    """x [..., heads, L(q), L(k)] summed over every leading dimension into [heads, 2 L - 1] by k - q + L - 1"""
    heads = x.shape[-3]
    i = torch.arange(L, device=x.device)
    idx = (i[None, :] - i[:, None] + (L - 1)).flatten()
    out = torch.zeros(heads, 2 * L - 1, dtype=x.dtype, device=x.device)
    return out.index_add_(1, idx, x.reshape(-1, heads, L * L).sum(0))


def heads_of(t, B, L, heads, D):
    """[B * L, heads * D] or [B, L, heads * D] -> float64 [B, heads, L, D]"""
    return t.double().reshape(B, L, heads, D).permute(0, 2, 1, 3)


def bwd_reference(qkv, dctx, mask, bias, B, L, heads, D, scale, keep=None, keep_scale=1.0, ctl=None):
    """float64 on the stored values, the formulas of the docstring written out.  ctl names a wrong kernel (a negative control):
    'no_delta' (delta omitted), 'no_keep_scale' (keep_scale missing from dP only), 'drop_pd_only' (the mask on Pd but not on dP).
    Returns g [3, B, heads, L, D] (dQ, dK, dV), drel [heads, 2 L - 1] and the magnitudes bwd_error_bound needs."""
    q, k, v = split_qkv(qkv, B, L, heads, D)
    dO = heads_of(dctx, B, L, heads, D)
    vis, _ = visibility(mask)
    vb = vis[:, None]
    s = scale * (q @ k.transpose(-1, -2))
    smag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    if bias is not None:
        s = s + bias.double()[None]
        smag = smag + bias.double().abs()[None]
    s = s.masked_fill(~vb, -math.inf)
    s = s.masked_fill(~(mask != 0).any(-1)[:, None, None, None], 0.0)       # no unmasked key: uniform
    P = torch.softmax(s, -1)
    kf = torch.ones_like(P) if keep is None else keep.to(P.device).double()
    M = kf * keep_scale
    Pd = P * M
    dPd = dO @ v.transpose(-1, -2)
    Mp = kf if ctl == "no_keep_scale" else torch.ones_like(P) if ctl == "drop_pd_only" else M
    dP = Mp * dPd
    delta = (P * dP).sum(-1, keepdim=True)
    if ctl == "no_delta":
        delta = torch.zeros_like(delta)
    dL = P * (dP - delta)                                                   # d loss / d (scaled score + bias)
    dS = scale * dL
    g = torch.stack([dS @ k, dS.transpose(-1, -2) @ q, Pd.transpose(-1, -2) @ dO])
    AdP = M * (dO.abs() @ v.abs().transpose(-1, -2))
    return NS(g=g, drel=rel_bins(dL, L), P=P, Pd=Pd, dL=dL, dS=dS, AdP=AdP, Ga=(P * AdP).sum(-1, keepdim=True), O=Pd @ v, dO=dO, q=q, k=k,
              smax=smag.masked_fill(~vb, 0.0).amax(-1), vis=vb.expand_as(P), kept=kf != 0, scale=scale, B=B, L=L, heads=heads, D=D)


def bwd_error_bound(R, dtype, family, ctx_err=None):
    """Per-element bounds (bg [3, B, heads, L, D] on dQ, dK, dV; bdrel [heads, 2 L - 1]) on |kernel - float64 reference|.  With u = 2^-24
    (f32), u16 the half ulp of the storage type (0 in float32: every product there is a true f32 MFMA), per query row q and key k:
      * P: the forward's score and exp terms.  Scores: f32 accumulation over D products, the scale (and log2 e) multiply, the bias add and
        the subtraction of the maximum, each one rounding of a value no larger than 2 smax -> ds = (D + 8) u 2 smax, which moves a
        probability by at most expm1(2 ds); the exponential and the normaliser: 2 EXP_REL; the normaliser's f32 sum over L terms
        (and 1 / sum, the product with it): (L + 16) u.  Together eP, relative.  Every family recomputes P in f32 (BWD16 once, in the
        log2 domain; GENERIC, LONG and D32 a second time lane-per-key from the stored row statistics: the same bound).
      * dPd = dO V^T: f32 accumulation over D -> with the keep_scale multiply eD = (D + 4) u of AdP = keep keep_scale sum_d |dO_d| |V_d|.
      * delta: BWD16, GENERIC, D32 sum P o dP over the L keys in f32 -> (eP + eD + (L + 4) u) Ga, Ga = sum_k P AdP.
        LONG takes dO . O with O the forward's STORED output: sum_d |dO_d| ctx_err_d with ctx_err the error of the stored O (its output
        rounding u16 |O| + floor when the test feeds the rounded reference; the forward file's error_bound when the forward kernel made
        it), plus the f32 dot over D: eD sum_d |dO_d| |O_d|.  Call either E_delta.
      * dL = P (dP - delta): (eP + 3 u) |dL| + P (eD AdP + E_delta) =: EL  (a subtraction and two multiplies).
      * dS = scale dL: scale EL + u |dS|.  In the 16-bit formats EVERY family rounds dS (after the scale) to the storage type before the
        second contraction -- the [query][key] LDS image of attention_bwd16.hip, the packed MFMA operand of SlabMma / ContractT16 in the
        other three -- u16 |dS|, and in float16 a value below 2^-14 lands on the subnormal grid: 2^-25 absolute per visible pair.
        Pd the same: (eP + 2 u + u16) Pd (+ 2^-25 per visible kept pair in float16).  These are E_dS, E_Pd.
      * dQ = sum_k dS K: sum_k E_dS |K| plus f32 accumulation over L: (L + 16) u sum_k |dS| |K|;  dK with Q over the queries, dV with
        E_Pd and dO over the queries, alike.
      * output rounding u_out |value| and the subnormal floor of the storage type.
      * drel (f32 atomics in arbitrary order: a workgroup's LDS histogram, then one global add per bin and workgroup): the sum of EL over
        the bin's addends plus n u (DREL_FILL + sum |dL|), n = B (pairs in the bin + 4) additions."""
    u16 = 0.0 if dtype == F32 else U_OUT[dtype]
    sub16 = 2.0 ** -25 if dtype == F16 else 0.0
    L, D, scale = R.L, R.D, R.scale
    ds = (D + 8) * U_ACC * 2.0 * R.smax
    eP = (torch.expm1(2.0 * ds) + 2.0 * EXP_REL + (L + 16) * U_ACC)[..., None]            # [B, heads, L, 1]
    eD = (D + 4) * U_ACC
    if family == "long":
        ce = heads_of(ctx_err, R.B, L, R.heads, D)
        Ed = (R.dO.abs() * ce).sum(-1, keepdim=True) + eD * (R.dO.abs() * R.O.abs()).sum(-1, keepdim=True)
    else:
        Ed = (eP + eD + (L + 4) * U_ACC) * R.Ga
    EL = (eP + 3 * U_ACC) * R.dL.abs() + R.P * (eD * R.AdP + Ed)
    EdS = scale * EL + (U_ACC + u16) * R.dS.abs() + sub16 * R.vis
    EPd = (eP + 2 * U_ACC + u16) * R.Pd + sub16 * (R.vis & R.kept)
    acc = (L + 16) * U_ACC
    T = lambda t: t.transpose(-1, -2)
    raw = torch.stack([EdS @ R.k.abs() + acc * (R.dS.abs() @ R.k.abs()),
                       T(EdS) @ R.q.abs() + acc * (T(R.dS.abs()) @ R.q.abs()),
                       T(EPd) @ R.dO.abs() + acc * (T(R.Pd) @ R.dO.abs())])
    u = U_OUT[dtype]
    bg = u * R.g.abs() + (1 + u) * raw + FLOOR[dtype]
    n = R.B * (L - (torch.arange(2 * L - 1, device=R.P.device) - (L - 1)).abs() + 4).double()[None]      # B (pairs in the bin + 4)
    bdrel = rel_bins(EL, L) + n * U_ACC * (DREL_FILL + rel_bins(R.dL.abs(), L))
    return bg, bdrel


CONTROLS = ("last_key", "seed+1", "scale", "bias_roll", "no_delta", "no_keep_scale", "drop_pd_only", "swap_dq_dk", "drel_shift", "do_roll")


def live_controls(mask, L, bias, p):
    """The controls that are NOT an identity, from the shape and the arguments alone: one token has dS = 0 and nothing to roll or
    exchange; seed + 1, the missing keep_scale and the mask on Pd alone need dropout; the rolled bias and the shifted bin a bias (which
    always comes with its gradient buffer here); the dropped last key a sequence with two unmasked keys or more."""
    if L < 2:
        return []
    live = ["scale", "no_delta", "swap_dq_dk", "do_roll"]                   # do_roll: dO read one query row off
    if bool(((mask != 0).sum(-1) >= 2).any()):
        live.append("last_key")
    if p > 0:
        live += ["seed+1", "no_keep_scale", "drop_pd_only"]
    if bias:
        live += ["bias_roll", "drel_shift"]
    return live


def missed_controls(c):
    """The names of the live controls the bound FAILED to reject (must be empty).  last_key must be rejected inside EVERY sequence it
    altered; every other somewhere in dQ, dK, dV or drel."""
    B, L, heads, D = c.B, c.L, c.heads, c.D
    ref = lambda **kw: bwd_reference(kw.pop("qkv", c.qkv), kw.pop("dctx", c.dctx), kw.pop("mask", c.mask), kw.pop("bias", c.pb), B, L, heads, D,
                                     kw.pop("scale", c.scale), kw.pop("keep", c.keep), c.ks, kw.pop("ctl", None))
    far = lambda x: bool(((x.g - c.R.g).abs() > c.bg).any()) or (c.pb is not None and bool(((x.drel - c.R.drel).abs() > c.bdrel).any()))
    missed = []
    for name in c.live:
        if name == "last_key":
            m2, altered = c.mask.clone(), []
            for b in range(B):
                nz = torch.nonzero(c.mask[b]).flatten()
                if nz.numel() >= 2:
                    m2[b, nz[-1]] = 0
                    altered.append(b)
            hit = ((ref(mask=m2).g - c.R.g).abs() > c.bg).transpose(0, 1).flatten(1).any(-1)
            missed += [f"last_key[b={b}]" for b in altered if not bool(hit[b])]
            continue
        if name == "seed+1":
            s, *rest = c.keep_args
            x = ref(keep=drop_keep(s + 1, *rest).to(c.qkv.device))
        elif name == "scale":
            x = ref(scale=c.scale * (1 + 2.0 ** -5))
        elif name == "bias_roll":
            x = ref(bias=torch.roll(c.pb, 1, dims=-1))
        elif name in ("no_delta", "no_keep_scale", "drop_pd_only"):
            x = ref(ctl=name)
        elif name == "swap_dq_dk":
            x = NS(g=c.R.g[[1, 0, 2]], drel=c.R.drel)
        elif name == "drel_shift":
            x = NS(g=c.R.g, drel=torch.roll(c.R.drel, 1, dims=-1))
        elif name == "do_roll":
            x = ref(dctx=torch.roll(c.dctx.view(B, L, -1), 1, dims=1).reshape(B * L, -1))
        if not far(x):
            missed.append(name)
    return missed


def prepare(dtype, B, L, heads, D, scale, mask, family, bias=False, p=0.0, seed=0, tag=0, device="cpu", zero_dctx_past_extent=False):
    """Inputs, the float64 reference (computed once) and the bound of one case."""
    c = NS(dtype=dtype, B=B, L=L, heads=heads, D=D, H=heads * D, scale=scale, family=family, p=p, seed=seed)
    c.qkv, c.pb = make_inputs(dtype, B, L, heads, D, scale, seed=2000 + 13 * L + D + tag, bias=bias, device=device)
    c.dctx = make_dctx(dtype, B, L, c.H, seed=3000 + 7 * L + D + tag, device=device)
    c.mask = mask.to(device)
    if zero_dctx_past_extent:
        ext = torch.tensor([int(torch.nonzero(m).max()) + 1 if m.any() else 0 for m in mask])
        c.dctx.view(B, L, c.H)[(torch.arange(L)[None, :] >= ext[:, None]).to(device)] = 0
    c.keep_args = (seed, B, heads, L, p) if p > 0 else None
    c.keep, c.ks = (drop_keep(*c.keep_args).to(device), drop_threshold(p)[1]) if p > 0 else (None, 1.0)
    c.R = bwd_reference(c.qkv, c.dctx, c.mask, c.pb, B, L, heads, D, scale, c.keep, c.ks)
    c.ctx_ref = c.R.O.permute(0, 2, 1, 3).reshape(B * L, c.H)
    c.ctx = c.ctx_ref.to(TORCH_DT[dtype])                                    # what LONG is fed unless a case says otherwise
    c.ctx_err = U_OUT[dtype] * c.ctx_ref.abs() + FLOOR[dtype]
    c.live = live_controls(mask, L, bias, p)
    return c


def verify(c, got, drel, label, controls=True, rows=None):
    """got [3, B, heads, L, D] and drel [heads, 2 L - 1] (minus the pre-fill) against the reference of c: bound, then controls.
    rows [B, L] (bool): the rows that exist (packed calls); None: all."""
    c.bg, c.bdrel = bwd_error_bound(c.R, c.dtype, c.family, c.ctx_err)
    got = got.double()
    sel = torch.ones_like(got, dtype=torch.bool) if rows is None else rows[None, :, None, :, None].expand_as(got)
    bad = sel & ~(torch.isfinite(got) & ((got - c.R.g).abs() <= c.bg))
    ratio = ((got - c.R.g).abs() / c.bg).masked_fill(~sel, 0.0).flatten(1).amax(-1)
    msg = f"attn bwd {label} {NAME[c.dtype]} B={c.B} L={c.L} heads={c.heads} D={c.D} scale={c.scale:.4f} bias={c.pb is not None} p={c.p:.4f}: " \
          f"max err/bound dQ {ratio[0].item():.3f} dK {ratio[1].item():.3f} dV {ratio[2].item():.3f}"
    if drel is not None:
        rr = ((drel.double() - c.R.drel).abs() / c.bdrel).max().item()
        msg += f" drel {rr:.3f}"
    print(msg)
    assert not bad.any(), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), ratio.tolist())
    if drel is not None:
        assert rr <= 1.0, rr
    if controls:
        assert c.L < 2 or len(c.live) >= 5, c.live
        missed = missed_controls(c)
        assert not missed, missed
    return ratio.max().item()


# ---------------------------------------------------------------------------------------------------------------
# CPU: the reference is the autograd of the forward; the bound admits an honest kernel and rejects the controls
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("p", [0.0, 0.3], ids=["nodrop", "drop"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_reference_is_the_autograd_of_the_forward(bias, p, ragged):
    """dQ, dK, dV and the binned bias gradient of bwd_reference against torch.autograd of the float64 forward (the forward file's
    attention_reference gives the value; the differentiable restatement below must equal it first).  The sequence without an unmasked
    key is uniform in both: its scores enter as s - stop_gradient(s), value 0 with the gradient passed on, which is what a kernel
    whose f32 mask term absorbs the score computes."""
    B, L, heads, D, scale = 4, 37, 2, 8, 0.3
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * L, 3 * heads * D, generator=g, dtype=torch.float64).requires_grad_()
    pb = torch.randn(heads, L, L, generator=g, dtype=torch.float64).requires_grad_() if bias else None
    dctx = torch.randn(B * L, heads * D, generator=g, dtype=torch.float64)
    mask = mixed_mask(B, L) if ragged else torch.ones(B, L, dtype=torch.long)
    if ragged:
        mask[3] = 0
    keep, ks = (drop_keep(11, B, heads, L, p), drop_threshold(p)[1]) if p > 0 else (None, 1.0)
    q, k, v = split_qkv(qkv, B, L, heads, D)
    s = scale * (q @ k.transpose(-1, -2))
    if bias:
        s = s + pb[None]
    nokey = ~(mask != 0).any(-1)[:, None, None, None]
    s = torch.where(nokey, s - s.detach(), s).masked_fill(~visibility(mask)[0][:, None], -math.inf)
    pd = torch.softmax(s, -1) * (1.0 if keep is None else keep.double() * ks)
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B, L, heads * D)
    value = attention_reference(qkv.detach(), mask, None if pb is None else pb.detach(), B, L, heads, D, scale, keep, ks)[0]
    assert torch.allclose(ctx.detach(), value, rtol=0, atol=1e-13)
    (ctx.reshape(B * L, -1) * dctx).sum().backward()
    R = bwd_reference(qkv.detach(), dctx, mask, None if pb is None else pb.detach(), B, L, heads, D, scale, keep, ks)
    want = torch.stack(split_qkv(qkv.grad, B, L, heads, D))
    assert torch.allclose(R.g, want, rtol=1e-11, atol=1e-12), (R.g - want).abs().max().item()
    assert torch.allclose(R.O.permute(0, 2, 1, 3).reshape(B, L, -1), value, rtol=0, atol=1e-13)
    if bias:
        assert torch.allclose(R.drel, rel_bins(pb.grad, L), rtol=1e-11, atol=1e-12)
        assert R.drel.shape == (heads, 2 * L - 1) and bool((R.drel.abs() > 0).all())
    if ragged:                                              # padded keys: exactly zero rows wherever the sequence has a key
        padded = ((mask == 0) & (mask != 0).any(-1, keepdim=True))[None, :, None, :, None].expand_as(R.g[1:])
        assert bool((R.g[1:][padded] == 0).all()) and bool((R.g[1:][~padded] != 0).any())


def emulate_bwd(c):
    """A kernel of the shape of the ones under test, in torch: f32 scores, softmax, dPd, delta and dS; dS (after the scale) and Pd
    rounded to the storage type before the f32 second contractions; the outputs rounded to the storage type; drel summed in f32.
    LONG: delta = dO . O with O the stored (rounded) forward output."""
    B, L, heads, D, dt = c.B, c.L, c.heads, c.D, TORCH_DT[c.dtype]
    x = c.qkv.float().view(B, L, 3, heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    dO = c.dctx.float().view(B, L, heads, D).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * torch.tensor(c.scale, dtype=torch.float32)
    if c.pb is not None:
        s = s + c.pb[None]
    s = s + ((c.mask == 0).float() * torch.finfo(torch.float32).min)[:, None, None, :]          # added in f32: absorbs the score
    e = torch.exp(s - s.amax(-1, keepdim=True))
    P = e * (1.0 / e.sum(-1, keepdim=True))
    M = torch.ones_like(P) if c.keep is None else c.keep.float() * np.float32(c.ks)
    r16 = (lambda t: t) if c.dtype == F32 else (lambda t: t.to(dt).float())
    dP = (dO @ v.transpose(-1, -2)) * M
    if c.family == "long":
        delta = (dO * c.ctx.float().view(B, L, heads, D).permute(0, 2, 1, 3)).sum(-1, keepdim=True)
    else:
        delta = (P * dP).sum(-1, keepdim=True)
    dL = P * (dP - delta)
    dS, Pd = r16(dL * np.float32(c.scale)), r16(P * M)
    g = torch.stack([dS @ k, dS.transpose(-1, -2) @ q, Pd.transpose(-1, -2) @ dO]).to(dt)
    return g, rel_bins(dL, L)


CPU_CASES = [(L, D, bias, p) for L, D in ((77, 64), (300, 64), (130, 32)) for bias, p in ((True, 0.0), (False, 0.1), (True, 0.1))]
CPU_FAMILY = {(77, 64): "generic", (300, 64): "long", (130, 32): "d32"}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L,D,bias,p", CPU_CASES)
def test_bound_admits_emulated_kernel_and_rejects_controls(dtype, L, D, bias, p):
    """Every case carries a bias or dropout, so that the reference alone gives at least five live controls (verify asserts the count;
    with both, all ten are live)."""
    B, heads, scale = 4, 2, SCALES[(L + D) % 3]
    mask = mixed_mask(B, L)
    mask[3] = 0                                              # a sequence without any unmasked key
    families = ["generic"] + (["long"] if CPU_FAMILY[(L, D)] == "long" and dtype != F32 else [])
    for family in families:                                  # the same inputs under both forms of delta
        c = prepare(dtype, B, L, heads, D, scale, mask, family, bias=bias, p=p, seed=1234)
        assert len(c.live) == (10 if bias and p else 7 if bias else 8), c.live
        got, drel = emulate_bwd(c)
        verify(c, got, drel if bias else None, "emulated " + family)


def test_live_controls_follow_the_shape():
    full = torch.ones(3, 8, dtype=torch.long)
    assert live_controls(full, 1, True, 0.1) == []                                       # one token: dS = 0
    assert set(live_controls(full, 8, False, 0.0)) == {"scale", "no_delta", "swap_dq_dk", "do_roll", "last_key"}
    one = torch.zeros(3, 8, dtype=torch.long)
    one[:, 0] = 1
    assert "last_key" not in live_controls(one, 8, False, 0.0)
    assert set(live_controls(full, 8, True, DROP_ODD)) == set(CONTROLS)
    for L in LENGTHS[1:]:                                                                # every GPU case of two tokens or more carries five
        assert len(live_controls(mixed_mask(3, L), L, False, 0.0)) >= 5


def test_hooks_are_bound():
    lib = N.lib()
    for name in ("om_debug_attention_bwd_ex", "om_debug_attention_bwd_stats_bytes", "om_debug_attention_bwd_last", "om_debug_attention_bwd_plan",
                 "om_debug_attn_drop_keep"):
        assert name in N.exported_symbols() and hasattr(lib, name)
    assert lib.om_debug_attention_bwd_stats_bytes(3, 5) == 3 * 5 * 3 * 512 * 4
    assert lib.om_debug_attention_bwd_ex(BF16, None, None, None, None, None, None, None, None, 1, 8, 64, 1, 0.125, 0.0, 0, None, 0, None) != 0
    assert b"null" in lib.om_last_error()
    assert lib.om_debug_attention_bwd_last() == 0                    # a refused call reads 0


def test_python_dropout_mask_equals_the_c_one():
    """the mask the reference applies to Pd and dP is attn_common.h's, at the pitches and rates the GPU cases use"""
    lib = N.lib()
    rng = np.random.default_rng(1)
    for (B, heads, Lm, p, seed) in ((3, 3, 100, 0.1, 0xBACC), (3, 3, 300, DROP_ODD, 0xBACC + 5), (6, 3, 200, 0.1, 4242)):
        keep = drop_keep(seed, B, heads, Lm, p).numpy()
        for _ in range(800):
            b, h, q, k = (int(rng.integers(B)), int(rng.integers(heads)), int(rng.integers(Lm)), int(rng.integers(Lm)))
            assert lib.om_debug_attn_drop_keep(seed, b, h, heads, Lm, q, k, p) == int(keep[b, h, q, k]), (Lm, p, b, h, q, k)


# ---------------------------------------------------------------------------------------------------------------
# the tables of the GPU cases, and the planner walk over them (no GPU)
# ---------------------------------------------------------------------------------------------------------------
B3, H3 = 3, 3                                    # B = heads = 3: a swapped blockIdx decomposition is not symmetric
BWD_LENGTHS = [1, 31, 32, 33, 64, 65, 100, 128, 129, 192, 193, 256, 257, 384, 511, 512]
D32_LENGTHS = [1, 31, 33, 64, 65, 128, 129, 192, 193, 256]


def letter(D, dtype, packed, fast, L):
    """BWD_TABLE's outcome at a length of the forward file's LENGTHS; at another length that of the next listed one on the same side
    of every threshold (100 -> 128)."""
    row = BWD_TABLE[(D, dtype != F32, packed)][fast]
    return row[LENGTHS.index(L if L in LENGTHS else min(x for x in LENGTHS if x >= L))]


def fam_of(D, dtype, L, fast=1, packed=False):
    f = BWD_LETTER[letter(D, dtype, packed, fast, L)]
    return (f, 4 if f == "long" else kt_of(L)) if isinstance(f, str) else f


# route -> (OM_OPT_ATTENTION_FAST, dtypes, lengths)
ROUTES = {
    "default": (1, DTYPES, lambda dtype: [L for L in BWD_LENGTHS if L <= (192 if dtype == F32 else 512)]),
    "fast0": (0, [BF16, F16], lambda dtype: [L for L in BWD_LENGTHS if L <= 256]),                 # GENERIC in 16 bits at every KT
    "long_all": (2, [BF16, F16], lambda dtype: [1, 33, 128, 129]),                                 # bit 1: LONG at every length
}
LENGTH_CASES = [(r, d, L) for r, (_, dts, ls) in ROUTES.items() for d in dts for L in ls(d)]
MASKS = [("bwd16", BF16, 64, 1), ("bwd16", F16, 64, 1), ("generic", F32, 64, 1), ("generic", BF16, 64, 0), ("generic", F16, 64, 0),
         ("long", BF16, 64, 2), ("long", F16, 64, 2), ("d32", F32, 32, 1), ("d32", BF16, 32, 1), ("d32", F16, 32, 1)]
BD = [(f, d, L, D, fast) for f, dts, Ls, D, fast in (("bwd16", (BF16, F16), (100, 128), 64, 1), ("generic", (F32,), (100, 128), 64, 1),
                                                    ("generic", (BF16, F16), (100, 128), 64, 0), ("long", (BF16, F16), (200, 300), 64, 1),
                                                    ("d32", DTYPES, (100, 128), 32, 1)) for d in dts for L in Ls]
DROPS = [0.0, 0.1, DROP_ODD]
# (family, dtype, D, L, fast, p, bias)
PACKED = [("bwd16", BF16, 64, 128, 1, 0.0, False), ("bwd16", F16, 64, 128, 1, 0.1, False), ("bwd16", BF16, 64, 128, 1, 0.1, True),
          ("d32", BF16, 32, 128, 1, 0.0, False), ("d32", F16, 32, 128, 1, 0.1, False), ("d32", BF16, 32, 200, 1, 0.1, False), ("d32", F16, 32, 200, 1, 0.0, False),
          ("generic", BF16, 64, 200, 1, 0.0, False), ("generic", F16, 64, 200, 1, 0.1, False), ("generic", BF16, 64, 200, 1, 0.1, True),
          ("generic", BF16, 64, 128, 0, 0.0, False), ("generic", F16, 64, 128, 0, 0.1, False)]


def packed_padded_fast(family, dtype, D, L, fast):
    """The switch under which the PADDED call runs the packed call's family: the case's own, except that at 200 tokens the shipped
    switch sends a padded 16-bit call to LONG where the packed one runs GENERIC -- the padded call then runs under 0."""
    return fast if fam_of(D, dtype, L, fast)[0] == family else 0


PACKED_REFUSALS = [(F32, 64, 128, "P"), (F32, 32, 128, "P"), (BF16, 64, 384, "C"), (F16, 64, 257, "C")]
# (family, dtype, D, L, fast)
NONFINITE = [("bwd16", BF16, 64, 100, 1), ("generic", F32, 64, 100, 1), ("generic", F16, 64, 200, 0), ("long", BF16, 64, 300, 1),
             ("d32", F16, 32, 100, 1), ("d32", F32, 32, 200, 1)]
NO_DREL_REFUSAL = b"a position bias needs its gradient buffer"
LONG_REFUSAL = b"needs the forward's output and a statistics buffer"


def test_backward_plan_names_what_the_gpu_cases_assert():
    n = 0
    for route, dtype, L in LENGTH_CASES:                                             # test_lengths
        fast = ROUTES[route][0]
        with option(N.OPT_ATTENTION_FAST, fast):
            assert planned_bwd(dtype, B3, L, H3, 64) == fam_of(64, dtype, L, fast), (route, NAME[dtype], L)
            n += 1
    want = {"default": {F32: "generic", BF16: None, F16: None}, "fast0": {BF16: "generic", F16: "generic"}, "long_all": {BF16: "long", F16: "long"}}
    for route, dtype, L in LENGTH_CASES:                                             # ... and the table of the issue, said once more
        f = want[route][dtype] or ("bwd16" if L <= 128 else "generic" if L <= 192 else "long")
        assert fam_of(64, dtype, L, ROUTES[route][0])[0] == f
    assert sorted({fam_of(64, d, L, 0)[1] for r, d, L in LENGTH_CASES if (r, d) == ("fast0", F16)}) == [1, 2, 4, 6, 8]
    for dtype in DTYPES:
        for L in D32_LENGTHS:                                                        # test_lengths_d32
            assert planned_bwd(dtype, B3, L, H3, 32) == ("d32", kt_of(L)) == fam_of(32, dtype, L)
            n += 1
    for family, dtype, D, fast in MASKS:                                             # test_masks
        with option(N.OPT_ATTENTION_FAST, fast):
            assert planned_bwd(dtype, 12, 128, H3, D) == (family, 4)
            n += 1
    for family, dtype, L, D, fast in BD:                                             # test_bias_dropout
        with option(N.OPT_ATTENTION_FAST, fast):
            for bias in (False, True):
                assert planned_bwd(dtype, B3, L, H3, D, bias=bias) == (family, 4 if family == "long" else kt_of(L)), (family, NAME[dtype], L, bias)
                n += 1
    for family, dtype, D, L, fast, p, bias in PACKED:                                # test_packed_rows: the padded call, then the packed one
        for packed in (False, True):
            with option(N.OPT_ATTENTION_FAST, fast if packed else packed_padded_fast(family, dtype, D, L, fast)):
                got = planned_bwd(dtype, 6, L, H3, D, bias=bias, packed=packed)
                assert got == (family, kt_of(L)) and (not packed or got == fam_of(D, dtype, L, fast, True)), (family, NAME[dtype], L, packed, got)
                n += 1
    for dtype, D, L, why in PACKED_REFUSALS:                                         # test_packed_refusals
        assert BWD_LETTER[why] in planned_bwd(dtype, 2, L, H3, D, packed=True) and letter(D, dtype, True, 1, L) == why
        n += 1
    for family, dtype, D, L, fast in NONFINITE:                                      # test_non_finite, test_deterministic
        with option(N.OPT_ATTENTION_FAST, fast):
            assert planned_bwd(dtype, B3, L, H3, D) == (family, 4 if family == "long" else kt_of(L)), (family, NAME[dtype], L)
            n += 1
    assert n == len(LENGTH_CASES) + 30 + len(MASKS) + 2 * len(BD) + 2 * len(PACKED) + len(PACKED_REFUSALS) + len(NONFINITE)
    assert len(LENGTH_CASES) == 10 + 2 * 16 + 2 * 12 + 2 * 4
    # test_bias_without_gradient_buffer, test_long_pairs_with_the_forward_kernel
    assert planned_bwd(BF16, B3, 100, H3, 64, bias=True, drel=False) == ("generic", 4) and planned_bwd(F16, B3, 100, H3, 64, bias=True) == ("bwd16", 4)
    assert NO_DREL_REFUSAL in planned_bwd(BF16, B3, 100, H3, 32, bias=True, drel=False)
    assert planned_bwd(BF16, B3, 300, H3, 64) == planned_bwd(F16, B3, 300, H3, 64) == ("long", 4)


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def new_drel(heads, L):
    n = heads * (2 * L - 1)
    t = torch.full((n + 64,), DREL_GUARD, dtype=torch.float32, device=DEV)
    t[:n] = DREL_FILL
    return t


def new_stats(B, heads):
    """NaN everywhere: a slot that pass B reads and pass A did not write shows up in dK / dV"""
    return torch.full((N.lib().om_debug_attention_bwd_stats_bytes(B, heads) // 4 + 64,), math.nan, dtype=torch.float32, device=DEV)


def launch(dtype, qkv, ctx, dctx, dqkv, mask, bias, drel, stats, B, L, H, heads, scale, p=0.0, seed=0, cu=None, packed=0):
    rc = N.lib().om_debug_attention_bwd_ex(dtype, N.ptr(qkv), N.ptr(ctx), N.ptr(dctx), N.ptr(dqkv), N.ptr(mask), N.ptr(bias), N.ptr(drel),
                                           N.ptr(stats), B, L, H, heads, scale, p, seed, N.ptr(cu), packed, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


def last_bwd():
    last = N.lib().om_debug_attention_bwd_last()
    return last & 0xFF, last >> 8


def grads_of(dqkv, B, L, heads, D):
    return torch.stack(split_qkv(dqkv, B, L, heads, D))


def run_launch(c, family, kt, use_drel=None, ctx=None):
    """One padded launch of case c with every guard: return code, family, inputs bit-unchanged, sentinels.  Returns (dqkv rows, drel - fill)."""
    dtype, B, L, heads, H = c.dtype, c.B, c.L, c.heads, c.H
    use_drel = (c.pb is not None) if use_drel is None else use_drel
    ctx = (c.ctx if ctx is None else ctx) if family == "long" else None
    stats = new_stats(B, heads) if family == "long" else None
    drel = new_drel(heads, L) if use_drel else None
    dqkv = new_ctx(B * L, 3 * H, dtype)
    held = [t if t is None else t.clone() for t in (c.qkv, ctx, c.dctx, c.mask, c.pb)]
    rc = launch(dtype, c.qkv, ctx, c.dctx, dqkv, c.mask, c.pb, drel, stats, B, L, H, heads, c.scale, c.p, c.seed)
    assert rc == 0, N.lib().om_last_error()
    assert last_bwd() == (BFAM[family], kt), (family, kt, last_bwd())
    for now, then in zip((c.qkv, ctx, c.dctx, c.mask, c.pb), held):
        assert now is None or torch.equal(now.view(torch.uint8), then.view(torch.uint8)), "an input was written"
    assert untouched(dqkv[B * L:], dtype), "rows after dqkv were written"
    if drel is not None:
        n = heads * (2 * L - 1)
        assert bool((drel[n:] == DREL_GUARD).all()), "floats after drel were written"
        drel = (drel[:n] - DREL_FILL).view(heads, 2 * L - 1)
    return dqkv[:B * L], drel


def run_case(dtype, B, L, heads, D, scale, mask, family, kt, bias=False, p=0.0, seed=0, tag=0, label=""):
    """One launch against the reference: family, guards, bound, controls; padded keys' dK / dV rows exactly zero."""
    c = prepare(dtype, B, L, heads, D, scale, mask, family, bias=bias, p=p, seed=seed, tag=tag, device=DEV)
    dqkv, drel = run_launch(c, family, kt)
    got = grads_of(dqkv, B, L, heads, D)
    verify(c, got, drel, f"{family}/{kt}{label}")
    m = c.mask != 0
    padded = (~m & m.any(-1, keepdim=True))[None, :, None, :, None].expand_as(got[1:])
    assert bool((got[1:][padded] == 0).all()), "dK / dV of a padded key is not zero"
    return c, dqkv, drel


@pytest.mark.gpu
@pytest.mark.parametrize("route,dtype,L", LENGTH_CASES, ids=[f"{r}-{NAME[d]}-{L}" for r, d, L in LENGTH_CASES])
def test_lengths(route, dtype, L):
    """Every 64-wide family x format at every length edge.  default: BWD16 up to 128, GENERIC to 192, LONG beyond (f32: GENERIC to
    192); fast0: GENERIC in 16 bits at every KT (1, 2, 4, 6, 8); long_all (bit 1): LONG below its usual range."""
    fast = ROUTES[route][0]
    family, kt = fam_of(64, dtype, L, fast)
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, B3, L, H3, 64, SCALES[BWD_LENGTHS.index(L) % 3], mixed_mask(B3, L), family, kt, tag=fast)


@pytest.mark.gpu
@pytest.mark.parametrize("L", D32_LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_lengths_d32(dtype, L):
    run_case(dtype, B3, L, H3, 32, SCALES[(D32_LENGTHS.index(L) + 1) % 3], mixed_mask(B3, L), "d32", kt_of(L))


@pytest.mark.gpu
@pytest.mark.parametrize("family,dtype,D,fast", MASKS, ids=[f"{f}-{NAME[d]}" for f, d, _, _ in MASKS])
def test_masks(family, dtype, D, fast):
    """The eleven mask patterns and a sequence without any key (compared against the uniform reference); run_case asserts the exactly
    zero dK / dV rows of the padded keys, and compares the padded QUERY rows like any other."""
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, 12, 128, H3, D, 0.125 if D == 64 else SCALES[1], masks_eleven(), family, 4, tag=fast)


@pytest.mark.gpu
@pytest.mark.parametrize("p", DROPS, ids=["nodrop", "drop", "dropodd"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("family,dtype,L,D,fast", BD, ids=[f"{f}-{NAME[d]}-{L}" for f, d, L, _, _ in BD])
def test_bias_dropout(family, dtype, L, D, fast, bias, p):
    """{bias + drel, none} x {p = 0, 0.1, DROP_ODD} at a length that fills its tiles and one that does not; drel is pre-filled with
    DREL_FILL and expected as reference + DREL_FILL."""
    i = BD.index((family, dtype, L, D, fast))
    with option(N.OPT_ATTENTION_FAST, fast):
        run_case(dtype, B3, L, H3, D, SCALES[i % 3], mixed_mask(B3, L), family, 4 if family == "long" else kt_of(L), bias=bias, p=p,
                 seed=0xBACC + i, tag=i)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_bias_without_gradient_buffer(dtype):
    """A bias without drel: 64-wide heads run GENERIC (where the same call with the buffer runs BWD16), add the bias and leave no
    gradient of it anywhere -- no buffer is passed, and rows after dqkv keep the sentinel; 32-wide heads refuse with the planner's text."""
    L = 100
    c = prepare(dtype, B3, L, H3, 64, 0.125, mixed_mask(B3, L), "generic", bias=True, device=DEV)
    dqkv, drel = run_launch(c, "generic", 4, use_drel=False)
    assert drel is None
    c.live = [x for x in c.live if x != "drel_shift"]
    verify(c, grads_of(dqkv, B3, L, H3, 64), None, "generic/4 bias, no drel")
    c = prepare(dtype, B3, L, H3, 32, SCALES[1], mixed_mask(B3, L), "d32", bias=True, device=DEV)
    dqkv = new_ctx(B3 * L, 3 * c.H, dtype)
    assert launch(dtype, c.qkv, None, c.dctx, dqkv, c.mask, c.pb, None, None, B3, L, c.H, H3, SCALES[1]) != 0
    assert NO_DREL_REFUSAL in N.lib().om_last_error() and last_bwd() == (0, 0) and untouched(dqkv, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_long_pairs_with_the_forward_kernel(dtype, p):
    """The real pairing: ctx from om_debug_attention_ex with the same (p, seed), so forward and backward must regenerate the same
    mask -- delta = dO . O only equals rowsum(P o dP) then.  ctx_err is the forward file's error_bound of that output."""
    B, L, heads, D, scale, seed = B3, 300, H3, 64, 0.125, 0xF00D
    c = prepare(dtype, B, L, heads, D, scale, mixed_mask(B, L), "long", p=p, seed=seed, tag=9, device=DEV)
    ctx = new_ctx(B * L, c.H, dtype)
    assert launch_fwd(dtype, c.qkv, ctx, c.mask, None, B, L, c.H, heads, scale, p, seed) == 0
    ref, mag, smax, vabs = attention_reference(c.qkv, c.mask, None, B, L, heads, D, scale, c.keep, c.ks)
    fb = error_bound(ref, mag, smax, vabs, L, D, dtype).reshape(B * L, c.H)
    assert bool(((ctx[:B * L].double() - c.ctx_ref).abs() <= fb).all())
    c.ctx_err = fb
    dqkv, _ = run_launch(c, "long", 4, ctx=ctx[:B * L].clone())
    verify(c, grads_of(dqkv, B, L, heads, D), None, "long/4 ctx of the forward kernel")


@pytest.mark.gpu
def test_long_needs_ctx_and_stats():
    L = 300
    c = prepare(BF16, B3, L, H3, 64, 0.125, mixed_mask(B3, L), "long", device=DEV)
    for ctx, stats in ((None, new_stats(B3, H3)), (c.ctx, None)):
        dqkv = new_ctx(B3 * L, 3 * c.H, BF16)
        assert launch(BF16, c.qkv, ctx, c.dctx, dqkv, c.mask, None, None, stats, B3, L, c.H, H3, 0.125) != 0
        assert LONG_REFUSAL in N.lib().om_last_error() and last_bwd() == (0, 0) and untouched(dqkv, BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("family,dtype,D,L,fast,p,bias", PACKED,
                         ids=[f"{f}-{NAME[d]}-{L}-fast{s}-{'drop' if p else 'nodrop'}{'-bias' if b else ''}" for f, d, _, L, s, p, b in PACKED])
def test_packed_rows(family, dtype, D, L, fast, p, bias):
    """cu: the rows that exist meet the bound against the reference of their own sequence and carry the bits of the padded call of the
    same family (dctx zero beyond each extent, see the docstring); the dropout mask is the padded call's, keyed on the pitch; rows from
    cu[B] on keep the sentinel; a sequence of length 0 (its mask row empty, its kmax set to 0) writes nothing; drel within its bound."""
    B, heads, H, kt, seed = 6, H3, H3 * D, kt_of(L), 4242
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate((L, 1, L // 2 + 1, 33, 0, 0)):
        mask[b, :n] = 1
    mask[4, 0] = 1; mask[4, 5] = 1                         # holes inside a packed sequence: rows 0 .. 5 exist
    with option(N.OPT_ATTENTION_FAST, packed_padded_fast(family, dtype, D, L, fast)):
        c = prepare(dtype, B, L, heads, D, 0.125, mask, family, bias=bias, p=p, seed=seed, tag=77, device=DEV, zero_dctx_past_extent=True)
        padded, drel0 = run_launch(c, family, kt)
        verify(c, grads_of(padded, B, L, heads, D), drel0, f"{family}/{kt} padded")
    with option(N.OPT_ATTENTION_FAST, fast):
        kmax = mask_extent(c.mask)
        assert kmax.tolist() == [L, 1, L // 2 + 1, 33, 6, L]
        kmax[5] = 0                                         # the empty sequence
        rows = int(kmax.sum()) + 7
        cu, _, row_map = pack_rows(kmax, L, rows)
        total = int(cu[B])
        assert total == rows - 7 and int(cu[5]) == int(cu[6])
        src = row_map[:total].long()
        qp = torch.zeros(rows, 3 * H, dtype=TORCH_DT[dtype], device=DEV)
        dp = torch.zeros(rows, H, dtype=TORCH_DT[dtype], device=DEV)
        qp[:total], dp[:total] = c.qkv[src], c.dctx[src]
        dqkv = new_ctx(rows, 3 * H, dtype)
        drel = new_drel(heads, L) if bias else None
        assert launch(dtype, qp, None, dp, dqkv, c.mask, c.pb, drel, None, B, L, H, heads, 0.125, p, seed, cu=cu, packed=1) == 0, N.lib().om_last_error()
        assert last_bwd() == (BFAM[family], kt)
    assert torch.equal(bits(dqkv, dtype)[:total], bits(padded, dtype)[src])
    assert untouched(dqkv[total:], dtype), "rows from cu[B] on were written"
    exist = torch.zeros(B * L, dtype=torch.bool, device=DEV)
    exist[src] = True
    full = torch.zeros(B * L, 3 * H, dtype=TORCH_DT[dtype], device=DEV)
    full[src] = dqkv[:total]
    d = None
    if bias:
        n = heads * (2 * L - 1)
        assert bool((drel[n:] == DREL_GUARD).all())
        d = (drel[:n] - DREL_FILL).view(heads, 2 * L - 1)
    verify(c, grads_of(full, B, L, heads, D), d, f"{family}/{kt} packed", controls=False, rows=exist.view(B, L))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,L,why", PACKED_REFUSALS, ids=[f"{NAME[d]}-{D}-{L}-{w}" for d, D, L, w in PACKED_REFUSALS])
def test_packed_refusals(dtype, D, L, why):
    """BWD_LETTER's "P" (packed rows are 16-bit only) and "C" (the tile-at-a-time pair does not read cu) through the hook"""
    B, H = 2, H3 * D
    c = prepare(dtype, B, L, H3, D, 0.125, torch.ones(B, L, dtype=torch.long), "generic", device=DEV)
    cu = torch.tensor([0, L, 2 * L, 2 * L], dtype=torch.int32, device=DEV)
    dqkv = new_ctx(B * L, 3 * H, dtype)
    assert launch(dtype, c.qkv, c.ctx, c.dctx, dqkv, c.mask, None, None, new_stats(B, H3), B, L, H, H3, 0.125, cu=cu, packed=1) != 0
    assert BWD_LETTER[why] in N.lib().om_last_error() and last_bwd() == (0, 0) and untouched(dqkv, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("family,dtype,D,L,fast", NONFINITE, ids=[f"{f}-{NAME[d]}-{L}" for f, d, _, L, _ in NONFINITE])
def test_non_finite_dctx_stays_where_it_belongs(family, dtype, D, L, fast):
    """A NaN in the dctx row of one unmasked query (one head's columns) under full attention: dQ of that row and dK / dV of that
    (sequence, head) are not finite -- every key of it sees the query -- the other queries of the (sequence, head) keep a finite dQ,
    and every other (sequence, head) stays inside the bound of the clean reference."""
    B, heads, kt = B3, H3, 4 if family == "long" else kt_of(L)
    b, h, j = 1, 2, L // 2
    with option(N.OPT_ATTENTION_FAST, fast):
        c = prepare(dtype, B, L, heads, D, 0.125, torch.ones(B, L, dtype=torch.long), family, tag=5, device=DEV)
        c.dctx[b * L + j, h * D:(h + 1) * D] = math.nan
        got = grads_of(run_launch(c, family, kt)[0], B, L, heads, D)
    hit = torch.zeros_like(got, dtype=torch.bool)
    hit[1:, b, h] = True
    hit[0, b, h, j] = True
    assert not torch.isfinite(got[hit]).any()
    assert torch.isfinite(got[0, b, h, torch.arange(L, device=DEV) != j]).all()
    other = torch.ones_like(got, dtype=torch.bool)
    other[:, b, h] = False
    c.dctx[b * L + j, h * D:(h + 1) * D] = 0
    c.R = bwd_reference(c.qkv, c.dctx, c.mask, None, B, L, heads, D, 0.125)
    c.ctx_ref = c.R.O.permute(0, 2, 1, 3).reshape(B * L, c.H)
    bg, _ = bwd_error_bound(c.R, dtype, family, c.ctx_err)
    ok = torch.isfinite(got) & ((got - c.R.g).abs() <= bg)
    assert bool(ok[other].all())


@pytest.mark.gpu
@pytest.mark.parametrize("family,dtype,D,L,fast", NONFINITE, ids=[f"{f}-{NAME[d]}-{L}" for f, d, _, L, _ in NONFINITE])
def test_deterministic(family, dtype, D, L, fast):
    """Two identical launches (bias, drel, dropout): dqkv bit-identical; drel, f32 atomics in arbitrary order, within its bound twice."""
    kt = 4 if family == "long" else kt_of(L)
    with option(N.OPT_ATTENTION_FAST, fast):
        c = prepare(dtype, B3, L, H3, D, 0.125, mixed_mask(B3, L), family, bias=True, p=0.1, seed=31, tag=3, device=DEV)
        c.bg, c.bdrel = bwd_error_bound(c.R, dtype, family, c.ctx_err)
        a, da = run_launch(c, family, kt)
        b, db = run_launch(c, family, kt)
    assert torch.equal(bits(a, dtype), bits(b, dtype))
    for d in (da, db):
        assert bool(((d.double() - c.R.drel).abs() <= c.bdrel).all())
