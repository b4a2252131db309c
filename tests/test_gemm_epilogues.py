"""The GEMM epilogues om_gemm_nt cannot express, kernel by kernel, against float64: the fused-LayerNorm and two-plane epilogues of
generation 7, the training epilogues (tape, dropout, gelu'), the f32-stream and pending-LayerNorm extras of the few-rows kernel and the
K-sliced weight-gradient contraction.  They are reached through om_debug_gemm_ex (the whole GemmEpilogue from C), om_debug_gemm_plan_ex
(the planner alone, no GPU) and om_debug_gemm_splitk.  The harness is tests/test_gemm_kernels.py's (Buf with its sentinel guard rows,
gemm_options, violations, act64, the U_* constants); the dropout hash and the eight-bit plane's index come from tests/test_row_kernels.py.

Every GPU case names the family it must reach (om_debug_gemm_last), compares every output element with a float64 reference computed from
the stored (rounded) inputs, carries a reference-side negative control its bound must reject, and checks that guard rows, the ldc padding
and every input come back bit-unchanged.

The bounds (u = 2^-24, U = half an ulp of the output format, S = 2^-16 bfloat16 | 2^-22 float16: the hi + lo split of an accumulator-init
factor, three cross terms of which are dropped or rounded):
  accumulation     (K + 8) u sum|a||b|        (K products, the six slots of the rank-2 initialisation, the bias; test_gemm_kernels: K + 2)
  LNF 1            out = act(rstd (A B^T - mu s) + b): the accumulation error times rstd, 3 S (|mu s| + |b| / rstd) rstd for the split,
                   2 u |rstd mu s| for the rounding of mu (the cancellation term), rel_rstd |rstd (acc - mu s)|, 2 RSQRT |b| (sqrt(var) times
                   rsqrt(var) is not 1), where rel_rstd = RSQRT_REL + 0.5 * 4 u (E[x^2] + mu^2) / var: var = E[x^2] - mu^2 is a difference of
                   f32 roundings and a row of mean 3 and deviation 1/4 amplifies them 145 times
  LNF 2 .. 4       y = A B^T + bias + ((r rstd - mu rstd) g + b): accumulation, 3 S |bias|, |g| (rel_rstd + 3 u)(|r rstd| + |mu rstd|), 2 u |r'|,
                   2 u |y|; C = round16(y): + U |y|; a statistics slot sums 128 unrounded y: sum of their bounds + 136 u sum|y| (squares:
                   sum(2 |y| e + e^2) + 136 u sum y^2); C + out_lo: + U^2 |y| (the second rounding); C + e5m2: + 2^-3 U |y| + 2^-27
  activation       the slope (GELU_LIP) times the error before it, + the fit: GRAD_FIT |x| (16-bit erf-GELU: the same Phi fit as gelu', below;
                   test_gemm_kernels.py's PHI_FIT = 7.4e-6 understates it and passes because the 16-bit rounding dominates), 16 u |x| (tanh),
                   8 u |x| (libm)
  gelu'            slope 0.8 (max |gelu''| = 2 phi(0)) times the error before it, + for 16-bit outputs GRAD_FIT = 1.34e-5: the error of
                   gelu_erf_grad_fast's degree-8 fit of Phi, computed in float64 from the kernel's own coefficients (1.3293e-5 at |x| = 2.23,
                   1 - Phi(4.2) = 1.335e-5 beyond the clamp: test_cpu_gelu_grad_fit_error); 16 u for f32 (libm)
  dropout          kept elements: everything above times keep_scale (DropCfg); dropped elements are compared on bits
  few rows         accumulation (K + 10) u sum|a||b|: K products, seven additions of the eight waves' partial sums, the bias, the residual, the
                   sum; a_ln32 / rln32: the normalisation is compared bit for bit with the LayerNorm kernels; against float64 the operand
                   rounding U |LN(x)| per element enters as U sum|LN(x)||w|; (mean, rstd) within RSQRT_REL + the f32 sums of a row
  split-K          (K + slices + 2) u sum|a||b| + u |C0|, nothing else; two runs within that bound of each other
Hardware constants: rsqrtf is tests/test_row_kernels.py's RSQRT_REL (measured there, 1.47e-7, doubled); no other constant is measured here
-- sqrtf only feeds the 16-bit split, exp2 sits inside GRAD_FIT's 5e-8 of evaluation slack, five orders below the 16-bit rounding it precedes.

Which test reaches which kernel (family / LNF / format -> test):
  G7 (restart per tile)  LNF 1 bf16 none erf relu tanh tanh x resid, f16 none erf relu     test_lnf1[...-restart], test_k128_selects_restart
                         LNF 2, LNF 3 bf16 f16                                              test_lnf2[...-restart], test_lnf3[...-restart]
  G7C16                  LNF 1 bf16 none erf relu tanh, f16 none erf relu                   test_lnf1[...-ring]
  G7R16                  LNF 2, LNF 3 bf16 f16; LNF 4 f16                                   test_lnf2[...-ring], test_lnf3[...-ring], test_lnf4
  G7C16 TRAIN            bf16 f16: erf + gelu' tape                                         test_pre_act_two_output_ring
  V1, V2 (bf16, f16, f32, bf16 -> f32) and V6 (bf16, f32: every training form of launch6_has), one test case per family and format:
    none + resid + dropout (p 0.1, 0.5; drop_rows NULL, identity, permutation)             test_dropout_residual
    erf + tape (acc + bias), erf + tape (gelu', OM_ACT_PRE_GRAD), ldp != ldc               test_pre_act
    relu + tape + dropout (T5 FFN1)                                                        test_pre_act
    tanh x resid + tape + dropout + drop_rows (gated T5 FFN1, one call)                    test_pre_act
    tanh + tape + dropout, none + tape + dropout (no residual)                             test_pre_act
    OM_ACT_GELU_ERF_GRAD x resid; none x resid (no training flag: the gelu' tape backward) test_gelu_grad
  few rows bf16 f16      resid32 / out32                                                    test_few_rows_f32_stream
                         a_ln32 (+ a_ln_stats_out); rln32; row m of 64 = the row alone      test_few_rows_a_ln32, _rln32, _batch_invariance
  split-K                bf16 f16 f32                                                       test_splitk
The CPU half checks the references against plain torch compositions, holds an emulated kernel (f32 accumulation, 16-bit rounding, the
hi + lo split, e5m2) inside every bound, has every control rejected, and walks om_debug_gemm_plan_ex over the case tables.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.test_gemm_kernels import (BF16, DEV, F16, F32, FAM, FLOOR, GELU_LIP, NAME, TORCH_DT, U_ACC, U_OUT, Buf, _bits, act64,
                                     gemm_options, violations)
from tests.test_row_kernels import RSQRT_REL, keep_of, lo8_offset

u = U_ACC
SPLIT = {BF16: 2.0 ** -16, F16: 2.0 ** -22}
SPLIT_FLOOR = {BF16: 2.0 ** -126, F16: 2.0 ** -25}          # a lo part below the format's normal range: half its subnormal spacing
GRAD_FIT = 1.34e-5                                            # |gelu_erf_grad_fast(x) - gelu'(x)| for every x: see grad_fast_port


def grad_fast_port(x):
    """gelu_erf_grad_fast (csrc/gemm_epilogue.h) in float64: Phi(x) = 0.5 + xc Q(xc^2), xc = clamp(x, +-4.2), plus x phi(x).  Against the
    exact gelu' its error is the fit's: largest 1.3293e-5 at |x| = 2.23 inside the clamp, and 1 - Phi(4.2) = 1.335e-5 in the limit beyond
    it (test_cpu_gelu_grad_fit_error).  GRAD_FIT is that supremum plus 5e-8 for the f32 evaluation (nine fused multiply-adds on values
    below 1, the hardware exp2 on x phi(x) <= 0.242).  The source comment's 7.4e-6 is not the maximum: 9.5e-6 already at x = -0.75."""
    xc = x.clamp(-4.2, 4.2)
    t = xc * xc
    q = torch.full_like(x, 5.998145036e-11)
    for c in (-5.633389311e-09, 2.343703613e-07, -5.760840850e-06, 9.457556007e-05, -1.114161685e-03, 9.830250405e-03, -6.636118144e-02,
              3.989123106e-01):
        q = q * t + c
    return 0.5 + xc * q + x * 0.3989422804014327 * torch.exp2(-0.7213475204444817 * x * x)


def grad_fast_err(x):
    return torch.full_like(x, GRAD_FIT)


GRAD_LIP = 0.8                                                # max |gelu''| = 2 phi(0)
EPS = 1e-5
ERF, RELU, TANH, NONE = N.ACT_GELU_ERF, N.ACT_RELU, N.ACT_GELU_TANH, N.ACT_NONE
CONT = 495                                                    # OM_OPT_GEMM_CONT's default: bits 0-3, 5-8
RESTART = CONT & ~3                                           # bits 0 / 1 cleared: one-plane epilogues on the restart-per-tile kernel


def record(label, got, ref, bound):
    """print the largest |error| / bound over the finite elements (pytest -s shows it: the figures of the commit message)"""
    fin = torch.isfinite(ref) & torch.isfinite(bound) & (bound > 0)
    if fin.any():
        d = (got.double() - ref).abs()
        r = float(torch.where(fin & torch.isfinite(d), d / bound, torch.zeros_like(d)).max())
        print(f"ratio {label}: {r:.3f}")


def assert_within(label, got, ref, bound, out_dt=None):
    record(label, got, ref, bound)
    bad = violations(got, ref, bound, out_dt)
    if bad.any():
        idx = bad.nonzero()[:4].tolist()
        detail = [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
        raise AssertionError(f"{label}: {int(bad.sum())} elements outside the float64 bound, e.g. (index, got, ref, bound) {detail}")


def rejected(ref, ctl, bound):
    """a negative control: somewhere the control differs from the reference by more than the bound"""
    fin = torch.isfinite(ref) & torch.isfinite(bound) & torch.isfinite(ctl)
    return bool((((ctl - ref).abs() > bound) & fin).any())


# ---------------------------------------------------------------------------------------------------------------
# float64 references and bounds (device-agnostic)
# ---------------------------------------------------------------------------------------------------------------
def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def row_stats(x):
    """(sum, sum of squares) per row in float64, rounded to the f32 the kernels read"""
    x = x.double()
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).float()


def ln_scalars(stats, inv_h, eps, rms=0):
    """mu, rstd in float64 from the STORED f32 statistics, and the relative error of the kernel's f32 rstd (module docstring)"""
    st = stats.double()
    m2 = st[:, 1] * inv_h
    mu = torch.zeros_like(m2) if rms else st[:, 0] * inv_h
    var = (m2 - mu * mu).clamp_min(0.0) + eps
    rel = RSQRT_REL + 0.5 * 4 * u * (m2.abs() + mu * mu) / var
    return mu, var.rsqrt(), rel


def tail(pre, e_pre, act, resid, mul, out_dt, fast=True, scale=1.0, keep=None):
    """out = round(keep scale act(pre) (+|x) resid) and its bound, given |kernel's pre - pre| <= e_pre"""
    U = U_OUT[out_dt]
    y = act64(act, pre)
    prop = e_pre * (GELU_LIP if act in (ERF, TANH) else 1.0)
    if act == ERF:
        prop = prop + pre.abs() * (GRAD_FIT if fast else 8 * u)        # the same Phi fit as gelu': GRAD_FIT, not test_gemm_kernels' PHI_FIT
    elif act == TANH:
        prop = prop + pre.abs() * 16 * u
    y, prop = y * scale, prop * scale * (1 + u)
    if keep is not None:
        y, prop = torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, prop, torch.zeros_like(prop))
    if resid is None:
        out, rnd = y, U * y.abs()
    else:
        r = resid.double()
        if mul:
            out, prop = y * r, prop * r.abs()
            rnd = U * out.abs()
        else:
            out, rnd = y + r, U * (y.abs() + r.abs())
    return out, rnd + prop * (1 + U) + FLOOR[out_dt]


def _vec(v, n, like):
    return v.double() if v is not None else torch.zeros(n, dtype=torch.float64, device=like.device)


def lnf1_reference(A, B, stats, colsum, bias, act, gate, inv_h, eps, rms, dt, ctl=None):
    """C = act(rstd_m (A B^T - mu_m s_n) + bias_n) [x gate] and its bound.  ctl: 'row' (the neighbouring row's statistics), 'colsum' /
    'bias' (rolled by one column)"""
    a, b = A.double(), B.double()
    K, Nn = a.shape[1], b.shape[0]
    acc, mag = a @ b.t(), a.abs() @ b.abs().t()
    mu, rstd, rel = ln_scalars(stats, inv_h, eps, rms)
    s, bb = _vec(colsum, Nn, a), _vec(bias, Nn, a)
    if ctl == "row":
        mu, rstd = torch.roll(mu, 1), torch.roll(rstd, 1)
    if ctl == "colsum":
        s = torch.roll(s, 1)
    if ctl == "bias":
        bb = torch.roll(bb, 1)
    mu, rstd, rel = mu[:, None], rstd[:, None], rel[:, None]
    mus = (mu * s).abs()
    core = acc - mu * s
    pre = rstd * core + bb
    binit = bb.abs() / rstd
    e_pre = (rstd * ((K + 8) * u * (mag + mus + binit) + 3 * SPLIT[dt] * (mus + binit) + 2 * u * mus +
                     SPLIT_FLOOR[dt] * (mu.abs() + s.abs() + 1 / rstd + bb.abs())) +
             rel * (rstd * core).abs() + 2 * RSQRT_REL * bb.abs() + 2 * u * pre.abs())
    return tail(pre, e_pre, act, gate, True, dt)


def lnf2_reference(A, B, bias, resid, resid_lo, rln_stats, g, b, inv_h, eps, dt, ctl=None):
    """y = A B^T + bias + LN(resid [+ resid_lo]) (no statistics: the residual itself), unrounded, and the bound of the kernel's f32 y.
    ctl: 'row' (the neighbouring row's statistics), 'rln_b' (rolled by one column), 'lo' (the second plane dropped)"""
    a, w = A.double(), B.double()
    K, Nn = a.shape[1], w.shape[0]
    acc, mag = a @ w.t(), a.abs() @ w.abs().t()
    bb = _vec(bias, Nn, a)
    r = resid.double()
    e_r = torch.zeros_like(r)
    if resid_lo is not None and ctl != "lo":
        r = r + resid_lo.double()
        e_r = u * r.abs()
    if rln_stats is not None:
        mu, rstd, rel = ln_scalars(rln_stats, inv_h, eps)
        if ctl == "row":
            mu, rstd = torch.roll(mu, 1), torch.roll(rstd, 1)
        beta = torch.roll(b.double(), 1) if ctl == "rln_b" else b.double()
        mu, rstd, rel = mu[:, None], rstd[:, None], rel[:, None]
        t = (r * rstd).abs() + (mu * rstd).abs()
        rp = (r * rstd - mu * rstd) * g.double() + beta
        e_r = g.double().abs() * ((rel + 3 * u) * t + e_r * rstd) + 2 * u * rp.abs()
    else:
        rp = r
    y = acc + bb + rp
    e_y = (K + 8) * u * (mag + bb.abs()) + 3 * SPLIT[dt] * bb.abs() + SPLIT_FLOOR[dt] * (1 + bb.abs()) + e_r + 2 * u * y.abs()
    return y, e_y


def stored_bound(y, e_y, dt):
    return U_OUT[dt] * y.abs() + e_y * (1 + U_OUT[dt]) + FLOOR[dt]


def slot_stats(y, e_y):
    """[N / 128 slots][M][2] (sum, sum of squares) of the unrounded y over each run of 128 columns, and the bound"""
    M, Nn = y.shape
    yy, ee = y.view(M, Nn // 128, 128), e_y.view(M, Nn // 128, 128)
    s1, s2 = yy.sum(2), (yy * yy).sum(2)
    b1 = ee.sum(2) + 136 * u * yy.abs().sum(2)
    b2 = (2 * yy.abs() * ee + ee * ee).sum(2) + 136 * u * s2
    return torch.stack([s1, s2], 2).permute(1, 0, 2).contiguous(), torch.stack([b1, b2], 2).permute(1, 0, 2).contiguous() + 2.0 ** -126


def half_ulp(c, dt):
    """half the spacing of the format at |c| (the largest remainder a round-to-nearest word can leave)"""
    a = c.detach().double().abs().cpu().clamp_min(2.0 ** -14 if dt == F16 else 2.0 ** -126)       # (frexp on the host)
    _, e = torch.frexp(a)
    return (torch.ldexp(torch.ones_like(a), e - 1) * U_OUT[dt]).to(c.device)


def lo8_index(M, Nn, device):
    m, n = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(Nn, dtype=np.int64), indexing="ij")
    return torch.from_numpy(lo8_offset(m, n, Nn)).to(device)


def lo8_decode(blob, M, Nn):
    """the eight-bit plane as float64 [M, N]: e5m2 of the remainder * 2^10"""
    b = blob[lo8_index(M, Nn, blob.device)].cpu()                                    # (the conversion itself on the host)
    return (b.view(torch.float8_e5m2).double() * 2.0 ** -10).to(blob.device)


def lo8_encode(rem, M, Nn):
    blob = torch.zeros((M + 255) // 256 * 256 * Nn, dtype=torch.uint8, device=rem.device)      # whole 256 x 256 tiles
    blob[lo8_index(M, Nn, rem.device)] = (rem.float().cpu() * 1024.0).to(torch.float8_e5m2).view(torch.uint8).to(rem.device)
    return blob


def drop_mask(seed, p, M, Nn, rows=None):
    """(keep [M, N], keep_scale): the hash port at token * N + n, token = rows[m] or m"""
    tok = torch.arange(M, dtype=torch.int64) if rows is None else rows.cpu().to(torch.int64)
    keys = tok[:, None] * Nn + torch.arange(Nn, dtype=torch.int64)[None, :]
    keep, scale = keep_of(seed, keys, p)
    return keep, float(scale)


def train_reference(A, B, bias, act, resid, mul, out_dt, K, p=0.0, seed=0, rows=None, pre_grad=False, k_used=None):
    """The training epilogue: v = acc + bias; tape = v | gelu'(v); y = dropout(act(v)); out = y (+|x) resid.
    Returns (out, bound, tape, tape_bound, keep)."""
    a, w = A.double(), B.double()
    if k_used:
        a, w = a[:, :k_used], w[:, :k_used]
    acc, mag = a @ w.t(), a.abs() @ w.abs().t()
    bb = _vec(bias, w.shape[0], a)
    v = acc + bb
    e_v = (K + 2) * u * (mag + bb.abs())
    keep, scale = None, 1.0
    if p > 0:
        keep, scale = drop_mask(seed, p, a.shape[0], w.shape[0], rows)
        keep = keep.to(a.device)
    fast = out_dt != F32
    out, bound = tail(v, e_v, act, resid, mul, out_dt, fast=fast, scale=scale, keep=keep)
    U = U_OUT[out_dt]
    if pre_grad:
        tape = gelu_grad64(v)
        e_t = GRAD_LIP * e_v + (grad_fast_err(v) if fast else 16 * u)
    else:
        tape, e_t = v, e_v
    return out, bound, tape, U * tape.abs() + e_t * (1 + U) + FLOOR[out_dt], keep


def grad_reference(A, B, bias, resid, out_dt, K, ctl=None):
    """OM_ACT_GELU_ERF_GRAD: out = (acc + bias) gelu'(resid); ctl 'tape': gelu' taken from the tape element one column on"""
    a, w = A.double(), B.double()
    acc, mag = a @ w.t(), a.abs() @ w.abs().t()
    bb = _vec(bias, w.shape[0], a)
    v = acc + bb
    r = resid.double()
    if ctl == "tape":
        r = torch.roll(r, 1, 1)
    gp = gelu_grad64(r)
    fast = out_dt != F32
    U = U_OUT[out_dt]
    out = v * gp
    e = (K + 2) * u * (mag + bb.abs()) * gp.abs() + v.abs() * (grad_fast_err(r) if fast else 16 * u) + 2 * u * out.abs()
    return out, U * out.abs() + e * (1 + U) + FLOOR[out_dt]


def ln64(x, g, b, eps):
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd * g.double() + b.double(), mean[:, 0], rstd[:, 0]


def splitk_slices(M, Nn, K, es):
    """omk_gemm_splitk's slice count (csrc/gemm.hip): (slices, K steps per slice, K steps)"""
    tiles = ((M + 127) // 128) * ((Nn + 127) // 128)
    nk = K * es // 128
    slices = (1024 + tiles - 1) // tiles
    if slices > nk // 4:
        slices = max(nk // 4, 1)
    per = (nk + slices - 1) // slices
    return (nk + per - 1) // per, per, nk


FEW_ACC = 10      # few rows: K products (K), up to eight partial sums added in wave order (7), the bias (1), the residual (1), the sum (1)


def few_f32_reference(A, B, bias, r32, K, ctl=None):
    """resid32 / out32: y = A B^T + bias + resid32 in f32 and the bound of the f32 sum; ctl 'resid': the residual one column off"""
    a, w = A.double(), B.double()
    r = torch.roll(r32.double(), 1, 1) if ctl == "resid" else r32.double()
    y = a @ w.t() + bias.double() + r
    return y, (K + FEW_ACC) * u * (a.abs() @ w.abs().t() + bias.double().abs()) + 2 * u * y.abs() + 2.0 ** -126


def a_ln_reference(x32, ag, ab, B, bias, K, dt, ctl=None):
    """a_ln32: y = LN(x32) W^T + bias with the operand rounded to 16 bits, and what a_ln_stats_out holds.  Returns (y, bound of the f32
    sum, mean, mean's bound, rstd, rstd's relative bound); ctl 'shift': the normalised row one column off"""
    lnx, mean, rstd = ln64(x32, ag, ab, EPS)
    if ctl == "shift":
        lnx = torch.roll(lnx, 1, 1)
    w, xd = B.double(), x32.double()
    rel = RSQRT_REL + (K + 8) * u                                                  # the f32 sum of K squares, the division, rsqrtf
    dmean = (K + 4) * u * xd.abs().mean(1)
    dev = (xd - mean[:, None]).abs() * rstd[:, None]
    e_ln = (dev * rel + dmean[:, None] * rstd[:, None] + 3 * u * (xd.abs() + mean.abs()[:, None]) * rstd[:, None]) * ag.double().abs() + 2 * u * lnx.abs()
    y = lnx @ w.t() + bias.double()
    e = (U_OUT[dt] * lnx.abs() + e_ln) @ w.abs().t() + (K + FEW_ACC) * u * (lnx.abs() @ w.abs().t() + bias.double().abs()) + 2 * u * y.abs()
    var = 1.0 / (rstd * rstd)
    rel_r = rel + 0.5 * (2 * dmean * (xd - mean[:, None]).abs().mean(1) + dmean * dmean) / var
    return y, e, mean, dmean + u * mean.abs() + 2.0 ** -126, rstd, rel_r


def rln_reference(A, B, bias, r32, g, b, K, ctl=None):
    """rln32: y = A B^T + bias + LN(r32) re-derived from the f32 (mean, rstd); returns (y, bound, the statistics as the kernel reads them);
    ctl 'shift': the normalised residual one column off"""
    lnr, rmean, rrstd = ln64(r32, g, b, EPS)
    a, w, rd = A.double(), B.double(), r32.double()
    y = a @ w.t() + bias.double() + (torch.roll(lnr, 1, 1) if ctl == "shift" else lnr)
    e_r = ((rd - rmean[:, None]).abs() * rrstd[:, None] * 4 * u + u * (rd.abs() + rmean.abs()[:, None]) * rrstd[:, None]) * g.double().abs() + 2 * u * lnr.abs()
    e = (K + FEW_ACC) * u * (a.abs() @ w.abs().t() + bias.double().abs()) + e_r + 2 * u * y.abs() + 2.0 ** -126
    return y, e, torch.stack([rmean, rrstd], 1).float()


def splitk_reference(A, B, C0, K, slices, ctl=None):
    """C0 + A B^T and the issue's bound (K + slices + 2) u sum|a||b| + u |C0|; ctl 'k_step': the last 128 bytes of K dropped, 'store': C
    overwritten instead of added to"""
    a, w = A.double(), B.double()
    if ctl == "k_step":
        kk = K - 128 // A.element_size()
        a, w = a[:, :kk], w[:, :kk]
    ref = a @ w.t() + (0 if ctl == "store" else C0.double())
    return ref, (K + slices + 2) * u * (A.double().abs() @ B.double().abs().t()) + u * C0.double().abs()


def few_inputs(dt, M, Nn, K, seed, device=DEV):
    gen = torch.Generator(device=device).manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, device=device, dtype=torch.float32)
    rows = torch.arange(M, device=device)
    x32 = rnd(M, K) * (2.0 ** ((rows % 4).float() - 2.0))[:, None] + (1.0 + (rows % 3).float())[:, None]
    r32 = rnd(M, Nn) * (2.0 ** (((rows + 1) % 4).float() - 2.0))[:, None] + (1.0 + ((rows + 2) % 3).float())[:, None]
    return dict(A=rnd(M, K).to(TORCH_DT[dt]), B=(rnd(Nn, K) / math.sqrt(K)).to(TORCH_DT[dt]), bias=rnd(Nn), x32=x32, r32=r32,
                ag=1.0 + 0.5 * rnd(K), ab=0.3 * rnd(K), g=1.0 + 0.5 * rnd(Nn), b=0.3 * rnd(Nn))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def ln_inputs(dt, M, Nn, K, seed, device):
    """A and the residual with row means of 1 to 3 and row scales 1/4 .. 2 (8 x between rows); B; independent random column vectors"""
    gen = torch.Generator(device=device).manual_seed(seed)
    td = TORCH_DT[dt]

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, device=device, dtype=torch.float32)
    rows = torch.arange(M, device=device)
    sc_a, mean_a = 2.0 ** ((rows % 4).float() - 2.0), 1.0 + (rows % 3).float()
    sc_r, mean_r = 2.0 ** (((rows + 1) % 4).float() - 2.0), 1.0 + ((rows + 2) % 3).float()
    d = dict(A=(rnd(M, K) * sc_a[:, None] + mean_a[:, None]).to(td), B=(rnd(Nn, K) / math.sqrt(K)).to(td),
             R=(rnd(M, Nn) * sc_r[:, None] + mean_r[:, None]).to(td), gate=rnd(M, Nn).to(td),
             colsum=rnd(Nn), bias=rnd(Nn), g=1.0 + 0.5 * rnd(Nn), b=0.3 * rnd(Nn))
    d["R_lo"] = (rnd(M, Nn) * d["R"].float().abs() * U_OUT[dt] * 0.9).to(td)       # a remainder plane: below half an ulp of R
    d["a_stats"], d["r_stats"] = row_stats(d["A"]), row_stats(d["R"].double() + d["R_lo"].double())
    d["r1_stats"] = row_stats(d["R"])
    return d


# ---------------------------------------------------------------------------------------------------------------
# CPU: the references against plain torch, an emulated kernel inside every bound, every control rejected
# ---------------------------------------------------------------------------------------------------------------
def _split(x, dt):
    hi = x.to(TORCH_DT[dt]).float()
    return hi, (x - hi).to(TORCH_DT[dt]).float()


def _rank2(uv, bv, dt):
    uh, ul = _split(uv, dt)
    bh, bl = _split(bv, dt)
    return uh[:, None] * bh[None, :] + ul[:, None] * bh[None, :] + uh[:, None] * bl[None, :]


def _emulate_lnf1(d, dt, act, gate, colsum, bias, rms, inv_h):
    A, B = d["A"].float(), d["B"].float()
    st = d["a_stats"]
    mu = torch.zeros_like(st[:, 0]) if rms else st[:, 0] * np.float32(inv_h)
    var = (st[:, 1] * np.float32(inv_h) - mu * mu).clamp_min(0.0) + np.float32(EPS)
    rs = var.rsqrt()
    Nn = B.shape[0]
    init = _rank2(var.sqrt(), bias if bias is not None else torch.zeros(Nn), dt)
    init = init + _rank2(-mu, colsum if colsum is not None else torch.zeros(Nn), dt)
    v = rs[:, None] * (A @ B.t() + init)
    y = act64(act, v.double()).float()
    if gate is not None:
        y = y * gate.float()
    return y.to(TORCH_DT[dt])


def _emulate_lnf2(d, dt, two, res_ln, inv_h):
    A, B = d["A"].float(), d["B"].float()
    v = A @ B.t() + _rank2(torch.ones(A.shape[0]), d["bias"], dt)
    r = d["R"].float()
    if two:
        r = r + d["R_lo"].float()
    if res_ln:
        st = d["r_stats"] if two else d["r1_stats"]
        mu = st[:, 0] * np.float32(inv_h)
        rstd = ((st[:, 1] * np.float32(inv_h) - mu * mu).clamp_min(0.0) + np.float32(EPS)).rsqrt()
        r = (r * rstd[:, None] + (-mu * rstd)[:, None]) * d["g"] + d["b"]
    v = v + r
    M, Nn = v.shape
    vv = v.view(M, Nn // 128, 128)
    slots = torch.stack([vv.sum(2), (vv * vv).sum(2)], 2).permute(1, 0, 2).contiguous()
    C = v.to(TORCH_DT[dt])
    return v, C, (v - C.float()).to(TORCH_DT[dt]), slots


CPU_M, CPU_N, CPU_K = 12, 256, 128


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("act,gated", [(NONE, False), (ERF, False), (RELU, False), (TANH, False), (TANH, True)],
                         ids=["none", "erf", "relu", "tanh", "tanh-x-resid"])
def test_cpu_lnf1_bound_holds_an_emulated_kernel_and_rejects_the_controls(dt, act, gated):
    d = ln_inputs(dt, CPU_M, CPU_N, CPU_K, 5, "cpu")
    inv_h = 1.0 / CPU_K
    gate = d["gate"] if gated else None
    for rms, colsum, bias in ((0, d["colsum"], d["bias"]), (1, d["colsum"], d["bias"]), (1, None, d["bias"]), (0, d["colsum"], None)):
        got = _emulate_lnf1(d, dt, act, gate, colsum, bias, rms, inv_h)
        ref, bound = lnf1_reference(d["A"], d["B"], d["a_stats"], colsum, bias, act, gate, inv_h, EPS, rms, dt)
        assert not violations(got, ref, bound, dt).any(), (rms, colsum is None, bias is None)
        ctls = ["row"] + (["colsum"] if colsum is not None and not rms else []) + (["bias"] if bias is not None else [])
        for c in ctls:
            ctl = lnf1_reference(d["A"], d["B"], d["a_stats"], colsum, bias, act, gate, inv_h, EPS, rms, dt, ctl=c)[0]
            assert rejected(ref, ctl, bound), (c, rms)
    # the reference is LayerNorm then Linear: W' = W gamma, s = colsum W', b' = b + W beta
    gen = torch.Generator().manual_seed(1)
    gamma, beta = 1 + 0.5 * torch.randn(CPU_K, generator=gen).double(), 0.3 * torch.randn(CPU_K, generator=gen).double()
    W, b0 = d["B"].double(), d["bias"].double()
    Wf = W * gamma
    st = torch.stack([d["A"].double().sum(1), (d["A"].double() ** 2).sum(1)], 1)
    ref = lnf1_reference(d["A"], Wf, st, Wf.sum(1), b0 + W @ beta, NONE, None, inv_h, EPS, 0, dt)[0]
    want = torch.nn.functional.linear(torch.nn.functional.layer_norm(d["A"].double(), (CPU_K,), gamma, beta, EPS), W, b0)
    assert (ref - want).abs().max() < 1e-9 * want.abs().max()


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_cpu_output_side_bounds_hold_an_emulated_kernel_and_reject_the_controls(dt):
    d = ln_inputs(dt, CPU_M, CPU_N, CPU_K, 6, "cpu")
    inv_h = 1.0 / CPU_N
    for two in (False, True):
        for res_ln in (True, False):
            v, C, lo, slots = _emulate_lnf2(d, dt, two, res_ln, inv_h)
            st = (d["r_stats"] if two else d["r1_stats"]) if res_ln else None
            args = (d["A"], d["B"], d["bias"], d["R"], d["R_lo"] if two else None, st, d["g"], d["b"], inv_h, EPS, dt)
            y, e_y = lnf2_reference(*args)
            assert not violations(v, y, e_y).any()
            assert not violations(C, y, stored_bound(y, e_y, dt), dt).any()
            sref, sb = slot_stats(y, e_y)
            assert not violations(slots, sref, sb).any()
            assert rejected(sref, torch.roll(sref, 1, 0), sb)                       # a slot one wave column off
            for c in (["row", "rln_b"] if res_ln else []) + (["lo"] if two and not res_ln else []):
                ctl = lnf2_reference(*args, ctl=c)[0]
                assert rejected(y, ctl, e_y if c == "lo" else stored_bound(y, e_y, dt)), (c, two)
            # two planes: C + lo carries y through a second rounding; the remainder is below half an ulp of C
            two_b = e_y + U_OUT[dt] ** 2 * y.abs() * 1.01 + SPLIT_FLOOR[dt]
            assert not violations(C.double() + lo.double(), y, two_b).any()
            assert (lo.double().abs() <= half_ulp(C, dt)).all()
            assert rejected(y, C.double(), two_b)                                   # the second plane dropped
            if dt == F16:
                blob = lo8_encode(v - C.float(), CPU_M, CPU_N)
                dec = lo8_decode(blob, CPU_M, CPU_N)
                b8 = e_y + 2.0 ** -3 * (U_OUT[dt] * y.abs() * 1.01 + e_y) + 2.0 ** -27
                assert not violations(C.double() + dec, y, b8).any()
                assert rejected(y, C.double(), b8)
    # the reference is the plain composition: x + LayerNorm(r)
    y = lnf2_reference(d["A"], d["B"], d["bias"], d["R"], None, torch.stack([d["R"].double().sum(1), (d["R"].double() ** 2).sum(1)], 1),
                       d["g"], d["b"], inv_h, EPS, dt)[0]
    want = (torch.nn.functional.linear(d["A"].double(), d["B"].double(), d["bias"].double()) +
            torch.nn.functional.layer_norm(d["R"].double(), (CPU_N,), d["g"].double(), d["b"].double(), EPS))
    assert (y - want).abs().max() < 1e-9 * want.abs().max()


def test_cpu_e5m2_plane_round_trip():
    """encode and decode through the index port: every (m, n) has a byte of its own, and e5m2 keeps a remainder to 2^-3 of itself"""
    M, Nn = 256, 512
    idx = lo8_index(M, Nn, "cpu")
    assert idx.unique().numel() == M * Nn and int(idx.max()) == M * Nn - 1
    rem = torch.randn(M, Nn, generator=torch.Generator().manual_seed(2)) * 2.0 ** -12
    dec = lo8_decode(lo8_encode(rem, M, Nn), M, Nn)
    assert ((dec - rem.double()).abs() <= 2.0 ** -3 * rem.double().abs() + 2.0 ** -27).all()


@pytest.mark.parametrize("out_dt", [BF16, F16, F32], ids=lambda d: NAME[d])
def test_cpu_training_references_are_torch_compositions(out_dt):
    gen = torch.Generator().manual_seed(4)
    M, Nn, K = 9, 24, 64
    in_dt = out_dt
    A = torch.randn(M, K, generator=gen).to(TORCH_DT[in_dt])
    B = (torch.randn(Nn, K, generator=gen) / 8).to(TORCH_DT[in_dt])
    bias = torch.randn(Nn, generator=gen)
    R = torch.randn(M, Nn, generator=gen).to(TORCH_DT[out_dt])
    lin = torch.nn.functional.linear(A.double(), B.double(), bias.double())
    # gelu' is autograd's
    x = lin.clone().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    assert (gelu_grad64(lin) - x.grad).abs().max() < 1e-12
    # dropout + residual: F.dropout's arithmetic with the port's mask
    rows = torch.randperm(M, generator=gen).to(torch.int32)
    for r in (None, rows):
        out, bound, tape, tb, keep = train_reference(A, B, bias, NONE, R, False, out_dt, K, p=0.5, seed=77, rows=r)
        assert torch.equal(out, torch.where(keep, lin * 2.0, torch.zeros_like(lin)) + R.double())
        assert 0.3 < keep.float().mean() < 0.7 and torch.equal(tape, lin)
        # an emulated kernel: f32 accumulation, one rounding
        v = (A.float() @ B.float().t() + bias)
        emu = (torch.where(keep, v * np.float32(2.0), torch.zeros(())) + R.float()).to(TORCH_DT[out_dt])
        assert not violations(emu, out, bound, out_dt).any()
        dropped = ~keep
        assert torch.equal(emu[dropped], R[dropped])
    keep_m = train_reference(A, B, bias, NONE, R, False, out_dt, K, p=0.5, seed=77, rows=None)[4]
    keep_r = train_reference(A, B, bias, NONE, R, False, out_dt, K, p=0.5, seed=77, rows=rows)[4]
    assert not torch.equal(keep_m, keep_r)                                          # the control: the mask taken at m, not at drop_rows[m]
    ref_r, bound_r = train_reference(A, B, bias, NONE, R, False, out_dt, K, p=0.5, seed=77, rows=rows)[:2]
    assert rejected(ref_r, train_reference(A, B, bias, NONE, R, False, out_dt, K, p=0.5, seed=77)[0], bound_r)
    # the gated T5 site: tape, dropout and a multiplied residual in one call
    gref, gbound, gtape, gtb, gkeep = train_reference(A, B, bias, TANH, R, True, out_dt, K, p=0.5, seed=77, rows=rows)
    v32f = A.float() @ B.float().t() + bias
    emu = (torch.where(gkeep, act64(TANH, v32f.double()).float() * np.float32(2.0), torch.zeros(())) * R.float()).to(TORCH_DT[out_dt])
    assert not violations(emu, gref, gbound, out_dt).any() and not violations(v32f.to(TORCH_DT[out_dt]), gtape, gtb, out_dt).any()
    assert rejected(gref, train_reference(A, B, bias, TANH, R, True, out_dt, K, p=0.5, seed=77)[0], gbound)
    assert torch.equal(keep_r, drop_mask(77, 0.5, int(rows.max()) + 1, Nn)[0][rows.long()])
    # tape and gelu' x tape
    out, bound, tape, tb, _ = train_reference(A, B, bias, ERF, None, False, out_dt, K, pre_grad=True)
    assert torch.equal(tape, gelu_grad64(lin)) and torch.allclose(out, torch.nn.functional.gelu(lin), atol=1e-12)
    v32 = (A.float() @ B.float().t() + bias).double()
    assert not violations(gelu_grad64(v32).to(TORCH_DT[out_dt]), tape, tb, out_dt).any()
    pre_tape, ptb = train_reference(A, B, bias, ERF, None, False, out_dt, K)[2:4]
    assert not violations(v32.to(TORCH_DT[out_dt]), pre_tape, ptb, out_dt).any()
    assert rejected(tape, pre_tape, tb) and rejected(pre_tape, tape, ptb)            # the other tape
    assert rejected(tape, torch.roll(tape, 1, 1), tb) and rejected(pre_tape, torch.roll(pre_tape, 1, 1), ptb)      # one column off
    gout, gb = grad_reference(A, B, bias, R, out_dt, K)
    assert torch.equal(gout, lin * gelu_grad64(R.double()))
    assert not violations((v32 * gelu_grad64(R.double())).to(TORCH_DT[out_dt]), gout, gb, out_dt).any()
    assert rejected(gout, grad_reference(A, B, bias, R, out_dt, K, ctl="tape")[0], gb)


def test_cpu_gelu_grad_fit_error():
    """GRAD_FIT is the error of the fast form's own coefficients, evaluated in float64 over +-12 -- not a figure taken from the kernel's output"""
    x = torch.linspace(-12.0, 12.0, 2400001, dtype=torch.float64)
    err = (grad_fast_port(x) - gelu_grad64(x)).abs()
    assert 1.32e-5 < float(err.max()) <= GRAD_FIT - 5e-8
    assert float(err[(x + 0.75).abs() < 0.1].max()) > 9e-6          # already at the zero of gelu', where the product is most exposed


def test_cpu_splitk_slice_port_and_bound():
    assert splitk_slices(130, 200, 64 * 4, 2)[0] == 1 and splitk_slices(130, 200, 64 * 8, 2)[0] == 2
    s, per, nk = splitk_slices(130, 200, 64 * 22, 2)
    assert (s, per, nk) == (5, 5, 22) and nk - (s - 1) * per == 2                    # a last slice shorter than the others
    assert splitk_slices(130, 200, 32 * 22, 4) == (5, 5, 22)
    # an emulated kernel: every slice summed in f32, the slices added to C one after the other in f32
    gen = torch.Generator().manual_seed(8)
    for dt, es in ((BF16, 2), (F32, 4)):
        K = 22 * 128 // es
        A, B = torch.randn(9, K, generator=gen).to(TORCH_DT[dt]), torch.randn(24, K, generator=gen).to(TORCH_DT[dt])
        C0 = torch.randn(9, 24, generator=gen) * 3
        got, step = C0.clone(), per * 128 // es
        for k0 in range(0, K, step):
            got = got + A[:, k0:k0 + step].float() @ B[:, k0:k0 + step].float().t()
        ref, bound = splitk_reference(A, B, C0, K, s)
        assert not violations(got, ref, bound).any()
        assert rejected(ref, splitk_reference(A, B, C0, K, s, ctl="k_step")[0], bound)
        assert rejected(ref, splitk_reference(A, B, C0, K, s, ctl="store")[0], bound)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_cpu_few_rows_bounds_hold_an_emulated_kernel_and_reject_the_controls(dt):
    M, Nn, K = 17, 48, 128
    d = few_inputs(dt, M, Nn, K, 9, "cpu")
    acc = d["A"].float() @ d["B"].float().t() + d["bias"]
    y, e = few_f32_reference(d["A"], d["B"], d["bias"], d["r32"], K)
    assert not violations(acc + d["r32"], y, e).any()
    assert not violations((acc + d["r32"]).to(TORCH_DT[dt]), y, stored_bound(y, e, dt), dt).any()
    assert rejected(y, few_f32_reference(d["A"], d["B"], d["bias"], d["r32"], K, ctl="resid")[0], e)
    # a_ln32: the row normalised in f32 (two passes, as ln_row.h), rounded to 16 bits, contracted in f32
    x = d["x32"]
    mean = x.sum(1) / np.float32(K)
    rstd = (((x - mean[:, None]) ** 2).sum(1) / np.float32(K) + np.float32(EPS)).rsqrt()
    xn = ((x - mean[:, None]) * rstd[:, None] * d["ag"] + d["ab"]).to(TORCH_DT[dt])
    y, e, m64, mb, r64, rrel = a_ln_reference(x, d["ag"], d["ab"], d["B"], d["bias"], K, dt)
    assert not violations((xn.float() @ d["B"].float().t() + d["bias"]).to(TORCH_DT[dt]), y, stored_bound(y, e, dt), dt).any()
    assert not violations(mean, m64, mb).any() and not violations(rstd, r64, r64 * rrel).any()
    assert rejected(y, a_ln_reference(x, d["ag"], d["ab"], d["B"], d["bias"], K, dt, ctl="shift")[0], stored_bound(y, e, dt))
    assert rejected(r64, torch.roll(r64, 1), r64 * rrel)
    # rln32: the residual re-derived from the f32 statistics
    y, e, st = rln_reference(d["A"], d["B"], d["bias"], d["r32"], d["g"], d["b"], K)
    lnr = ((d["r32"] - st[:, :1]) * st[:, 1:]) * d["g"] + d["b"]
    assert not violations(acc + lnr, y, e).any()
    assert rejected(y, rln_reference(d["A"], d["B"], d["bias"], d["r32"], d["g"], d["b"], K, ctl="shift")[0], e)
    # the reference is the plain composition
    want = torch.nn.functional.linear(torch.nn.functional.layer_norm(x.double(), (K,), d["ag"].double(), d["ab"].double(), EPS), d["B"].double(), d["bias"].double())
    assert (a_ln_reference(x, d["ag"], d["ab"], d["B"], d["bias"], K, dt)[0] - want).abs().max() < 1e-9 * want.abs().max()


# ---------------------------------------------------------------------------------------------------------------
# the call: one description of an epilogue serves the GPU launch (real addresses) and the planner walk (made-up ones)
# ---------------------------------------------------------------------------------------------------------------
POINTER_FIELDS = ("bias", "resid", "pre_act", "drop_rows", "ln_stats", "ln_colsum", "rln_stats", "rln_g", "rln_b", "stats_out", "resid_lo",
                  "out_lo", "resid32", "out32", "a_ln32", "a_ln_g", "a_ln_b", "a_ln_stats_out", "rln32", "rln32_stats")


def _addr(v):
    if v is None:
        return None
    if isinstance(v, Buf):
        return v.ptr()
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return int(v)


def make_ep(**kw):
    ep = N.OmDebugGemmEpilogue()
    for k, v in kw.items():
        assert k in dict(N.OmDebugGemmEpilogue._fields_), k
        setattr(ep, k, _addr(v) if k in POINTER_FIELDS else v)
    return ep


def fake_ep(spec, misalign=()):
    """the epilogue of a case with a made-up 512-byte aligned address for every pointer the case sets"""
    kw = dict(spec)
    for i, k in enumerate(POINTER_FIELDS):
        if kw.get(k):
            kw[k] = (16 + i) << 32 | (4 if k in misalign else 0)
    return make_ep(**kw)


def plan(in_dt, out_dt, M, Nn, K, ep, lda=None, ldb=None, ldc=None):
    return N.lib().om_debug_gemm_plan_ex(in_dt, 1 << 32, lda or K, 2 << 32, ldb or K, out_dt, 3 << 32, ldc or Nn, M, Nn, K, ctypes.byref(ep))


def gemm_ex(in_dt, out_dt, A, B, C, M, Nn, K, ep, lda=None, ldb=None, ldc=None):
    """om_debug_gemm_ex on device tensors / Bufs; returns (rc, family reached)"""
    lib = N.lib()
    with torch.cuda.device(DEV):
        rc = lib.om_debug_gemm_ex(in_dt, _addr(A), lda or K, _addr(B), ldb or K, out_dt, _addr(C), ldc or (C.ld if isinstance(C, Buf) else Nn),
                                  M, Nn, K, ctypes.byref(ep), N.stream_ptr(torch.device(DEV)))
    sync()
    return rc, lib.om_debug_gemm_last()


def sync():
    """wait for the device; a device error ends the session -- nothing more is launched on a GPU that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


class Frozen:
    """inputs that must come back bit-unchanged"""

    def __init__(self, **tensors):
        self.items = {k: (t, t.clone()) for k, t in tensors.items() if t is not None}

    def check(self, label):
        for k, (t, snap) in self.items.items():
            assert torch.equal(t.view(torch.uint8), snap.view(torch.uint8)), f"{label}: input {k} modified"


def out_buf(dt, rows, cols, ld=None):
    return Buf(dt, rows, cols, ld or cols)


def guards_ok(label, *bufs_and_snaps):
    for b, s in bufs_and_snaps:
        assert b.outside_changed(s) == 0, f"{label}: written outside the window"


# ---------------------------------------------------------------------------------------------------------------
# A. fused LayerNorm on generation 7
# ---------------------------------------------------------------------------------------------------------------
LM, LN_, LK = 512, 768, 256
WALKS = [(None, 0), (None, 1), (1, 0), (1, 1), (4, 0), (4, 1)]              # (OM_OPT_GEMM_MAX_GRID, reverse); the first is the default


def walk(label, family, launch_once):
    """launch_once(reverse) -> (rc, family, {name: tensor}); all six walks give the same bits; returns the default walk's outputs"""
    first = None
    for cap, rev in WALKS:
        with gemm_options(**({} if cap is None else dict(max_grid=cap))):
            rc, fam, outs = launch_once(rev)
        assert rc == 0, (label, cap, rev, N.lib().om_last_error())
        assert fam == FAM[family], f"{label}: ran family {fam}, expected {family}"
        if first is None:
            first = outs
        else:
            for k, t in outs.items():
                diff = int((t.view(torch.uint8) != first[k].view(torch.uint8)).sum())
                assert diff == 0, f"{label}: max_grid={cap} reverse={rev} changes {diff} bytes of {k}"
    return first


LNF1_ACTS = {BF16: ["none", "erf", "relu", "tanh", "tanh-x-resid"], F16: ["none", "erf", "relu"]}
ACT_CODE = {"none": NONE, "erf": ERF, "relu": RELU, "tanh": TANH, "tanh-x-resid": TANH | N.ACT_MUL_RESID}
# variant -> (ln_rms, colsum?, bias?)
LNF1_VARIANTS = {"ln": (0, True, True), "rms": (1, True, True), "rms-nocolsum": (1, False, True), "nobias": (0, True, False)}


def lnf1_kernels(act):
    return [("restart", RESTART, "g7")] + ([] if act == "tanh-x-resid" else [("ring", CONT, "7c16")])


def lnf1_spec(act, variant, K=LK):
    rms, cs, bias = LNF1_VARIANTS[variant]
    spec = dict(act=ACT_CODE[act], ln_stats=1, ln_inv_h=1.0 / K, ln_eps=EPS, ln_rms=rms)
    if cs:
        spec["ln_colsum"] = 1
    if bias:
        spec["bias"] = 1
    if act == "tanh-x-resid":
        spec.update(resid=1, ldr=LN_)
    return spec


LNF1_CASES = [pytest.param(dt, act, kern, cont, fam, id=f"{NAME[dt]}-{act}-{kern}")
              for dt in (BF16, F16) for act in LNF1_ACTS[dt] for kern, cont, fam in lnf1_kernels(act)]


def run_lnf1(dt, act, variant, d, family, K=LK, walks=True):
    rms, cs, has_bias = LNF1_VARIANTS[variant]
    A = d["A"][:, :K].contiguous()
    B = d["B"][:, :K].contiguous()
    stats = row_stats(A).to(DEV)
    colsum, bias = (d["colsum"] if cs else None), (d["bias"] if has_bias else None)
    gate = d["gate"] if act == "tanh-x-resid" else None
    frozen = Frozen(A=A, B=B, stats=stats, colsum=colsum, bias=bias, gate=gate)
    label = f"LNF1 {NAME[dt]} {act} {variant} {family} K={K}"

    def once(rev):
        C = out_buf(dt, LM, LN_, LN_ + 64)
        snap = C.snapshot()
        ep = make_ep(act=ACT_CODE[act], ln_stats=stats, ln_colsum=colsum, bias=bias, resid=gate, ldr=LN_ if gate is not None else 0,
                     ln_inv_h=1.0 / K, ln_eps=EPS, ln_rms=rms, reverse=rev)
        rc, fam = gemm_ex(dt, dt, A, B, C, LM, LN_, K, ep)
        guards_ok(label, (C, snap))
        return rc, fam, {"C": C.window.clone()}
    if walks:
        C = walk(label, family, once)["C"]
    else:
        rc, fam, outs = once(0)
        assert rc == 0 and fam == FAM[family], (label, rc, fam, N.lib().om_last_error())
        C = outs["C"]
    frozen.check(label)
    base = ACT_CODE[act] & 0xff
    ref, bound = lnf1_reference(A, B, stats, colsum, bias, base, gate, 1.0 / K, EPS, rms, dt)
    assert_within(f"lnf1/{family}/{NAME[dt]}", C, ref, bound, dt)
    for c in ["row"] + (["colsum"] if cs and not rms else []) + (["bias"] if has_bias else []):
        ctl = lnf1_reference(A, B, stats, colsum, bias, base, gate, 1.0 / K, EPS, rms, dt, ctl=c)[0]
        assert rejected(ref, ctl, bound), f"{label}: the bound accepts the control '{c}'"
    return C


@pytest.mark.gpu
@pytest.mark.parametrize("dt,act,kern,cont,family", LNF1_CASES)
def test_lnf1(dt, act, kern, cont, family):
    """C = act(rstd_m (A B^T - mu_m s_n) + bias_n) [x resid]: LayerNorm, RMSNorm, RMSNorm without a column sum, no bias -- six walks each"""
    d = ln_inputs(dt, LM, LN_, LK, 11, DEV)
    with gemm_options(cont=cont, skinny_m=0):
        for variant in LNF1_VARIANTS:
            run_lnf1(dt, act, variant, d, family)


def run_output_side(dt, lnf, family, d, res_ln=True, lo_in=True, K=LK, walks=True, blob_in=None):
    """LNF 2 (one plane), 3 (two 16-bit planes), 4 (an eight-bit second plane); returns the default walk's outputs and (y, e_y)"""
    two = lnf >= 3
    A, B = d["A"][:, :K].contiguous(), d["B"][:, :K].contiguous()
    R = d["R"]
    R_lo = d["R_lo"] if two and lo_in and lnf == 3 else None
    lo_val = R_lo
    if lnf == 4 and blob_in is not None:
        lo_val = lo8_decode(blob_in, LM, LN_)
    if not res_ln:
        stats = None
    else:
        stats = row_stats(R.double() + (lo_val.double() if lo_val is not None else 0)).to(DEV)
    nslots = LN_ // 128
    frozen = Frozen(A=A, B=B, R=R, R_lo=R_lo, blob=blob_in, stats=stats, g=d["g"], b=d["b"], bias=d["bias"])
    label = f"LNF{lnf} {NAME[dt]} {family} res_ln={res_ln} lo_in={lo_val is not None} K={K}"

    def once(rev):
        C = out_buf(dt, LM, LN_, LN_ + 64)
        S = out_buf(F32, nslots * LM, 2)
        bufs = [(C, C.snapshot()), (S, S.snapshot())]
        outs = {}
        kw = dict(act=NONE, bias=d["bias"], resid=R, ldr=LN_, rln_stats=stats, rln_g=d["g"] if res_ln else None,
                  rln_b=d["b"] if res_ln else None, stats_out=S, ln_inv_h=1.0 / LN_, ln_eps=EPS, reverse=rev)
        if lnf == 3:
            LO = out_buf(dt, LM, LN_, LN_ + 64)                     # the second plane shares C's pitch
            bufs.append((LO, LO.snapshot()))
            kw.update(out_lo=LO, resid_lo=R_lo)
        if lnf == 4:
            LO = out_buf(F16, 1, LM * LN_ // 2)                     # M N bytes
            bufs.append((LO, LO.snapshot()))
            kw.update(out_lo=LO, resid_lo=blob_in, lo8=1)
        rc, fam = gemm_ex(dt, dt, A, B, C, LM, LN_, K, make_ep(**kw))
        guards_ok(label, *bufs)
        outs["C"], outs["S"] = C.window.clone(), S.window.clone().view(nslots, LM, 2)
        if lnf >= 3:
            outs["LO"] = LO.window.clone()
        return rc, fam, outs
    if walks:
        outs = walk(label, family, once)
        again = once(0)[2]
        assert all(torch.equal(again[k].view(torch.uint8), outs[k].view(torch.uint8)) for k in outs), f"{label}: two runs differ"
    else:
        rc, fam, outs = once(0)
        assert rc == 0 and fam == FAM[family], (label, rc, fam, N.lib().om_last_error())
    frozen.check(label)
    args = (A, B, d["bias"], R, lo_val, stats, d["g"], d["b"], 1.0 / LN_, EPS, dt)
    y, e_y = lnf2_reference(*args)
    tag = f"lnf{lnf}/{family}/{NAME[dt]}"
    assert_within(tag + "/C", outs["C"], y, stored_bound(y, e_y, dt), dt)
    sref, sb = slot_stats(y, e_y)
    assert_within(tag + "/stats", outs["S"], sref, sb)
    assert rejected(sref, torch.roll(sref, 1, 0), sb), f"{label}: the bound accepts statistics one slot off"
    # the slots reduce to the row totals through the reduction the encoder uses
    tot = torch.full((LM + 2, 2), 7.5, device=DEV)
    assert N.lib().om_debug_ln_stats_reduce(N.ptr(outs["S"].contiguous()), nslots, LM, N.ptr(tot), N.stream_ptr(torch.device(DEV))) == 0
    torch.cuda.synchronize()
    assert_within(tag + "/row stats", tot[:LM], sref.sum(0), sb.sum(0) + (nslots + 1) * u * sref.abs().sum(0))
    assert bool((tot[LM:] == 7.5).all())
    for c in (["row", "rln_b"] if res_ln else []):
        ctl = lnf2_reference(*args, ctl=c)[0]
        assert rejected(y, ctl, stored_bound(y, e_y, dt)), f"{label}: the bound accepts the control '{c}'"
    if lnf == 3:
        two_b = e_y + U_OUT[dt] ** 2 * y.abs() * 1.01 + SPLIT_FLOOR[dt]
        assert_within(tag + "/C+lo", outs["C"].double() + outs["LO"].double(), y, two_b)
        lo_ratio = float((outs["LO"].double().abs() / half_ulp(outs["C"], dt)).max())
        print(f"ratio {tag}/|out_lo| over half an ulp of C: {lo_ratio:.4f}")
        assert lo_ratio <= 1.0, f"{label}: a remainder of {lo_ratio:.4f} half ulps of C"
        assert rejected(y, outs["C"].double(), two_b), f"{label}: the two-plane bound accepts one plane"
        if lo_val is not None and not res_ln:
            assert rejected(y, lnf2_reference(*args, ctl="lo")[0], two_b), f"{label}: the bound accepts a dropped resid_lo"
    if lnf == 4:
        blob = outs["LO"].view(torch.uint8).flatten()
        b8 = e_y + 2.0 ** -3 * (U_OUT[dt] * y.abs() * 1.01 + e_y) + 2.0 ** -27
        assert_within(tag + "/C+lo8", outs["C"].double() + lo8_decode(blob, LM, LN_), y, b8)
        assert rejected(y, outs["C"].double(), b8), f"{label}: the eight-bit bound accepts one plane"
        outs["blob"] = blob.clone()
    return outs, y, e_y


@pytest.mark.gpu
@pytest.mark.parametrize("kern,cont,family", [("restart", RESTART, "g7"), ("ring", CONT, "7r16")], ids=["restart", "ring"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_lnf2(dt, kern, cont, family):
    """y = A B^T + bias + LN(resid) with and without rln_stats; C = round16(y); stats_out slot by slot against the UNROUNDED y"""
    d = ln_inputs(dt, LM, LN_, LK, 12, DEV)
    with gemm_options(cont=cont, skinny_m=0):
        run_output_side(dt, 2, family, d, res_ln=True)
        run_output_side(dt, 2, family, d, res_ln=False)


# two-plane kernels: float16 on the ring by default (bit 8), bfloat16 on the restart-per-tile kernel (bit 9 clear)
LNF3_CASES = [(F16, "ring", CONT, "7r16"), (F16, "restart", CONT & ~256, "g7"), (BF16, "restart", CONT, "g7"), (BF16, "ring", CONT | 512, "7r16")]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,kern,cont,family", LNF3_CASES, ids=[f"{NAME[c[0]]}-{c[1]}" for c in LNF3_CASES])
def test_lnf3(dt, kern, cont, family):
    """the residual is resid + resid_lo (or one plane: resid_lo NULL); C + out_lo carries y through a second rounding"""
    d = ln_inputs(dt, LM, LN_, LK, 13, DEV)
    with gemm_options(cont=cont, skinny_m=0):
        run_output_side(dt, 3, family, d, res_ln=True, lo_in=True)
        run_output_side(dt, 3, family, d, res_ln=False, lo_in=True)
        run_output_side(dt, 3, family, d, res_ln=True, lo_in=False)


@pytest.mark.gpu
def test_lnf4():
    """float16 with the eight-bit second plane: decoded through the omk_lo8_offset port as e5m2 2^-10; the blob of the first launch is
    the resid_lo of a second one, whose reference adds the decoded values"""
    d = ln_inputs(F16, LM, LN_, LK, 14, DEV)
    with gemm_options(skinny_m=0):
        outs, _, _ = run_output_side(F16, 4, "7r16", d, res_ln=True)
        d2 = dict(d, R=outs["C"])
        run_output_side(F16, 4, "7r16", d2, res_ln=True, blob_in=outs["blob"])
        run_output_side(F16, 4, "7r16", d2, res_ln=False, blob_in=outs["blob"], walks=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_k128_selects_restart(dt):
    """two K steps: the ring does not fit, every LNF <= 3 runs on the restart-per-tile kernel; the eight-bit plane is refused"""
    d = ln_inputs(dt, LM, LN_, LK, 15, DEV)
    with gemm_options(cont=CONT | 512, skinny_m=0):
        run_lnf1(dt, "erf", "ln", d, "g7", K=128, walks=False)
        run_output_side(dt, 2, "g7", d, K=128, walks=False)
        run_output_side(dt, 3, "g7", d, K=128, walks=False)
        if dt == F16:
            C, S, LO = out_buf(dt, LM, LN_), out_buf(F32, 6 * LM, 2), out_buf(F16, 1, LM * LN_ // 2)
            ep = make_ep(bias=d["bias"], resid=d["R"], ldr=LN_, stats_out=S, out_lo=LO, lo8=1, ln_inv_h=1.0 / LN_, ln_eps=EPS)
            rc, fam = gemm_ex(dt, dt, d["A"], d["B"], C, LM, LN_, 128, ep, lda=LK, ldb=LK)
            assert rc != 0 and fam == 0 and b"K >= 192" in N.lib().om_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_chain_fold_lnf2_lnf1_is_linear_of_layernorm(dt):
    """om_debug_ln_fold, an LNF 2 launch whose stats_out is reduced, an LNF 1 launch reading those statistics: together
    Linear(LayerNorm(x)) of the first launch's STORED output x.  The statistics describe the unrounded y (x = round16(y)) and the folded
    weight is rounded once, so the bound adds: U sum|LN(x)_k||W gamma|_k (the fold), the shift of mean and variance by |y - x| <= U |x| + e_y,
    through rstd |s_n| and 0.5 dvar / var |out - b'|."""
    d = ln_inputs(dt, LM, LN_, LK, 16, DEV)
    H, N2 = LN_, 256
    gen = torch.Generator(device=DEV).manual_seed(3)
    W = (torch.randn(N2, H, generator=gen, device=DEV) / math.sqrt(H)).to(TORCH_DT[dt])
    gamma, beta = 1 + 0.5 * torch.randn(H, generator=gen, device=DEV), 0.3 * torch.randn(H, generator=gen, device=DEV)
    b0 = torch.randn(N2, generator=gen, device=DEV)
    Wf, cs, bf = torch.empty_like(W), torch.empty(N2, device=DEV), torch.empty(N2, device=DEV)
    assert N.lib().om_debug_ln_fold(dt, N.ptr(W), N.ptr(gamma), N.ptr(beta), N.ptr(b0), N.ptr(Wf), N.ptr(cs), N.ptr(bf), N2, H,
                                    N.stream_ptr(torch.device(DEV))) == 0
    with gemm_options(skinny_m=0):
        outs, y, e_y = run_output_side(dt, 2, "7r16", d, res_ln=False, walks=False)
        x = outs["C"].contiguous()
        tot = torch.empty(LM, 2, device=DEV)
        assert N.lib().om_debug_ln_stats_reduce(N.ptr(outs["S"].contiguous()), H // 128, LM, N.ptr(tot), N.stream_ptr(torch.device(DEV))) == 0
        C = out_buf(dt, LM, N2)
        snap = C.snapshot()
        ep = make_ep(bias=bf, ln_stats=tot, ln_colsum=cs, ln_inv_h=1.0 / H, ln_eps=EPS)
        rc, fam = gemm_ex(dt, dt, x, Wf, C, LM, N2, H, ep)
        assert rc == 0 and fam == FAM["7c16"], (rc, fam, N.lib().om_last_error())
        guards_ok("chain", (C, snap))
    # the kernel's own arithmetic on what it read (statistics of y, the folded weight): inside the LNF 1 bound
    ref1, bound1 = lnf1_reference(x, Wf, tot, cs, bf, NONE, None, 1.0 / H, EPS, 0, dt)
    assert_within(f"chain/{NAME[dt]}/lnf1", C.window, ref1, bound1, dt)
    # ... and against Linear(LayerNorm(x)) in float64
    xd, U = x.double(), U_OUT[dt]
    lnx, mean, rstd = ln64(xd, gamma, beta, EPS)
    want = lnx @ W.double().t() + b0.double()
    Wg = (W.double() * gamma.double()).abs()
    dx = 1.01 * U * xd.abs() + e_y
    dmu = dx.mean(1)
    dvar = (2 * xd.abs() * dx + dx * dx).mean(1) + 2 * mean.abs() * dmu + dmu * dmu
    var = 1.0 / (rstd * rstd)
    fold = U * (((xd - mean[:, None]) * rstd[:, None]).abs() @ Wg.t()) + 4 * H * u * (beta.double().abs() @ W.double().abs().t())
    extra = (fold + (rstd * dmu)[:, None] * Wg.sum(1)[None, :] * (1 + U) + (0.5 * dvar / var)[:, None] * 1.05 * (want - bf.double()).abs()
             + 4 * H * u * rstd[:, None] * (xd.abs() @ Wg.t()))
    assert_within(f"chain/{NAME[dt]}/linear-of-layernorm", C.window, want, bound1 + extra * 1.01, dt)
    ctl = (torch.roll(lnx, 1, 0) @ W.double().t() + b0.double())
    assert rejected(want, ctl, bound1 + extra * 1.01), "chain: the bound accepts the neighbouring row's LayerNorm"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_nan_stays_in_its_row(dt):
    """a NaN in one row of A reaches only that row of C and that row's statistics"""
    d = ln_inputs(dt, LM, LN_, LK, 17, DEV)
    d["A"][133, 7] = float("nan")
    with gemm_options(skinny_m=0):
        C = run_lnf1(dt, "none", "ln", d, "7c16", walks=False)
        outs, _, _ = run_output_side(dt, 2, "7r16", d, res_ln=True, walks=False)
    for name, t in (("LNF 1 C", C), ("LNF 2 C", outs["C"]), ("LNF 2 stats", outs["S"].permute(1, 0, 2).reshape(LM, -1))):
        nan_rows = torch.isnan(t.double()).any(1).nonzero().flatten().tolist()
        assert nan_rows == [133] and bool(torch.isnan(t[133].double()).all()), (name, nan_rows)


# (name, dtype, M, K, spec, misaligned pointers, message) -- refused by the planner: om_debug_gemm_plan_ex -1, om_debug_gemm_ex an error
_LN1 = dict(bias=1, ln_stats=1, ln_colsum=1, ln_inv_h=1.0 / LK, ln_eps=EPS)
_LN2 = dict(bias=1, resid=1, ldr=LN_, rln_stats=1, rln_g=1, rln_b=1, stats_out=1, ln_inv_h=1.0 / LN_, ln_eps=EPS)
REFUSALS = [
    ("ln_stats with stats_out", BF16, LM, LK, dict(_LN1, stats_out=1), (), b"fused LayerNorm"),
    ("ln_stats with stats_out f16", F16, LM, LK, dict(_LN1, stats_out=1), (), b"fused LayerNorm"),
    ("LNF 2 without stats_out", BF16, LM, LK, {k: v for k, v in _LN2.items() if k != "stats_out"}, (), b"fused LayerNorm"),
    ("LNF 2 without stats_out f16", F16, LM, LK, {k: v for k, v in _LN2.items() if k != "stats_out"}, (), b"fused LayerNorm"),
    ("out_lo without an output-side LayerNorm", BF16, LM, LK, dict(bias=1, resid=1, ldr=LN_, out_lo=1), (), b"two-plane"),
    ("out_lo without an output-side LayerNorm f16", F16, LM, LK, dict(bias=1, resid=1, ldr=LN_, out_lo=1), (), b"two-plane"),
    ("resid_lo without out_lo", BF16, LM, LK, dict(_LN2, resid_lo=1), (), b"two-plane"),
    ("ldr * 2 % 128", BF16, LM, LK, dict(_LN2, ldr=LN_ + 8), (), b"fused LayerNorm"),
    ("ldr * 2 % 128 f16", F16, LM, LK, dict(_LN2, ldr=LN_ + 8), (), b"fused LayerNorm"),
    ("misaligned bias", BF16, LM, LK, _LN1, ("bias",), b"aligned bias"),
    ("misaligned bias f16", F16, LM, LK, _LN1, ("bias",), b"fused LayerNorm"),
    ("ragged M", BF16, LM - 12, LK, _LN1, (), b"fused LayerNorm"),
    ("ragged M f16", F16, LM + 8, LK, _LN1, (), b"fused LayerNorm"),
    ("f16 MUL_RESID with LNF 1", F16, LM, LK, dict(_LN1, act=TANH | N.ACT_MUL_RESID, resid=1, ldr=LN_), (), b"fused LayerNorm"),
    ("LNF 4 at K = 128", F16, LM, 128, dict(_LN2, out_lo=1, lo8=1), (), b"K >= 192"),
    ("gelu' without resid", BF16, 130, LK, dict(bias=1, act=N.ACT_GELU_ERF_GRAD), (), b"needs resid"),
    ("a_ln32 with K > 1024", BF16, 17, 2048, dict(a_ln32=1, a_ln_g=1, a_ln_b=1, ln_eps=EPS), (), b"few-rows kernel only"),
    ("a_ln32 without a_ln_b", BF16, 17, 768, dict(a_ln32=1, a_ln_g=1, ln_eps=EPS), (), b"few-rows kernel only"),
    ("a_ln32 at 64 rows per workgroup", BF16, 1024, 768, dict(a_ln32=1, a_ln_g=1, a_ln_b=1, ln_eps=EPS), (), b"few-rows kernel only"),
    ("rln32 without statistics", F16, 17, 768, dict(rln32=1, rln_g=1, rln_b=1, ldr=LN_), (), b"few-rows kernel only"),
]


@pytest.mark.parametrize("name,dt,M,K,spec,misalign,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_through_both_hooks(name, dt, M, K, spec, misalign, text):
    """no GPU: a refusal comes before any launch and reads no pointer"""
    lib = N.lib()
    ep = fake_ep(spec, misalign)
    assert plan(dt, dt, M, LN_, K, ep) == -1
    rc = lib.om_debug_gemm_ex(dt, 1 << 32, K, 2 << 32, K, dt, 3 << 32, LN_, M, LN_, K, ctypes.byref(ep), None)
    assert rc != 0 and lib.om_debug_gemm_last() == 0 and text in lib.om_last_error(), lib.om_last_error()
    assert lib.om_debug_gemm_ex(dt, 1 << 32, K, 2 << 32, K, dt, 3 << 32, LN_, M, LN_, K, None, None) != 0       # a null epilogue
    assert plan(dt, dt, 0, LN_, K, ep) == 0                                                                      # an empty problem
    assert lib.om_debug_gemm_splitk(dt, 1 << 32, 100, 2 << 32, 100, 3 << 32, LN_, M, LN_, 100, None) != 0 and b"128" in lib.om_last_error()


# ---------------------------------------------------------------------------------------------------------------
# B. training epilogues
# ---------------------------------------------------------------------------------------------------------------
# family -> (options, dtype pairs, (M, N, K steps of 128 bytes))
TRAIN_FAMILIES = {
    "v1": (dict(variant=1), [(BF16, BF16), (F16, F16), (F32, F32), (BF16, F32)], (130, 200, 4)),
    "v2": (dict(variant=2), [(BF16, BF16), (F16, F16), (F32, F32), (BF16, F32)], (512, 200, 3)),
    "v6": (dict(variant=6), [(BF16, BF16), (F32, F32)], (512, 520, 3)),
}
TRAIN_CASES = [pytest.param(fam, i, o, id=f"{fam}-{NAME[i]}->{NAME[o]}") for fam, (_, pairs, _) in TRAIN_FAMILIES.items() for i, o in pairs]


def ksteps(in_dt, n):
    return n * (32 if in_dt == F32 else 64)


def train_inputs(in_dt, out_dt, M, Nn, K, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, device=DEV, dtype=torch.float32)
    return dict(A=rnd(M, K).to(TORCH_DT[in_dt]), B=(rnd(Nn, K) / math.sqrt(K)).to(TORCH_DT[in_dt]), bias=rnd(Nn),
                R=rnd(M, Nn).to(TORCH_DT[out_dt]))


def launch_train(label, family, in_dt, out_dt, d, M, Nn, K, ldc=None, tape_ld=None, **kw):
    """one launch with guard-checked C (and tape); returns (C window, tape window or None)"""
    C = out_buf(out_dt, M, Nn, ldc or Nn + 8)
    bufs = [(C, C.snapshot())]
    T = None
    if tape_ld:
        T = out_buf(out_dt, M, Nn, tape_ld)
        bufs.append((T, T.snapshot()))
        kw.update(pre_act=T, ldp=tape_ld)
    frozen = Frozen(**{k: v for k, v in d.items() if isinstance(v, torch.Tensor)})
    rc, fam = gemm_ex(in_dt, out_dt, d["A"], d["B"], C, M, Nn, K, make_ep(**kw))
    assert rc == 0, (label, N.lib().om_last_error())
    assert fam == FAM[family], f"{label}: ran family {fam}, expected {family}"
    guards_ok(label, *bufs)
    frozen.check(label)
    return C.window.clone(), (T.window.clone() if T is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,in_dt,out_dt", TRAIN_CASES)
def test_dropout_residual(fam, in_dt, out_dt):
    """out = dropout(A B^T + bias) + resid (the out-projection and FFN2 site): dropped elements ARE the residual, kept ones lie inside the
    bound with DropCfg's keep scale; drop_rows = identity gives the bits of NULL; a permutation gives the rows of the padded call, permuted"""
    opts, _, (M, Nn, ks) = TRAIN_FAMILIES[fam]
    K = ksteps(in_dt, ks)
    d = train_inputs(in_dt, out_dt, M, Nn, K, 21)
    seed = 0x1234_5678_9ABC
    with gemm_options(**opts):
        for p in (0.1, 0.5):
            label = f"drop {fam} {NAME[in_dt]}->{NAME[out_dt]} p={p}"
            kw = dict(bias=d["bias"], resid=d["R"], ldr=Nn, drop_p=p, seed=seed)
            C, _ = launch_train(label, fam, in_dt, out_dt, d, M, Nn, K, **kw)
            ref, bound, _, _, keep = train_reference(d["A"], d["B"], d["bias"], NONE, d["R"], False, out_dt, K, p=p, seed=seed)
            assert_within(f"drop/{fam}/{NAME[in_dt]}->{NAME[out_dt]}", C, ref, bound, out_dt)
            assert torch.equal(_bits(C[~keep].contiguous()), _bits(d["R"][~keep].contiguous())), f"{label}: a dropped element is not the residual"
            assert rejected(ref, train_reference(d["A"], d["B"], d["bias"], NONE, d["R"], False, out_dt, K, p=p, seed=seed, k_used=K - K // ks)[0], bound)
            ident = torch.arange(M, dtype=torch.int32, device=DEV)
            Ci, _ = launch_train(label + " identity", fam, in_dt, out_dt, dict(d, rows=ident), M, Nn, K, drop_rows=ident, **kw)
            assert torch.equal(_bits(Ci), _bits(C)), f"{label}: drop_rows = identity changes the output"
            perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).to(torch.int32).to(DEV)
            dp = dict(d, A=d["A"][perm.long()].contiguous(), R=d["R"][perm.long()].contiguous(), rows=perm)
            Cp, _ = launch_train(label + " permuted", fam, in_dt, out_dt, dp, M, Nn, K, **dict(kw, resid=dp["R"], drop_rows=perm))
            assert torch.equal(_bits(Cp), _bits(C[perm.long()].contiguous())), f"{label}: a permuted drop_rows does not give the padded call's rows"
            # the control: the mask taken at m where drop_rows[m] was asked for
            refp, boundp, _, _, keep_p = train_reference(dp["A"], dp["B"], d["bias"], NONE, dp["R"], False, out_dt, K, p=p, seed=seed, rows=perm)
            assert_within(f"drop/{fam}/{NAME[in_dt]}->{NAME[out_dt]}", Cp, refp, boundp, out_dt)
            wrong = train_reference(dp["A"], dp["B"], d["bias"], NONE, dp["R"], False, out_dt, K, p=p, seed=seed)[0]
            assert rejected(refp, wrong, boundp), f"{label}: the bound accepts the mask of row m for drop_rows[m]"


@pytest.mark.gpu
@pytest.mark.parametrize("fam,in_dt,out_dt", TRAIN_CASES)
def test_pre_act(fam, in_dt, out_dt):
    """erf-GELU with a tape: acc + bias without OM_ACT_PRE_GRAD, gelu'(acc + bias) with it (ldp != ldc); the T5 sites -- a ReLU tape with
    dropout behind it, and the gated tanh-GELU x resid with tape, dropout and drop_rows; tanh and no activation with tape + dropout"""
    opts, _, (M, Nn, ks) = TRAIN_FAMILIES[fam]
    K = ksteps(in_dt, ks)
    d = train_inputs(in_dt, out_dt, M, Nn, K, 22)
    tag = f"{fam}/{NAME[in_dt]}->{NAME[out_dt]}"
    with gemm_options(cont=CONT & ~32, **opts):
        for grad in (False, True):
            label = f"tape {tag} grad={grad}"
            C, T = launch_train(label, fam, in_dt, out_dt, d, M, Nn, K, tape_ld=Nn + 16, bias=d["bias"],
                                act=ERF | (N.ACT_PRE_GRAD if grad else 0))
            ref, bound, tape, tb, _ = train_reference(d["A"], d["B"], d["bias"], ERF, None, False, out_dt, K, pre_grad=grad)
            assert_within(f"tape/{tag}/C", C, ref, bound, out_dt)
            assert_within(f"tape/{tag}/{'grad' if grad else 'pre'}", T, tape, tb, out_dt)
            other = train_reference(d["A"], d["B"], d["bias"], ERF, None, False, out_dt, K, pre_grad=not grad)[2]
            assert rejected(tape, other, tb), f"{label}: the bound accepts the other tape"
            assert rejected(tape, torch.roll(tape, 1, 1), tb), f"{label}: the bound accepts the tape one column off"
        label = f"T5 tape + dropout {tag}"
        seed, p = 99, 0.1
        C, T = launch_train(label, fam, in_dt, out_dt, d, M, Nn, K, tape_ld=Nn + 16, bias=d["bias"], act=RELU, drop_p=p, seed=seed)
        ref, bound, tape, tb, keep = train_reference(d["A"], d["B"], d["bias"], RELU, None, False, out_dt, K, p=p, seed=seed)
        assert_within(f"tape/{tag}/T5 C", C, ref, bound, out_dt)
        assert_within(f"tape/{tag}/T5 pre", T, tape, tb, out_dt)
        assert bool((C[~keep].double() == 0).all()), f"{label}: a dropped element is not zero"
        # the gated T5 FFN1 (train.hip): tanh-GELU, the tape, dropout keyed on drop_rows and the multiplied residual in ONE call
        label = f"gated T5 {tag}"
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(6)).to(torch.int32).to(DEV)
        dg = dict(d, rows=perm)
        C, T = launch_train(label, fam, in_dt, out_dt, dg, M, Nn, K, tape_ld=Nn + 16, bias=d["bias"], act=TANH | N.ACT_MUL_RESID, resid=d["R"],
                            ldr=Nn, drop_p=0.5, seed=seed, drop_rows=perm)
        ref, bound, tape, tb, keep = train_reference(d["A"], d["B"], d["bias"], TANH, d["R"], True, out_dt, K, p=0.5, seed=seed, rows=perm)
        assert_within(f"gated/{tag}/C", C, ref, bound, out_dt)
        assert_within(f"gated/{tag}/pre", T, tape, tb, out_dt)
        assert bool((C[~keep].double() == 0).all()), f"{label}: a dropped element is not zero"
        assert rejected(ref, train_reference(d["A"], d["B"], d["bias"], TANH, d["R"], True, out_dt, K, p=0.5, seed=seed)[0], bound), \
            f"{label}: the bound accepts the mask of row m for drop_rows[m]"
        assert rejected(ref, train_reference(d["A"], d["B"], d["bias"], TANH, torch.roll(d["R"], 1, 1), True, out_dt, K, p=0.5, seed=seed, rows=perm)[0], bound)
        # the remaining training forms: tanh-GELU without a residual, and no activation without a residual (tape + dropout)
        for act, name in ((TANH, "tanh"), (NONE, "none")):
            label = f"{name} tape + dropout {tag}"
            C, T = launch_train(label, fam, in_dt, out_dt, d, M, Nn, K, tape_ld=Nn + 16, bias=d["bias"], act=act, drop_p=0.5, seed=seed)
            ref, bound, tape, tb, keep = train_reference(d["A"], d["B"], d["bias"], act, None, False, out_dt, K, p=0.5, seed=seed)
            assert_within(f"tape/{tag}/{name} C", C, ref, bound, out_dt)
            assert_within(f"tape/{tag}/{name} pre", T, tape, tb, out_dt)
            assert bool((C[~keep].double() == 0).all()), f"{label}: a dropped element is not zero"
            assert rejected(ref, train_reference(d["A"], d["B"], d["bias"], act, None, False, out_dt, K, p=0.5, seed=seed + 1)[0], bound)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_pre_act_two_output_ring(dt):
    """the training forward's FFN1 on the continuous ring: C = gelu(v) and the tape gelu'(v), 512 x 512 x 256, ldp == ldc"""
    M, Nn, K = 512, 512, 256
    d = train_inputs(dt, dt, M, Nn, K, 23)
    with gemm_options(skinny_m=0):
        first = None
        for cap in (None, 1, 4):
            with gemm_options(**({} if cap is None else dict(max_grid=cap))):
                C, T = launch_train(f"7c16 TRAIN {NAME[dt]} max_grid={cap}", "7c16", dt, dt, d, M, Nn, K, ldc=Nn + 64, tape_ld=Nn + 64,
                                    bias=d["bias"], act=ERF | N.ACT_PRE_GRAD)
            if first is None:
                first = (C, T)
            assert torch.equal(_bits(C), _bits(first[0])) and torch.equal(_bits(T), _bits(first[1])), f"max_grid={cap} changes the output"
    ref, bound, tape, tb, _ = train_reference(d["A"], d["B"], d["bias"], ERF, None, False, dt, K, pre_grad=True)
    assert_within(f"tape/7c16/{NAME[dt]}/C", first[0], ref, bound, dt)
    assert_within(f"tape/7c16/{NAME[dt]}/grad", first[1], tape, tb, dt)
    assert rejected(tape, torch.roll(tape, 1, 1), tb) and rejected(tape, ref, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,in_dt,out_dt", TRAIN_CASES)
def test_gelu_grad(fam, in_dt, out_dt):
    """OM_ACT_GELU_ERF_GRAD: (acc + bias) gelu'(resid); and the backward with a gelu' tape, OM_ACT_NONE | OM_ACT_MUL_RESID"""
    opts, _, (M, Nn, ks) = TRAIN_FAMILIES[fam]
    K = ksteps(in_dt, ks)
    d = train_inputs(in_dt, out_dt, M, Nn, K, 24)
    d["R"] = (d["R"].float() * 2).to(d["R"].dtype)                     # pre-activations out to +-6: the clamp of the fast form at 4.2 is reached
    tag = f"{fam}/{NAME[in_dt]}->{NAME[out_dt]}"
    with gemm_options(**opts):
        C, _ = launch_train(f"gelu' {tag}", fam, in_dt, out_dt, d, M, Nn, K, bias=d["bias"], resid=d["R"], ldr=Nn, act=N.ACT_GELU_ERF_GRAD)
        ref, bound = grad_reference(d["A"], d["B"], d["bias"], d["R"], out_dt, K)
        assert_within(f"grad/{tag}", C, ref, bound, out_dt)
        assert rejected(ref, grad_reference(d["A"], d["B"], d["bias"], d["R"], out_dt, K, ctl="tape")[0], bound)
        C, _ = launch_train(f"none x resid {tag}", fam, in_dt, out_dt, d, M, Nn, K, bias=d["bias"], resid=d["R"], ldr=Nn,
                            act=NONE | N.ACT_MUL_RESID)
        ref, bound, _, _, _ = train_reference(d["A"], d["B"], d["bias"], NONE, d["R"], True, out_dt, K)
        assert_within(f"none x resid/{tag}", C, ref, bound, out_dt)
        assert rejected(ref, train_reference(d["A"], d["B"], d["bias"], NONE, torch.roll(d["R"], 1, 1), True, out_dt, K)[0], bound)


# ---------------------------------------------------------------------------------------------------------------
# C. the few-rows kernel
# ---------------------------------------------------------------------------------------------------------------
FEW_M = [1, 17, 32, 33, 64]
FEW_SHAPES = [(208, 128), (768, 768), (208, 1024), (768, 1024)]            # (N, K)
FEW_PARAMS = [pytest.param(dt, n, k, id=f"{NAME[dt]}-N{n}-K{k}") for dt in (BF16, F16) for n, k in FEW_SHAPES]


def few_launch(label, dt, d, M, Nn, K, A=None, want32=False, **kw):
    C = out_buf(dt, M, Nn, Nn + 8)
    bufs = [(C, C.snapshot())]
    O = None
    if want32:
        O = out_buf(F32, M, Nn, Nn + 8)                    # out32 shares ldc
        bufs.append((O, O.snapshot()))
        kw["out32"] = O
    frozen = Frozen(**{k: v for k, v in d.items() if isinstance(v, torch.Tensor)})
    rc, fam = gemm_ex(dt, dt, d["A"] if A is None else A, d["B"], C, M, Nn, K, make_ep(**kw))
    assert rc == 0 and fam == FAM["skinny"], (label, rc, fam, N.lib().om_last_error())
    if want32:                                             # the header: the sum goes to out32 INSTEAD of C
        assert torch.equal(C.snapshot(), bufs[0][1]), f"{label}: C touched although out32 takes the sum"
    guards_ok(label, *bufs)
    frozen.check(label)
    return C.window.clone(), (O.window.clone() if O is not None else None)


def rows_of(full, M):
    """the first M rows of every per-row tensor of a 64-row input set"""
    return {k: (v[:M].contiguous() if k in ("A", "x32", "r32") else v) for k, v in full.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Nn,K", FEW_PARAMS)
def test_few_rows_f32_stream(dt, Nn, K):
    """resid32 / out32: the f32 sum acc + bias + resid32, into C (rounded) or into out32 (C untouched)"""
    for M in FEW_M:
        d = few_inputs(dt, M, Nn, K, 31 + M)
        y, e = few_f32_reference(d["A"], d["B"], d["bias"], d["r32"], K)
        label = f"few rows f32 stream {NAME[dt]} M={M} N={Nn} K={K}"
        _, O = few_launch(label, dt, d, M, Nn, K, want32=True, bias=d["bias"], resid32=d["r32"], ldr=Nn)
        assert_within(f"few/{NAME[dt]}/out32", O, y, e)
        C, _ = few_launch(label, dt, d, M, Nn, K, bias=d["bias"], resid32=d["r32"], ldr=Nn)
        assert_within(f"few/{NAME[dt]}/resid32", C, y, stored_bound(y, e, dt), dt)
        assert torch.equal(_bits(C), _bits(O.to(TORCH_DT[dt]))), f"{label}: C is not out32 rounded once"
        assert rejected(y, few_f32_reference(d["A"], d["B"], d["bias"], d["r32"], K, ctl="resid")[0], e), f"{label}: the bound accepts the residual one column off"


def a_ln_launch(label, dt, d, M, Nn, K):
    st = torch.full((M + 2, 2), 7.5, device=DEV)
    C, _ = few_launch(label, dt, d, M, Nn, K, bias=d["bias"], a_ln32=d["x32"], a_ln_g=d["ag"], a_ln_b=d["ab"], a_ln_stats_out=st, ln_eps=EPS)
    assert bool((st[M:] == 7.5).all()), f"{label}: a_ln_stats_out written past row M"
    return C, st[:M]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Nn,K", FEW_PARAMS)
def test_few_rows_a_ln32(dt, Nn, K):
    """the operand rows are LN(a_ln32): C equals, bit for bit, the plain call on om_debug_layernorm_from_f32's rows and lies inside the float64
    bound; a_ln_stats_out is the float64 (mean, rstd)"""
    full = few_inputs(dt, 64, Nn, K, 41)
    for M in FEW_M:
        d = rows_of(full, M)
        label = f"few rows a_ln32 {NAME[dt]} M={M} N={Nn} K={K}"
        C, st = a_ln_launch(label, dt, d, M, Nn, K)
        xn = torch.empty(M, K, dtype=TORCH_DT[dt], device=DEV)
        assert N.lib().om_debug_layernorm_from_f32(dt, N.ptr(d["x32"]), K, N.ptr(xn), K, N.ptr(d["ag"]), N.ptr(d["ab"]), M, K, EPS, 0,
                                                   N.stream_ptr(torch.device(DEV))) == 0
        sync()
        Cp, _ = few_launch(label + " plain", dt, d, M, Nn, K, A=xn, bias=d["bias"])
        assert torch.equal(_bits(C), _bits(Cp)), f"{label}: differs from the plain call on the LayerNorm kernel's rows"
        y, e, mean, mb, rstd, rrel = a_ln_reference(d["x32"], d["ag"], d["ab"], d["B"], d["bias"], K, dt)
        assert_within(f"few/{NAME[dt]}/a_ln32", C, y, stored_bound(y, e, dt), dt)
        assert rejected(y, a_ln_reference(d["x32"], d["ag"], d["ab"], d["B"], d["bias"], K, dt, ctl="shift")[0], stored_bound(y, e, dt))
        assert_within(f"few/{NAME[dt]}/a_ln mean", st[:, 0], mean, mb)
        assert_within(f"few/{NAME[dt]}/a_ln rstd", st[:, 1], rstd, rstd * rrel)
        if M > 1:
            assert rejected(rstd, torch.roll(rstd, 1), rstd * rrel), f"{label}: the bound accepts the neighbouring row's rstd"


def rln_launch(label, dt, d, M, Nn, K, stats):
    return few_launch(label, dt, d, M, Nn, K, want32=True, bias=d["bias"], rln32=d["r32"], rln32_stats=stats, rln_g=d["g"], rln_b=d["b"], ldr=Nn)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Nn,K", FEW_PARAMS)
def test_few_rows_rln32(dt, Nn, K):
    """the residual is LN(rln32) re-derived from rln32_stats: inside the float64 bound; and, with the statistics an a_ln32 launch left, bit for
    bit the resid32 call fed the LayerNorm kernel's f32 output (N = 768: a row the a_ln32 form takes)"""
    full = few_inputs(dt, 64, Nn, K, 42)
    for M in FEW_M:
        d = rows_of(full, M)
        label = f"few rows rln32 {NAME[dt]} M={M} N={Nn} K={K}"
        y, e, st = rln_reference(d["A"], d["B"], d["bias"], d["r32"], d["g"], d["b"], K)
        O = rln_launch(label, dt, d, M, Nn, K, st.contiguous())
        assert_within(f"few/{NAME[dt]}/rln32", O, y, e)
        assert rejected(y, rln_reference(d["A"], d["B"], d["bias"], d["r32"], d["g"], d["b"], K, ctl="shift")[0], e)
        if Nn == 768:
            zeros = dict(d, A=torch.zeros(M, Nn, dtype=TORCH_DT[dt], device=DEV), B=torch.zeros(16, Nn, dtype=TORCH_DT[dt], device=DEV),
                         x32=d["r32"], ag=d["g"], ab=d["b"], bias=torch.zeros(16, device=DEV))
            _, st2 = a_ln_launch(label + " statistics", dt, zeros, M, 16, Nn)
            y32 = torch.empty(M, Nn, device=DEV)
            assert N.lib().om_debug_layernorm_f32out(F32, N.ptr(d["r32"]), Nn, N.ptr(y32), Nn, N.ptr(d["g"]), N.ptr(d["b"]), M, Nn, EPS, 0, None, None, 0,
                                                     N.stream_ptr(torch.device(DEV))) == 0
            sync()
            O1 = rln_launch(label + " own statistics", dt, d, M, Nn, K, st2.contiguous())
            _, O2 = few_launch(label + " resid32", dt, d, M, Nn, K, want32=True, bias=d["bias"], resid32=y32, ldr=Nn)
            assert torch.equal(_bits(O1), _bits(O2)), f"{label}: rln32 differs from resid32 fed the LayerNorm kernel's f32 output"


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Nn,K", FEW_PARAMS)
def test_few_rows_batch_invariance(dt, Nn, K):
    """row m of an M = 64 call equals the M = 1 call of that row (rows 0, 33 -- the third row tile -- and 63), for the plain, resid32, a_ln32
    and rln32 forms"""
    full = few_inputs(dt, 64, Nn, K, 43)
    st = rln_reference(full["A"], full["B"], full["bias"], full["r32"], full["g"], full["b"], K)[2].contiguous()

    def forms(d, M, stats):
        lab = f"batch invariance {NAME[dt]} M={M} N={Nn} K={K}"
        return {"plain": few_launch(lab, dt, d, M, Nn, K, bias=d["bias"])[0],
                "resid32": few_launch(lab, dt, d, M, Nn, K, bias=d["bias"], resid32=d["r32"], ldr=Nn)[0],
                "a_ln32": a_ln_launch(lab, dt, d, M, Nn, K)[0],
                "rln32": rln_launch(lab, dt, d, M, Nn, K, stats)}
    big = forms(full, 64, st)
    for m in (0, 33, 63):
        one = {k: (v[m:m + 1].contiguous() if k in ("A", "x32", "r32") else v) for k, v in full.items()}
        small = forms(one, 1, st[m:m + 1].contiguous())
        for k in big:
            assert torch.equal(_bits(small[k][0]), _bits(big[k][m])), f"{k}: row {m} of the M = 64 call differs from the M = 1 call of that row"


# ---------------------------------------------------------------------------------------------------------------
# D. split-K
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nk", [4, 8, 22], ids=["1-slice", "2-slices", "5-slices-short-last"])
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=lambda d: NAME[d])
def test_splitk(dt, nk):
    """C (f32, pre-filled) += A B^T with K = nk steps of 128 bytes sliced over workgroups that meet in f32 atomics: each run inside the bound,
    and the two runs within the bound of each other (the order of the atomics is free)"""
    M, Nn = 130, 200
    es = 4 if dt == F32 else 2
    K = nk * 128 // es
    slices = splitk_slices(M, Nn, K, es)[0]
    assert slices == {4: 1, 8: 2, 22: 5}[nk]
    gen = torch.Generator(device=DEV).manual_seed(50 + nk)
    A = torch.randn(M, K, generator=gen, device=DEV).to(TORCH_DT[dt])
    B = torch.randn(Nn, K, generator=gen, device=DEV).to(TORCH_DT[dt])
    C0 = torch.randn(M, Nn, generator=gen, device=DEV) * 3
    ref, bound = splitk_reference(A, B, C0, K, slices)
    frozen = Frozen(A=A, B=B)
    outs = []
    for _ in range(2):
        C = Buf(F32, M, Nn, Nn + 4, fill=C0)
        snap = C.snapshot()
        with torch.cuda.device(DEV):
            rc = N.lib().om_debug_gemm_splitk(dt, N.ptr(A), K, N.ptr(B), K, C.ptr(), C.ld, M, Nn, K, N.stream_ptr(torch.device(DEV)))
        sync()
        assert rc == 0, N.lib().om_last_error()
        guards_ok("split-K", (C, snap))
        assert_within(f"splitk/{NAME[dt]}", C.window, ref, bound)
        outs.append(C.window.clone())
    frozen.check("split-K")
    assert bool(((outs[0].double() - outs[1].double()).abs() <= bound).all()), "split-K: two runs farther apart than the bound"
    assert rejected(ref, splitk_reference(A, B, C0, K, slices, ctl="k_step")[0], bound)      # the last K step dropped
    assert rejected(ref, splitk_reference(A, B, C0, K, slices, ctl="store")[0], bound)       # C overwritten, not added to


# ---------------------------------------------------------------------------------------------------------------
# E. the decision table of the cases above, without a GPU
# ---------------------------------------------------------------------------------------------------------------
def _plan_table():
    """(label, options, in, out, M, N, K, spec, ldc, family) of every GPU case above"""
    for p in LNF1_CASES:
        dt, act, kern, cont, fam = p.values
        for variant in LNF1_VARIANTS:
            yield f"lnf1 {act} {variant} {kern}", dict(cont=cont, skinny_m=0), dt, dt, LM, LN_, LK, lnf1_spec(act, variant), LN_ + 64, fam
    out2 = dict(bias=1, resid=1, ldr=LN_, stats_out=1, ln_inv_h=1.0 / LN_, ln_eps=EPS)
    ln2 = dict(out2, rln_stats=1, rln_g=1, rln_b=1)
    for dt in (BF16, F16):
        for cont, fam in ((RESTART, "g7"), (CONT, "7r16")):
            for spec in (ln2, out2):
                yield "lnf2", dict(cont=cont, skinny_m=0), dt, dt, LM, LN_, LK, spec, LN_ + 64, fam
        yield "chain lnf1", dict(skinny_m=0), dt, dt, LM, 256, LN_, dict(bias=1, ln_stats=1, ln_colsum=1), 256, "7c16"
        yield "nan lnf1", dict(skinny_m=0), dt, dt, LM, LN_, LK, lnf1_spec("none", "ln"), LN_ + 64, "7c16"
        for lnf, spec in ((1, lnf1_spec("erf", "ln", 128)), (2, ln2), (3, dict(ln2, out_lo=1, resid_lo=1))):
            yield f"K=128 lnf{lnf}", dict(cont=CONT | 512, skinny_m=0), dt, dt, LM, LN_, 128, spec, LN_ + 64, "g7"
        yield "7c16 TRAIN", dict(skinny_m=0), dt, dt, 512, 512, 256, dict(bias=1, act=ERF | N.ACT_PRE_GRAD, pre_act=1, ldp=576), 576, "7c16"
    for dt, kern, cont, fam in LNF3_CASES:
        for spec in (dict(ln2, out_lo=1, resid_lo=1), dict(out2, out_lo=1, resid_lo=1), dict(ln2, out_lo=1)):
            yield f"lnf3 {kern}", dict(cont=cont, skinny_m=0), dt, dt, LM, LN_, LK, spec, LN_ + 64, fam
    for spec in (dict(ln2, out_lo=1, lo8=1), dict(ln2, out_lo=1, resid_lo=1, lo8=1), dict(out2, out_lo=1, resid_lo=1, lo8=1)):
        yield "lnf4", dict(skinny_m=0), F16, F16, LM, LN_, LK, spec, LN_ + 64, "7r16"
    for fam, (opts, pairs, (M, Nn, ks)) in TRAIN_FAMILIES.items():
        for i, o in pairs:
            K = ksteps(i, ks)
            for spec in (dict(bias=1, resid=1, ldr=Nn, drop_p=0.1, seed=1), dict(bias=1, resid=1, ldr=Nn, drop_p=0.5, seed=1, drop_rows=1),
                         dict(bias=1, resid=1, ldr=Nn, act=N.ACT_GELU_ERF_GRAD), dict(bias=1, resid=1, ldr=Nn, act=NONE | N.ACT_MUL_RESID)):
                yield f"train {fam}", opts, i, o, M, Nn, K, spec, Nn + 8, fam
            for spec in (dict(bias=1, act=ERF, pre_act=1, ldp=Nn + 16), dict(bias=1, act=ERF | N.ACT_PRE_GRAD, pre_act=1, ldp=Nn + 16),
                         dict(bias=1, act=RELU, pre_act=1, ldp=Nn + 16, drop_p=0.1, seed=1),
                         dict(bias=1, act=TANH | N.ACT_MUL_RESID, resid=1, ldr=Nn, pre_act=1, ldp=Nn + 16, drop_p=0.5, seed=1, drop_rows=1),
                         dict(bias=1, act=TANH, pre_act=1, ldp=Nn + 16, drop_p=0.5, seed=1),
                         dict(bias=1, act=NONE, pre_act=1, ldp=Nn + 16, drop_p=0.5, seed=1)):
                yield f"tape {fam}", dict(opts, cont=CONT & ~32), i, o, M, Nn, K, spec, Nn + 8, fam
    for dt in (BF16, F16):
        for Nn, K in FEW_SHAPES:
            for M in FEW_M:
                for spec in (dict(bias=1, resid32=1, ldr=Nn, out32=1), dict(bias=1, resid32=1, ldr=Nn),
                             dict(bias=1, a_ln32=1, a_ln_g=1, a_ln_b=1, a_ln_stats_out=1, ln_eps=EPS),
                             dict(bias=1, rln32=1, rln32_stats=1, rln_g=1, rln_b=1, ldr=Nn, out32=1)):
                    yield "few rows", {}, dt, dt, M, Nn, K, spec, Nn + 8, "skinny"


def test_plan_table_without_a_gpu():
    """om_debug_gemm_plan_ex names, for every GPU case of this file, the family that case asserts; every refusal is -1 (test_refusals_through_both_hooks)"""
    wrong, n = [], 0
    for label, opts, i, o, M, Nn, K, spec, ldc, fam in _plan_table():
        with gemm_options(**opts):
            got = plan(i, o, M, Nn, K, fake_ep(spec), ldc=ldc)
        n += 1
        if got != FAM[fam]:
            wrong.append((label, opts, NAME[i], NAME[o], M, Nn, K, spec, fam, got))
    assert n > 300, n
    assert not wrong, f"{len(wrong)} of {n} cases planned another family, e.g. {wrong[:4]}"
