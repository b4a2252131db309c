"""The last three stages of a training step, kernel by kernel, against float64 references on the exact stored float32 inputs, element by
element, within bounds derived from the arithmetic: csrc/contrastive.hip (the loss and its two gradients), csrc/optim.hip (squared
gradient norm, AdamW with clipping and shadow copies, the dynamic loss scale) and the two small f32 contractions of
csrc/train_kernels.hip behind om_linear_f32_backward.  Everything is called through the public C ABI with hand-built tables
(native.OmAdamTensor); one case per group goes through the Python wrapper and must give the same bits.

References (float64 on the CPU; test_references_are_torchs checks each against torch):
    loss        S = q p^T;  lse_i = log sum_j exp S_ij;  l_i = lse_i - S[i, t_i] (0 for t_i = -100);  t_i = i n_psg by default
                mean: scale sum l / valid;  sum: scale sum l;  none: scale l_i         (F.cross_entropy(S, t, reduction) * scale)
                dS_ij = (softmax_ij - [j = t_i]) coef_i, coef_i = scale / valid | scale | scale row_grad_i, 0 for an ignored row
                d_q = (dS p)[q_row0 : q_row0 + q_rows],  d_p = (dS^T q)[p_row0 : p_row0 + p_rows]          (autograd of the above)
    AdamW       G = g gs c, gs = grad_scale / loss scale, c = min(1, max_norm / (|g gs|_2 + 1e-6))         (clip_grad_norm_)
                p1 = p (1 - lr wd);  m' = m + (G - m)(1 - b1);  v' = v b2 + (1 - b2) G G;
                p' = p1 - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc = 1 - b^n, n = step - skipped steps
                (torch.optim.AdamW(foreach=False, fused=False), one step from the given m, v and step; every hyper-parameter is a
                float32 value, the reference takes it as that value in float64)
    head        dW = dy^T x, dx = dy W

Bounds (u = 2^-24, first order in u; the functions carry the same text):
    scores   one wave per dot product: a lane's fmaf chain of at most ceil(d / 64) (scalar loads) or 4 ceil(d / 256) terms, then six
             additions of the wave tree; the f32 MFMA GEMM sums in another order.  Any order of an f32 sum of d products is within
             (d + 8) u sum_c |q_c p_c|; that is e_S.
    lse      The kernel reads its own stored scores S' (|S' - S| <= e_S); lse is 1-Lipschitz in the largest perturbation of a row,
             E_i = max_j e_S.  Then t_j = S'_j - max: u |t_j|, which the exponential turns into a relative u |t_j|; expf: EXP_REL
             relative plus 2^-126 absolute (underflow); the sum of Pg non-negative terms through ceil(Pg / 64) + 6 additions:
             r_sum = sum_j P_j (u |t_j| + EXP_REL) + (ceil(Pg / 64) + 6) u + Pg 2^-126; logf turns r_sum into an absolute error and
             adds LOG_ABS max(1, |log sum| / log 2) (the measured absolute error for results up to log 2, growing with the result's
             binade as an error of a fixed number of ulps does); max + log: u |lse|; lse - S[t]: e_S[i, t] + u |l_i|.
    loss     none: scale e_l + u |loss_i|.  sum / mean: the wave's sum of Qg terms, (ceil(Qg / 64) + 6) u sum |l_i| + sum e_l, times
             scale (/ valid), one division (DIVSQRT_REL, the allowance test_row_kernels gives a single division) and one product.
    dS       P_j = expf(t_j) (1 / sum): relative u |t_j| + EXP_REL + r_sum + DIVSQRT_REL + u, from S' relative e_S[i, j] +
             sum_k P_k e_S[i, k], absolute 2^-126;  P - onehot: u;  coef: one division (mean) or one product (none);  times coef: u.
    d_q, d_p the serial fmaf chain over Pg (Qg) terms: Pg u sum_j |dS_ij p_jc| + sum_j e_dS_ij |p_jc|, and the same with Qg.
    sq. norm A sum of non-negative terms: relative (longest chain of additions a term passes through) u.  grad_sqnorm_kernel,
             scalar path (the longer one): the square, 16384 / 256 = 64 additions of a thread, six of the wave tree, three of the
             four waves = 74 (vector path: 1 + 3 + 16 + 1 + 6 + 3 = 30).  sqnorm_reduce_kernel: ceil(n / 1024) per thread, six,
             sixteen.  SS_CHAIN(n_chunks) = 74 + 22 + ceil(n_chunks / 1024).
    AdamW    r_gs: u when the loss-scale state multiplies grad_scale.  Clip factor x = max_norm / (sqrtf(ss) |gs| + 1e-6f):
             r_x = SS_CHAIN u / 2 + r_gs + DIVSQRT_REL (the root and the division) + 3 u (the product, the addition, the constant);
             x (1 - r_x) >= 1: the factor is exactly 1 and adds nothing; otherwise min(1, .) is 1-Lipschitz and the factor carries
             r_x x / min(1, x), and gs * factor one more u.  G = g gs: e_G = |G| (r_gs' + u).
             m' = m + (G - m) a1, a1 = 1 - b1 in f32:   e_m = a1 e_G + 3 u a1 |G - m| + u |m'|
             v' = v b2 + G G a2:                       e_v = u v b2 + 2 |G| e_G a2 + 3 u G G a2 + u v' + 2^-125 (G G a2 may underflow)
             den = sqrtf(v') bc2i + eps:               e_den = (sqrt v' - sqrt max(v' - e_v, 0)) bc2i + 2 u sqrt(v') bc2i + u den
             quot = m' / den:                          e_quot = e_m / den + |m'| e_den / den^2 + DIVSQRT_REL |quot| (root, division)
             p' = p decay - ss quot, decay = 1 - lr wd: e_p = |p| u (lr wd + |decay|) + u |p decay| + ss e_quot + 2 u |ss quot| + u |p'|
             The scalar path runs the same expressions, so the same bound holds and two runs agree within twice the bound.
    head     the serial fmaf chain: n u sum |terms|, n = B for dW and D for dx.

Two constants are not derivable here (the installation carries no ULP tables for the HIP math library) and were MEASURED with the
float32 kernel against float64 as RSQRT_MEASURED was, then doubled: EXP_MEASURED and LOG_MEASURED below, with date, sweep and raw
value; test_math_constants_still_hold repeats the measurement.  No other bound is fitted to output; no element is excluded.

Contracts pinned on bits:
  * every shadow element is the STORED float32 p rounded once (to nearest even) to the shadow's type; an f32 shadow equals it.
    Before this file the scalar path did not keep that: the compiler folded the last fma of the update into the f16 conversion
    (v_fma_mixlo_f16), so an f16 shadow written through the scalar loop was the UNSTORED sum rounded once -- the control
    'shadow_pre_rounding'; test_adamw_alignment found it on random data (two elements of the table), the constructed ties find
    it on every element;
  * a tensor with g == NULL keeps the bits of p, m, v and its shadows and adds 0 to the norm; with skip_nonfinite and a non-finite
    norm every buffer keeps its bits; guard elements before and behind every buffer (shadows included) keep theirs;
  * a norm below max_norm leaves the same bits as max_norm = 0;  om_grad_sqnorm gives the same bits twice;
  * om_loss_scale_update: the table LOSS_SCALE_TABLE, written out from the kernel's comment, bit for bit;
  * dW is written, not added: the pre-filled value is gone;  d_q, d_p, loss and the workspace write nothing past their extents;
    with d_q = d_p = NULL the dS region of the workspace keeps its sentinel;
  * om_debug_gemm_last() after a loss call is the family om_debug_gemm_plan gives where the restated condition (uses_gemm) says
    GEMM, and 0 everywhere else.

kernel -> GPU cases
  scores_small_kernel        test_loss_shapes (d % 4 == 0; d = 260, 768: second trip of c += 64), test_loss_score_path_boundary[256x256]
  scores_scalar_kernel       test_loss_d_and_alignment_domain (d in {1, 6, 30, 48}, q or p one float off, d = 48 above the boundary)
  om_gemm_nt branch          test_loss_score_path_boundary[128x516 | 128x515 | 512x132, d 32 | 64]: family v1 (1) observed at 128 rows, v2 (2) at 512,
                             test_loss_d_and_alignment_domain[big-d64-aligned]
  ce_count_kernel            test_loss_targets_and_reductions (Qg = 70, 130: second trip), test_loss_slices_and_outputs
  ce_rows_kernel             every loss case; Pg in {65, 130}: second and third trip; Qg in {1, 3, 5, 70, 130}: the i >= Qg exit
  ce_reduce_kernel           every loss case; Qg in {70, 130}: second trip, all three reductions
  dq_kernel / dp_kernel      every loss case with a gradient; d = 260, 768: second (partial) column block; slices first / middle / last
  grad_sqnorm_kernel         test_grad_sqnorm, test_adamw_* with clipping (vector, scalar, NULL gradient)
  sqnorm_reduce_kernel       test_grad_sqnorm[1025 tensors] (strided loop), [n_chunks 0]
  adamw_kernel               test_adamw_hyper, test_adamw_alignment (scalar path), test_adamw_shadows, test_adamw_nonfinite
  loss_scale_update_kernel   test_loss_scale_update
  small_tn_kernel / small_nn_kernel      test_linear_backward
The path expectations come from uses_gemm, a plain restatement of the entry point's condition, which
test_score_path_table_matches_the_planner checks against om_debug_gemm_plan without a GPU.

The d and alignment domain: on the parent commit d % 4 != 0 and unaligned q / p went to om_gemm_nt at every size and d % 32 != 0
above 65536 scores, and plan_gemm refuses all of those: on the parent test_loss_d_and_alignment_domain fails with the GEMM's text in
nine of its eleven cases.  [d48] passes there too: below the boundary d = 48 is a multiple of 4 and aligned, so it always ran the
wave-per-dot kernel -- the issue's reading that it would fail was wrong for that one case, which stays.

Negative controls (test_bounds_admit_an_emulated_kernel_and_reject_the_controls, CPU: the kernel emulated in float32 in its own
order passes every bound, each control is rejected); worst error / bound, at the shape where it is smallest, recorded 2026-10-19:
CONTROL_RATIOS_RECORDED below.  The GPU cases repeat 'mean_Qg', 'q_row0_ignored' and 'dw_accumulated' on the device's output
(test_controls_on_device_output).
"""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openmatch_amd import native as N
from tests.conftest import REPO
from tests.test_attention_kernels import BF16, BITS_DT, DEV, F16, F32, FLOOR, NAME, TORCH_DT, U_ACC, U_OUT, bits
from tests.test_row_kernels import DIVSQRT_REL, FAKE, GUARD_F, PREFILL, worst

# Relative error of a softmax probability as ce_rows_kernel forms it, expf(t) * (1 / (1 + expf(t))): MEASURED on an MI355X,
# 2026-10-19, rows of Pg = 2, d = 4, q and p multiples of a unit vector (both scores exact, the larger one 0), so
# that d_q[i, 0] is the probability itself (one call, a row per gap, reduction none); 8192 gaps swept over [-80, 0] against float64: largest relative error 1.5485e-7 = 2.60 u (this
# includes the sum, the reciprocal and the product, about 3 u); the constant is twice that.
EXP_MEASURED = 1.55e-7
EXP_REL = 2 * EXP_MEASURED
# Absolute error of the row loss logf(1 + expf(t)) on the same sweep (results in (0, log 2]; includes the exponential and the sum):
# MEASURED the same day, largest absolute error 7.2296e-8 = 1.21 u; doubled.
LOG_MEASURED = 7.23e-8
LOG_ABS = 2 * LOG_MEASURED

u = U_ACC
TINY = 2.0 ** -126
MEAN, SUM, NONE = 0, 1, 2
RED = {MEAN: "mean", SUM: "sum", NONE: "none"}
IGN = -100
CHUNK = N.ADAM_CHUNK
BOUNDARY = 65536
D64 = torch.float64


def f32(x):
    return float(np.float32(x))


def nl(n):
    """additions a term passes through in a wave's strided sum of n terms"""
    return -(-n // 64) + 6


def SS_CHAIN(n_chunks):
    return 74 + 22 + -(-max(n_chunks, 1) // 1024)


def uses_gemm(Qg, Pg, d, q_aligned=True, p_aligned=True):
    """om_contrastive_fwd_bwd_ex restated: the GEMM above 65536 scores where its planner takes the operands (f32: K * 4 a multiple of
    128 bytes, 16-byte aligned rows and pointers); one wave per dot product everywhere else"""
    return Qg * Pg > BOUNDARY and d % 32 == 0 and q_aligned and p_aligned


# ---------------------------------------------------------------------------------------------------------------
# references and bounds (pure torch, in the dtype of their inputs)
# ---------------------------------------------------------------------------------------------------------------
def ce_reference(q, p, target, n_psg, red, row_grad, scale, ctl=None):
    """The loss written out.  ctl (negative controls): 'mean_Qg' divides the gradient by Qg instead of the valid rows, 'target_i'
    takes i instead of i n_psg as the default target, 'no_max' leaves the maximum in the exponentials."""
    Qg, Pg = q.shape[0], p.shape[0]
    S = q @ p.T
    tgt = target if target is not None else torch.arange(Qg) * (1 if ctl == "target_i" else n_psg)
    live = tgt != IGN
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    mx = torch.zeros_like(S[:, :1]) if ctl == "no_max" else S.max(1, keepdim=True).values
    T = S - mx
    E = torch.exp(T)
    sm = E.sum(1, keepdim=True)
    lse = mx + torch.log(sm)
    rl = torch.where(live, (lse - S.gather(1, t[:, None]))[:, 0], torch.zeros_like(lse[:, 0]))
    valid = live.sum().to(S.dtype)
    if red == MEAN:
        loss = rl.sum() / valid * scale
        coef = (scale / (torch.tensor(float(Qg), dtype=S.dtype) if ctl == "mean_Qg" else valid.clamp_min(1.0))).expand(Qg)
    elif red == SUM:
        loss, coef = rl.sum() * scale, torch.full((Qg,), scale, dtype=S.dtype)
    else:
        loss, coef = rl * scale, scale * (row_grad if row_grad is not None else torch.ones(Qg, dtype=S.dtype))
    P = E / sm
    onehot = torch.zeros_like(S)
    onehot[torch.arange(Qg), t] = 1
    dS = (P - onehot) * coef[:, None] * live[:, None].to(S.dtype)
    return NS(S=S, T=T, P=P, sm=sm, lse=lse, rl=rl, loss=loss, coef=coef, dS=dS, dq=dS @ p, dp=dS.T @ q, live=live, t=t, valid=valid,
              onehot=onehot, mag=q.abs() @ p.abs().T)


def ce_bounds(R, q, p, red, scale, row_grad):
    """(e_S, e_loss, e_dq, e_dp) of the float64 reference R; the module docstring has the derivation line by line"""
    Qg, Pg, d = q.shape[0], p.shape[0], q.shape[1]
    live = R.live.to(D64)
    e_S = (d + 8) * u * R.mag
    E_i = e_S.max(1, keepdim=True).values
    r_t = u * R.T.abs() + EXP_REL
    r_sum = (R.P * r_t).sum(1, keepdim=True) + nl(Pg) * u + Pg * TINY
    e_log = LOG_ABS * (torch.log(R.sm).abs() / math.log(2.0)).clamp_min(1.0)
    e_l = (E_i + r_sum + e_log + u * R.lse.abs())[:, 0] + e_S.gather(1, R.t[:, None])[:, 0] + u * R.rl.abs()
    e_l = e_l * live
    if red == NONE:
        e_loss = abs(scale) * e_l + u * R.loss.abs()
    else:
        e_sum = nl(Qg) * u * R.rl.abs().sum() + e_l.sum()
        div = R.valid if red == MEAN else torch.tensor(1.0, dtype=D64)
        e_loss = abs(scale) * e_sum / div + ((DIVSQRT_REL if red == MEAN else 0.0) + u) * R.loss.abs()
    r_P = r_t + r_sum + DIVSQRT_REL + u + e_S + (R.P * e_S).sum(1, keepdim=True)
    e_P = R.P * r_P + TINY
    r_coef = DIVSQRT_REL if red == MEAN else (u if red == NONE and row_grad is not None else 0.0)
    e_dS = ((e_P + u * (R.P - R.onehot).abs()) * R.coef.abs()[:, None] + R.dS.abs() * (r_coef + u)) * live[:, None] + 2.0 ** -149
    e_dq = Pg * u * (R.dS.abs() @ p.abs()) + e_dS @ p.abs()
    e_dp = Qg * u * (R.dS.abs().T @ q.abs()) + e_dS.T @ q.abs()
    return e_S, e_loss, e_dq, e_dp


def adam_hyper(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, step=2, max_norm=0.0, grad_scale=1.0, skip=0, state=None):
    """every figure as the float32 the C ABI receives; state = [scale, 1 / scale, clean steps, skipped] or None"""
    return NS(lr=f32(lr), b1=f32(b1), b2=f32(b2), eps=f32(eps), step=step, max_norm=f32(max_norm), grad_scale=f32(grad_scale), skip=skip,
              state=None if state is None else [f32(s) for s in state])


def adam_scalars(H, ss, r_ss, ctl=None):
    """What every element shares, from the squared norm ss (float; None: no norm given): gs, the clip factor and its relative error,
    the bias corrections.  ctl 'bc_counts_skipped': n = step; 'clip_without_scale': the factor from the norm of the unscaled g."""
    gs, r_gs = H.grad_scale, 0.0
    n = H.step
    if H.state is not None:
        gs, r_gs = gs * H.state[1], u
        if H.state[3] > 0 and ctl != "bc_counts_skipped":
            n = H.step - H.state[3]
    clip, r_clip = 1.0, 0.0
    if ss is not None and H.max_norm > 0:
        nrm = math.sqrt(ss) * (1.0 if ctl == "clip_without_scale" else abs(gs))
        x = H.max_norm / (nrm + 1e-6)
        r_x = r_ss / 2 + r_gs + DIVSQRT_REL + 3 * u
        clip = min(1.0, x)
        r_clip = 0.0 if x * (1 - r_x) >= 1 else r_x * x / clip + u
    return NS(gs=gs * clip, r_gs=r_gs + r_clip, n=n, bc1=1 - H.b1 ** n, bc2=1 - H.b2 ** n, clip=clip)


def adam_written_out(p, g, m, v, wd, H, A, ctl=None):
    """torch.optim.AdamW's single-tensor update as the comment above adamw_kernel has it, in the dtype of p.  ctl 'decay_after':
    the decay multiplies the stepped parameter."""
    dt = p.dtype
    c = lambda x: torch.tensor(x, dtype=D64).to(dt)
    one = c(1.0)
    G = g * c(A.gs)
    decay = one - c(H.lr) * c(f32(wd))
    a1, a2 = one - c(H.b1), one - c(H.b2)
    m1 = m + (G - m) * a1
    v1 = v * c(H.b2) + G * G * a2
    ss = c(f32(H.lr / A.bc1)) if dt == torch.float32 else c(H.lr / A.bc1)
    bc2i = c(f32(1 / math.sqrt(A.bc2))) if dt == torch.float32 else c(1 / math.sqrt(A.bc2))
    den = torch.sqrt(v1) * bc2i + c(H.eps)
    quot = m1 / den
    p1 = (p - ss * quot) * decay if ctl == "decay_after" else p * decay - ss * quot
    return NS(p=p1, m=m1, v=v1, G=G, den=den, quot=quot, ss=float(ss), bc2i=float(bc2i), decay=float(decay), a1=float(a1), a2=float(a2),
              p0=p, m0=m, v0=v)


def adam_bounds(W, wd, H, A):
    """(e_p, e_m, e_v) per element of the float64 update W; the module docstring has the derivation"""
    e_G = W.G.abs() * (A.r_gs + u)
    e_m = W.a1 * e_G + 3 * u * W.a1 * (W.G - W.m0).abs() + u * W.m.abs()
    e_v = u * W.v0 * H.b2 + 2 * W.G.abs() * e_G * W.a2 + 3 * u * W.G * W.G * W.a2 + u * W.v + 2 * TINY
    root = torch.sqrt(W.v)
    e_den = (root - torch.sqrt((W.v - e_v).clamp_min(0.0))) * W.bc2i + 2 * u * root * W.bc2i + u * W.den
    e_quot = e_m / W.den + W.m.abs() * e_den / (W.den * W.den) + DIVSQRT_REL * W.quot.abs()
    lrwd = H.lr * f32(wd)
    e_p = W.p0.abs() * u * (lrwd + abs(W.decay)) + u * (W.p0 * W.decay).abs() + W.ss * e_quot + 2 * u * (W.ss * W.quot).abs() + u * W.p.abs()
    return e_p + 2.0 ** -149, e_m + 2.0 ** -149, e_v + 2.0 ** -149


def adam_torch(tensors, H, A):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False, fused=False) on float64 copies, one step from the given m, v and step.
    tensors: [NS(p, g, m, v (float64; g None: no gradient), wd)] -> [(p, m, v)]"""
    params, groups = [], []
    for t in tensors:
        P = torch.nn.Parameter(t.p.clone())
        if t.g is not None:
            P.grad = t.g * (A.gs / A.clip)                     # grad_scale and the loss scale; the clipping is torch's below
        params.append(P)
        groups.append(dict(params=[P], weight_decay=f32(t.wd)))
    opt = torch.optim.AdamW(groups, lr=H.lr, betas=(H.b1, H.b2), eps=H.eps, foreach=False, fused=False)
    for t, P in zip(tensors, params):
        opt.state[P] = dict(step=torch.tensor(float(A.n - 1)), exp_avg=t.m.clone(), exp_avg_sq=t.v.clone())
    if H.max_norm > 0:
        torch.nn.utils.clip_grad_norm_([P for P in params if P.grad is not None], H.max_norm, foreach=False)
    opt.step()
    return [(P.detach(), opt.state[P]["exp_avg"], opt.state[P]["exp_avg_sq"]) for P in params]


def round_to(x64, dtype):
    """one rounding to nearest even of float64 values to f32 / bf16 / f16 (normal range; torch's .to(bfloat16) of a double goes
    through float32 and rounds twice, which is what the shadow control is about)"""
    if dtype == F32:
        return x64.to(torch.float32)
    bits_kept = 8 if dtype == BF16 else 11
    x = x64.numpy()
    e = np.floor(np.log2(np.abs(np.where(x == 0, 1.0, x))))
    scale = np.exp2(e - (bits_kept - 1))
    return torch.from_numpy(np.round(x / scale) * scale).to(TORCH_DT[dtype])


def linear_bwd_reference(dy, x, w):
    return dy.T @ x, dy @ w


def linear_bwd_bounds(dy, x, w):
    B, D = dy.shape
    return B * u * (dy.abs().T @ x.abs()) + 2.0 ** -149, D * u * (dy.abs() @ w.abs()) + 2.0 ** -149


# ---------------------------------------------------------------------------------------------------------------
# the kernels emulated in float32, in their own order
# ---------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 tensors: the product is exact in float64, one rounding of the sum"""
    return (a.double() * b.double() + c.double()).float()


def wave_tree(v, op):
    """wave_sum / wave_max: v [..., 64] -> [...], the xor butterfly 32, 16, .., 1"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., idx ^ o])
    return v[..., 0]


def lane_reduce(x, op, ident):
    """for (j = lane; j < n; j += 64) acc = op(acc, x[j]); then the tree.  x [..., n]"""
    n = x.shape[-1]
    trips = -(-n // 64)
    x = torch.cat([x, torch.full(x.shape[:-1] + (trips * 64 - n,), ident, dtype=x.dtype)], -1).view(*x.shape[:-1], trips, 64)
    acc = torch.full(x.shape[:-2] + (64,), ident, dtype=x.dtype)
    for t in range(trips):
        acc = op(acc, x[..., t, :])
    return wave_tree(acc, op)


def emu_scores(q, p, vec):
    """scores_small_kernel (vec: float4 c = lane, lane + 64, ..) or scores_scalar_kernel (c = lane, lane + 64, ..)"""
    d = q.shape[1]
    e = torch.arange(d)
    lane, pos = ((e // 4) % 64, (e // 256) * 4 + e % 4) if vec else (e % 64, e // 64)
    steps = int(pos.max()) + 1
    qz, pz = torch.cat([q, torch.zeros_like(q[:, :1])], 1), torch.cat([p, torch.zeros_like(p[:, :1])], 1)
    acc = torch.zeros(q.shape[0], p.shape[0], 64)
    for s in range(steps):
        idx = torch.full((64,), d, dtype=torch.long)
        sel = pos == s
        idx[lane[sel]] = e[sel]
        acc = fma32(qz[:, idx][:, None, :], pz[:, idx][None, :, :], acc)
    return wave_tree(acc, torch.add)


def emu_loss(q, p, target, n_psg, red, row_grad, scale, q0, qr, p0, pr, ctl=None):
    """the whole entry point in float32: scores, ce_count, ce_rows, ce_reduce, dq, dp.  ctl: the controls of ce_reference plus
    'q_row0_ignored' / 'p_row0_ignored' (the slice starts at row 0)."""
    Qg, Pg, d = q.shape[0], p.shape[0], q.shape[1]
    S = emu_scores(q, p, d % 4 == 0)
    tgt = target if target is not None else torch.arange(Qg) * (1 if ctl == "target_i" else n_psg)
    live = tgt != IGN
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    valid = lane_reduce(live.float(), torch.add, 0.0) if target is not None else torch.tensor(float(Qg))
    mx = torch.zeros(Qg) if ctl == "no_max" else lane_reduce(S, torch.maximum, -math.inf)
    E = torch.exp(S - mx[:, None])
    sm = lane_reduce(E, torch.add, 0.0)
    lse = mx + torch.log(sm)
    rl = torch.where(live, lse - S.gather(1, t[:, None])[:, 0], torch.zeros(Qg))
    sc = torch.tensor(scale, dtype=torch.float32)
    if red == NONE:
        loss = rl * sc
        coef = sc * row_grad if row_grad is not None else sc.expand(Qg)
    else:
        acc = lane_reduce(rl, torch.add, 0.0)
        loss = acc / valid * sc if red == MEAN else acc * sc
        coef = (sc / (torch.tensor(float(Qg)) if ctl == "mean_Qg" else valid.clamp_min(1.0)) if red == MEAN else sc).expand(Qg)
    inv = 1.0 / sm
    onehot = torch.zeros_like(S)
    onehot[torch.arange(Qg), t] = 1
    dS = (E * inv[:, None] - onehot) * coef[:, None]
    dS = torch.where(live[:, None], dS, torch.zeros_like(dS))
    qa = 0 if ctl == "q_row0_ignored" else q0
    pa = 0 if ctl == "p_row0_ignored" else p0
    dq = torch.zeros(qr, d)
    for j in range(Pg):
        dq = fma32(dS[qa:qa + qr, j][:, None], p[j][None, :], dq)
    dp = torch.zeros(pr, d)
    for i in range(Qg):
        dp = fma32(dS[i, pa:pa + pr][:, None], q[i][None, :], dp)
    return NS(S=S, loss=loss, dq=dq, dp=dp)


def emu_sqnorm(gs, vec=True):
    """grad_sqnorm_kernel + sqnorm_reduce_kernel on a list of float32 gradients (None: absent), chunk by chunk in table order"""
    partial = []
    for g in gs:
        n = 0 if g is None else g.numel()
        for base in range(0, max(n, 1), CHUNK):
            if g is None:
                partial.append(torch.tensor(0.0))
                continue
            x = g[base:base + CHUNK]
            n4 = x.numel() // 4 if vec else 0
            acc = torch.zeros(256)
            if n4:
                y = torch.cat([x[:n4 * 4].view(n4, 4), torch.zeros(-n4 % 256, 4)]).view(-1, 256, 4)
                for it in range(y.shape[0]):
                    sq = y[it] * y[it]
                    acc = acc + (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3])
            tail = x[n4 * 4:]
            tail = torch.cat([tail, torch.zeros(-tail.numel() % 256)]).view(-1, 256)
            for it in range(tail.shape[0]):
                acc = acc + tail[it] * tail[it]
            w = wave_tree(acc.view(4, 64), torch.add)
            partial.append(((w[0] + w[1]) + w[2]) + w[3])
    part = torch.stack(partial) if partial else torch.zeros(0)
    y = torch.cat([part, torch.zeros(-part.numel() % 1024)]).view(-1, 1024)
    acc = torch.zeros(1024)
    for it in range(y.shape[0]):
        acc = acc + y[it]
    w = wave_tree(acc.view(16, 64), torch.add)
    tot = torch.tensor(0.0)
    for i in range(16):
        tot = tot + w[i]
    return tot


def emu_linear_bwd(dy, x, w, dw0=None):
    """small_tn_kernel / small_nn_kernel: serial fmaf chains.  dw0: a wrong kernel that adds into what dW holds (control)."""
    B, D = dy.shape
    dw = torch.zeros(D, x.shape[1]) if dw0 is None else dw0.clone()
    for i in range(B):
        dw = fma32(dy[i][:, None], x[i][None, :], dw)
    dx = torch.zeros(B, w.shape[1])
    for j in range(D):
        dx = fma32(dy[:, j][:, None], w[j][None, :], dx)
    return dw, dx


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def loss_inputs(Qg, Pg, d, seed=0, qscale=1.0):
    """rows of norm about 1.5 (scores of a few units: a softmax that is neither flat nor one-hot), scaled by qscale"""
    gen = torch.Generator().manual_seed(1000 * Qg + 10 * Pg + d + seed)
    q = torch.randn(Qg, d, generator=gen) * (1.5 / math.sqrt(d)) * qscale
    p = torch.randn(Pg, d, generator=gen) * (1.5 / math.sqrt(d))
    return q, p


ADAM_SIZES = [1, 3, 4, 5, 1023, 16383, 16384, 16385, 2 * 16384 + 7]
SHADOW_SETS = {"none": (), "bf16": (BF16,), "f16": (F16,), "f32": (F32,), "bf16+f16": (BF16, F16)}
WDS = [0.0, 0.01, 0.5]


def adam_inputs(sizes, seed=0, null_at=None, sweep=True, zeros=True):
    """[NS(p, g, m, v float32 (g None at null_at), wd)]: gradients swept over 2^-60 .. 2^20 with exact zeros, m and v non-zero"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k, n in enumerate(sizes):
        p = torch.randn(n, generator=gen)
        g = torch.randn(n, generator=gen)
        if sweep:
            g = g * torch.exp2(torch.randint(-60, 21, (n,), generator=gen).float())
        if zeros:
            g[torch.rand(n, generator=gen) < 0.1] = 0.0
        m = 0.1 * torch.randn(n, generator=gen) * g.abs().clamp(2.0 ** -40, 2.0 ** 10)
        v = (0.3 * torch.randn(n, generator=gen) * g.abs().clamp(2.0 ** -40, 2.0 ** 10)) ** 2
        out.append(NS(p=p, g=None if k == null_at else g, m=m, v=v, wd=WDS[k % 3]))
    return out


def adam_reference(tens, H, ss, n_chunks, ctl=None):
    """The float64 reference of one step and its bounds: torch's AdamW, with the written-out form (which the bounds are built from)
    held to it.  ss: the squared norm the kernel is given (the device's own, float), or None.  -> [NS(p, m, v, e_p, e_m, e_v)]"""
    r_ss = SS_CHAIN(n_chunks) * u
    if ss is not None:                                          # a norm is given: the reference takes the exact one, r_ss bounds the kernel's
        ss = float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None))
    A = adam_scalars(H, ss, r_ss, ctl)
    d = lambda t: None if t is None else t.double()
    T64 = [NS(p=d(t.p), g=d(t.g), m=d(t.m), v=d(t.v), wd=t.wd) for t in tens]
    tor = adam_torch(T64, H, A) if ctl is None else None
    out = []
    for k, t in enumerate(T64):
        if t.g is None:
            out.append(None)
            continue
        W = adam_written_out(t.p, t.g, t.m, t.v, t.wd, H, A, "decay_after" if ctl == "decay_after" else None)
        if tor is not None:
            # float64 against float64: a few roundings of 2^-53 relative to the operands of each expression, far below u
            mags = (W.p0.abs() + (W.ss * W.quot).abs(), W.m0.abs() + W.G.abs(), W.v)
            for a, b, mag in zip((W.p, W.m, W.v), tor[k], mags):
                fin = torch.isfinite(b)
                assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(((a - b).abs()[fin] <= 1e-13 * mag[fin]).all())
        e_p, e_m, e_v = adam_bounds(W, t.wd, H, A)
        out.append(NS(p=W.p, m=W.m, v=W.v, e_p=e_p, e_m=e_m, e_v=e_v))
    return out


def emu_adam(tens, H, vec=True):
    """adamw_kernel in float32 (the squared norm from emu_sqnorm when the step clips) -> [NS(p, m, v)], and the float norm"""
    f = np.float32
    gs, n, ss = f(H.grad_scale), H.step, None
    if H.state is not None:
        gs = gs * f(H.state[1])
        if H.state[3] > 0:
            n = H.step - H.state[3]
    if H.max_norm > 0:
        ss = float(emu_sqnorm([t.g for t in tens], vec))
        gs = gs * min(f(1.0), f(H.max_norm) / (np.sqrt(f(ss)) * abs(gs) + f(1e-6)))
    A = NS(gs=float(gs), n=n, bc1=1 - H.b1 ** n, bc2=1 - H.b2 ** n)
    out = []
    for t in tens:
        out.append(None if t.g is None else adam_written_out(t.p, t.g, t.m, t.v, t.wd, H, A))
    return out, ss


def close(got, ref, bound):
    """worst(), with non-finite reference elements compared by kind (NaN where the reference has NaN, the same infinity)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    fin = torch.isfinite(ref)
    if not torch.equal(torch.isnan(got), torch.isnan(ref)) or not torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)]):
        return math.inf
    b = torch.as_tensor(bound, dtype=D64).expand_as(ref)
    return worst(got[fin], ref[fin], b[fin])


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_references_are_torchs():
    """the written-out loss and its gradients are F.cross_entropy and its autograd; the written-out AdamW is torch's (adam_reference
    asserts that on every call, here over the hyper-parameter table); the head's backward is the autograd of x W^T"""
    gen = torch.Generator().manual_seed(0)
    for Qg, Pg, n_psg, red, tkind in ((5, 12, 2, MEAN, None), (6, 7, 1, SUM, "some"), (4, 9, 1, NONE, "some"), (3, 5, 1, MEAN, "all"),
                                      (3, 5, 1, SUM, "all"), (7, 7, 1, NONE, None)):
        q = torch.randn(Qg, 6, generator=gen, dtype=D64).requires_grad_()
        p = torch.randn(Pg, 6, generator=gen, dtype=D64).requires_grad_()
        target = None
        if tkind:
            target = torch.randint(0, Pg, (Qg,), generator=gen)
            target[::2 if tkind == "some" else 1] = IGN
        rg = torch.randn(Qg, generator=gen, dtype=D64) if red == NONE else None
        tt = target if target is not None else torch.arange(Qg) * n_psg
        loss = F.cross_entropy(q @ p.T, tt, reduction=RED[red], ignore_index=IGN) * 0.125
        (loss * rg).sum().backward() if red == NONE else loss.backward()
        R = ce_reference(q.detach(), p.detach(), target, n_psg, red, rg, 0.125)
        assert torch.equal(torch.isnan(R.loss), torch.isnan(loss.detach()))
        if tkind != "all" or red != MEAN:
            assert torch.allclose(R.loss, loss.detach(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(R.dq, q.grad, rtol=1e-11, atol=1e-14) and torch.allclose(R.dp, p.grad, rtol=1e-11, atol=1e-14)
    for H in HYPERS.values():
        tens = adam_inputs([5, 33, 7], seed=3, null_at=1)
        ss = float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None))
        adam_reference(tens, H, ss if H.max_norm > 0 else None, 3)
    dy, x, w = (torch.randn(s, generator=gen, dtype=D64) for s in ((5, 3), (5, 7), (3, 7)))
    x.requires_grad_(), w.requires_grad_()
    ((x @ w.T) * dy).sum().backward()
    dw, dx = linear_bwd_reference(dy, x.detach(), w.detach())
    assert torch.allclose(dw, w.grad, rtol=1e-12) and torch.allclose(dx, x.grad, rtol=1e-12)


HYPERS = {
    "plain": adam_hyper(),
    "beta1_0": adam_hyper(b1=0.0, step=1),
    "beta2_0": adam_hyper(b2=0.0, step=100000, eps=1e-3),
    "step1_eps1e-3": adam_hyper(step=1, eps=1e-3),
    "step100000": adam_hyper(step=100000),
    "clip_above": adam_hyper(max_norm=1.0),
    "clip_scaled": adam_hyper(max_norm=1.0, grad_scale=1.0 / 1024),
    "clip_negative_scale": adam_hyper(max_norm=0.5, grad_scale=-1.0, step=100000),
    "scale_only": adam_hyper(grad_scale=1.0 / 1024),
    "state_skipped0": adam_hyper(step=2, max_norm=1.0, skip=1, state=[1024.0, 1.0 / 1024, 5.0, 0.0]),
    "state_skipped3": adam_hyper(step=5, max_norm=1.0, skip=1, state=[1000.0, 1.0 / 1000, 0.0, 3.0]),
    "state_skipped3_noclip": adam_hyper(step=5, state=[1024.0, 1.0 / 1024, 0.0, 3.0]),
}
CONTROL_RATIOS = {}
# worst error / bound of each control, recorded 2026-10-19 from test_bounds_admit_an_emulated_kernel_and_reject_the_controls (its
# printed 'control ratios'), each at the case of its loop where it was smallest
CONTROL_RATIOS_RECORDED = {"mean_Qg": 4.55e4, "target_i": 5.66e5, "no_max": math.inf, "q_row0_ignored": 8.54e4, "p_row0_ignored": 2.73e5,
                           "decay_after": 5.52e2, "bc_counts_skipped": 2.86e5, "clip_without_scale": 2.62e3, "dw_accumulated": 3.19e3,
                           "shadow_pre_rounding": "a bit comparison: every constructed element differs"}


def test_bounds_admit_an_emulated_kernel_and_reject_the_controls():
    # ---- loss
    cases = [dict(Qg=5, Pg=12, d=64, n_psg=2), dict(Qg=70, Pg=130, d=260, n_psg=1, red=MEAN, ignore=True, q0=3, qr=9, p0=64, pr=66),
             dict(Qg=9, Pg=65, d=6, n_psg=4, red=NONE, rg=True, q0=2, qr=7, p0=1, pr=3), dict(Qg=4, Pg=8, d=30, n_psg=2, red=SUM, scale=8.0, q0=1, qr=2, p0=5, pr=3),
             dict(Qg=3, Pg=5, d=4, n_psg=1, red=MEAN, ignore=True, q0=1, qr=2, p0=1, pr=4)]
    for c in cases:
        Qg, Pg, d, n_psg, red, scale = c["Qg"], c["Pg"], c["d"], c["n_psg"], c.get("red", MEAN), c.get("scale", 0.125)
        q0, qr, p0, pr = c.get("q0", 0), c.get("qr", Qg), c.get("p0", 0), c.get("pr", Pg)
        q, p = loss_inputs(Qg, Pg, d)
        gen = torch.Generator().manual_seed(Qg)
        target = None
        if c.get("ignore"):
            target = torch.randint(0, Pg, (Qg,), generator=gen)
            target[1::3] = IGN
        rg = torch.randn(Qg, generator=gen) if c.get("rg") else None
        rg64 = None if rg is None else rg.double()
        R = ce_reference(q.double(), p.double(), target, n_psg, red, rg64, scale)
        e_S, e_loss, e_dq, e_dp = ce_bounds(R, q.double(), p.double(), red, scale, rg64)
        E = emu_loss(q, p, target, n_psg, red, rg, scale, q0, qr, p0, pr)
        sl = lambda X: (X.dq[q0:q0 + qr], X.dp[p0:p0 + pr])
        assert close(E.S, R.S, e_S) <= 1 and close(E.loss, R.loss, e_loss) <= 1
        assert close(E.dq, sl(R)[0], e_dq[q0:q0 + qr]) <= 1 and close(E.dp, sl(R)[1], e_dp[p0:p0 + pr]) <= 1
        ctls = []
        if red == MEAN and target is not None:
            ctls.append("mean_Qg")
        if target is None and n_psg > 1:
            ctls.append("target_i")
        if q0:
            ctls.append("q_row0_ignored")
        if p0:
            ctls.append("p_row0_ignored")
        for ctl in ctls:
            X = emu_loss(q, p, target, n_psg, red, rg, scale, q0, qr, p0, pr, ctl=ctl)
            w_dq, w_dp = close(X.dq, sl(R)[0], e_dq[q0:q0 + qr]), close(X.dp, sl(R)[1], e_dp[p0:p0 + pr])
            w = w_dq if ctl == "q_row0_ignored" else w_dp if ctl == "p_row0_ignored" else max(w_dq, w_dp)
            assert w > 1.0, (ctl, c, w)
            CONTROL_RATIOS[ctl] = min(w, CONTROL_RATIOS.get(ctl, math.inf))
    # scores of magnitude 100: without the maximum expf overflows
    q, p = loss_inputs(5, 12, 64, qscale=200.0)
    R = ce_reference(q.double(), p.double(), None, 2, MEAN, None, 1.0)
    assert float(R.S.abs().max()) > 100
    e_S, e_loss, e_dq, e_dp = ce_bounds(R, q.double(), p.double(), MEAN, 1.0, None)
    E = emu_loss(q, p, None, 2, MEAN, None, 1.0, 0, 5, 0, 12)
    assert close(E.loss, R.loss, e_loss) <= 1 and close(E.dq, R.dq, e_dq) <= 1 and close(E.dp, R.dp, e_dp) <= 1
    X = emu_loss(q, p, None, 2, MEAN, None, 1.0, 0, 5, 0, 12, ctl="no_max")
    w = max(close(X.loss, R.loss, e_loss), close(X.dq, R.dq, e_dq))
    assert w > 1.0
    CONTROL_RATIOS["no_max"] = w
    # ---- optimizer: the emulation (vector and scalar order of the norm) passes at every hyper-parameter set
    for name, H in HYPERS.items():
        tens = adam_inputs([5, 1023, 16385, 3], seed=5, null_at=2 if name == "plain" else None)
        for vec in (True, False):
            E, ss = emu_adam(tens, H, vec)
            ref = adam_reference(tens, H, ss, 5)
            if ss is not None:
                exact = float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None))
                assert abs(ss - exact) <= SS_CHAIN(5) * u * exact
            for e, r in zip(E, ref):
                if r is not None:
                    assert close(e.p, r.p, r.e_p) <= 1 and close(e.m, r.m, r.e_m) <= 1 and close(e.v, r.v, r.e_v) <= 1, name
    # the controls, each at hyper-parameters where it changes the update
    tens = adam_inputs([5, 1023, 3], seed=6, sweep=False)
    for ctl, H in (("decay_after", HYPERS["plain"]), ("bc_counts_skipped", HYPERS["state_skipped3"]), ("bc_counts_skipped", HYPERS["state_skipped3_noclip"]),
                   ("clip_without_scale", HYPERS["clip_scaled"]), ("clip_without_scale", HYPERS["state_skipped0"])):
        E, ss = emu_adam(tens, H)
        good = adam_reference(tens, H, ss, 3)
        bad = adam_reference(tens, H, ss, 3, ctl=ctl)
        w = max(close(e.p, b.p, r.e_p) for e, b, r in zip(E, bad, good) if r is not None)
        assert w > 1.0, (ctl, w)
        CONTROL_RATIOS[ctl] = min(w, CONTROL_RATIOS.get(ctl, math.inf))
    # a shadow rounded from the value before its float32 store: differs exactly where the store lands on a tie of the shadow's type
    for dtype in (BF16, F16):
        p, decay = shadow_tie_inputs(dtype)
        pre = p.double() * decay
        stored = pre.float()
        right, wrong = stored.to(TORCH_DT[dtype]), round_to(pre, dtype)
        assert torch.equal(right, round_to(stored.double(), dtype))
        assert bool((bits(right, dtype) != bits(wrong, dtype)).all()) and p.numel() >= 8
    CONTROL_RATIOS["shadow_pre_rounding"] = "bits differ on every constructed element"
    # ---- head backward
    for B, D, K in ((1, 1, 1), (5, 257, 33), (64, 255, 257)):
        gen = torch.Generator().manual_seed(B)
        dy, x, w = torch.randn(B, D, generator=gen), torch.randn(B, K, generator=gen), torch.randn(D, K, generator=gen)
        rw, rx = linear_bwd_reference(dy.double(), x.double(), w.double())
        bw, bx = linear_bwd_bounds(dy.double(), x.double(), w.double())
        dw, dx = emu_linear_bwd(dy, x, w)
        assert close(dw, rw, bw) <= 1 and close(dx, rx, bx) <= 1
        wrong, _ = emu_linear_bwd(dy, x, w, dw0=torch.full((D, K), PREFILL))
        w_ = close(wrong, rw, bw)
        assert w_ > 1.0
        CONTROL_RATIOS["dw_accumulated"] = min(w_, CONTROL_RATIOS.get("dw_accumulated", math.inf))
    print("control ratios:", {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in CONTROL_RATIOS.items()})


def shadow_tie_inputs(dtype):
    """p in [1, 2) and decay = 1 - 2^-12 (lr 2^-11, weight decay 0.5, g = m = v = 0: p' = p decay exactly) chosen so that the exact
    product lies just above a tie of the 16-bit type and its float32 rounding lands ON the tie: rounding the stored value goes to
    even (down), rounding the unstored value goes up."""
    decay = 1.0 - 2.0 ** -12
    keep = 8 if dtype == BF16 else 11
    p = (1.0 + torch.arange(2 ** 23, dtype=D64) * 2.0 ** -23)
    pre = p * decay
    stored = pre.float().double()
    step = 2.0 ** -(keep - 1)                                      # spacing of the 16-bit type in [1, 2)
    frac = stored / step - torch.floor(stored / step)
    even = torch.floor(stored / step) % 2 == 0
    sel = (frac == 0.5) & even & (pre > stored) & (stored >= 1.0) & (stored < 2.0 - step)
    return p[sel][:64].float(), decay


def test_score_path_table_matches_the_planner():
    """uses_gemm against om_debug_gemm_plan (no GPU: made-up addresses): where the restated condition says GEMM the planner names a
    family, where it says no because of d or alignment the planner refuses, and the GPU cases' expectations are what it gives"""
    lib = N.lib()
    plan = lambda Qg, Pg, d, qo=0, po=0: lib.om_debug_gemm_plan(F32, C.c_void_p(FAKE + 4 * qo), d, C.c_void_p(FAKE + (1 << 24) + 4 * po), d, F32,
                                                                 C.c_void_p(FAKE + (2 << 24)), Pg, Qg, Pg, d, None, None, 0, 0)
    for Qg, Pg in ((256, 256), (128, 516), (128, 515), (512, 132), (256, 2048), (257, 256)):
        for d in (1, 4, 6, 30, 32, 48, 64, 252, 260, 768):
            for qo, po in ((0, 0), (1, 0), (0, 1)):
                fam = plan(Qg, Pg, d, qo, po)
                assert (fam > 0) == (d % 32 == 0 and qo == 0 and po == 0), (Qg, Pg, d, qo, po, fam)
                assert uses_gemm(Qg, Pg, d, qo == 0, po == 0) == (Qg * Pg > BOUNDARY and fam > 0)
    for (Qg, Pg, d), want in BOUNDARY_CASES.items():
        assert uses_gemm(Qg, Pg, d) == want
    assert not uses_gemm(256, 256, 32) and uses_gemm(128, 516, 32) and not uses_gemm(128, 516, 48) and not uses_gemm(128, 516, 64, p_aligned=False)


def test_docstring_table_lists_every_kernel():
    """every __global__ of contrastive.hip and optim.hip, and the two small contractions, is named in the 'kernel -> GPU cases' table"""
    table = __doc__.split("kernel -> GPU cases")[1].split("Negative controls")[0]
    names = ["small_tn_kernel", "small_nn_kernel"]
    for src in ("contrastive.hip", "optim.hip"):
        text = open(os.path.join(REPO, "openmatch_amd", "csrc", src)).read()
        found = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", text)
        assert len(found) >= 4, src
        names += found
    assert len(names) == 2 + 7 + 4 and all(n in table for n in names), [n for n in names if n not in table]


BOUNDARY_CASES = {(256, 256, 32): False, (128, 516, 32): True, (128, 516, 64): True, (128, 515, 32): True, (128, 515, 64): True,
                  (512, 132, 32): True, (512, 132, 64): True}


def test_refusals():
    """every refusal before any launch (made-up addresses)"""
    lib = N.lib()
    p, z = C.c_void_p(FAKE), C.c_void_p(0)
    err = lambda: lib.om_last_error()
    # the loss: a default target that does not exist ((Qg - 1) n_psg == Pg), a reduction, a slice, null outputs, an empty batch
    ce = lambda Qg, Pg, d, n_psg=1, red=MEAN, q0=0, qr=0, p0=0, pr=0, loss=p, ws=p: lib.om_contrastive_fwd_bwd_ex(
        p, p, Qg, Pg, d, z, n_psg, red, z, 1.0, q0, qr, p0, pr, loss, z, z, z, ws, z)
    assert ce(5, 8, 4, n_psg=2) != 0 and b"target index out of range" in err()
    assert lib.om_contrastive_fwd_bwd(p, p, 3, 4, 4, 2, 1.0, 0, 0, 0, 0, p, z, z, z, p, z) != 0 and b"target index out of range" in err()
    assert ce(4, 8, 4, red=3) != 0 and b"reduction" in err()
    assert ce(4, 8, 4, q0=3, qr=2) != 0 and b"slice" in err() and ce(4, 8, 4, p0=-1, pr=2) != 0 and b"slice" in err()
    assert ce(4, 8, 4, loss=z) != 0 and b"null" in err() and ce(4, 8, 4, ws=z) != 0 and b"null" in err()
    assert ce(0, 8, 4) != 0 and ce(4, 0, 4) != 0 and ce(4, 8, 0) != 0 and b"empty" in err()
    # the optimizer
    st = lambda **k: lib.om_adamw_step(k.get("tab", p), k.get("ch", p), k.get("n", 1), 0.01, k.get("b1", 0.9), k.get("b2", 0.999), 1e-8, k.get("step", 1),
                                       k.get("norm", z), k.get("max_norm", 0.0), 1.0, 0, z, z)
    assert st(step=0) != 0 and b"step counts from 1" in err()
    for k in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-1e-3), dict(b1=float("nan"))):
        assert st(**k) != 0 and b"betas" in err()
    assert st(max_norm=1.0) != 0 and b"clipping needs" in err()
    assert st(tab=z) != 0 and b"null" in err() and st(ch=z) != 0 and b"null" in err() and st(n=-1) != 0
    assert st(n=0, tab=z, ch=z) == 0                                                 # nothing to do, nothing launched
    assert lib.om_grad_sqnorm(z, p, 1, p, p, z) != 0 and b"null" in err() and lib.om_grad_sqnorm(p, z, 1, p, p, z) != 0
    assert lib.om_grad_sqnorm(p, p, 1, z, p, z) != 0 and lib.om_grad_sqnorm(p, p, 1, p, z, z) != 0 and lib.om_grad_sqnorm(z, z, 0, z, z, z) != 0
    assert lib.om_loss_scale_update(p, p, 0, z) != 0 and b"bad argument" in err()
    assert lib.om_loss_scale_update(z, p, 1, z) != 0 and lib.om_loss_scale_update(p, z, 1, z) != 0
    assert lib.om_linear_f32_backward(z, p, p, p, p, 1, 1, 1, z) != 0 and b"null" in err()
    assert lib.om_linear_f32_backward(p, p, p, p, p, 0, 1, 1, z) == 0
    assert C.sizeof(N.OmAdamTensor) == 72


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
GUARD_N = 8


def guarded(n, fill=GUARD_F, off=0, dtype=torch.float32):
    """(buffer, view of n elements 16-byte aligned + off elements) with guard elements before and behind"""
    lead = 16 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((lead + off + n + GUARD_N,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead + off:lead + off + n]


def guards_intact(buf, view, fill=GUARD_F):
    start = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    ref = torch.full_like(buf, fill)
    ib = lambda t: t.view(torch.int32 if t.element_size() == 4 else torch.int16)
    return torch.equal(ib(buf[:start]), ib(ref[:start])) and torch.equal(ib(buf[start + view.numel():]), ib(ref[start + view.numel():]))


def ce_call(q, p, target=None, n_psg=1, red=MEAN, row_grad=None, scale=1.0, q0=0, qr=None, p0=0, pr=None, want_dq=True, want_dp=True,
            want_scores=True, q_off=0, p_off=0, legacy=False):
    """One call of om_contrastive_fwd_bwd_ex on guarded buffers -> NS(loss, S, dq, dp, dS region, family, guards intact)"""
    lib = N.lib()
    Qg, d = q.shape
    Pg = p.shape[0]
    qr = Qg - q0 if qr is None else qr
    pr = Pg - p0 if pr is None else pr
    qb, qv = guarded(Qg * d, off=q_off)
    pb, pv = guarded(Pg * d, off=p_off)
    qv.copy_(q.flatten()), pv.copy_(p.flatten())
    n_loss = Qg if red == NONE else 1
    lb, lv = guarded(n_loss)
    sb, sv = guarded(Qg * Pg)
    dqb, dqv = guarded(qr * d)
    dpb, dpv = guarded(pr * d)
    n_ws = 2 * Qg * Pg + Qg + 1
    wb, wv = guarded(n_ws)
    tg = None if target is None else target.to(DEV)
    rg = None if row_grad is None else row_grad.to(DEV)
    args = (N.ptr(lv), N.ptr(sv) if want_scores else None, N.ptr(dqv) if want_dq else None, N.ptr(dpv) if want_dp else None, N.ptr(wv), N.stream_ptr())
    if legacy:
        rc = lib.om_contrastive_fwd_bwd(N.ptr(qv), N.ptr(pv), Qg, Pg, d, n_psg, scale, q0, qr, p0, pr, *args)
    else:
        rc = lib.om_contrastive_fwd_bwd_ex(N.ptr(qv), N.ptr(pv), Qg, Pg, d, N.ptr(tg), n_psg, red, N.ptr(rg), scale, q0, qr, p0, pr, *args)
    fam = lib.om_debug_gemm_last()
    if rc != 0:
        raise N.NativeError(lib.om_last_error().decode())
    torch.cuda.synchronize()
    plan = lib.om_debug_gemm_plan(F32, N.ptr(qv), d, N.ptr(pv), d, F32, N.ptr(sv if want_scores else wv), Pg, Qg, Pg, d, None, None, 0, 0)
    ok = all(guards_intact(b, v) for b, v in ((lb, lv), (sb, sv), (dqb, dqv), (dpb, dpv), (wb, wv), (qb, qv), (pb, pv)))
    S = (sv if want_scores else wv[:Qg * Pg]).view(Qg, Pg).cpu()
    ds0 = 0 if want_scores else Qg * Pg
    untouched = lambda v: bool((v == GUARD_F).all())
    return NS(loss=(lv if red == NONE else lv[0]).cpu(), S=S, dq=dqv.view(qr, d).cpu(), dp=dpv.view(pr, d).cpu(), fam=fam, plan=plan, guards=ok,
              dS_kept=untouched(wv[ds0:ds0 + Qg * Pg]), scores_kept=untouched(sv), dq_kept=untouched(dqv), dp_kept=untouched(dpv),
              ws_tail_kept=untouched(wv[ds0 + Qg * Pg + Qg + (1 if target is not None else 0):]) if want_scores else None)


def ce_check(q, p, target=None, n_psg=1, red=MEAN, row_grad=None, scale=1.0, q0=0, qr=None, p0=0, pr=None, want_dq=True, want_dp=True,
             want_scores=True, q_off=0, p_off=0, legacy=False, tag=""):
    """the call, the float64 reference, every comparison and the path"""
    Qg, d = q.shape
    Pg = p.shape[0]
    qr = Qg - q0 if qr is None else qr
    pr = Pg - p0 if pr is None else pr
    G = ce_call(q, p, target, n_psg, red, row_grad, scale, q0, qr, p0, pr, want_dq, want_dp, want_scores, q_off, p_off, legacy)
    rg64 = None if row_grad is None else row_grad.double()
    R = ce_reference(q.double(), p.double(), target, n_psg, red, rg64, f32(scale))
    e_S, e_loss, e_dq, e_dp = ce_bounds(R, q.double(), p.double(), red, f32(scale), rg64)
    w = NS(S=close(G.S, R.S, e_S), loss=close(G.loss, R.loss, e_loss),
           dq=close(G.dq, R.dq[q0:q0 + qr], e_dq[q0:q0 + qr]) if want_dq else 0.0, dp=close(G.dp, R.dp[p0:p0 + pr], e_dp[p0:p0 + pr]) if want_dp else 0.0)
    print(f"{tag} Qg {Qg} Pg {Pg} d {d} n_psg {n_psg} {RED[red]}: error / bound S {w.S:.3f} loss {w.loss:.3f} dq {w.dq:.3f} dp {w.dp:.3f} family {G.fam}")
    assert w.S <= 1 and w.loss <= 1 and w.dq <= 1 and w.dp <= 1, (tag, vars(w))
    assert G.guards, "a guard float changed"
    if not want_dq:
        assert G.dq_kept
    if not want_dp:
        assert G.dp_kept
    if not want_dq and not want_dp:
        assert G.dS_kept, "forward only: the dS region of the workspace is not written"
    if not want_scores:
        assert G.scores_kept
    else:
        assert G.ws_tail_kept, "the workspace behind dS | row_loss | valid is not written"
    want_gemm = uses_gemm(Qg, Pg, d, q_off == 0, p_off == 0)
    assert (G.fam == G.plan and G.fam > 0) if want_gemm else G.fam == 0, (tag, G.fam, G.plan, want_gemm)
    G.R, G.bounds = R, (e_S, e_loss, e_dq, e_dp)
    return G


def measure_loss_constants():
    """(largest relative error of a probability, largest absolute error of a row loss) on the sweep EXP_MEASURED describes"""
    n = 8192
    gaps = -80.0 * torch.arange(n, dtype=D64) / (n - 1)
    gaps = gaps.float()                                     # the float32 gaps are the inputs; the reference takes them as they are
    q = torch.zeros(n, 4)
    q[:, 0] = gaps
    p = torch.zeros(2, 4)
    p[1, 0] = 1.0                                           # scores (0, gap): both exact; target 0 is the maximum
    G = ce_call(q, p, target=torch.zeros(n, dtype=torch.int64), red=NONE, pr=0)
    loss, dq = G.loss, G.dq
    g = gaps.double()
    prob = torch.exp(g) / (1 + torch.exp(g))                # d_q[0] = dS[0, 1] * p[1, 0] = the probability of column 1, exactly
    rel = ((dq[:, 0].double() - prob).abs() / prob)
    ab = (loss.double() - torch.log1p(torch.exp(g))).abs()
    return float(rel.max()), float(ab.max())


@pytest.mark.gpu
def test_math_constants_still_hold():
    pe, la = measure_loss_constants()
    print(f"measured: probability {pe:.4e} ({pe / u:.2f} u), row loss {la:.4e} ({la / u:.2f} u)")
    assert pe <= EXP_MEASURED * 1.001 and la <= LOG_MEASURED * 1.001
    assert pe >= EXP_MEASURED / 4 and la >= LOG_MEASURED / 4               # and the recorded figures are not slack by a wide margin


LOSS_Q = [1, 3, 4, 5, 70, 130]
LOSS_P = [1, 8, 63, 64, 65, 130]
LOSS_D = [4, 64, 252, 260, 768]


@pytest.mark.gpu
@pytest.mark.parametrize("Qg", LOSS_Q)
def test_loss_shapes(Qg):
    """every (Pg, n_psg) whose default target exists, d cycling through LOSS_D; every d at Pg = 130"""
    k = 0
    for Pg in LOSS_P:
        for n_psg in (1, 2, 4):
            if (Qg - 1) * n_psg >= Pg:
                continue
            for d in (LOSS_D if Pg == 130 and n_psg == 1 else [LOSS_D[k % 5]]):
                q, p = loss_inputs(Qg, Pg, d)
                ce_check(q, p, n_psg=n_psg, scale=0.125, legacy=k % 2 == 0, tag="shapes")
            k += 1
    assert k > 0


@pytest.mark.gpu
@pytest.mark.parametrize("Qg,Pg,d", list(BOUNDARY_CASES), ids=lambda v: str(v))
def test_loss_score_path_boundary(Qg, Pg, d):
    """Qg * Pg == 65536 runs the wave-per-dot kernel; above it the GEMM, with a ragged ldc (Pg = 515) and with M >= 512"""
    q, p = loss_inputs(Qg, Pg, d)
    G = ce_check(q, p, target=None if Qg <= Pg else torch.arange(Qg) % Pg, q0=Qg // 2, qr=5, p0=Pg - 7, pr=7, tag="boundary")
    assert (G.fam > 0) == BOUNDARY_CASES[(Qg, Pg, d)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["d1", "d6", "d30", "d48", "q+1", "p+1", "q+1p+1-d6", "big-d48", "big-d64-aligned", "big-d64-q+1", "big-d30"])
def test_loss_d_and_alignment_domain(case):
    """every d >= 1 and every float-aligned q / p, at every Qg * Pg: the wave-per-dot kernels serve what plan_gemm refuses, and aligned
    d % 32 == 0 calls above the boundary stay on the GEMM (ce_check asserts the family)"""
    big = case.startswith("big")
    Qg, Pg = (128, 516) if big else (5, 65)
    d = int(case.split("d")[1].split("-")[0]) if "d" in case else 64
    q, p = loss_inputs(Qg, Pg, d)
    G = ce_check(q, p, n_psg=2, scale=0.125, q0=1, qr=3, p0=2, pr=9, q_off=1 if "q+1" in case else 0, p_off=1 if "p+1" in case else 0, tag=case)
    assert (G.fam > 0) == (case == "big-d64-aligned")


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [(0, 3, 0, 4), (33, 5, 60, 9), (67, 3, 126, 4), (0, 0, 0, 130), (10, 4, 5, 0), (0, 70, 0, 130)], ids=str)
def test_loss_slices_and_outputs(slices):
    """slices at the first, a middle and the last position, empty slices, each output absent in turn, S in the workspace"""
    q0, qr, p0, pr = slices
    q, p = loss_inputs(70, 130, 260)
    target = torch.arange(70) * 1
    target[5] = IGN
    for k, (dq, dp, sc) in enumerate(((True, True, True), (False, True, True), (True, False, True), (False, False, True), (True, True, False), (False, False, False))):
        ce_check(q, p, target=target if k % 2 else None, red=(MEAN, SUM, NONE)[k % 3], scale=0.125, q0=q0, qr=qr, p0=p0, pr=pr, want_dq=dq, want_dp=dp,
                 want_scores=sc, tag=f"slices{k}")


def targets_for(kind, Qg, Pg):
    gen = torch.Generator().manual_seed(Qg + Pg)
    t = torch.randint(0, Pg, (Qg,), generator=gen)
    t[0], t[-1] = 0, Pg - 1                                   # the first and the last column
    if kind == "some":
        t[1::3] = IGN
    if kind == "all":
        t[:] = IGN
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("red", [MEAN, SUM, NONE], ids=lambda r: RED[r])
@pytest.mark.parametrize("kind", ["default", "none_ignored", "some", "all"])
def test_loss_targets_and_reductions(red, kind):
    """explicit targets with no, some and all rows ignored (the all-ignored mean is NaN with zero gradients, as the reference's), the
    first and the last column, row_grad with negative and zero weights or absent, three loss scales"""
    for Qg, Pg, d in ((5, 8, 64), (70, 130, 260), (130, 130, 4)):
        q, p = loss_inputs(Qg, Pg, d)
        target = None if kind == "default" else targets_for({"none_ignored": "none"}.get(kind, kind), Qg, Pg)
        for scale in (1.0, 0.125, 8.0):
            rgs = [None]
            if red == NONE:
                rg = torch.randn(Qg, generator=torch.Generator().manual_seed(7))
                rg[0], rg[-1] = 0.0, -2.0
                rgs = [None, rg]
            for rg in rgs:
                G = ce_check(q, p, target=target, red=red, row_grad=rg, scale=scale, q0=Qg // 3, qr=Qg - Qg // 3, tag=f"targets-{kind}")
                if kind == "all" and red == MEAN:
                    assert bool(torch.isnan(G.loss)) and not G.dq.any() and not G.dp.any()


@pytest.mark.gpu
def test_loss_stability():
    """scores of magnitude 100 (expf overflows unless the maximum is subtracted), a row of equal scores, a target that is the row's
    maximum and one that is its minimum by a margin of 80"""
    q, p = loss_inputs(5, 12, 64, qscale=200.0)
    G = ce_check(q, p, n_psg=2, tag="large")
    assert float(G.R.S.abs().max()) > 100 and bool(torch.isfinite(G.loss))
    Qg, Pg, d = 4, 70, 8
    q, p = torch.zeros(Qg, d), torch.zeros(Pg, d)
    q[:, 0] = 1.0
    p[:, 0] = 0.5                                             # row 0: all scores equal
    q[1, 1], q[2, 1], q[3, 1] = 1.0, 1.0, 2.0
    p[3, 1], p[7, 1] = 80.0, -80.0                            # rows 1, 2: column 3 is the maximum by 80, column 7 the minimum by 80
    q[0, 1] = 0.0
    target = torch.tensor([5, 3, 7, 7])
    for red in (MEAN, NONE):
        G = ce_check(q, p, target=target, red=red, tag="margins")
    assert abs(float(G.loss[0]) - math.log(Pg)) < 1e-5 and float(G.loss[1]) < 1e-30 and abs(float(G.loss[2]) - 160.0) < 1e-3


@pytest.mark.gpu
def test_loss_wrapper_passes_the_same_arguments():
    from openmatch_amd.ops import contrastive_loss
    q, p = loss_inputs(9, 40, 64)
    target = targets_for("some", 9, 40)
    qd, pd = q.to(DEV), p.to(DEV)
    ql, pl = qd[2:6].clone().requires_grad_(), pd[8:20].clone().requires_grad_()
    loss, scores = contrastive_loss(qd, pd, 2, 0.125, ql, 2, pl, 8, target=target.to(DEV), reduction="sum")
    loss.backward()
    G = ce_call(q, p, target, 2, SUM, None, 0.125, 2, 4, 8, 12)
    assert torch.equal(bits(loss.detach().cpu(), F32), bits(G.loss, F32)) and torch.equal(bits(scores.cpu(), F32), bits(G.S, F32))
    assert torch.equal(bits(ql.grad.cpu(), F32), bits(G.dq, F32)) and torch.equal(bits(pl.grad.cpu(), F32), bits(G.dp, F32))


# ---- optimizer ----
def build_table(tens, shadow_set, offsets=(), order=None, fill=GUARD_F):
    """Device buffers (guarded) and the two tables of one launch.  offsets: names among p g m v shadow0 shadow1 whose pointer is moved
    on by one element in every tensor.  order: a permutation of the chunk list (default: reversed, then rotated by one)."""
    recs = (N.OmAdamTensor * len(tens))()
    T, chunks = [], []
    for k, t in enumerate(tens):
        n = t.p.numel()
        B = NS(n=n)
        for name in ("p", "g", "m", "v"):
            src = getattr(t, name)
            if src is None:
                setattr(B, name, None)
                continue
            buf, view = guarded(n, fill, 1 if name in offsets else 0)
            view.copy_(src)
            setattr(B, name, (buf, view))
        B.shadows = []
        for s, dt in enumerate(shadow_set):
            buf, view = guarded(n, fill, 1 if f"shadow{s}" in offsets else 0, TORCH_DT[dt])
            B.shadows.append((buf, view, dt))
        r = recs[k]
        r.p, r.m, r.v = B.p[1].data_ptr(), B.m[1].data_ptr(), B.v[1].data_ptr()
        r.g = B.g[1].data_ptr() if B.g is not None else None
        r.shadow0 = B.shadows[0][1].data_ptr() if len(B.shadows) > 0 else None
        r.shadow1 = B.shadows[1][1].data_ptr() if len(B.shadows) > 1 else None
        r.shadow0_dtype = B.shadows[0][2] if len(B.shadows) > 0 else 0
        r.shadow1_dtype = B.shadows[1][2] if len(B.shadows) > 1 else 0
        r.n, r.weight_decay, r.reserved = n, t.wd, 0
        T.append(B)
        chunks += [(k, c) for c in range(-(-n // CHUNK))]
    if order is None:
        chunks = chunks[::-1]
        chunks = chunks[1:] + chunks[:1]
    else:
        chunks = [chunks[i] for i in order]
    tab = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)
    ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).to(DEV)
    return NS(T=T, tab=tab, ch=ch, n_chunks=len(chunks), partial=guarded(max(len(chunks), 1)), out=guarded(1), fill=fill)


def run_sqnorm(tb):
    N.check(N.lib().om_grad_sqnorm(N.ptr(tb.tab), N.ptr(tb.ch), tb.n_chunks, N.ptr(tb.partial[1]), N.ptr(tb.out[1]), N.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(*tb.partial) and guards_intact(*tb.out)
    return tb.out[1].clone()


def run_adam(tb, H, norm=None):
    state = None if H.state is None else torch.tensor(H.state, dtype=torch.float32, device=DEV)
    N.check(N.lib().om_adamw_step(N.ptr(tb.tab), N.ptr(tb.ch), tb.n_chunks, H.lr, H.b1, H.b2, H.eps, H.step, N.ptr(norm), H.max_norm, H.grad_scale, H.skip,
                                  N.ptr(state), N.stream_ptr()))
    torch.cuda.synchronize()
    if state is not None:
        assert state.cpu().tolist() == H.state                  # the step reads the state, om_loss_scale_update alone writes it


def check_adam(tb, tens, H, norm, tag=""):
    """after run_adam: every tensor against the reference within its bounds, the shadow contract, guards, NULL-gradient tensors"""
    ss = None if norm is None else float(norm.cpu()[0])
    gs_abs = abs(H.grad_scale * (H.state[1] if H.state else 1.0))
    skipped = bool(H.skip) and ss is not None and not (math.sqrt(ss) * gs_abs <= 3.0e38)      # (a NaN norm compares false)
    ref = adam_reference(tens, H, ss, tb.n_chunks) if not skipped else [None] * len(tens)
    worst_all = 0.0
    for B, t, r in zip(tb.T, tens, ref):
        for name in ("p", "g", "m", "v"):
            if getattr(B, name) is not None:
                assert guards_intact(*getattr(B, name), tb.fill), (tag, name, "guard")
        for buf, view, dt in B.shadows:
            assert guards_intact(buf, view, tb.fill), (tag, "shadow guard")
        assert B.g is None or torch.equal(bits(B.g[1].cpu(), F32), bits(t.g, F32))
        if r is None:                                           # no gradient, or a skipped step: every bit stays
            for name in ("p", "m", "v"):
                assert torch.equal(bits(getattr(B, name)[1].cpu(), F32), bits(getattr(t, name), F32)), (tag, name, "must keep its bits")
            for buf, view, dt in B.shadows:
                assert bool((view == tb.fill).all())
            continue
        got_p = B.p[1].cpu()
        w = max(close(got_p, r.p, r.e_p), close(B.m[1].cpu(), r.m, r.e_m), close(B.v[1].cpu(), r.v, r.e_v))
        worst_all = max(worst_all, w)
        assert w <= 1, (tag, B.n, w)
        for buf, view, dt in B.shadows:                         # the stored float32 p rounded once (a NaN stays a NaN, whatever its payload)
            got_s, want_s = view.cpu(), got_p.to(TORCH_DT[dt])
            nan = torch.isnan(want_s)
            diff = (bits(got_s, dt) != bits(want_s, dt)) & ~nan
            assert torch.equal(torch.isnan(got_s), nan) and not bool(diff.any()), \
                (tag, NAME[dt], "shadow", int(diff.sum()), got_p[diff][:4].tolist(), got_s[diff][:4].tolist(), want_s[diff][:4].tolist())
    print(f"{tag}: worst error / bound {worst_all:.3f}, squared norm {ss}")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYPERS))
def test_adamw_hyper(name):
    H = HYPERS[name]
    tens = adam_inputs(ADAM_SIZES[:4] + [40] + ADAM_SIZES[4:], seed=11, null_at=4)
    tb = build_table(tens, (BF16, F16))
    norm = run_sqnorm(tb) if (H.max_norm > 0 or H.skip) else None
    if norm is not None:
        exact = float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None))
        assert abs(float(norm.cpu()[0]) - exact) <= SS_CHAIN(tb.n_chunks) * u * exact
    run_adam(tb, H, norm)
    check_adam(tb, tens, H, norm, name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["aligned", "p", "g", "m", "v", "shadow0", "shadow1"])
def test_adamw_alignment(which):
    """each pointer in turn one element off: the scalar path, the same bound, the shadow contract, and agreement with the aligned run"""
    H = HYPERS["clip_above"]
    tens = adam_inputs(ADAM_SIZES, seed=12)
    runs = []
    for off in ((), () if which == "aligned" else (which,)):
        tb = build_table(tens, (BF16, F16), offsets=off)
        norm = run_sqnorm(tb)
        run_adam(tb, H, norm)
        ref = check_adam(tb, tens, H, norm, f"off-{which}")
        runs.append((tb, ref))
    for Ba, Bb, r in zip(runs[0][0].T, runs[1][0].T, runs[1][1]):
        for name, e in (("p", r.e_p), ("m", r.e_m), ("v", r.e_v)):
            assert close(getattr(Ba, name)[1].cpu(), getattr(Bb, name)[1].cpu().double(), 2 * e) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", list(SHADOW_SETS))
def test_adamw_shadows(shadows):
    """every shadow set on tensors with a tail of 1 to 3 elements and a chunk tail, both chunk orders; a norm below max_norm leaves
    the bits of max_norm = 0; the constructed ties where rounding the unstored value would differ"""
    tens = adam_inputs([5, 1023, 16385, 2 * 16384 + 7, 3], seed=13, null_at=1, sweep=False)
    H0 = HYPERS["plain"]
    exact = math.sqrt(float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None)))
    Hc = adam_hyper(max_norm=2.0 * exact)
    outs = []
    n_chunks = sum(-(-t.p.numel() // CHUNK) for t in tens)
    for H, order in ((H0, None), (Hc, list(range(n_chunks)))):
        tb = build_table(tens, SHADOW_SETS[shadows], order=order)
        norm = run_sqnorm(tb) if H.max_norm > 0 else None
        run_adam(tb, H, norm)
        check_adam(tb, tens, H, norm, f"shadows-{shadows}")
        outs.append(tb)
    for Ba, Bb in zip(outs[0].T, outs[1].T):
        for name in ("p", "m", "v"):
            assert torch.equal(bits(getattr(Ba, name)[1], F32), bits(getattr(Bb, name)[1], F32)), "a clip factor of 1 and another chunk order change no bit"
    for k, dt in enumerate(SHADOW_SETS[shadows]):
        if dt == F32:
            continue
        p, decay = shadow_tie_inputs(dt)
        n = p.numel()
        t = NS(p=p, g=torch.zeros(n), m=torch.zeros(n), v=torch.zeros(n), wd=0.5)
        for off in ((), ("p",)):                                 # the vector path (and its tail), the scalar path
            tb = build_table([t], SHADOW_SETS[shadows], offsets=off)
            run_adam(tb, adam_hyper(lr=2.0 ** -11, step=1), None)
            check_adam(tb, [t], adam_hyper(lr=2.0 ** -11, step=1), None, f"ties-{NAME[dt]}{off}")
            wrong = round_to(p.double() * decay, dt)
            assert bool((bits(tb.T[0].shadows[k][1].cpu(), dt) != bits(wrong, dt)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan], ids=["inf", "-inf", "nan"])
def test_adamw_nonfinite(bad):
    """a non-finite gradient in the last element of the last chunk: with skip_nonfinite every bit stays; without it and without a
    norm the reference decides (that element becomes inf / nan, nothing else changes course)"""
    tens = adam_inputs([5, 16385], seed=14, sweep=False)
    tens[1].g[-1] = bad
    for H, with_norm in ((adam_hyper(skip=1, max_norm=1.0), True), (adam_hyper(skip=1), True), (adam_hyper(skip=0), False)):
        tb = build_table(tens, (BF16, F32), order=[0, 1, 2])
        norm = run_sqnorm(tb) if with_norm else None
        if with_norm:
            assert not math.isfinite(float(norm.cpu()[0]))
        run_adam(tb, H, norm)
        ref = check_adam(tb, tens, H, norm, f"nonfinite-{bad}-{H.skip}")
        if not with_norm:
            assert not bool(torch.isfinite(tb.T[1].p[1][-1])) and bool(torch.isfinite(tb.T[1].p[1][:-1]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1025 tensors", "one 40000", "unaligned", "null between", "n_chunks 0"])
def test_grad_sqnorm(case):
    gen = torch.Generator().manual_seed(15)
    sizes = {"1025 tensors": [1] * 1025, "one 40000": [40000], "unaligned": [40000, 5, 16385], "null between": [1023, 16385, 7], "n_chunks 0": []}[case]
    tens = adam_inputs(sizes, seed=16, null_at=1 if case == "null between" else None, zeros=False) if sizes else []
    if not sizes:
        out = guarded(1)
        N.check(N.lib().om_grad_sqnorm(None, None, 0, None, N.ptr(out[1]), N.stream_ptr()))
        torch.cuda.synchronize()
        assert float(out[1][0]) == 0.0 and guards_intact(*out)
        H = adam_hyper()
        N.check(N.lib().om_adamw_step(None, None, 0, H.lr, H.b1, H.b2, H.eps, 1, None, 0.0, 1.0, 0, None, N.stream_ptr()))
        return
    tb = build_table(tens, (), offsets=("g",) if case == "unaligned" else ())
    a = run_sqnorm(tb)
    b = run_sqnorm(tb)
    assert torch.equal(bits(a, F32), bits(b, F32)), "one fixed order: the same bits twice"
    exact = float(sum((t.g.double() ** 2).sum() for t in tens if t.g is not None))
    got = float(a.cpu()[0])
    print(f"{case}: relative error / bound {abs(got - exact) / exact / (SS_CHAIN(tb.n_chunks) * u):.3f}")
    assert abs(got - exact) <= SS_CHAIN(tb.n_chunks) * u * exact
    if case == "null between":
        assert exact == float(sum((t.g.double() ** 2).sum() for t in (tens[0], tens[2])))


T24 = 16777216.0
# (scale, clean steps, skipped, gnorm_sq, interval) -> (scale, clean steps, skipped), from the comment above loss_scale_update_kernel: a
# non-finite norm halves the scale (floor 1.0), restarts the count and counts a skipped step; `interval` clean steps double it (ceiling 2^24)
LOSS_SCALE_TABLE = [
    ((1024.0, 5.0, 0.0, math.inf, 2000), (512.0, 0.0, 1.0)),
    ((1024.0, 5.0, 2.0, math.nan, 2000), (512.0, 0.0, 3.0)),
    ((1.5, 0.0, 0.0, math.inf, 10), (1.0, 0.0, 1.0)),
    ((1.0, 7.0, 4.0, math.inf, 10), (1.0, 0.0, 5.0)),
    ((1024.0, 5.0, 1.0, 3.5, 2000), (1024.0, 6.0, 1.0)),
    ((1024.0, 1998.0, 0.0, 0.0, 2000), (1024.0, 1999.0, 0.0)),
    ((1024.0, 1999.0, 0.0, 1e30, 2000), (2048.0, 0.0, 0.0)),
    ((T24 / 2, 9.0, 0.0, 1.0, 10), (T24, 0.0, 0.0)),
    ((T24, 9.0, 0.0, 1.0, 10), (T24, 0.0, 0.0)),
    ((12000000.0, 0.0, 0.0, 1.0, 1), (T24, 0.0, 0.0)),
    ((1000.0, 0.0, 2.0, 1.0, 1), (2000.0, 0.0, 2.0)),
    ((1000.0, 3.0, 0.0, 2.0, 2000), (1000.0, 4.0, 0.0)),
    ((1000.0, 3.0, 0.0, math.inf, 2000), (500.0, 0.0, 1.0)),
    ((3000.0, 0.0, 0.0, 2.9e38, 5), (3000.0, 1.0, 0.0)),
]


@pytest.mark.gpu
def test_loss_scale_update():
    lib = N.lib()
    for (scale, good, skipped, nsq, interval), (s1, g1, k1) in LOSS_SCALE_TABLE:
        sb, state = guarded(4)
        state.copy_(torch.tensor([scale, -7.0, good, skipped]))
        norm = torch.tensor([nsq], dtype=torch.float32, device=DEV)
        N.check(lib.om_loss_scale_update(N.ptr(norm), N.ptr(state), interval, N.stream_ptr()))
        torch.cuda.synchronize()
        want = torch.tensor([s1, 1.0, g1, k1])
        want[1] = torch.tensor(1.0) / torch.tensor(s1)           # the f32 quotient
        assert torch.equal(bits(state.cpu(), F32), bits(want, F32)), ((scale, good, skipped, nsq, interval), state.cpu().tolist())
        assert guards_intact(sb, state)
    assert float(np.float32(1.0) / np.float32(1000.0)) != 1.0 / 1000.0


@pytest.mark.gpu
def test_optimizer_wrapper_passes_the_same_arguments():
    """FusedAdamW and LossScaler against the hand-built table, bit for bit"""
    from openmatch_amd.optim import FusedAdamW, LossScaler
    tens = adam_inputs([5, 16385, 1023], seed=17, sweep=False)
    params = [torch.nn.Parameter(t.p.to(DEV)) for t in tens]
    opt = FusedAdamW([dict(params=[P], weight_decay=f32(t.wd)) for P, t in zip(params, tens)], lr=0.01, max_grad_norm=1.0)
    opt.grad_scale = 1.0 / 1024
    for P, t in zip(params, tens):
        P.grad = t.g.to(DEV)
        st = opt._state_of(P)
        st["step"], st["exp_avg"], st["exp_avg_sq"] = 1, t.m.to(DEV), t.v.to(DEV)
    opt.step()
    H = adam_hyper(max_norm=1.0, grad_scale=1.0 / 1024, step=2)
    tb = build_table(tens, (), order=[0, 1, 2, 3])
    norm = run_sqnorm(tb)
    run_adam(tb, H, norm)
    assert torch.equal(bits(norm, F32), bits(opt._norm_sq, F32))
    for P, B in zip(params, tb.T):
        assert torch.equal(bits(P.detach(), F32), bits(B.p[1], F32)) and torch.equal(bits(opt.state[P]["exp_avg"], F32), bits(B.m[1], F32))
        assert torch.equal(bits(opt.state[P]["exp_avg_sq"], F32), bits(B.v[1], F32))
    sc = LossScaler(DEV, init_scale=1000.0, growth_interval=1)
    sc.update(opt)
    assert sc.state.cpu().tolist() == [2000.0, f32(np.float32(1.0) / np.float32(2000.0)), 0.0, 0.0]


# ---- head backward ----
def linear_call(dy, x, w, want_dw=True, want_dx=True, prefill=PREFILL):
    B, D = dy.shape
    K = x.shape[1]
    dwb, dwv = guarded(D * K)
    dxb, dxv = guarded(B * K)
    dwv.fill_(prefill), dxv.fill_(prefill)
    a, b, c = dy.to(DEV), x.to(DEV), w.to(DEV)
    N.check(N.lib().om_linear_f32_backward(N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(dwv) if want_dw else None, N.ptr(dxv) if want_dx else None, B, D, K, N.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(dwb, dwv) and guards_intact(dxb, dxv)
    return dwv.view(D, K).cpu(), dxv.view(B, K).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 64])
def test_linear_backward(B):
    for D in (1, 255, 257, 768):
        for K in (1, 33, 256, 257, 768):
            gen = torch.Generator().manual_seed(B * 7 + D + K)
            dy, x, w = torch.randn(B, D, generator=gen), torch.randn(B, K, generator=gen), torch.randn(D, K, generator=gen)
            rw, rx = linear_bwd_reference(dy.double(), x.double(), w.double())
            bw, bx = linear_bwd_bounds(dy.double(), x.double(), w.double())
            dw, dx = linear_call(dy, x, w)
            assert close(dw, rw, bw) <= 1 and close(dx, rx, bx) <= 1, (B, D, K)          # dW is written: the prefill is gone
            if (D, K) in ((257, 33), (1, 1), (768, 768)):
                dw1, dx1 = linear_call(dy, x, w, want_dw=False)
                assert bool((dw1 == PREFILL).all()) and torch.equal(dx1, dx)
                dw2, dx2 = linear_call(dy, x, w, want_dx=False)
                assert bool((dx2 == PREFILL).all()) and torch.equal(dw2, dw)


@pytest.mark.gpu
def test_linear_wrapper_passes_the_same_arguments():
    from openmatch_amd.encoder import hip_linear_f32_autograd
    gen = torch.Generator().manual_seed(3)
    dy, x, w = torch.randn(5, 257, generator=gen), torch.randn(5, 64, generator=gen), torch.randn(257, 64, generator=gen)
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    hip_linear_f32_autograd(xd, wd).backward(dy.to(DEV))
    dw, dx = linear_call(dy, x, w)
    assert torch.equal(bits(wd.grad.cpu(), F32), bits(dw, F32)) and torch.equal(bits(xd.grad.cpu(), F32), bits(dx, F32))


@pytest.mark.gpu
def test_controls_on_device_output():
    """three of the controls against what the device itself returned: each reference with the mistake is out of the bound"""
    Qg, Pg, d = 9, 40, 64
    q, p = loss_inputs(Qg, Pg, d)
    target = targets_for("some", Qg, Pg)
    G = ce_check(q, p, target=target, red=MEAN, scale=0.125, q0=3, qr=4, tag="controls")
    e_dq = G.bounds[2][3:7]
    bad = ce_reference(q.double(), p.double(), target, 1, MEAN, None, 0.125, ctl="mean_Qg")
    w1 = close(G.dq, bad.dq[3:7], e_dq)
    w2 = close(G.dq, G.R.dq[0:4], e_dq)                       # q_row0 ignored
    dy, x, w = torch.randn(5, 33), torch.randn(5, 65), torch.randn(33, 65)
    dw, _ = linear_call(dy, x, w)
    rw, _ = linear_bwd_reference(dy.double(), x.double(), w.double())
    bw, _ = linear_bwd_bounds(dy.double(), x.double(), w.double())
    w3 = close(dw, rw + PREFILL, bw)                          # dW accumulated
    print(f"controls on the device's output: mean_Qg {w1:.2e}, q_row0_ignored {w2:.2e}, dw_accumulated {w3:.2e}")
    assert w1 > 1 and w2 > 1 and w3 > 1 and close(dw, rw, bw) <= 1
