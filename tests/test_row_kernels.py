"""The row kernels of the encode and train paths, kernel by kernel, against float64 references on the exact stored (rounded) inputs,
element by element, within bounds derived from the arithmetic: csrc/elementwise.hip (layernorm_kernel, layernorm_bf16x8_kernel,
ln_fold_kernel, pool_kernel, l2norm_kernel, ln_stats_reduce_kernel) and the first part of csrc/train_kernels.hip (colsum_kernel,
dropout_kernel, ln_bwd_kernel in both modes, ln_param_reduce_kernel, pool_bwd_kernel, l2norm_bwd_kernel).  Every kernel is called
alone through an om_debug_* hook that checks its pointers and dtype and forwards every argument to the omk_* launcher; every
normalisation launch stores which kernel it chose (om_debug_row_kernel_last) and every GPU case asserts the variant it was written
for, so a case that fell back to the generic kernel fails instead of passing for the wrong reason.

References (written out below; test_backward_references_are_the_autograd_of_the_forward checks the backward ones):
    LayerNorm   xhat = (x - mean) rstd, rstd = 1 / sqrt(var + eps) (biased variance), y = xhat g + b;  RMSNorm: no mean, no shift
    backward    a = dy g;  dx = rstd (a - mean(a) - xhat mean(a xhat)) [+ add];  dg = sum_rows dy xhat;  db = sum_rows dy
                (RMSNorm: the mean(a) term is absent)
    embedding   the same backward through x = word[id] + type[tt] + pos[t], dx scattered into dword[id], dtype[tt], dpos[t]
    pooling     first: x[b, 0];  mean: sum_t x m / max(sum_t m, 1e-9);  adjoints dh[b, t] = dp [t == 0] resp. dp m[b, t] / cnt
    L2          y = x / max(|x|, 1e-12);  dx = (dy - y (y . dy)) / |x| when |x| > 1e-12, else dy 1e12

Bounds (u = 2^-24; each function's docstring has its derivation): f32 sums of n terms in ANY order are within (n + c) u of the sum
of magnitudes, one rounding per multiply, U_OUT and FLOOR of the storage type; in the two-plane inputs the reference takes hi + lo
exactly and the kernel's one f32 rounding of that sum is a term of the bound.  Two constants are not derivable from the code and
were MEASURED with the float32 kernels against float64 (test_math_constants_still_hold repeats the measurement), doubled:
    RSQRT_REL    rsqrtf: LayerNorm rms rows of four elements whose variance sweeps 2^-20 .. 2^20
    DIVSQRT_REL  sqrtf followed by an f32 division: L2 normalisation of rows of four elements whose norm sweeps 2^-20 .. 2^20
(the HIP math documentation with ULP figures is not part of the ROCm installation this was written on).  No bound is fitted to a
16-bit kernel, and no case excludes an element from its comparison.

Contracts pinned on bits:
  * omk_dropout equals the Python port of om_hash64 / DropCfg / dropout_keep element by element; with `rows` the key is
    (rows[r], c), so a packed and a padded call of the same tokens draw the same mask; a row with rows[r] < 0 is keyed on that
    negative token like any other (nothing is skipped);
  * dx_drop of omk_ln_bwd_drop is omk_dropout of its own stored dx under the same seed (and the same drop_rows);
  * omk_layernorm_dual: y is y32 rounded once; omk_ln_fold: Wf is the f32 product W gamma rounded once, colsum is the sum of the
    ROUNDED Wf (the sum of W gamma is rejected by the bound at K = 64), bf = b + sum beta W with or without beta / b;
  * determinism: dx, the partial + omk_ln_param_reduce path and omk_ln_stats_reduce give identical bits twice; the atomic paths
    (dg, db, table gradients, colsum) are held to the bound only;
  * dg, db, dword, dpos, dtype, colsum's out and the reduce's dg / db ADD into what the buffer holds (pre-filled with PREFILL,
    guard floats behind them); omk_ln_stats_reduce and the fold's outputs overwrite;
  * prefetch on versus off (OM_OPT_TRAIN_WGRAD_STREAM bit 3): both meet the bound and their dx bits are EQUAL -- the prefetching
    body loads raw words one row ahead and then runs the same arithmetic in the same order;
  * pool_bwd writes all L rows of a padded sequence and exactly cu[b + 1] - cu[b] rows of a packed one; rows from cu[B] on, and the
    rows of a zero-length sequence, keep the sentinel; the embedding backward reads no row of dy for a position past a sequence's
    packed length;
  * mean pooling counts the mask over the packed extent in the forward and over the full pitch L in the backward: the two agree
    whenever cu's extents cover every unmasked key, which is what the packed step guarantees and what the cases here use;
  * a fully masked sequence pools to 0 (0 / 1e-9), not NaN;
  * the x8 kernel is a silent choice: unaligned rows (ldx = H + 4), pointers off by 8 bytes, H not a multiple of 8 or above 1024
    run the generic kernel.  g offset by four floats stays 16-byte aligned (the generic kernel's own float4 loads need that much),
    so it does NOT leave the x8 kernel; the case asserts that, and the pointer fallback is reached with x offset by four elements.

kernel variant -> GPU cases
  layernorm_kernel<TIn, TOut, 4 | 8>      test_forward_norms[layernorm|f32out|from_f32|dual-*] at every H the x8 kernel does not take,
                                          test_forward_refusals; MAX_VEC 8 at H in {1028, 1032, 2048}
  layernorm_bf16x8_kernel<NV = 1..4>      test_forward_norms[layernorm|f32out-bf16-H] (H % 8 == 0, H <= 1024: NV 1 at 8 / 256, 2 at 264 / 512,
                                          3 at 520 / 768, 4 at 776 / 1024), test_two_plane[bf16|f16-*] (16-bit plane, every NV),
                                          test_eight_bit_plane (f16, NV 1 and 2, plain and the CLS gather), test_row_gather
  ln_bwd_kernel<T, 3, 0>                  test_norm_bwd / test_ln_bwd_drop at H in {4, 64, 252, 768}; PF: 16-bit, x32 without dy32
  ln_bwd_kernel<T, 4, 0>                  H in {772, 1024} (eight waves);  <T, 8, 0>: H in {1028, 2048} (four waves)
  ln_bwd_kernel<T, 4 | 8, 1>              test_embed_bwd
  ln_param_reduce_kernel                  test_ln_bwd_drop (partial arm), test_ln_param_reduce
  pool_kernel / pool_bwd_kernel           test_pool;  l2norm_kernel / l2norm_bwd_kernel: test_l2norm;  colsum_kernel: test_colsum
  dropout_kernel                          test_dropout_*;  ln_fold_kernel: test_ln_fold;  ln_stats_reduce_kernel: test_ln_stats_reduce
Every expected variant comes from a table of this file (FWD_X8_NV, FWD_GENERIC_MV, BWD_VARIANT, EMBED_VARIANT) that
test_variant_tables_match_the_launchers_conditions checks against a plain restatement of the launchers' conditions, without a GPU.
That restatement (launcher_fwd, launcher_bwd) is held to the library's own plan (csrc/row_plan.h) through the host-only hooks
om_debug_row_fwd_plan / om_debug_row_bwd_plan by test_forward_restatement_matches_the_plan_hook and
test_backward_restatement_matches_the_plan_hook, also without a GPU; and every GPU case that asserts the noted word asserts that the
plan hook, asked with the case's own pitches and pointer alignments, answers the same word (PLANNED).

Negative controls (test_bounds_admit_an_emulated_kernel_and_reject_the_controls, CPU, against the reference in float32 in the
kernel's order, rounded to the storage type); worst error / bound of each at the shape where it is smallest, recorded 2026-10-18:
    ln_bwd 'no_mean' (mean(dy g) omitted)       dx     4.8e2 (f32, H 2048)   4.0e2 (bf16, H 2048)   up to 1.3e5 (H 64)
    ln_bwd 'dg_from_x' (dg = sum dy x)          dg     4.6e2 (f32 and bf16, M 4100 x H 64)          up to 2.4e5 (H 252)
    embedding 'type_row0' (every tt -> row 0)   dtype  1.1e5
    pool_bwd 'cnt_packed' (mask counted over a packed extent that misses a key)         9.6e5
    l2 bwd 'no_projection' (dx = dy / |x|)      dx     2.9e4
    dropout keyed on the packed row instead of the token (test_dropout_port_control_packed_row_key_is_rejected): a bit comparison;
    more than 80 % of the rows whose packed index is not their token differ.  The GPU cases repeat 'no_mean', 'no_projection', the
    packed-row key, a dropped last sequence (dpos), a dropped row tail (colsum) and a dropped second plane on the device's own output.

Measured constants: see RSQRT_MEASURED and DIVSQRT_MEASURED below.

What this list used to name as untested at kernel level now has its tests: the transposes (omk_transpose, omk_transpose_batch), the T5 activation,
embedding and bias kernels and omk_zero_rows_from are in tests/test_train_leftover_kernels.py, the weight-gradient contractions in
tests/test_gemm_tn_kernels.py, the GEMM epilogue's dropout in tests/test_gemm_epilogues.py (test_dropout_residual, test_pre_act).
One file was not on that list and had no kernel-level test either: csrc/decoder.hip, the T5 decoder position (dec_cross, dec_cross_bwd,
dec_final, dec_head_drop, dec_start, dec_cast and the hand-written train forward / backward pair with its seven dropout sites per
layer).  Its kernels and its whole step against float64 autograd under the kernels' own masks are in tests/test_decoder_kernels.py.
"""
import ctypes as C
import math
import os
import re
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.conftest import REPO
from tests.test_attention_kernels import (BF16, BITS_DT, DEV, DTYPES, F16, F32, FLOOR, NAME, SENTINEL, TORCH_DT, U_ACC, U_OUT, bits,
                                          drop_threshold, hash64, option)

# Relative error of rsqrtf as the normalisation kernels call it.  MEASURED on an MI355X, 2026-10-18: om_debug_layernorm in float32,
# rms = 1, g = 1, no shift, 4096 rows of four elements with the row's mean square swept over 2^-20 .. 2^20, against float64: largest
# relative error of an output 1.4672e-7 = 2.46 u (this includes the three additions and the division of the mean square, about 3 u);
# the constant is twice that.  test_math_constants_still_hold repeats the measurement.
RSQRT_MEASURED = 1.47e-7
RSQRT_REL = 2 * RSQRT_MEASURED
# Relative error of sqrtf followed by one f32 division (l2norm_kernel; the reciprocal and the mean pooling's division are single
# divisions and are given the same allowance).  MEASURED the same day through om_debug_l2norm: 4096 rows of four elements, norm swept
# over 2^-20 .. 2^20, largest relative error of an output 1.4882e-7 = 2.50 u (sum of squares included); doubled.
DIVSQRT_MEASURED = 1.49e-7
DIVSQRT_REL = 2 * DIVSQRT_MEASURED

u = U_ACC
PREFILL = 0.25             # accumulated-into buffers start from this
GUARD_F = 7.5              # floats behind them
GUARD = 3                  # sentinel rows behind a written tensor
EPS = 1e-5
ROW = N.ROW_KERNEL
FWD_H = [4, 8, 252, 256, 264, 512, 520, 768, 776, 1024, 1028, 1032, 2048]
FWD_M = [1, 3, 4, 5, 8, 9, 17]
BWD_H = [4, 64, 252, 768, 772, 1024, 1028, 2048]
BWD_M = [1, 7, 8, 9, 33]
# ---- the variant tables the GPU cases assert (checked against the launchers' conditions by a CPU test) ----
FWD_X8_NV = {8: 1, 256: 1, 264: 2, 512: 2, 520: 3, 768: 3, 776: 4, 1024: 4}                      # aligned 16-bit rows that take the x8 body
FWD_GENERIC_MV = {4: 4, 8: 4, 252: 4, 256: 4, 264: 4, 512: 4, 520: 4, 768: 4, 776: 4, 1024: 4, 1028: 8, 1032: 8, 2048: 8}
BWD_VARIANT = {4: (3, 8), 64: (3, 8), 252: (3, 8), 768: (3, 8), 772: (4, 8), 1024: (4, 8), 1028: (8, 4), 2048: (8, 4)}      # H -> (NV, waves), MODE 0
BWD_PF_H = {4: True, 64: True, 252: True, 768: True, 772: False, 1024: False, 1028: False, 2048: False}      # 16-bit, x32, no dy32
EMBED_VARIANT = {4: (4, 4), 768: (4, 4), 1024: (4, 4), 1028: (8, 4), 2048: (8, 4)}                            # H -> (NV, waves), MODE 1


def fwd_word(body, nv, tin, tout, plane=False, lo8=False):
    return ROW[body] | nv << 4 | tin << 8 | tout << 12 | (1 << 16 if plane else 0) | (1 << 17 if plane and lo8 else 0)


def bwd_word(nv, mode, waves, pf, partial):
    return ROW["ln_bwd"] | nv << 4 | mode << 8 | waves << 12 | (1 << 16 if pf else 0) | (1 << 17 if partial else 0)


def launcher_fwd(launcher, dtype, H, ldx, ldy, x_al=True, y_al=True, lo_al=True, g_al=True, plane=False, lo8=False):
    """A plain restatement of the four forward launchers' conditions (row_fwd_plan, csrc/row_plan.h): the note word, or the refusal's text."""
    if lo8 and not (plane and dtype == F16 and H % 256 == 0 and ldx % H == 0):
        return "eight-bit second plane"
    if H % 4 or H > 2048:
        return "multiple of 4 and <= 2048"
    mv = 4 if H <= 1024 else 8
    if launcher == "from_f32":
        return fwd_word("fwd_generic", mv, F32, dtype)
    if launcher == "dual":
        return fwd_word("fwd_generic", mv, F32, dtype) if dtype != F32 else "16-bit output format"
    ld_ok = ldy % 8 == 0 if launcher == "layernorm" else ldy % 4 == 0
    vec = dtype != F32 and H % 8 == 0 and H <= 1024 and ldx % 8 == 0 and ld_ok and x_al and y_al and g_al
    tout = dtype if launcher == "layernorm" else F32
    if launcher == "layernorm":
        if plane and not (vec and lo_al):
            return "two-plane LayerNorm input"
        if (dtype == BF16 or (dtype == F16 and plane)) and vec:
            return fwd_word("fwd_x8", max(1, (H // 8 + 31) // 32), dtype, tout, plane, lo8)
    else:
        if (dtype == BF16 or (dtype == F16 and plane)) and vec and lo_al:
            return fwd_word("fwd_x8", max(1, (H // 8 + 31) // 32), dtype, tout, plane, lo8)
        if plane:
            return "two-plane LayerNorm input"
    return fwd_word("fwd_generic", mv, dtype, tout)


def launcher_bwd(dtype, H, mode, x32=False, dy32=False, partial=False, pf_off=False):
    """row_bwd_plan's conditions (csrc/row_plan.h) restated."""
    waves = 8 if H <= 1024 and mode == 0 else 4
    pf = mode == 0 and dtype != F32 and x32 and not dy32 and H <= 768 and not pf_off
    nv = 3 if H <= 768 and mode == 0 else 4 if H <= 1024 else 8
    return bwd_word(nv, mode, waves, pf, mode == 0 and partial)


def last():
    return N.lib().om_debug_row_kernel_last()


ENTRY = {"layernorm": 0, "f32out": 1, "from_f32": 2, "dual": 3}      # om_debug_row_fwd_plan's entry
PLANNED = NS(word=None)      # what the plan hook returned for the arguments of this file's last launcher call (call_fwd, call_norm_bwd, ...)


def plan_fwd(launcher, dtype, M, H, ldx, ldy, data_al=True, param_al=True, plane=False, lo8=False):
    """om_debug_row_fwd_plan (host only): the note word the launcher would store, 0 for nothing to do, or the refusal's text"""
    lib = N.lib()
    w = lib.om_debug_row_fwd_plan(ENTRY[launcher], dtype, M, H, ldx, ldy, int(data_al), int(param_al), int(plane), int(lo8))
    assert w >= -1 and last() == 0
    return w if w >= 0 else lib.om_last_error().decode()


def plan_bwd(dtype, mode, M, H, L=1, x32=False, dy32=False, partial=False):
    """om_debug_row_bwd_plan (host only, at the current switches): (word, [grid, threads, LDS bytes, partial_blocks]), or the refusal's text"""
    lib = N.lib()
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    w = lib.om_debug_row_bwd_plan(dtype, mode, M, H, L, int(x32), int(dy32), int(partial), out)
    assert w >= -1 and last() == 0
    return (w, list(out)) if w >= 0 else lib.om_last_error().decode()


def agrees(want, got):
    """a restated launcher's answer (a word, or a piece of the refusal's text) against a plan hook's (the word, or the whole text)"""
    return isinstance(got, str) and want in got if isinstance(want, str) else (not isinstance(got, str) and want == got)


# ---------------------------------------------------------------------------------------------------------------
# references and bounds (pure torch, in the dtype of their inputs: float64 is the reference, float32 the emulated kernel)
# ---------------------------------------------------------------------------------------------------------------
def ln_forward(x, g, b, eps, rms):
    mean = torch.zeros_like(x[..., :1]) if rms else x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd
    y = xhat * g
    if b is not None:
        y = y + b
    return NS(y=y, xhat=xhat, rstd=rstd, mean=mean, var=var, d=d, x=x, g=g, eps=eps, rms=rms)


def ln_fwd_bound(R, H, out_dtype, xin_err=None):
    """|kernel - reference| per element of y, R the float64 forward, xin_err the error of the f32 value of x the kernel holds
    (two planes: one rounding of hi + lo, u |x|; embedding: two roundings of the table sum).  With dm the error of the mean,
      dm    = (H + 2) u mean|x| + mean(xin_err)                       f32 sum of H terms and one division (0 for RMSNorm)
      e_d   = dm + u |d| + xin_err                                    d = x - mean
      e_var = (H + 8) u var + 2 mean(|d| xin_err) + dm^2              sum (x - m')^2 / H = var + (m' - mean)^2 exactly; squares, sum, division
      r     = e_var / (2 (var + eps)) + RSQRT_REL + 3 u               rstd, relative (the add of eps, the call)
      e_xh  = e_d rstd + |xhat| (r + u)
      e_y   = |g| (e_xh + u |xhat|) + u |y| + U_OUT |y| + FLOOR       the multiply by g, the shift (one rounding), the store."""
    xe = torch.zeros_like(R.x) if xin_err is None else xin_err
    dm = torch.zeros_like(R.mean) if R.rms else (H + 2) * u * R.x.abs().mean(-1, keepdim=True) + xe.mean(-1, keepdim=True)
    e_d = dm + u * R.d.abs() + xe
    e_var = (H + 8) * u * R.var + 2 * (R.d.abs() * xe).mean(-1, keepdim=True) + dm * dm
    r = e_var / (2 * (R.var + R.eps)) + RSQRT_REL + 3 * u
    e_xh = e_d * R.rstd + R.xhat.abs() * (r + u)
    R.e_xh, R.r = e_xh, r
    return R.g.abs() * (e_xh + u * R.xhat.abs()) + (u + U_OUT[out_dtype]) * R.y.abs() + FLOOR[out_dtype]


def ln_backward(x, dy, g, eps, rms, add=None, ctl=None):
    """ctl: 'no_mean' omits mean(dy g), 'dg_from_x' builds dg from x instead of xhat (negative controls)."""
    R = ln_forward(x, g, None, eps, rms)
    a = dy * g
    m1 = torch.zeros_like(R.mean) if (rms or ctl == "no_mean") else a.mean(-1, keepdim=True)
    m2 = (a * R.xhat).mean(-1, keepdim=True)
    dx0 = R.rstd * (a - m1 - R.xhat * m2)
    R.dx = dx0 if add is None else dx0 + add
    R.dx0, R.a, R.m1, R.m2, R.dy, R.add = dx0, a, m1, m2, dy, add
    R.dg = (dy * (x if ctl == "dg_from_x" else R.xhat)).sum(0)
    R.db = dy.sum(0)
    return R


def ln_bwd_bound(R, H, M, dtype, xin_err=None, prefill=PREFILL, store=True):
    """Bounds (on dx per element, on dg and db per column), R the float64 backward.  ln_fwd_bound gives e_xh (error of xhat) and r
    (relative error of rstd).  a = dy g carries u |a|; then
      e_m1 = (H + 3) u mean|a|                                        (0 for RMSNorm)
      e_m2 = (H + 4) u mean|a xhat| + mean(|a| e_xh)
      e_in = 3 u |a| + e_m1 + 2 u |m1| + e_xh |m2| + |xhat| e_m2 + 3 u |xhat m2|        a - m1 - xhat m2: a product and two subtractions
      e_dx = rstd e_in + |dx0| (r + u) [+ u |dx| for the add] + U_OUT |dx| + FLOOR
      e_dg = (M + 4) u (sum_rows |dy xhat| + |prefill|) + sum_rows |dy| e_xh ;  e_db = (M + 4) u (sum_rows |dy| + |prefill|)
    the column sums are f32 sums of M terms in whatever order the rows, waves, blocks and atomics take them."""
    ln_fwd_bound(R, H, F32, xin_err)
    a = R.a.abs()
    e_m1 = torch.zeros_like(R.m1) if R.rms else (H + 3) * u * a.mean(-1, keepdim=True)
    e_m2 = (H + 4) * u * (R.a * R.xhat).abs().mean(-1, keepdim=True) + (a * R.e_xh).mean(-1, keepdim=True)
    e_in = 3 * u * a + e_m1 + 2 * u * R.m1.abs() + R.e_xh * R.m2.abs() + R.xhat.abs() * e_m2 + 3 * u * (R.xhat * R.m2).abs()
    e_dx = R.rstd * e_in + R.dx0.abs() * (R.r + u)
    if R.add is not None:
        e_dx = e_dx + u * R.dx.abs()
    R.e_dx32 = e_dx
    if store:
        e_dx = e_dx + U_OUT[dtype] * R.dx.abs() + FLOOR[dtype]
    e_dg = (M + 4) * u * ((R.dy * R.xhat).abs().sum(0) + abs(prefill)) + (R.dy.abs() * R.e_xh).sum(0)
    e_db = (M + 4) * u * (R.dy.abs().sum(0) + abs(prefill))
    return e_dx, e_dg, e_db


def embed_rows(ids, tts, L, vocab, type_vocab, has_type):
    """the table rows every token reads, clamped as embed_kernel / ln_bwd_kernel clamp them"""
    idc = ids.clamp(0, vocab - 1)
    ttc = (tts.clamp(0, type_vocab - 1) if tts is not None else torch.zeros_like(ids)) if has_type else torch.zeros_like(ids)
    t = torch.arange(ids.numel(), device=ids.device) % L
    return idc, ttc, t


def embed_backward(dy, ids, tts, word, pos, typ, g, eps, L, vocab, type_vocab, live=None, ctl=None):
    """dy [B * L, H] in the padded layout (rows that do not exist: live False, they contribute nothing).  ctl 'type_row0': a wrong
    kernel that adds every token's gradient into token-type row 0."""
    idc, ttc, t = embed_rows(ids, tts, L, vocab, type_vocab, typ is not None)
    x = word[idc] + (typ[ttc] if typ is not None else 0) + pos[t]
    if live is None:
        live = torch.ones_like(ids, dtype=torch.bool)
    sel = live.nonzero().flatten()
    R = ln_backward(x[sel], dy[sel], g, eps, 0)
    R.sel, R.idc, R.ttc, R.t = sel, idc[sel], ttc[sel], t[sel]
    R.xparts = word[idc][sel].abs() + (typ[ttc][sel].abs() if typ is not None else 0) + pos[t][sel].abs()
    R.dword = torch.zeros_like(word).index_add_(0, R.idc, R.dx)
    R.dpos = torch.zeros_like(pos).index_add_(0, R.t, R.dx)
    R.dtype = None if typ is None else torch.zeros_like(typ).index_add_(0, torch.zeros_like(R.ttc) if ctl == "type_row0" else R.ttc, R.dx)
    return R


def embed_bwd_bound(R, H, M, word, pos, typ, prefill=PREFILL):
    """x = (word + type) + pos is two f32 roundings: xin_err = u (|word| + |type| + |pos|) + u |x|.  dx stays in f32 and is added
    into the tables: per table row, (count + 4) u (sum |dx| + |prefill|) + sum e_dx over the tokens that hit the row."""
    e_dx, e_dg, e_db = ln_bwd_bound(R, H, M, F32, xin_err=u * R.xparts + u * R.x.abs(), prefill=prefill, store=False)

    def scatter(table, index):
        cnt = torch.zeros(table.shape[0], dtype=table.dtype, device=table.device).index_add_(0, index, torch.ones_like(index, dtype=table.dtype))
        mag = torch.zeros_like(table).index_add_(0, index, R.dx.abs())
        err = torch.zeros_like(table).index_add_(0, index, e_dx)
        return (cnt[:, None] + 4) * u * (mag + abs(prefill)) + err
    return scatter(word, R.idc), scatter(pos, R.t), None if typ is None else scatter(typ, R.ttc), e_dg, e_db


def pool_forward(x, mask, lens, mode):
    """x [B, L, H]; lens [B]: the rows the kernel visits (L when padded, the packed extent otherwise)"""
    B, L, H = x.shape
    if mode == N.POOL_FIRST:
        return x[:, 0], torch.zeros_like(x[:, 0])
    vis = (torch.arange(L, device=x.device)[None] < lens[:, None]).to(x.dtype) * mask.to(x.dtype)
    cnt = vis.sum(1).clamp_min(1e-9)[:, None]
    y = (x * vis[:, :, None]).sum(1) / cnt
    mag = (x.abs() * vis[:, :, None]).sum(1) / cnt
    return y, mag


def pool_fwd_bound(y, mag, L):
    """mean: an f32 sum of at most L products with 0 / 1 (exact), (L + 2) u sum |x m| / cnt, and one division"""
    return (L + 2) * u * mag + (DIVSQRT_REL + u) * y.abs() + FLOOR[F32]


def pool_backward(dp, mask, L, mode, ctl_lens=None):
    """dh [B, L, H]; ctl_lens: a wrong kernel that counts the mask over the packed extent (negative control)"""
    B, H = dp.shape
    if mode == N.POOL_FIRST:
        w = torch.zeros(B, L, dtype=dp.dtype, device=dp.device)
        w[:, 0] = 1
    else:
        m = mask.to(dp.dtype)
        mc = m if ctl_lens is None else m * (torch.arange(L, device=dp.device)[None] < ctl_lens[:, None])
        w = m / mc.sum(1).clamp_min(1e-9)[:, None]
    return dp[:, None, :] * w[:, :, None]


def pool_bwd_bound(dh, dtype):
    """dp m / cnt: an exact product with 0 / 1, one division, the store"""
    return (DIVSQRT_REL + u + U_OUT[dtype]) * dh.abs() + FLOOR[dtype]


L2_EPS = float(np.float32(1e-12))


def l2_forward(x):
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    return x / n.clamp_min(L2_EPS), n


def l2_fwd_bound(y, D):
    """sum of D squares (all positive: (D + 2) u relative, halved by the root), sqrtf and the division"""
    return (0.5 * (D + 2) * u + DIVSQRT_REL + 2 * u) * y.abs() + 2.0 ** -149


def l2_backward(x, dy, ctl=None):
    """ctl 'no_projection': dx = dy / |x| (negative control)"""
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    big = n > L2_EPS
    inv = 1.0 / torch.where(big, n, torch.ones_like(n))
    y = x * inv
    t = (x * dy).sum(-1, keepdim=True) * inv
    p = torch.zeros_like(y) if ctl == "no_projection" else y * t
    dx = torch.where(big, (dy - p) * inv, dy * float(np.float32(1e12)))
    return NS(dx=dx, inv=inv, y=y, t=t, p=p, big=big, dy=dy, xdy=(x * dy).abs().sum(-1, keepdim=True))


def l2_bwd_bound(R, D):
    """rn = (D + 2) u / 2 + DIVSQRT_REL + u: relative error of inv = 1 / sqrt(ss).  y = x inv: rn + u.  t = dot inv with dot an f32 sum:
    e_t = (D + 2) u sum|x dy| inv + |t| (rn + u);  p = y t: e_p = |y| e_t + |p| (rn + 2 u);  dy - p: + u (|dy| + |p|);  times inv:
    e = (e_p + u (|dy| + |p|)) inv + |dx| (rn + u).  The clamped branch is one multiply: u |dx|."""
    rn = 0.5 * (D + 2) * u + DIVSQRT_REL + u
    e_t = (D + 2) * u * R.xdy * R.inv + R.t.abs() * (rn + u)
    e_p = R.y.abs() * e_t + R.p.abs() * (rn + 2 * u)
    e = (e_p + u * (R.dy.abs() + R.p.abs())) * R.inv + R.dx.abs() * (rn + u)
    return torch.where(R.big, e, u * R.dx.abs()) + 2.0 ** -149


def keep_of(seed, keys, p):
    """dropout_keep (csrc/kernels.h) for int64 element keys (token * H + column): one hash per four consecutive keys, the 16-bit field
    key & 3 of it kept iff >= thresh.  Returns (bool tensor of keys' shape, keep scale as the kernel's f32)."""
    thresh, _ = drop_threshold(p)
    k = keys.cpu().numpy().astype(np.int64).view(np.uint64)
    word = hash64(seed, k >> np.uint64(2))
    field = (word >> (np.uint64(16) * (k & np.uint64(3)))) & np.uint64(0xFFFF)
    scale = np.float32(65536.0) / np.float32(65536 - thresh)
    return torch.from_numpy(field >= np.uint64(thresh)), scale


def dropout_port(x, p, seed, rows=None, H=0):
    """omk_dropout in Python: y = keep ? x scale : 0 in f32, rounded once to x's type"""
    n = x.numel()
    i = torch.arange(n, dtype=torch.int64)
    if rows is not None:
        i = rows.cpu().to(torch.int64)[i // H] * H + i % H
    keep, scale = keep_of(seed, i, p)
    y = torch.where(keep, x.detach().cpu().flatten().float() * torch.tensor(scale), torch.zeros(()))
    return y.to(x.dtype).view(x.shape)


def lo8_offset(m, n, Ncols):
    """omk_lo8_offset (csrc/kernels.h) on numpy int64 arrays"""
    tile = (m >> 8) * (Ncols >> 8) + (n >> 8)
    wave = ((m >> 7) & 1) * 2 + ((n >> 7) & 1)
    r, c = m & 127, n & 127
    P = 2 * (r >> 5) + (c >> 6)
    G = 2 * ((r >> 4) & 1) + ((c >> 5) & 1)
    lane = ((c >> 2) & 3) * 16 + (r & 15)
    return ((tile * 4 + wave) * 8 + P) * 2048 + (G >> 1) * 1024 + lane * 16 + (G & 1) * 8 + ((c >> 4) & 1) * 4 + (c & 3)


def make_rows(M, H, seed, device="cpu", spread=True):
    """rows whose scale spreads over five binades and whose mean is not zero"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=gen)
    if spread:
        x = x * (2.0 ** ((torch.arange(M) % 5).float() - 2.0))[:, None] + (torch.arange(M) % 3).float()[:, None] * 0.5
    return x.to(device)


def make_affine(H, seed, device="cpu"):
    gen = torch.Generator().manual_seed(seed + 1000)
    return (1.0 + 0.5 * torch.randn(H, generator=gen)).to(device), (0.3 * torch.randn(H, generator=gen)).to(device)


def worst(got, ref, bound):
    """largest |got - ref| / bound (<= 1: every element within its bound); inf if anything is not finite"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    diff = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=diff.device).expand_as(diff)
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / bound).max()) if got.numel() else 0.0      # (0 <= 0 holds)


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_backward_references_are_the_autograd_of_the_forward():
    torch.manual_seed(0)
    M, H = 5, 12
    g, b = make_affine(H, 1)
    for rms in (0, 1):
        x = make_rows(M, H, 2).double().requires_grad_()
        gg = g.double().requires_grad_()
        bb = b.double().requires_grad_()
        dy = make_rows(M, H, 3, spread=False).double()
        y = ln_forward(x, gg, None if rms else bb, EPS, rms).y
        y.backward(dy)
        R = ln_backward(x.detach(), dy, g.double(), EPS, rms)
        assert torch.allclose(R.dx, x.grad, rtol=1e-11, atol=1e-13) and torch.allclose(R.dg, gg.grad, rtol=1e-11, atol=1e-13)
        if not rms:
            assert torch.allclose(R.db, bb.grad, rtol=1e-11, atol=1e-13)
    # embedding: through the three tables, clamped ids, token types 0..3, a packed batch with a dead row
    B, L, vocab, tv = 3, 4, 7, 4
    word, pos, typ = (torch.randn(n, H, dtype=torch.float64, requires_grad=True) for n in (vocab, L, tv))
    ids = torch.tensor([0, 6, 9, -2, 3, 3, 3, 1, 2, 5, 6, 0])
    tts = torch.tensor([0, 1, 2, 3, 5, -1, 0, 1, 2, 2, 0, 1])
    live = torch.ones(B * L, dtype=torch.bool); live[7] = False
    dy = torch.randn(B * L, H, dtype=torch.float64)
    idc, ttc, t = embed_rows(ids, tts, L, vocab, tv, True)
    y = ln_forward(word[idc] + typ[ttc] + pos[t], g.double(), b.double(), EPS, 0).y
    (y * dy)[live].sum().backward()
    R = embed_backward(dy, ids, tts, word.detach(), pos.detach(), typ.detach(), g.double(), EPS, L, vocab, tv, live)
    for got, want in ((R.dword, word.grad), (R.dpos, pos.grad), (R.dtype, typ.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-13)
    # pooling (mean, a hole in the mask, a fully masked row) and L2 (with a clamped row)
    x = torch.randn(3, 5, H, dtype=torch.float64, requires_grad=True)
    mask = torch.tensor([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    dp = torch.randn(3, H, dtype=torch.float64)
    lens = torch.tensor([5, 5, 5])
    for mode in (N.POOL_FIRST, N.POOL_MEAN):
        x.grad = None
        (pool_forward(x, mask, lens, mode)[0] * dp).sum().backward()
        assert torch.allclose(pool_backward(dp, mask, 5, mode), x.grad, rtol=1e-12, atol=1e-14)
    x = torch.randn(4, H, dtype=torch.float64)
    x[2] *= 1e-22
    x.requires_grad_()
    dy = torch.randn(4, H, dtype=torch.float64)
    (l2_forward(x)[0] * dy).sum().backward()
    got = l2_backward(x.detach(), dy).dx
    live = torch.tensor([True, True, False, True])
    assert torch.allclose(got[live], x.grad[live], rtol=1e-9, atol=1e-13)
    # the clamped row: the kernel's adjoint is dy * 1e12f while its forward divides by 1e-12f, and 1e12f * 1e-12f = 1 - 8.3e-9
    assert torch.allclose(got[2], x.grad[2], rtol=2e-8, atol=0) and not torch.allclose(got[2], x.grad[2], rtol=1e-9, atol=0)


CONTROL_RATIOS = {}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: NAME[d])
def test_bounds_admit_an_emulated_kernel_and_reject_the_controls(dtype):
    """The emulated kernel is the reference computed in float32 on the same stored inputs, rounded to the storage type."""
    td = TORCH_DT[dtype]
    for (M, H, rms, use_add) in ((33, 768, 0, False), (9, 252, 1, True), (7, 2048, 0, True), (4100, 64, 0, False)):
        g, b = make_affine(H, H)
        x, dy = make_rows(M, H, 5).to(td), make_rows(M, H, 6, spread=False).to(td)
        add = make_rows(M, H, 7, spread=False).to(td) if use_add else None
        f = lambda t, k=torch.float64: None if t is None else t.to(k)
        Rf = ln_forward(f(x), f(g), f(b), EPS, rms)
        assert worst(ln_forward(f(x, torch.float32), g, b, EPS, rms).y.to(td), Rf.y, ln_fwd_bound(Rf, H, dtype)) <= 1.0
        R = ln_backward(f(x), f(dy), f(g), EPS, rms, f(add))
        e_dx, e_dg, e_db = ln_bwd_bound(R, H, M, dtype, prefill=0.0)
        E = ln_backward(f(x, torch.float32), f(dy, torch.float32), g, EPS, rms, f(add, torch.float32))
        assert worst(E.dx.to(td), R.dx, e_dx) <= 1.0 and worst(E.dg, R.dg, e_dg) <= 1.0 and worst(E.db, R.db, e_db) <= 1.0
        if not rms:
            w = worst(E.dx.to(td), ln_backward(f(x), f(dy), f(g), EPS, rms, f(add), ctl="no_mean").dx, e_dx)
            assert w > 1.0
            CONTROL_RATIOS[("no_mean", NAME[dtype], H)] = w
        w = worst(E.dg, ln_backward(f(x), f(dy), f(g), EPS, rms, f(add), ctl="dg_from_x").dg, e_dg)
        assert w > 1.0
        CONTROL_RATIOS[("dg_from_x", NAME[dtype], H)] = w
    if dtype != F32:
        print("control ratios:", {k: f"{v:.2e}" for k, v in CONTROL_RATIOS.items() if NAME[dtype] in k})
        return
    # embedding backward: token types 0..3, the control adds every token into type row 0
    H, B, L, vocab, tv = 64, 6, 5, 11, 4
    gen = torch.Generator().manual_seed(3)
    word, pos, typ = (torch.randn(n, H, generator=gen) for n in (vocab, L, tv))
    ids, tts = torch.randint(-1, vocab + 1, (B * L,), generator=gen), torch.randint(0, tv, (B * L,), generator=gen)
    g, _ = make_affine(H, 9)
    dy = make_rows(B * L, H, 8, spread=False)
    d = lambda t: t.double()
    R = embed_backward(d(dy), ids, tts, d(word), d(pos), d(typ), d(g), EPS, L, vocab, tv)
    bw, bp, bt, _, _ = embed_bwd_bound(R, H, B * L, d(word), d(pos), d(typ), prefill=0.0)
    E = embed_backward(dy, ids, tts, word, pos, typ, g, EPS, L, vocab, tv)
    assert worst(E.dword, R.dword, bw) <= 1.0 and worst(E.dpos, R.dpos, bp) <= 1.0 and worst(E.dtype, R.dtype, bt) <= 1.0
    w = worst(E.dtype, embed_backward(d(dy), ids, tts, d(word), d(pos), d(typ), d(g), EPS, L, vocab, tv, ctl="type_row0").dtype, bt)
    assert w > 1.0
    CONTROL_RATIOS[("type_row0",)] = w
    # pooling backward: the control counts the mask over a packed extent that misses an unmasked key
    mask = torch.ones(3, 7, dtype=torch.long); mask[1, 3] = 0
    dp = torch.randn(3, H, generator=gen)
    ref = pool_backward(d(dp), mask, 7, N.POOL_MEAN)
    emu = pool_backward(dp, mask, 7, N.POOL_MEAN)
    assert worst(emu, ref, pool_bwd_bound(ref, F32)) <= 1.0
    w = worst(emu, pool_backward(d(dp), mask, 7, N.POOL_MEAN, ctl_lens=torch.tensor([7, 6, 5])), pool_bwd_bound(ref, F32))
    assert w > 1.0
    CONTROL_RATIOS[("cnt_packed",)] = w
    # L2 normalisation, both directions
    x, dy = l2_case_inputs(5, 65), torch.randn(5, 65, generator=gen)
    yr, _ = l2_forward(d(x))
    assert worst(l2_forward(x)[0], yr, l2_fwd_bound(yr, 65)) <= 1.0
    R = l2_backward(d(x), d(dy))
    emu = l2_backward(x, dy).dx
    assert worst(emu, R.dx, l2_bwd_bound(R, 65)) <= 1.0
    w = worst(emu, l2_backward(d(x), d(dy), ctl="no_projection").dx, l2_bwd_bound(R, 65))
    assert w > 1.0
    CONTROL_RATIOS[("no_projection",)] = w
    print("control ratios:", {k: f"{v:.2e}" for k, v in CONTROL_RATIOS.items()})


def l2_case_inputs(M, D, seed=11):
    """row 1 zero, row 2 of norm 1e-20 (clamped), row 3 of norm ~1e15 (its squares stay finite in f32), the others O(1)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=gen)
    if M > 1:
        x[1] = 0
    if M > 2:
        x[2] = x[2] / x[2].norm() * 1e-20
    if M > 3:
        x[3] = x[3] / x[3].norm() * 1e15
    return x


def test_l2_large_row_is_finite_in_f32():
    for D in (1, 63, 64, 65, 768):
        x = l2_case_inputs(5, D)
        assert bool(torch.isfinite((x * x).sum(-1)).all())                     # the f32 sum of squares itself
        y, n = l2_forward(x.double())
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(n.float()).all())
        R = l2_backward(x.double(), torch.ones(5, D, dtype=torch.float64))
        assert bool(torch.isfinite(R.dx.float()).all())
        assert float(n[2]) < 1e-12 < float(n[0]) and float(n[1]) == 0.0 and 5e14 < float(n[3]) < 2e15


def test_dropout_port_control_packed_row_key_is_rejected():
    """A packed call keyed on the packed row r instead of the token rows[r] draws another mask: the bit comparison the GPU cases
    make (packed == padded at the same tokens) rejects it."""
    H, p, seed = 64, 0.1, 77
    rows = torch.tensor([0, 1, 2, 8, 9, 16, 17, 18, 19, 24, -1])
    x = torch.ones(rows.numel(), H)
    right = dropout_port(x, p, seed, rows, H)
    wrong = dropout_port(x, p, seed, torch.arange(rows.numel()), H)
    padded = dropout_port(torch.ones(32, H), p, seed)
    live = rows >= 0
    assert torch.equal(right[live], padded[rows[live]])
    differs = (right != wrong).any(-1)
    assert not differs[:3].any() and differs[3:].float().mean() > 0.8          # rows 0..2 hold tokens 0..2: the same keys
    for pp, (t, s) in {0.0: (0, 1.0), 2.0 ** -17: (1, 65536 / 65535), 0.1: (6554, 65536 / 58982), 0.5: (32768, 2.0), 0.99999: (65535, 65536.0),
                       1.0: (65535, 65536.0)}.items():
        assert drop_threshold(pp) == (t, s)
    k0 = keep_of(5, torch.arange(4096), 0.0)[0]
    k1 = keep_of(5, torch.arange(4096), 1.0)[0]
    assert k0.all() and k1.float().mean() < 0.01                               # p = 1 keeps the field 65535 only


def test_lo8_offset_port_matches_the_header(tmp_path):
    text = open(os.path.join(REPO, "openmatch_amd", "csrc", "kernels.h")).read()
    fn = re.search(r"__host__ __device__ inline size_t omk_lo8_offset\(.*?\n}\n", text, re.S).group(0)
    src = tmp_path / "lo8.cpp"
    src.write_text("#include <cstdio>\n#include <cstdint>\n#include <cstddef>\n#define __host__\n#define __device__\n" + fn +
                   "int main() { const int64_t Ns[2] = {256, 768}; for (int64_t N : Ns) for (int64_t m = 0; m < 512; ++m) for (int64_t n = 0; n < N; ++n)\n"
                   "  std::printf(\"%zu\\n\", omk_lo8_offset(m, n, N)); return 0; }\n")
    exe = tmp_path / "lo8"
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "hipcc") if subprocess.run(["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cxx, "no C++ compiler"
    subprocess.run([cxx] + (["-x", "c++"] if cxx == "hipcc" else []) + ["-O1", "-std=c++17", str(src), "-o", str(exe)], check=True)
    got = np.array(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split(), dtype=np.int64)
    at = 0
    for Nc in (256, 768):
        m, n = np.meshgrid(np.arange(512, dtype=np.int64), np.arange(Nc, dtype=np.int64), indexing="ij")
        want = lo8_offset(m, n, Nc).ravel()
        assert np.array_equal(got[at:at + want.size], want)
        assert np.array_equal(np.sort(want), np.arange(512 * Nc))              # a bijection onto the blob
        at += want.size


def fwd_cases(launcher, dtype, H):
    """(tag, ldx, ldy, x_off, g_off) of one forward case: dense, padded rows, rows that break the 16-byte vectors, g four floats on,
    x four elements on"""
    return [("dense", H, H, 0, 0), ("ld+8", H + 8, H + 8, 0, 0), ("ld+4", H + 4, H + 4, 0, 0), ("g+4", H, H, 0, 4), ("x+4", H, H, 4, 0)]


def fwd_expected(launcher, dtype, H, tag):
    """from the tables: the x8 body where its table has the H and the rows are whole aligned vectors, else the generic body"""
    x8 = launcher in ("layernorm", "f32out") and dtype == BF16 and H in FWD_X8_NV and tag in ("dense", "ld+8", "g+4")
    tin = F32 if launcher in ("from_f32", "dual") else dtype
    tout = F32 if launcher == "f32out" else dtype
    return fwd_word("fwd_x8", FWD_X8_NV[H], tin, tout) if x8 else fwd_word("fwd_generic", FWD_GENERIC_MV[H], tin, tout)


def bwd_expected(dtype, H, x32, dy32, partial, pf_off=False):
    nv, waves = BWD_VARIANT[H]
    return bwd_word(nv, 0, waves, BWD_PF_H[H] and dtype != F32 and x32 and not dy32 and not pf_off, partial)


def test_variant_tables_match_the_launchers_conditions():
    for launcher in ("layernorm", "f32out", "from_f32", "dual"):
        for dtype in DTYPES:
            if launcher == "dual" and dtype == F32:
                continue
            for H in FWD_H:
                for tag, ldx, ldy, x_off, g_off in fwd_cases(launcher, dtype, H):
                    want = launcher_fwd(launcher, dtype, H, ldx, ldy, x_al=(x_off * (2 if dtype != F32 else 4)) % 16 == 0, g_al=(g_off * 4) % 16 == 0)
                    assert fwd_expected(launcher, dtype, H, tag) == want, (launcher, NAME[dtype], H, tag)
    for dtype in (BF16, F16):
        for H, nv in FWD_X8_NV.items():
            for launcher in ("layernorm", "f32out"):
                assert launcher_fwd(launcher, dtype, H, H, H, plane=True) == fwd_word("fwd_x8", nv, dtype, dtype if launcher == "layernorm" else F32, True)
                assert launcher_fwd(launcher, dtype, H, H + 4, H, plane=True) == "two-plane LayerNorm input"
        for H in (256, 512):
            want = fwd_word("fwd_x8", H // 256, F16, F32, True, True)
            assert launcher_fwd("f32out", F16, H, H, H, plane=True, lo8=True) == want == launcher_fwd("f32out", F16, H, 32 * H, H, plane=True, lo8=True)
            assert launcher_fwd("layernorm", F16, H, H, H, plane=True, lo8=True) == fwd_word("fwd_x8", H // 256, F16, F16, True, True)
    assert launcher_fwd("layernorm", BF16, 256, 256, 256, plane=True, lo8=True) == "eight-bit second plane"
    assert launcher_fwd("layernorm", F32, 2052, 2052, 2052) == "multiple of 4 and <= 2048" == launcher_fwd("f32out", F32, 6, 6, 6)
    assert sorted(set(FWD_X8_NV.values())) == [1, 2, 3, 4] and set(FWD_GENERIC_MV) == set(FWD_H) and set(BWD_VARIANT) == set(BWD_H)
    for dtype in DTYPES:
        for H in BWD_H:
            for x32 in (False, True):
                for dy32 in (False, True):
                    for partial in (False, True):
                        for pf_off in (False, True):
                            assert bwd_expected(dtype, H, x32, dy32, partial, pf_off) == launcher_bwd(dtype, H, 0, x32, dy32, partial, pf_off)
        for H, (nv, waves) in EMBED_VARIANT.items():
            assert bwd_word(nv, 1, waves, False, False) == launcher_bwd(dtype, H, 1, partial=True)
    assert bwd_expected(BF16, 768, True, False, True) >> 16 == 3 and bwd_expected(BF16, 772, True, False, True) >> 16 == 2
    assert bwd_expected(F32, 768, True, False, False) >> 16 == 0


REFUSALS = [
    ("layernorm", dict(dtype=F32, H=6), b"multiple of 4 and <= 2048"),
    ("layernorm", dict(dtype=BF16, H=2052), b"multiple of 4 and <= 2048"),
    ("f32out", dict(dtype=F16, H=2056), b"multiple of 4 and <= 2048"),
    ("from_f32", dict(dtype=F16, H=10), b"multiple of 4 and <= 2048"),
    ("dual", dict(dtype=BF16, H=4100), b"multiple of 4 and <= 2048"),
    ("layernorm", dict(dtype=BF16, H=256, plane=True, lo8=1), b"eight-bit second plane"),
    ("f32out", dict(dtype=BF16, H=256, plane=True, lo8=1), b"eight-bit second plane"),
    ("layernorm", dict(dtype=F16, H=264, plane=True, lo8=1), b"eight-bit second plane"),
    ("layernorm", dict(dtype=F16, H=256, lo8=1), b"eight-bit second plane"),
    ("layernorm", dict(dtype=BF16, H=256, ldx=260, plane=True), b"two-plane LayerNorm input"),
    ("f32out", dict(dtype=F16, H=256, ldx=260, plane=True), b"two-plane LayerNorm input"),
    ("layernorm", dict(dtype=F32, H=256, plane=True), b"two-plane LayerNorm input"),
    ("layernorm", dict(dtype=BF16, H=252, plane=True), b"two-plane LayerNorm input"),
    ("layernorm", dict(dtype=F16, H=1032, plane=True), b"two-plane LayerNorm input"),
]
FAKE = 0x7000_0000_0000      # made-up 16-byte aligned addresses: the refusals come before any launch and read no pointer


def test_forward_restatement_matches_the_plan_hook():
    """launcher_fwd, to which the variant tables are held, is itself held to csrc/row_plan.h through om_debug_row_fwd_plan, without a
    device: the whole grid of the GPU cases, the plane and eight-bit cases, every refusal with its text, every alignment input flipped
    alone, and M = 0"""
    n = 0

    def check(launcher, dtype, H, ldx, ldy, x_al=True, y_al=True, lo_al=True, g_al=True, plane=False, lo8=False, M=4):
        nonlocal n
        want = launcher_fwd(launcher, dtype, H, ldx, ldy, x_al=x_al, y_al=y_al, lo_al=lo_al, g_al=g_al, plane=plane, lo8=lo8)
        got = plan_fwd(launcher, dtype, M, H, ldx, ldy, data_al=x_al and y_al and (lo_al or not plane), param_al=g_al, plane=plane, lo8=lo8)
        assert agrees(want, got), (launcher, NAME[dtype], H, ldx, ldy, x_al, y_al, lo_al, g_al, plane, lo8, want, got)
        n += 1
        return got

    for launcher in ENTRY:
        for dtype in DTYPES:
            for H in FWD_H:
                for tag, ldx, ldy, x_off, g_off in fwd_cases(launcher, dtype, H):
                    got = check(launcher, dtype, H, ldx, ldy, x_al=(x_off * (2 if dtype != F32 else 4)) % 16 == 0, g_al=(g_off * 4) % 16 == 0)
                    if not (launcher == "dual" and dtype == F32):
                        assert got == fwd_expected(launcher, dtype, H, tag)
    for dtype in (BF16, F16):
        for H in FWD_X8_NV:
            for launcher in ("layernorm", "f32out"):
                check(launcher, dtype, H, H, H, plane=True)
                check(launcher, dtype, H, H + 4, H, plane=True)
        for H in (256, 512):
            for launcher in ("layernorm", "f32out"):
                check(launcher, dtype, H, H, H, plane=True, lo8=True)
                check(launcher, dtype, H, 32 * H, H, plane=True, lo8=True)
    check("layernorm", F32, 2052, 2052, 2052)
    check("f32out", F32, 6, 6, 6)
    for launcher, kw, text in REFUSALS:
        H = kw["H"]
        got = check(launcher, kw["dtype"], H, kw.get("ldx", H), H, plane=bool(kw.get("plane")), lo8=bool(kw.get("lo8")))
        assert isinstance(got, str) and text.decode() in got and got.startswith("om_debug_row_fwd_plan: ")
    # every alignment input flipped alone: with the x8 body's other conditions met it alone decides (the tables' H = 256 and 1024)
    for H in (256, 1024):
        for launcher in ("layernorm", "f32out"):
            for dtype in DTYPES:
                for plane in (False, True):
                    base = check(launcher, dtype, H, H, H, plane=plane)
                    flips = [dict(x_al=False), dict(y_al=False), dict(g_al=False), dict(ldx=H + 4), dict(ldy=H + 4), dict(ldy=H + 2)]
                    flips += [dict(lo_al=False)] if plane else []
                    for flip in flips:
                        kw = dict(ldx=H, ldy=H, plane=plane)
                        kw.update(flip)
                        got = check(launcher, dtype, H, **kw)
                        x8 = dtype == BF16 or (dtype == F16 and plane)
                        keeps = flip == dict(ldy=H + 4) and launcher == "f32out"          # f32 output rows: whole vectors of FOUR elements
                        assert (got == base) == (keeps or not x8), (launcher, NAME[dtype], H, plane, flip)
    # nothing to do: after the eight-bit and the width refusals, before everything else (dual: before its format check)
    for launcher in ENTRY:
        for dtype in DTYPES:
            assert plan_fwd(launcher, dtype, 0, 256, 256, 256) == 0 == plan_fwd(launcher, dtype, -3, 2048, 2052, 2052, data_al=False, param_al=False)
            assert "multiple of 4 and <= 2048" in plan_fwd(launcher, dtype, 0, 2052, 2052, 2052)
    assert plan_fwd("dual", F32, 0, 256, 256, 256) == 0 and "a 16-bit output format" in plan_fwd("dual", F32, 1, 256, 256, 256)
    assert "eight-bit second plane" in plan_fwd("layernorm", BF16, 0, 256, 256, 256, plane=True, lo8=True)
    assert "eight-bit second plane" in plan_fwd("f32out", BF16, 0, 2304, 2304, 2304, plane=True, lo8=True)     # (before the width)
    assert "two-plane LayerNorm input" in plan_fwd("layernorm", F16, 1, 256, 260, 256, plane=True) and plan_fwd("layernorm", F16, 0, 256, 260, 256, plane=True) == 0
    lib = N.lib()
    assert lib.om_debug_row_fwd_plan(4, BF16, 1, 8, 8, 8, 1, 1, 0, 0) == -1 and b"entry must be" in lib.om_last_error()
    assert lib.om_debug_row_fwd_plan(0, 7, 1, 8, 8, 8, 1, 1, 0, 0) == -1 and b"dtype must be" in lib.om_last_error()
    assert n > 4 * 3 * len(FWD_H) * 5


def test_backward_restatement_matches_the_plan_hook():
    """launcher_bwd against csrc/row_plan.h through om_debug_row_bwd_plan, without a device: the variant at every combination the GPU
    cases run and with switch bit 3 either way, the grids, the LDS bytes and the refusals"""
    lib = N.lib()
    old = lib.om_debug_option_value(N.OPT_TRAIN_WGRAD_STREAM)
    for pf_off in (False, True):
        with option(N.OPT_TRAIN_WGRAD_STREAM, (old | 8) if pf_off else (old & ~8)):
            for dtype in DTYPES:
                for H in BWD_H:
                    nv, waves = BWD_VARIANT[H]
                    for x32 in (False, True):
                        for dy32 in (False, True):
                            for partial in (False, True):
                                word, out = plan_bwd(dtype, 0, 33, H, x32=x32, dy32=dy32, partial=partial)
                                assert word == launcher_bwd(dtype, H, 0, x32, dy32, partial, pf_off) == bwd_expected(dtype, H, x32, dy32, partial, pf_off)
                                assert out == [(33 + waves - 1) // waves, 64 * waves, 2 * waves * H * 4, (33 + waves - 1) // waves]
                for H, (nv, waves) in EMBED_VARIANT.items():
                    word, out = plan_bwd(dtype, 1, 10, H, L=5, x32=True, partial=True)      # MODE 1 reads neither
                    assert word == launcher_bwd(dtype, H, 1, x32=True, partial=True, pf_off=pf_off) == bwd_word(nv, 1, waves, False, False)
                    assert out == [5 * 51, 64 * waves, 2 * waves * H * 4, 3]
    for M in (1, 7, 8, 9, 33, 4096, 4097):
        for L in (1, 128, 256, 300):
            for H in BWD_H:
                waves = BWD_VARIANT[H][1]
                out = plan_bwd(F32, 0, M, H, L=L)[1]
                assert out[0] == out[3] == min((M + waves - 1) // waves, 512) and out[2] == 2 * waves * H * 4
            for H in EMBED_VARIANT:
                out = plan_bwd(BF16, 1, M * L, H, L=L)[1]                  # M sequences of L positions
                assert out[0] == L * max(256 // L, 1) and out[1] == 256 and out[2] == 2 * 4 * H * 4
                assert out[3] == min((M * L + 3) // 4, 512)              # the MODE 0 figure, though MODE 1 launches out[0] blocks
            if L > 1:
                assert "embedding backward: M must be B * L" in plan_bwd(F16, 1, M * L + 1, 768, L=L)
                assert plan_bwd(F16, 0, M * L + 1, 768, L=L)[0] == bwd_word(3, 0, 8, False, False)      # MODE 0 does not read L
    assert "M must be B * L" in plan_bwd(F32, 1, 4, 8, L=0) and "M must be B * L" in plan_bwd(F32, 1, 4, 8, L=-2)
    # nothing to do comes first, then the width
    for mode in (0, 1):
        assert plan_bwd(BF16, mode, 0, 768, L=3) == (0, [0, 0, 0, 0]) == plan_bwd(BF16, mode, -1, 2052, L=0)
        for H in (6, 2052):
            assert "multiple of 4 and <= 2048" in plan_bwd(BF16, mode, 4, H, L=3)
    out = (C.c_int64 * 4)()
    assert lib.om_debug_row_bwd_plan(BF16, 0, 1, 8, 1, 0, 0, 0, None) == -1 and b"null argument" in lib.om_last_error()
    assert lib.om_debug_row_bwd_plan(7, 0, 1, 8, 1, 0, 0, 0, out) == -1 and b"dtype must be" in lib.om_last_error()
    assert lib.om_debug_row_bwd_plan(BF16, 2, 1, 8, 1, 0, 0, 0, out) == -1 and b"mode must be" in lib.om_last_error()


def call_fwd(launcher, dtype, x, ldx, y, ldy, g, b, M, H, rms=0, x_lo=None, rows=None, lo8=0, y32=None, eps=EPS, stream=None):
    lib = N.lib()
    v = lambda a: a if isinstance(a, C.c_void_p) else N.ptr(a)
    s = stream if stream is not None else N.stream_ptr()
    al = lambda *ps: all((v(p).value or 0) % 16 == 0 for p in ps)
    w = lib.om_debug_row_fwd_plan(ENTRY[launcher], dtype, M, H, ldx, ldy, al(x, y, x_lo), al(g, b), x_lo is not None, lo8)
    PLANNED.word = w if w >= 0 else lib.om_last_error()       # (first: the launcher's own refusal is what om_last_error holds afterwards)
    if launcher == "layernorm":
        return lib.om_debug_layernorm(dtype, v(x), ldx, v(y), ldy, v(g), v(b), M, H, eps, rms, v(x_lo), lo8, s)
    if launcher == "f32out":
        return lib.om_debug_layernorm_f32out(dtype, v(x), ldx, v(y), ldy, v(g), v(b), M, H, eps, rms, v(x_lo), v(rows), lo8, s)
    if launcher == "from_f32":
        return lib.om_debug_layernorm_from_f32(dtype, v(x), ldx, v(y), ldy, v(g), v(b), M, H, eps, rms, s)
    return lib.om_debug_layernorm_dual(dtype, v(x), ldx, v(y), v(y32), ldy, v(g), v(b), M, H, eps, s)


@pytest.mark.parametrize("launcher,kw,text", REFUSALS, ids=[f"{l}-{NAME[k['dtype']]}-{k['H']}-{i}" for i, (l, k, _) in enumerate(REFUSALS)])
def test_forward_refusals(launcher, kw, text):
    """each refusal with its om_last_error text, before any launch (made-up addresses, no device), and the note reads 0; the table's
    reason is what the restated launcher gives"""
    lib = N.lib()
    H, dtype = kw["H"], kw["dtype"]
    ldx = kw.get("ldx", H)
    p = lambda k: C.c_void_p(FAKE + 4096 * k)
    rc = call_fwd(launcher, dtype, p(1), ldx, p(2), H, p(3), p(4), 4, H, x_lo=p(5) if kw.get("plane") else None, lo8=kw.get("lo8", 0), y32=p(6),
                  stream=C.c_void_p(0))
    assert rc != 0 and text in lib.om_last_error(), lib.om_last_error()
    assert last() == 0 and isinstance(PLANNED.word, bytes) and text in PLANNED.word
    assert launcher_fwd(launcher, dtype, H, ldx, H, plane=bool(kw.get("plane")), lo8=bool(kw.get("lo8"))).encode() in text + b" "


def test_hooks_check_their_arguments():
    lib = N.lib()
    names = ["om_debug_row_kernel_last", "om_debug_row_fwd_plan", "om_debug_row_bwd_plan", "om_debug_layernorm", "om_debug_layernorm_f32out", "om_debug_layernorm_from_f32", "om_debug_layernorm_dual",
             "om_debug_norm_bwd", "om_debug_ln_bwd_drop", "om_debug_ln_param_reduce", "om_debug_embed_bwd", "om_debug_pool", "om_debug_pool_bwd",
             "om_debug_l2norm", "om_debug_l2norm_bwd", "om_debug_colsum", "om_debug_dropout", "om_debug_ln_fold", "om_debug_ln_stats_reduce"]
    for name in names:
        assert name in N.exported_symbols() and hasattr(lib, name)
    p, z, s = C.c_void_p(FAKE), C.c_void_p(0), C.c_void_p(0)
    calls = {
        "om_debug_layernorm": lambda dt, a: lib.om_debug_layernorm(dt, a, 8, p, 8, p, z, 1, 8, EPS, 0, z, 0, s),
        "om_debug_layernorm_f32out": lambda dt, a: lib.om_debug_layernorm_f32out(dt, a, 8, p, 8, p, z, 1, 8, EPS, 0, z, z, 0, s),
        "om_debug_layernorm_from_f32": lambda dt, a: lib.om_debug_layernorm_from_f32(dt, a, 8, p, 8, p, z, 1, 8, EPS, 0, s),
        "om_debug_layernorm_dual": lambda dt, a: lib.om_debug_layernorm_dual(dt, a, 8, p, p, 8, p, z, 1, 8, EPS, s),
        "om_debug_norm_bwd": lambda dt, a: lib.om_debug_norm_bwd(dt, a, p, p, p, p, z, 1, 8, EPS, 0, z, s),
        "om_debug_ln_bwd_drop": lambda dt, a: lib.om_debug_ln_bwd_drop(dt, a, p, p, p, z, 0.0, 0, p, z, 1, 8, EPS, z, z, z, None, z, s),
        "om_debug_embed_bwd": lambda dt, a: lib.om_debug_embed_bwd(dt, a, p, z, p, p, z, p, p, p, z, p, z, 4, 4, 8, 5, 1, EPS, z, s),
        "om_debug_pool": lambda dt, a: lib.om_debug_pool(dt, a, p, p, 1, 4, 8, N.POOL_MEAN, z, s),
        "om_debug_pool_bwd": lambda dt, a: lib.om_debug_pool_bwd(dt, a, p, p, 1, 4, 8, N.POOL_MEAN, z, s),
        "om_debug_colsum": lambda dt, a: lib.om_debug_colsum(dt, a, 8, 4, 8, p, s),
        "om_debug_dropout": lambda dt, a: lib.om_debug_dropout(dt, a, p, 16, 0.1, 1, z, 0, s),
        "om_debug_ln_fold": lambda dt, a: lib.om_debug_ln_fold(dt, a, p, z, z, p, p, p, 4, 8, s),
    }
    for name, f in calls.items():
        assert f(BF16, z) != 0 and b"null argument" in lib.om_last_error() and name.encode() in lib.om_last_error(), name
        assert f(7, p) != 0 and b"dtype must be" in lib.om_last_error(), name
        assert last() == 0
    assert lib.om_debug_ln_fold(F32, p, p, z, z, p, p, p, 4, 8, s) != 0 and b"OM_BF16 or OM_F16" in lib.om_last_error()
    assert lib.om_debug_layernorm_dual(F32, p, 8, p, p, 8, p, z, 1, 8, EPS, s) != 0 and b"OM_BF16 or OM_F16" in lib.om_last_error()
    assert lib.om_debug_l2norm(z, p, 1, 4, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_l2norm_bwd(p, z, p, 1, 4, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_ln_stats_reduce(z, 1, 1, p, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_ln_param_reduce(None, 1, 8, s) != 0 and b"null" in lib.om_last_error()
    # a token-type table comes with its gradient buffer; refusals of the launchers themselves, before any launch
    assert lib.om_debug_embed_bwd(F32, p, p, z, p, p, p, p, p, p, z, p, z, 4, 4, 8, 5, 2, EPS, z, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_embed_bwd(F32, p, p, z, p, p, z, p, p, p, z, p, z, 5, 4, 8, 5, 1, EPS, z, s) != 0 and b"M must be B * L" in lib.om_last_error()
    assert lib.om_debug_norm_bwd(F32, p, p, p, p, p, z, 1, 6, EPS, 0, z, s) != 0 and b"multiple of 4" in lib.om_last_error()
    assert lib.om_debug_ln_bwd_drop(F32, p, p, p, p, z, 0.0, 0, p, z, 1, 2052, EPS, z, z, z, None, z, s) != 0 and b"<= 2048" in lib.om_last_error()
    assert lib.om_debug_pool(F32, p, p, p, 1, 4, 6, N.POOL_MEAN, z, s) != 0 and b"multiple of 4" in lib.om_last_error()
    assert lib.om_debug_pool_bwd(F32, p, p, p, 1, 4, 6, N.POOL_MEAN, z, s) != 0 and b"multiple of 4" in lib.om_last_error()
    assert lib.om_debug_dropout(F32, p, p, 17, 0.1, 1, p, 4, s) != 0 and b"n must be rows * H" in lib.om_last_error()
    assert lib.om_debug_ln_fold(BF16, p, p, z, z, p, p, p, 4, 12, s) != 0 and b"multiple of 8" in lib.om_last_error()
    blocks = C.c_int(-5)
    assert lib.om_debug_ln_bwd_drop(F32, p, p, p, p, z, 0.0, 0, p, z, 0, 8, EPS, z, z, z, C.byref(blocks), z, s) == 0 and blocks.value == 0
    assert last() == 0 and lib.om_abi_version() == 6


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def sentinel_rows(rows, ld, dtype):
    return torch.full((rows, ld), SENTINEL[dtype], dtype=BITS_DT[dtype], device=DEV).view(TORCH_DT[dtype])


def is_sentinel(t, dtype):
    return bool((bits(t.contiguous(), dtype) == SENTINEL[dtype]).all())


def acc_buffer(n):
    """an accumulated-into f32 buffer of n elements: PREFILL, then guard floats"""
    t = torch.full((n + 5,), GUARD_F, device=DEV)
    t[:n] = PREFILL
    return t


def guard_ok(t, n):
    return bool((t[n:] == GUARD_F).all())


def strided(values, ld, off=0):
    """values [M, H] placed in a buffer of row pitch ld starting `off` elements in; the gaps hold 77.0.  Returns (buffer, view)"""
    M, H = values.shape
    buf = torch.full((M * ld + off + 8,), 77.0, dtype=values.dtype, device=values.device)
    view = buf[off:off + M * ld].view(M, ld)
    view[:, :H] = values
    return buf, view


def run_forward(launcher, dtype, H, M, ldx, ldy, x_off, g_off, rms, has_b, seed, expect):
    tin = torch.float32 if launcher in ("from_f32", "dual") else TORCH_DT[dtype]
    out_dt = F32 if launcher == "f32out" else dtype
    x = make_rows(M, H, seed, DEV).to(tin)
    xbuf, xv = strided(x, ldx, x_off)
    gb, bb = make_affine(H, seed, DEV)
    gbuf, bbuf = torch.zeros(H + 8, device=DEV), torch.zeros(H + 8, device=DEV)
    g, b = gbuf[g_off:g_off + H], bbuf[g_off:g_off + H]
    g.copy_(gb); b.copy_(bb)
    y = sentinel_rows(M + GUARD, ldy, out_dt)
    y32 = sentinel_rows(M + GUARD, ldy, F32) if launcher == "dual" else None
    frozen = xbuf.clone()
    rc = call_fwd(launcher, dtype, xv, ldx, y, ldy, g, b if has_b else None, M, H, rms=rms, y32=y32)
    torch.cuda.synchronize()
    assert rc == 0, N.lib().om_last_error()
    assert last() == expect == PLANNED.word, (hex(last()), hex(expect), PLANNED.word)
    R = ln_forward(x.double(), g.double(), b.double() if has_b else None, EPS, rms)
    bound = ln_fwd_bound(R, H, out_dt)
    w = worst(y[:M, :H], R.y, bound)
    assert w <= 1.0, (launcher, NAME[dtype], H, M, ldx, w)
    assert is_sentinel(y[M:], out_dt) and is_sentinel(y[:M, H:], out_dt) and torch.equal(xbuf, frozen)
    if launcher == "dual":
        assert worst(y32[:M, :H], R.y, ln_fwd_bound(R, H, F32)) <= 1.0
        assert torch.equal(bits(y32[:M, :H].to(TORCH_DT[dtype]).contiguous(), dtype), bits(y[:M, :H].contiguous(), dtype))      # y is y32 rounded once
        assert is_sentinel(y32[M:], F32) and is_sentinel(y32[:M, H:], F32)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("H", FWD_H)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("launcher", ["layernorm", "f32out", "from_f32", "dual"])
def test_forward_norms(launcher, dtype, H):
    if launcher == "dual" and dtype == F32:
        rc = call_fwd("dual", F32, torch.zeros(8, device=DEV), 8, torch.zeros(8, device=DEV), 8, torch.ones(8, device=DEV), None, 1, 8,
                      y32=torch.zeros(8, device=DEV))
        assert rc != 0 and b"OM_BF16 or OM_F16" in N.lib().om_last_error()
        return
    k = FWD_H.index(H)
    for i, (tag, ldx, ldy, x_off, g_off) in enumerate(fwd_cases(launcher, dtype, H)):
        if x_off and tin_is_f32(launcher, dtype):
            continue                                   # four f32 elements on is still 16-byte aligned: the dense case again
        M = FWD_M[(k + i) % len(FWD_M)]
        rms = 0 if launcher == "dual" else (k + i) % 2
        run_forward(launcher, dtype, H, M, ldx, ldy, x_off, g_off, rms, has_b=not rms and i != 1, seed=H + i, expect=fwd_expected(launcher, dtype, H, tag))
    run_forward(launcher, dtype, H, 17, H, H, 0, 0, 0, True, seed=H + 9, expect=fwd_expected(launcher, dtype, H, "dense"))       # five blocks, a partial one


def tin_is_f32(launcher, dtype):
    return launcher in ("from_f32", "dual") or dtype == F32


def two_planes(M, H, dtype, seed):
    """an f32 stream split into hi + lo of the 16-bit type; returns (hi, lo, exact float64 sum of the two stored planes)"""
    full = make_rows(M, H, seed, DEV)
    hi = full.to(TORCH_DT[dtype])
    lo = (full - hi.float()).to(TORCH_DT[dtype])
    return hi, lo, hi.double() + lo.double()


@pytest.mark.gpu
@pytest.mark.parametrize("H", sorted(FWD_X8_NV))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_two_plane(dtype, H):
    """x + x_lo in 16-bit planes, both launchers that take them, every NV; the reference takes the stored sum exactly"""
    g, b = make_affine(H, H, DEV)
    for i, (launcher, ld) in enumerate((("layernorm", H), ("f32out", H), ("layernorm", H + 8), ("f32out", H + 8))):
        M = FWD_M[(FWD_H.index(H) + i) % len(FWD_M)]
        rms = i % 2
        out_dt = dtype if launcher == "layernorm" else F32
        hi, lo, x64 = two_planes(M, H, dtype, H + i)
        (_, hv), (_, lv) = strided(hi, ld), strided(lo, ld)
        y = sentinel_rows(M + GUARD, ld, out_dt)
        assert call_fwd(launcher, dtype, hv, ld, y, ld, g, None if rms else b, M, H, rms=rms, x_lo=lv) == 0, N.lib().om_last_error()
        torch.cuda.synchronize()
        assert last() == fwd_word("fwd_x8", FWD_X8_NV[H], dtype, out_dt, True) == PLANNED.word
        R = ln_forward(x64, g.double(), None if rms else b.double(), EPS, rms)
        assert worst(y[:M, :H], R.y, ln_fwd_bound(R, H, out_dt, xin_err=u * x64.abs())) <= 1.0
        assert is_sentinel(y[M:], out_dt) and is_sentinel(y[:M, H:], out_dt)
        # the planes matter: the one-plane result of hi alone is outside the bound somewhere
        R1 = ln_forward(hi.double(), g.double(), None if rms else b.double(), EPS, rms)
        assert out_dt != F32 or worst(y[:M, :H], R1.y, ln_fwd_bound(R, H, out_dt, xin_err=u * x64.abs())) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("H", [256, 512])
def test_eight_bit_plane(H):
    """float16 rows with the second plane in eight bits (e5m2 of the remainder 2^10) in the lane order of omk_lo8_offset: M = 256
    plain through both launchers, and the CLS gather (ldx = L H with rows) through omk_layernorm_f32out"""
    B, L = 8, 32
    M = B * L
    full = make_rows(M, H, H, DEV, spread=False)
    hi = full.half()
    rem = ((full - hi.float()) * 1024.0).to(torch.float8_e5m2)
    m, n = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(H, dtype=np.int64), indexing="ij")
    blob = torch.zeros(M * H, dtype=torch.uint8, device=DEV)
    blob[torch.from_numpy(lo8_offset(m, n, H).ravel()).to(DEV)] = rem.view(torch.uint8).flatten()
    x64 = hi.double() + rem.double() / 1024.0
    g, b = make_affine(H, H, DEV)
    R = ln_forward(x64, g.double(), b.double(), EPS, 0)
    for launcher, out_dt in (("layernorm", F16), ("f32out", F32)):
        y = sentinel_rows(M + GUARD, H, out_dt)
        assert call_fwd(launcher, F16, hi, H, y, H, g, b, M, H, x_lo=blob, lo8=1) == 0, N.lib().om_last_error()
        torch.cuda.synchronize()
        assert last() == fwd_word("fwd_x8", H // 256, F16, out_dt, True, True) == PLANNED.word
        assert worst(y[:M], R.y, ln_fwd_bound(R, H, out_dt, xin_err=u * x64.abs())) <= 1.0 and is_sentinel(y[M:], out_dt)
        if out_dt == F32:      # the plane is read where the port says: without it the f32 output leaves the bound
            assert worst(y[:M], ln_forward(hi.double(), g.double(), b.double(), EPS, 0).y, ln_fwd_bound(R, H, F32, xin_err=u * x64.abs())) > 1.0
    rows = torch.tensor([3, 0, 7, 7, 1, 6, 2, 5, 4, 0, 3], dtype=torch.int32, device=DEV)
    y = sentinel_rows(rows.numel() + GUARD, H, F32)
    assert call_fwd("f32out", F16, hi, L * H, y, H, g, b, rows.numel(), H, x_lo=blob, rows=rows, lo8=1) == 0, N.lib().om_last_error()
    torch.cuda.synchronize()
    assert last() == fwd_word("fwd_x8", H // 256, F16, F32, True, True) == PLANNED.word
    tok = rows.long() * L
    Rg = ln_forward(x64[tok], g.double(), b.double(), EPS, 0)
    assert worst(y[:rows.numel()], Rg.y, ln_fwd_bound(Rg, H, F32, xin_err=u * x64[tok].abs())) <= 1.0 and is_sentinel(y[rows.numel():], F32)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [252, 768, 1032])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_row_gather(dtype, H):
    """omk_layernorm_f32out with rows: a permutation with repeats, in the generic and the x8 body, with and without a second plane"""
    Mx = 9
    rows = torch.tensor([8, 0, 3, 3, 7, 1, 8, 2, 6, 5, 4, 0, 0], dtype=torch.int32, device=DEV)
    M = rows.numel()
    g, b = make_affine(H, H, DEV)
    x = make_rows(Mx, H, H + 1, DEV).to(TORCH_DT[dtype])
    y = sentinel_rows(M + GUARD, H, F32)
    assert call_fwd("f32out", dtype, x, H, y, H, g, b, M, H, rows=rows) == 0, N.lib().om_last_error()
    torch.cuda.synchronize()
    assert last() == fwd_expected("f32out", dtype, H, "dense") == PLANNED.word
    R = ln_forward(x.double()[rows.long()], g.double(), b.double(), EPS, 0)
    assert worst(y[:M], R.y, ln_fwd_bound(R, H, F32)) <= 1.0 and is_sentinel(y[M:], F32)
    if dtype != F32 and H in FWD_X8_NV:
        hi, lo, x64 = two_planes(Mx, H, dtype, H + 2)
        y = sentinel_rows(M + GUARD, H, F32)
        assert call_fwd("f32out", dtype, hi, H, y, H, g, b, M, H, x_lo=lo, rows=rows) == 0, N.lib().om_last_error()
        torch.cuda.synchronize()
        assert last() == fwd_word("fwd_x8", FWD_X8_NV[H], dtype, F32, True) == PLANNED.word
        R = ln_forward(x64[rows.long()], g.double(), b.double(), EPS, 0)
        assert worst(y[:M], R.y, ln_fwd_bound(R, H, F32, xin_err=u * x64[rows.long()].abs())) <= 1.0 and is_sentinel(y[M:], F32)


def call_norm_bwd(dtype, dy, x, g, dx, dg, db, M, H, rms, add):
    PLANNED.word = plan_bwd(dtype, 0, M, H)[0]
    rc = N.lib().om_debug_norm_bwd(dtype, N.ptr(dy), N.ptr(x), N.ptr(g), N.ptr(dx), N.ptr(dg), N.ptr(db), M, H, EPS, rms, N.ptr(add), N.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("H,M", [(H, BWD_M[i % len(BWD_M)]) for i, H in enumerate(BWD_H)] + [(64, 4100), (768, 33), (4, 9)])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_norm_bwd(dtype, H, M):
    """omk_norm_bwd, rms x add; dg / db by atomics into pre-filled buffers (db absent for RMSNorm's callers: run with and without);
    dx identical across two runs; M = 4100 at H = 64 makes the 512 blocks stride"""
    td = TORCH_DT[dtype]
    g, _ = make_affine(H, H, DEV)
    x, dy, add = make_rows(M, H, H, DEV).to(td), make_rows(M, H, H + 1, DEV, spread=False).to(td), make_rows(M, H, H + 2, DEV, spread=False).to(td)
    nv, waves = BWD_VARIANT[H]
    for rms in (0, 1):
        for use_add in (False, True):
            dx = sentinel_rows(M + GUARD, H, dtype)
            dg, db = acc_buffer(H), acc_buffer(H) if not (rms and use_add) else None
            assert call_norm_bwd(dtype, dy, x, g, dx, dg, db, M, H, rms, add if use_add else None) == 0, N.lib().om_last_error()
            assert last() == bwd_word(nv, 0, waves, False, False) == PLANNED.word
            R = ln_backward(x.double(), dy.double(), g.double(), EPS, rms, add.double() if use_add else None)
            e_dx, e_dg, e_db = ln_bwd_bound(R, H, M, dtype)
            ws = (worst(dx[:M], R.dx, e_dx), worst(dg[:H], R.dg + PREFILL, e_dg), worst(db[:H], R.db + PREFILL, e_db) if db is not None else 0.0)
            assert max(ws) <= 1.0, (NAME[dtype], H, M, rms, use_add, ws)
            assert is_sentinel(dx[M:], dtype) and guard_ok(dg, H) and (db is None or guard_ok(db, H))
            if not rms:            # the control on the device's own output: the bound rejects a backward without mean(dy g)
                assert worst(dx[:M], ln_backward(x.double(), dy.double(), g.double(), EPS, 0, add.double() if use_add else None, ctl="no_mean").dx, e_dx) > 1.0
            dx2 = sentinel_rows(M + GUARD, H, dtype)
            assert call_norm_bwd(dtype, dy, x, g, dx2, acc_buffer(H), None, M, H, rms, add if use_add else None) == 0
            assert torch.equal(bits(dx, dtype), bits(dx2, dtype))


def call_bwd_drop(dtype, dy, x, g, dx, dx_drop, p, seed, dg, db, M, H, dy32, x32, partial, drop_rows):
    blocks = C.c_int(-1)
    PLANNED.word, PLANNED.out = plan_bwd(dtype, 0, M, H, x32=x32 is not None, dy32=dy32 is not None, partial=partial is not None)
    rc = N.lib().om_debug_ln_bwd_drop(dtype, N.ptr(dy), N.ptr(x), N.ptr(g), N.ptr(dx), N.ptr(dx_drop), p, seed, N.ptr(dg), N.ptr(db), M, H, EPS,
                                      N.ptr(dy32), N.ptr(x32), N.ptr(partial), C.byref(blocks), N.ptr(drop_rows), N.stream_ptr())
    torch.cuda.synchronize()
    return rc, blocks.value


def call_dropout(dtype, x, y, p, seed, rows=None, H=0):
    rc = N.lib().om_debug_dropout(dtype, N.ptr(x), N.ptr(y), x.numel(), p, seed, N.ptr(rows), H, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


def reduce_sites(sites, H):
    arr = (N.OmLnSite * len(sites))(*[N.OmLnSite(partial=p.data_ptr(), dg=dg.data_ptr(), db=db.data_ptr() if db is not None else None, blocks=nb)
                                      for (p, dg, db, nb) in sites])
    rc = N.lib().om_debug_ln_param_reduce(arr, len(sites), H, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("H", BWD_H)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_ln_bwd_drop(dtype, H):
    """omk_ln_bwd_drop: {dy32, x32, both, neither} x {partial, atomics} x {p = 0, 0.1} x {drop_rows, none}; the variant (prefetch
    included), dx within the bound and identical twice, dx_drop == omk_dropout(stored dx), dg / db within the bound on either path and
    bit-identical twice on the partial path"""
    td = TORCH_DT[dtype]
    g, _ = make_affine(H, H, DEV)
    seed = 2 ** 63 + 99
    nv, waves = BWD_VARIANT[H]
    combo = 0
    for src in ("neither", "dy32", "x32", "both"):
        for use_partial in (False, True):
            for p in (0.0, 0.1):
                for use_rows in (False, True):
                    M = BWD_M[combo % len(BWD_M)]
                    combo += 1
                    x32 = make_rows(M, H, H + combo, DEV)
                    dy32 = make_rows(M, H, H + combo + 50, DEV, spread=False)
                    x, dy = x32.to(td), dy32.to(td)
                    has_x32, has_dy32 = src in ("x32", "both"), src in ("dy32", "both")
                    rows = (torch.arange(M, dtype=torch.int32, device=DEV) * 3 + 5) if use_rows else None        # packed row r holds token 3 r + 5
                    run = lambda: _bwd_drop_once(dtype, dy if not has_dy32 else None, x if not has_x32 else None, g, p, seed, M, H,
                                                 dy32 if has_dy32 else None, x32 if has_x32 else None, use_partial, rows)
                    a, b2 = run(), run()
                    assert a.note == bwd_expected(dtype, H, has_x32, has_dy32, use_partial), (src, use_partial, hex(a.note))
                    assert a.blocks == min(512, (M + waves - 1) // waves)
                    R = ln_backward((x32 if has_x32 else x).double(), (dy32 if has_dy32 else dy).double(), g.double(), EPS, 0)
                    e_dx, e_dg, e_db = ln_bwd_bound(R, H, M, dtype)
                    ws = (worst(a.dx[:M], R.dx, e_dx), worst(a.dg[:H], R.dg + PREFILL, e_dg), worst(a.db[:H], R.db + PREFILL, e_db))
                    assert max(ws) <= 1.0, (NAME[dtype], H, M, src, use_partial, p, use_rows, ws)
                    assert torch.equal(bits(a.dx, dtype), bits(b2.dx, dtype)) and is_sentinel(a.dx[M:], dtype)
                    assert guard_ok(a.dg, H) and guard_ok(a.db, H)
                    if use_partial:
                        assert torch.equal(a.dg, b2.dg) and torch.equal(a.db, b2.db)
                    if p > 0:
                        want = sentinel_rows(M, H, dtype)
                        assert call_dropout(dtype, a.dx[:M], want, p, seed, rows, H) == 0
                        assert torch.equal(bits(a.drop[:M], dtype), bits(want, dtype)) and is_sentinel(a.drop[M:], dtype)
                        assert torch.equal(bits(want.cpu(), dtype), bits(dropout_port(a.dx[:M], p, seed, rows, H), dtype))
                        assert 0.5 < float((a.drop[:M] == 0).float().mean()) * 10 < 2.0 or M * H < 2000
                    else:
                        assert is_sentinel(a.drop, dtype)                      # p = 0: dx_drop is not written
    assert combo == 32


def _bwd_drop_once(dtype, dy, x, g, p, seed, M, H, dy32, x32, use_partial, rows):
    dx, drop = sentinel_rows(M + GUARD, H, dtype), sentinel_rows(M + GUARD, H, dtype)
    dg, db = acc_buffer(H), acc_buffer(H)
    partial = torch.full((512 * 2 * H + 4,), GUARD_F, device=DEV) if use_partial else None
    rc, blocks = call_bwd_drop(dtype, dy, x, g, dx, drop, p, seed, None if use_partial else dg, None if use_partial else db, M, H, dy32, x32,
                               partial, rows)
    assert rc == 0, N.lib().om_last_error()
    note = last()
    assert note == PLANNED.word and blocks == PLANNED.out[3] == PLANNED.out[0]
    if use_partial:
        assert bool((partial[blocks * 2 * H:] == GUARD_F).all())               # exactly `blocks` blocks wrote
        assert reduce_sites([(partial, dg, db, blocks)], H) == 0
    return NS(dx=dx, drop=drop, dg=dg, db=db, note=note, blocks=blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [64, 768, 772])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_prefetch_on_versus_off(dtype, H):
    """OM_OPT_TRAIN_WGRAD_STREAM bit 3 switches the prefetching body off: both meet the bound, and dx / dx_drop carry the same bits
    (the prefetch only moves the loads one row ahead); at H = 772 neither is the prefetching body"""
    td = TORCH_DT[dtype]
    M = 4100 if H == 64 else 33
    g, _ = make_affine(H, H, DEV)
    x32, dy = make_rows(M, H, 1, DEV), make_rows(M, H, 2, DEV, spread=False).to(td)
    R = ln_backward(x32.double(), dy.double(), g.double(), EPS, 0)
    e_dx, e_dg, e_db = ln_bwd_bound(R, H, M, dtype)
    old = N.lib().om_debug_option_value(N.OPT_TRAIN_WGRAD_STREAM)
    out = []
    for off in (False, True):
        with option(N.OPT_TRAIN_WGRAD_STREAM, (old | 8) if off else (old & ~8)):
            a = _bwd_drop_once(dtype, dy, None, g, 0.1, 5, M, H, None, x32, True, None)
        assert a.note == bwd_expected(dtype, H, True, False, True, pf_off=off)
        assert bool(a.note >> 16 & 1) == (H <= 768 and not off)
        assert max(worst(a.dx[:M], R.dx, e_dx), worst(a.dg[:H], R.dg + PREFILL, e_dg), worst(a.db[:H], R.db + PREFILL, e_db)) <= 1.0
        out.append(a)
    assert torch.equal(bits(out[0].dx, dtype), bits(out[1].dx, dtype)) and torch.equal(bits(out[0].drop, dtype), bits(out[1].drop, dtype))
    assert torch.equal(out[0].dg, out[1].dg) and torch.equal(out[0].db, out[1].db)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [4, 252, 768])
def test_ln_param_reduce(H):
    """blocks in {1, 15, 16, 17, 512}; 33 sites (two launches), one of them without db; adds into what dg / db hold; identical twice"""
    gen = torch.Generator().manual_seed(H)
    nbs = [1, 15, 16, 17, 512] + [1 + (7 * i) % 40 for i in range(28)]
    assert len(nbs) == 33
    parts = [torch.randn(nb, 2, H, generator=gen).to(DEV) for nb in nbs]
    outs = []
    for _ in range(2):
        dgs, dbs = [acc_buffer(H) for _ in nbs], [acc_buffer(H) if i != 20 else None for i in range(33)]
        assert reduce_sites([(parts[i], dgs[i], dbs[i], nbs[i]) for i in range(33)], H) == 0, N.lib().om_last_error()
        outs.append((dgs, dbs))
    for i, nb in enumerate(nbs):
        ref = parts[i].double().sum(0) + PREFILL
        bound = (nb + 3) * u * (parts[i].double().abs().sum(0) + PREFILL)
        assert worst(outs[0][0][i][:H], ref[0], bound[0]) <= 1.0 and guard_ok(outs[0][0][i], H), (i, nb)
        assert torch.equal(outs[0][0][i], outs[1][0][i])
        if outs[0][1][i] is not None:
            assert worst(outs[0][1][i][:H], ref[1], bound[1]) <= 1.0 and guard_ok(outs[0][1][i], H) and torch.equal(outs[0][1][i], outs[1][1][i])


EMBED_CASES = [(L, B, H, var) for (L, B, H) in ((1, 9, 768), (5, 7, 768), (128, 3, 768), (256, 2, 4), (257, 3, 4), (300, 2, 768), (5, 3, 4), (5, 3, 1024),
                                                 (5, 3, 1028), (1, 5, 2048), (128, 32, 4))
               for var in (("plain", "types4", "cu") if (L, B, H) != (5, 7, 768) else
                           ("plain", "no_type_ids", "no_type_table", "type_vocab1", "types4", "bad_ids", "same_id", "cu"))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("L,B,H,var", EMBED_CASES, ids=[f"L{l}-B{b}-H{h}-{v}" for l, b, h, v in EMBED_CASES])
def test_embed_bwd(dtype, L, B, H, var):
    """ln_bwd_kernel MODE 1: one position per block, 256 / L blocks per position; the table gradients, dg and db add into pre-filled
    buffers with guards; ids and token types clamped; packed rows walk cu (lengths 0 and L included) and read no other row of dy"""
    td = TORCH_DT[dtype]
    M, vocab = B * L, 50
    tv = 1 if var == "type_vocab1" else 4 if var == "types4" else 2
    gen = torch.Generator().manual_seed(L * 1000 + H)
    word, pos = torch.randn(vocab, H, generator=gen).to(DEV), torch.randn(L, H, generator=gen).to(DEV)
    typ = None if var == "no_type_table" else torch.randn(tv, H, generator=gen).to(DEV)
    ids = torch.randint(0, vocab, (M,), generator=gen)
    if var == "bad_ids":
        ids[::3] = -4; ids[1::5] = vocab; ids[2::7] = vocab + 1000
    if var == "same_id":
        ids[:] = 17
    tts = None if var == "no_type_ids" else torch.randint(-1 if var == "bad_ids" else 0, (tv + 2) if var in ("bad_ids", "type_vocab1") else tv, (M,), generator=gen)
    ids, tts = ids.to(DEV), None if tts is None else tts.to(DEV)
    g, _ = make_affine(H, H, DEV)
    live, cu, rows = None, None, M
    if var == "cu":
        lens = torch.tensor([(0, L, max(1, L // 3), L - 1 if L > 1 else 1)[b % 4] for b in range(B)])
        cu_h = torch.zeros(B + 2, dtype=torch.int32)
        cu_h[1:B + 1] = lens.cumsum(0)
        cu_h[B + 1] = cu_h[B]
        cu, rows = cu_h.to(DEV), int(cu_h[B])
        live = (torch.arange(L)[None] < lens[:, None]).flatten().to(DEV)
    dy_pad = make_rows(M, H, H + L, DEV, spread=False).to(td)
    dy = dy_pad if live is None else torch.cat([dy_pad[live], torch.full((GUARD, H), float("nan"), device=DEV).to(td)])       # NaN behind cu[B]: read -> visible
    dword, dpos, dg, db = acc_buffer(vocab * H), acc_buffer(L * H), acc_buffer(H), acc_buffer(H)
    dtyp = None if typ is None else acc_buffer(tv * H)
    rc = N.lib().om_debug_embed_bwd(dtype, N.ptr(dy), N.ptr(ids), N.ptr(tts), N.ptr(word), N.ptr(pos), N.ptr(typ), N.ptr(g), N.ptr(dword),
                                    N.ptr(dpos), N.ptr(dtyp), N.ptr(dg), N.ptr(db), M, L, H, vocab, tv, EPS, N.ptr(cu), N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, N.lib().om_last_error()
    nv, waves = EMBED_VARIANT[H]
    assert last() == bwd_word(nv, 1, waves, False, False) == plan_bwd(dtype, 1, M, H, L=L)[0]
    d = lambda t: None if t is None else t.double()
    R = embed_backward(d(dy_pad), ids, tts, d(word), d(pos), d(typ), d(g), EPS, L, vocab, tv, live)
    bw, bp, bt, e_dg, e_db = embed_bwd_bound(R, H, M, d(word), d(pos), d(typ))
    ws = [worst(dword[:vocab * H].view(vocab, H), R.dword + PREFILL, bw), worst(dpos[:L * H].view(L, H), R.dpos + PREFILL, bp),
          worst(dg[:H], R.dg + PREFILL, e_dg), worst(db[:H], R.db + PREFILL, e_db)]
    if typ is not None:
        ws.append(worst(dtyp[:tv * H].view(tv, H), R.dtype + PREFILL, bt))
        assert guard_ok(dtyp, tv * H)
    assert max(ws) <= 1.0, (NAME[dtype], L, B, H, var, ws)
    assert guard_ok(dword, vocab * H) and guard_ok(dpos, L * H) and guard_ok(dg, H) and guard_ok(db, H)
    if var == "bad_ids":      # the forward hook clamps the same way: out-of-range ids and types give the bits of the clamped ones
        idc, ttc, _ = embed_rows(ids, tts, L, vocab, tv, True)
        outs = []
        for i_, t_ in ((ids, tts), (idc, ttc)):
            o = sentinel_rows(M, H, dtype)
            assert N.lib().om_debug_embed(dtype, N.ptr(i_), N.ptr(t_), N.ptr(word), N.ptr(pos), N.ptr(typ), N.ptr(g), N.ptr(g), N.ptr(o), M, L, H, vocab, tv,
                                          EPS, N.stream_ptr()) == 0
            torch.cuda.synchronize()
            outs.append(o)
        assert torch.equal(bits(outs[0], dtype), bits(outs[1], dtype)) and bool((ids != idc).any()) and bool((tts != ttc).any())
    if var == "plain" and L > 1:      # a position block that skipped a sequence, seen from the reference side: drop the last sequence
        keep = torch.ones(M, dtype=torch.bool, device=DEV); keep[(B - 1) * L:] = False
        assert worst(dpos[:L * H].view(L, H), embed_backward(d(dy_pad), ids, tts, d(word), d(pos), d(typ), d(g), EPS, L, vocab, tv, keep).dpos + PREFILL, bp) > 1.0


POOL_CASES = [(B, L, H) for (B, L, H) in ((1, 1, 4), (3, 7, 4), (3, 128, 4), (2049, 7, 4), (3, 7, 1024), (1, 128, 1028), (3, 1, 1028), (3, 128, 1024), (2049, 1, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("B,L,H", POOL_CASES)
def test_pool(dtype, B, L, H):
    """both modes, padded and packed, both directions: a fully masked sequence gives 0, a hole in the middle of a mask, pool_bwd writes
    all L rows when padded and exactly the sequence's rows when packed (the other rows keep the sentinel)"""
    td = TORCH_DT[dtype]
    gen = torch.Generator().manual_seed(B * 7 + L)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0] = L
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    if B > 1:
        mask[1] = 0; lens[1] = 0                                               # a fully masked sequence: packed length 0
    if B > 2 and L > 2:
        mask[2, :] = 1; mask[2, L // 2] = 0; lens[2] = L                      # a hole in the middle
    mask, lens_d = mask.to(DEV), lens.to(DEV)
    x = make_rows(B * L, H, H + B, DEV).to(td).view(B, L, H)
    dp = make_rows(B, H, H + B + 1, DEV, spread=False)
    for mode in (N.POOL_FIRST, N.POOL_MEAN):
        for packed in (False, True):
            # first-token pooling reads row cu[b] whatever the length: its packed case gives the empty sequence one row
            pl = lens.clamp_min(1) if mode == N.POOL_FIRST else lens
            cu_h = torch.zeros(B + 2, dtype=torch.int32)
            cu_h[1:B + 1] = pl.cumsum(0)
            cu_h[B + 1] = cu_h[B]
            cu, rows, pl_d = cu_h.to(DEV), int(cu_h[B]), pl.to(DEV)
            live = (torch.arange(L, device=DEV)[None] < pl_d[:, None])
            xp = torch.cat([x[live], torch.full((GUARD, H), float("nan"), device=DEV).to(td)])      # packed rows, NaN behind cu[B]
            out = sentinel_rows(B + GUARD, H, F32)
            rc = N.lib().om_debug_pool(dtype, N.ptr(xp if packed else x), N.ptr(mask), N.ptr(out), B, L, H, mode, N.ptr(cu if packed else None), N.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, N.lib().om_last_error()
            y, mag = pool_forward(x.double(), mask, pl_d if packed else torch.full_like(pl_d, L), mode)
            assert worst(out[:B], y, pool_fwd_bound(y, mag, L)) <= 1.0 and is_sentinel(out[B:], F32), (mode, packed)
            if mode == N.POOL_MEAN and B > 1:
                assert bool((out[1] == 0).all())                               # fully masked: 0, not NaN
            nrows = rows if packed else B * L
            dh = sentinel_rows(nrows + GUARD, H, dtype)
            rc = N.lib().om_debug_pool_bwd(dtype, N.ptr(dp), N.ptr(mask), N.ptr(dh), B, L, H, mode, N.ptr(cu if packed else None), N.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, N.lib().om_last_error()
            ref = pool_backward(dp.double(), mask, L, mode)
            ref = ref[live] if packed else ref.reshape(B * L, H)
            assert worst(dh[:nrows], ref, pool_bwd_bound(ref, dtype)) <= 1.0 and is_sentinel(dh[nrows:], dtype), (mode, packed)


def test_pool_bwd_split():
    """omk_pool_bwd's grid: min(L, 2048 / B) blocks per sequence, at least one -- what the B of POOL_CASES cross"""
    parts = lambda B, L: max(1, min(L, 2048 // B))
    assert [parts(B, L) for B, L, _ in POOL_CASES] == [1, 7, 128, 1, 7, 128, 1, 128, 1] and parts(2049, 7) == 1 and parts(2048, 7) == 1 and parts(1024, 7) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 4, 5])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 768])
def test_l2norm(D, M):
    x = l2_case_inputs(M, D).to(DEV)
    dy = make_rows(M, D, D + M, DEV, spread=False)
    y, dx = sentinel_rows(M + GUARD, D, F32), sentinel_rows(M + GUARD, D, F32)
    lib = N.lib()
    assert lib.om_debug_l2norm(N.ptr(x), N.ptr(y), M, D, N.stream_ptr()) == 0 and lib.om_debug_l2norm_bwd(N.ptr(x), N.ptr(dy), N.ptr(dx), M, D, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    yr, n = l2_forward(x.double())
    assert worst(y[:M], yr, l2_fwd_bound(yr, D)) <= 1.0 and is_sentinel(y[M:], F32)
    R = l2_backward(x.double(), dy.double())
    assert worst(dx[:M], R.dx, l2_bwd_bound(R, D)) <= 1.0 and is_sentinel(dx[M:], F32)
    if M > 2:
        assert bool((y[1] == 0).all()) and torch.equal(dx[1], dy[1] * 1e12) and torch.equal(dx[2], dy[2] * 1e12)     # zero row, clamped row
        assert torch.equal(y[2], x[2] / torch.tensor(1e-12, device=DEV))
    if D > 1:
        assert worst(dx[:1], l2_backward(x.double()[:1], dy.double()[:1], ctl="no_projection").dx, l2_bwd_bound(R, D)[:1]) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 255, 256, 257, 16385])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_colsum(dtype, M):
    """N in {1, 63, 64, 65} x ld in {N, N + 3}; the row split caps at 64 blocks (M = 16385: 257 rows per block); adds into out"""
    for Nc in (1, 63, 64, 65):
        for ld in (Nc, Nc + 3):
            x = make_rows(M, Nc, M + Nc, DEV).to(TORCH_DT[dtype])
            xbuf, xv = strided(x, ld)
            out = acc_buffer(Nc)
            assert N.lib().om_debug_colsum(dtype, N.ptr(xv), ld, M, Nc, N.ptr(out), N.stream_ptr()) == 0, N.lib().om_last_error()
            torch.cuda.synchronize()
            ref = x.double().sum(0) + PREFILL
            bound = (M + 6) * u * (x.double().abs().sum(0) + PREFILL)
            assert worst(out[:Nc], ref, bound) <= 1.0 and guard_ok(out, Nc), (M, Nc, ld)
            # control: a row split that loses its tail (the last row; at M = 16385, where the bound has grown with M, the last of the
            # 64 blocks' 257-row share) is outside the bound somewhere
            lost = 1 if M < 16385 else M - 63 * 257
            if M > 1:
                assert worst(out[:Nc], ref - x[M - lost:].double().sum(0), bound) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 255, 256, 257])
@pytest.mark.parametrize("nslots", [1, 6, 24])
def test_ln_stats_reduce(nslots, M):
    slots = make_rows(nslots * M, 2, M + nslots, DEV)
    outs = []
    for _ in range(2):
        out = sentinel_rows(M + GUARD, 2, F32)
        assert N.lib().om_debug_ln_stats_reduce(N.ptr(slots), nslots, M, N.ptr(out), N.stream_ptr()) == 0
        torch.cuda.synchronize()
        outs.append(out)
    s = slots.double().view(nslots, M, 2)
    assert worst(outs[0][:M], s.sum(0), (nslots + 1) * u * s.abs().sum(0) + 2.0 ** -149) <= 1.0 and is_sentinel(outs[0][M:], F32)
    assert torch.equal(outs[0], outs[1])
    seq = torch.zeros(M, 2, device=DEV)            # the slot order is the contract: the f32 sum in slot order, bit for bit
    for k in range(nslots):
        seq = seq + slots.view(nslots, M, 2)[k]
    assert torch.equal(outs[0][:M], seq)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 2.0 ** -17, 0.1, 0.5, 0.99999, 1.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_dropout_is_the_python_port(dtype, p):
    """element by element on bits; n % 4 != 0, and n = 8192 * 256 + 1 (the grid-stride loop wraps once) at p = 0.1"""
    td = TORCH_DT[dtype]
    seed = 0xDEADBEEFCAFEF00D
    for n in (1, 7, 1023, 4098) + ((8192 * 256 + 1,) if p == 0.1 else ()):
        x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.01 + 0.02).to(td).to(DEV)       # small: x 65536 stays finite in float16
        y = sentinel_rows(1, n + GUARD, dtype)[0]
        assert N.lib().om_debug_dropout(dtype, N.ptr(x), N.ptr(y), n, p, seed, None, 0, N.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(y[:n].cpu(), dtype), bits(dropout_port(x, p, seed), dtype)), (n, p)
        assert is_sentinel(y[n:], dtype)
        if p == 0.0:
            assert torch.equal(bits(y[:n], dtype), bits(x, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_dropout_rows_key_the_token(dtype):
    """with rows the key is (rows[r], c): the packed call carries the bits of the padded call at the same tokens; a negative entry is
    a key like any other"""
    td = TORCH_DT[dtype]
    H, B, L, p, seed = 68, 4, 9, 0.3, 12345
    lens = [9, 0, 4, 7]
    row_map = torch.tensor([b * L + t for b in range(B) for t in range(lens[b])] + [-1, -1], dtype=torch.int32)
    xpad = make_rows(B * L, H, 3, DEV).to(td)
    live = row_map >= 0
    xpk = torch.zeros(row_map.numel(), H, dtype=td, device=DEV)
    xpk[live.to(DEV)] = xpad[row_map[live].long().to(DEV)]
    xpk[~live.to(DEV)] = 1.0
    ypad, ypk = sentinel_rows(B * L, H, dtype), sentinel_rows(row_map.numel() + GUARD, H, dtype)
    assert call_dropout(dtype, xpad, ypad, p, seed) == 0
    assert N.lib().om_debug_dropout(dtype, N.ptr(xpk), N.ptr(ypk), xpk.numel(), p, seed, N.ptr(row_map.to(DEV)), H, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(ypk[:row_map.numel()][live.to(DEV)].contiguous(), dtype), bits(ypad[row_map[live].long().to(DEV)].contiguous(), dtype))
    assert torch.equal(bits(ypk[:row_map.numel()].cpu(), dtype), bits(dropout_port(xpk, p, seed, row_map, H), dtype)) and is_sentinel(ypk[row_map.numel():], dtype)
    wrong = dropout_port(xpk, p, seed, torch.arange(row_map.numel()), H)         # keyed on the packed row: not what the kernel draws
    assert not torch.equal(bits(ypk[:row_map.numel()].cpu(), dtype), bits(wrong, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("Nr,K", [(1, 8), (5, 64), (9, 520), (4, 768), (7, 2048)])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_ln_fold(dtype, Nr, K):
    """Wf is the f32 product rounded once (bits); colsum sums the ROUNDED Wf; bf = b + sum beta W; with beta and b NULL"""
    td = TORCH_DT[dtype]
    W = make_rows(Nr, K, K, DEV, spread=False).to(td)
    gamma, beta = make_affine(K, K, DEV)
    b = make_rows(1, Nr, K + 1, DEV, spread=False)[0].contiguous()
    for use_beta, use_b in ((True, True), (False, False), (True, False)):
        Wf = sentinel_rows(Nr + GUARD, K, dtype)
        cs, bf = sentinel_rows(1, Nr + GUARD, F32)[0], sentinel_rows(1, Nr + GUARD, F32)[0]
        rc = N.lib().om_debug_ln_fold(dtype, N.ptr(W), N.ptr(gamma), N.ptr(beta if use_beta else None), N.ptr(b if use_b else None), N.ptr(Wf), N.ptr(cs),
                                      N.ptr(bf), Nr, K, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, N.lib().om_last_error()
        want = (W.float() * gamma).to(td)
        assert torch.equal(bits(Wf[:Nr], dtype), bits(want, dtype)) and is_sentinel(Wf[Nr:], dtype)
        ref = want.double().sum(1)
        bound = (K + 2) * u * want.double().abs().sum(1) + 2.0 ** -149
        assert worst(cs[:Nr], ref, bound) <= 1.0 and is_sentinel(cs[Nr:], F32)
        if K == 64:
            assert worst(cs[:Nr], (W.double() * gamma.double()).sum(1), bound) > 1.0          # not the sum of the unrounded products
        t = (W.double() * beta.double()).sum(1) if use_beta else torch.zeros(Nr, dtype=torch.float64, device=DEV)
        refb = t + (b.double() if use_b else 0)
        boundb = (K + 3) * u * ((W.double() * beta.double()).abs().sum(1) if use_beta else 0) + u * refb.abs() + 2.0 ** -149
        assert worst(bf[:Nr], refb, boundb) <= 1.0 and is_sentinel(bf[Nr:], F32)


def measure_constants():
    """(rsqrt, divsqrt): the largest relative error of the float32 kernels on four-element rows whose scale sweeps 2^-10 .. 2^10
    (variance / squared norm 2^-20 .. 2^20)"""
    M, H = 4096, 4
    gen = torch.Generator().manual_seed(0)
    x = (torch.randn(M, H, generator=gen).abs() + 0.25) * (2.0 ** torch.linspace(-10, 10, M))[:, None]
    x = x.to(DEV)
    ones = torch.ones(H, device=DEV)
    y = torch.empty_like(x)
    assert call_fwd("layernorm", F32, x, H, y, H, ones, None, M, H, rms=1, eps=0.0) == 0
    torch.cuda.synchronize()
    ref = ln_forward(x.double(), ones.double(), None, 0.0, 1).y
    rsq = float(((y.double() - ref).abs() / ref.abs()).max())
    assert N.lib().om_debug_l2norm(N.ptr(x), N.ptr(y), M, H, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = l2_forward(x.double())[0]
    return rsq, float(((y.double() - ref).abs() / ref.abs()).max())


@pytest.mark.gpu
def test_math_constants_still_hold():
    rsq, dsq = measure_constants()
    print(f"measured: rsqrt path {rsq:.4e} ({rsq / u:.2f} u), sqrt + division path {dsq:.4e} ({dsq / u:.2f} u)")
    assert rsq <= RSQRT_MEASURED * 1.001 and dsq <= DIVSQRT_MEASURED * 1.001
    assert rsq >= RSQRT_MEASURED / 4 and dsq >= DIVSQRT_MEASURED / 4          # and the recorded figures are not slack by a wide margin
