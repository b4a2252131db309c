"""The weight-gradient contraction of csrc/gemm_tn.hip, kernel by kernel, against float64:

    C[N, K] += A[M, N]^T B[M, K]        bias[N] += sum_m A[m, :]        (A, B bfloat16 or float16; C, bias f32, accumulated into)

through om_gemm_tn_acc (gemm_tn_dma_kernel for whole 64-token steps, gemm_tn_kernel for ragged tails and short token axes) and
om_gemm_tn_acc_batch (gemm_tn_wide_kernel over whole 32-token steps, gemm_tn_kernel for the tail).  The harness is that of
tests/test_gemm_kernels.py and tests/test_gemm_epilogues.py (Buf with sentinel guard rows and columns, Frozen, guards_ok, assert_within,
rejected, violations, sync; option from tests/test_attention_kernels.py).

Reference and bound, both in float64 on the stored 16-bit values (u = 2^-24):
    ref   = C0 + A^T B          |C    - ref|   <= (M + slices + 2) u sum_m |a||b| + u |C0|
    ref_b = b0 + sum_m A        |bias - ref_b| <= (M + slices + 2) u sum_m |a|    + u |b0|
Products of two bfloat16 or two float16 values are exact in f32, so only additions round: M of them in ANY order, one per partial sum
that meets in the element (`slices`: DMA slices + register-staged slices, or 1 + 1 for the 256 x 256 kernel and its tail), the add into
what the buffer held.  It is the form tests/test_gemm_epilogues.py::splitk_reference uses.  Nothing in it is measured and no element is
excluded from a comparison.  C starts from random values, bias from PREFILL; A is randn, B is 0.5 randn + 0.1: asymmetric, with a
non-zero mean, so that a transposition or a dropped row cannot cancel.

Every GPU case asserts om_debug_gemm_tn_last -- which kernels ran, over how many rows, in how many slices -- against plan_single /
plan_batch below, a plain restatement of csrc/gemm_tn_plan.h that test_plan_table_without_a_gpu holds to om_debug_gemm_tn_plan at every
case and at the training shapes.

Which case reaches which pipeline shape (steps are per slice):
  gemm_tn_kernel       M 1 .. 320: 1 to 5 steps of one slice, ragged and whole last steps, both register sets      test_register_staged
                       M 1100 with OM_OPT_WGRAD_DEBUG 8: slices of 5, 5, 5 and 3 steps, the last ragged            test_register_staged
                       tails of 1, 31 and 37 rows behind the other two kernels                                      test_dma_*, test_wide_*
  gemm_tn_dma_kernel   M 512 (4 + 4), 613 (5 + 4, tail 37), 832 (5, 5, 3), 1088 (.., 2), 1344 (.., 1)             test_dma_and_tail
                       M 8448 with the grid aim set (value >> 4 = 1): 27 slices instead of 33                      test_dma_grid_aim
  strides              lda = N + 8, ldb = K + 72, pointers 8 elements in, ldc = K + 4, bias NULL                   test_strides_and_windows
  gemm_tn_wide_kernel  M 32 .. 224, 352: 1 to 7 and 11 steps (prologue shorter than the ring, its wrap, `issue` off)  test_wide
                       five problems of mixed shape, 10 tiles on 16 workgroups, some without bias                  test_wide_mixed_batch
                       49 problems: two launches                                                                    test_wide_two_launches
  non-finite values    one NaN in A, one +Inf in B, in each part                                                   test_nan_in_a, test_inf_in_b
  f16 subnormals       a column of A that holds only float16 subnormals, on each kernel                            test_f16_subnormal_bias_column
  fallback             omk_transpose x 2 + omk_gemm_splitk as train.hip composes them                              test_transpose_splitk_fallback

Bits: a batch call is bit-identical when repeated (one owner per tile, the tail at most one slice), and so is a single-slice
register-staged call; multi-slice calls meet in atomics and are held to the bound, two runs within the bound of each other.

Negative controls (test_bound_admits_an_emulated_kernel_and_rejects_the_controls, CPU, at every case's shape; the emulated kernel is
the reference accumulated in float32 in the kernel's slice order; a control runs wherever the shape has what it names: a tail, a
square output, more than one k tile).  Largest error / bound of each control at the shape where it is
smallest, recorded 2026-10-20 (bfloat16 and float16 agree to the digits given):
    last token dropped                         2.3     M 8448, 128 x 256 (one token of 8448: the bound grows with M, the control does not)
    first token of the tail dropped            161     M 1100, 256 x 128
    C overwritten instead of added to          8.9     M 8448, 128 x 256
    bias summed once per k tile (x ntk)        72      M 8448, 128 x 256
    output transposed (square shapes)          3.0e3   M 1344, 128 x 128
    B's rows rotated by 4 in every 16 tokens   202     M 8448, 128 x 256
Largest kernel error / bound on the MI355X, recorded 2026-10-20 (pytest -s prints every case's):
    gemm_tn_kernel alone       C 0.995 (M = 1: the one rounding of C0 + a b against u |C0| + 4 u |a||b|), 0.73 from M = 7 on; bias 0.004
    gemm_tn_dma_kernel + tail  C 0.002, bias below 0.001; strided operands 0.009; the grid-aim case below 0.001
    gemm_tn_wide_kernel + tail C 0.091, bias 0.008; the mixed batch 0.023
    f16 subnormal column       bias 0.002 on all three kernels: v_dot2_f32_f16 keeps float16 subnormals under the kernel's mode bits, so
                               tw_sum2<f16_t> stays as it is
    transposes + split-K       C 0.008
"""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import option
from tests.test_gemm_epilogues import Frozen, assert_within, guards_ok, rejected, splitk_slices, sync
from tests.test_gemm_kernels import BF16, DEV, F16, F32, NAME, TORCH_DT, U_ACC, Buf, violations
from tests.test_row_kernels import FAKE, PREFILL

u = U_ACC
DTS = [BF16, F16]
DT_IDS = ["bf16", "f16"]


# ---------------------------------------------------------------------------------------------------------------
# the plan, restated (csrc/gemm_tn_plan.h), in the words of om_debug_gemm_tn_last
# ---------------------------------------------------------------------------------------------------------------
def tn_split(steps, tiles, dbg):
    """slices of a token axis of `steps` steps: 320 workgroups (or the aim, dbg >> 4, in units of 64) over the tiles, at least four
    steps per slice; returns (slices, steps per slice)"""
    want = (dbg >> 4) * 64 if dbg >> 4 else 320
    slices = -(-want // tiles)
    if slices > steps // 4:
        slices = max(steps // 4, 1)
    per = -(-steps // slices)
    return -(-steps // per), per


def plan_single(M, Nn, K, lda=None, ldb=None, dbg=0):
    """om_gemm_tn_acc: [mask, DMA rows, DMA slices, DMA steps per slice, register-staged rows, its slices, its rows per slice, 0]"""
    lda, ldb = lda or Nn, ldb or K
    tiles = (Nn // 128) * (K // 128)
    whole = 0 if dbg & 8 else M // 64
    v = [0] * 8
    if whole >= 8 and 128 * lda < 2 ** 31 and 128 * ldb < 2 ** 31:
        v[1] = whole * 64
        v[2], v[3] = tn_split(whole, tiles, dbg)
    v[4] = M - v[1]
    if v[4]:
        v[5], per = tn_split(-(-v[4] // 64), tiles, dbg)
        v[6] = per * 64
    v[0] = (1 if v[1] else 0) | (2 if v[4] else 0)
    return v


def plan_batch(M, shapes):
    """om_gemm_tn_acc_batch over problems of (N, K) `shapes`: [mask, whole 32-token steps, tiles, chunk of the last launch, launches,
    tail rows, slices and rows per slice of the last problem's tail]"""
    steps, tail = M // 32, M % 32
    tiles = [(n // 256) * (k // 256) for n, k in shapes]
    launches = -(-len(shapes) // 48)
    v = [4 | (2 if tail else 0), steps, sum(tiles), -(-sum(tiles[48 * (launches - 1):]) // 8), launches, tail, 0, 0]
    if tail:
        n, k = shapes[-1]
        v[6], per = tn_split(1, (n // 128) * (k // 128), 0)
        v[7] = per * 64
    return v


def parts_single(M, Nn, K, lda=None, ldb=None, dbg=0):
    """the row ranges whose partial sums meet in an element, in launch order, and where the register-staged rows begin"""
    v = plan_single(M, Nn, K, lda, ldb, dbg)
    parts = [(s * v[3] * 64, min((s + 1) * v[3] * 64, v[1])) for s in range(v[2])]
    parts += [(v[1] + s * v[6], min(v[1] + (s + 1) * v[6], M)) for s in range(v[5])]
    return parts, (v[1] if v[4] else None)


def parts_batch(M):
    whole = M // 32 * 32
    return [(0, whole)] + ([(whole, M)] if M > whole else []), (whole if M > whole else None)


def hook_plan(dt, M, Nn, K, lda, ldb, batch):
    out = (C.c_int64 * 8)()
    rc = N.lib().om_debug_gemm_tn_plan(dt, M, Nn, K, lda, ldb, batch, out)
    return N.lib().om_last_error() if rc else list(out)


def last():
    out = (C.c_int64 * 8)()
    assert N.lib().om_debug_gemm_tn_last(out) == 0
    return list(out)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [(128, 128), (256, 128), (128, 256)]
REG_M = [1, 7, 63, 64, 65, 129, 200, 257, 320]
REG_STEPS = {1: 1, 7: 1, 63: 1, 64: 1, 65: 2, 129: 3, 200: 4, 257: 5, 320: 5}
DMA_M = {512: [4, 4], 613: [5, 4], 832: [5, 5, 3], 1088: [5, 5, 5, 2], 1344: [5, 5, 5, 5, 1]}      # M -> DMA steps of each slice
AIM_M, AIM_DBG = 8448, 1 << 4
WIDE_SHAPES = [(256, 256), (256, 512), (512, 256), (512, 512)]
WIDE_M = [32, 64, 96, 128, 160, 192, 224, 352, 33, 63, 191]
MIXED = [(256, 256, True), (256, 512, False), (512, 256, True), (512, 512, True), (256, 256, False)]      # (N, K, bias?)
MIXED_M = 97
STRIDE_M = [200, 613]


def single_cases():
    """(label, M, N, K, dbg, lda, ldb) of every om_gemm_tn_acc case"""
    for n, k in SHAPES:
        for M in REG_M:
            yield "regs", M, n, k, 0, n, k
        yield "regs-4-slices", 1100, n, k, 8, n, k
        for M in DMA_M:
            yield "dma", M, n, k, 0, n, k
        for M in STRIDE_M:
            yield "strides", M, n, k, 0, n + 8, k + 72
    yield "aim", AIM_M, 128, 256, AIM_DBG, 128, 256
    yield "aim-off", AIM_M, 128, 256, 0, 128, 256


def batch_cases():
    """(label, M, [(N, K)]) of every om_gemm_tn_acc_batch case"""
    for n, k in WIDE_SHAPES:
        for M in WIDE_M:
            yield "wide", M, [(n, k)]
    yield "mixed", MIXED_M, [(n, k) for n, k, _ in MIXED]
    yield "two-launches", 32, [(256, 256)] * 49


# ---------------------------------------------------------------------------------------------------------------
# float64 reference, bound, controls
# ---------------------------------------------------------------------------------------------------------------
def operands(dt, M, Nn, K, seed, device):
    gen = torch.Generator(device=device).manual_seed(seed)
    A = torch.randn(M, Nn, generator=gen, device=device).to(TORCH_DT[dt])
    B = (0.5 * torch.randn(M, K, generator=gen, device=device) + 0.1).to(TORCH_DT[dt])
    C0 = torch.randn(Nn, K, generator=gen, device=device) * 3
    return A, B, C0


def rot4(b):
    """B's rows rotated by four inside every 16-token group, rows past the end read as the zero fill: token m of A meets token
    16 g + (m + 4) % 16 of B"""
    M = b.shape[0]
    pad = torch.zeros(-(-M // 16) * 16, b.shape[1], dtype=b.dtype, device=b.device)
    pad[:M] = b
    return torch.roll(pad.view(-1, 16, b.shape[1]), -4, 1).reshape(-1, b.shape[1])[:M]


def tn_reference(A, B, C0, b0, slices, ctl=None, tail_start=None, ntk=1):
    """(ref, bound, ref_b, bound_b) in float64; ctl builds a negative control: 'last' the last token dropped, 'tail_first' the first
    token of the register-staged rows dropped, 'store' C overwritten, 'bias_ntk' the bias summed once per k tile, 'transposed' the
    product transposed, 'rot4' the B tokens of every 16-token group rotated by four"""
    a, b = A.double(), B.double()
    M = a.shape[0]
    c0 = C0.double()
    bound = (M + slices + 2) * u * (a.abs().t() @ b.abs()) + u * c0.abs()
    bound_b = (M + slices + 2) * u * a.abs().sum(0) + u * abs(b0)
    if ctl == "last":
        a, b = a[:-1], b[:-1]
    elif ctl == "tail_first":
        keep = torch.arange(M, device=a.device) != tail_start
        a, b = a[keep], b[keep]
    elif ctl == "rot4":
        b = rot4(b)
    prod = a.t() @ b
    if ctl == "transposed":
        prod = prod.t()
    ref = prod if ctl == "store" else c0 + prod
    ref_b = b0 + a.sum(0) * (ntk if ctl == "bias_ntk" else 1)
    return ref, bound, ref_b, bound_b


def emulate(A, B, C0, b0, parts):
    """the reference accumulated in float32 in the kernel's slice order: every part summed in f32 step by step (64 tokens), the parts
    added into C and the bias one after the other"""
    Cf = C0.float().clone()
    bf = torch.full((A.shape[1],), b0, dtype=torch.float32)
    for lo, hi in parts:
        acc = torch.zeros_like(Cf)
        bs = torch.zeros_like(bf)
        for s in range(lo, hi, 64):
            a, b = A[s:min(s + 64, hi)].float(), B[s:min(s + 64, hi)].float()
            acc = acc + a.t() @ b
            bs = bs + a.sum(0)
        Cf, bf = Cf + acc, bf + bs
    return Cf, bf


def control_shapes():
    """(label, M, N, K, parts, tail_start, k tiles) of every case, each shape once"""
    seen = set()
    for label, M, n, k, dbg, lda, ldb in single_cases():
        parts, tail = parts_single(M, n, k, lda, ldb, dbg)
        key = (M, n, k, tuple(parts))
        if key not in seen:
            seen.add(key)
            yield label, M, n, k, parts, tail, k // 128
    for label, M, shapes in batch_cases():
        for n, k in shapes:
            parts, tail = parts_batch(M)
            key = (M, n, k, tuple(parts))
            if key not in seen:
                seen.add(key)
                yield label, M, n, k, parts, tail, k // 256


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_bound_admits_an_emulated_kernel_and_rejects_the_controls(dt):
    worst = {}
    n_shapes = 0
    for label, M, n, k, parts, tail, ntk in control_shapes():
        n_shapes += 1
        A, B, C0 = operands(dt, M, n, k, 1000 + M, "cpu")
        ref, bound, ref_b, bound_b = tn_reference(A, B, C0, PREFILL, len(parts))
        got, got_b = emulate(A, B, C0, PREFILL, parts)
        assert not violations(got, ref, bound).any(), (label, M, n, k)
        assert not violations(got_b, ref_b, bound_b).any(), (label, M, n, k)
        ctls = ["last", "store", "rot4"] + (["tail_first"] if tail is not None else []) + (["transposed"] if n == k else []) + \
               (["bias_ntk"] if ntk > 1 else [])
        for ctl in ctls:
            c, _, cb, _ = tn_reference(A, B, C0, PREFILL, len(parts), ctl=ctl, tail_start=tail, ntk=ntk)
            if ctl == "bias_ntk":
                ok, ratio = rejected(ref_b, cb, bound_b), float(((cb - ref_b).abs() / bound_b).max())
            else:
                ok, ratio = rejected(ref, c, bound), float(((c - ref).abs() / bound).max())
            assert ok, (ctl, label, M, n, k, ratio)
            if ratio < worst.get(ctl, (float("inf"),))[0]:
                worst[ctl] = (ratio, M, n, k)
    assert n_shapes > 80 and set(worst) == {"last", "store", "rot4", "tail_first", "transposed", "bias_ntk"}
    print(f"control ratios {NAME[dt]}:", {c: f"{r:.3g} at M {M} {n}x{k}" for c, (r, M, n, k) in worst.items()})


def test_plan_table_without_a_gpu():
    """the Python restatement against om_debug_gemm_tn_plan: every case of this file and the training shapes; the hook leaves
    om_debug_gemm_tn_last alone"""
    before = last()
    n_cases = 0
    for dt in DTS:
        for label, M, n, k, dbg, lda, ldb in single_cases():
            with option(N.OPT_WGRAD_DEBUG, dbg):
                assert hook_plan(dt, M, n, k, lda, ldb, 0) == plan_single(M, n, k, lda, ldb, dbg), (label, M, n, k, dbg)
            n_cases += 1
        for label, M, shapes in batch_cases():
            if len(set(shapes)) == 1:
                assert hook_plan(dt, M, shapes[0][0], shapes[0][1], shapes[0][0], shapes[0][1], len(shapes)) == plan_batch(M, shapes), (label, M, shapes)
            for n, k in shapes:                                  # a mixed batch: problem by problem
                assert hook_plan(dt, M, n, k, n, k, 1) == plan_batch(M, [(n, k)]), (label, M, n, k)
            n_cases += 1
        for M in (9216, 4099):
            for n, k in ((768, 768), (768, 3072), (3072, 768), (2304, 768)):
                for dbg in (0, 8, 5 << 4):
                    with option(N.OPT_WGRAD_DEBUG, dbg):
                        assert hook_plan(dt, M, n, k, n, k, 0) == plan_single(M, n, k, dbg=dbg), (M, n, k, dbg)
                        assert hook_plan(dt, M, n, k, n, k, 24) == plan_batch(M, [(n, k)] * 24), (M, n, k)      # the tail ignores the switches
                assert hook_plan(dt, M, n, k, n, k, 49) == plan_batch(M, [(n, k)] * 49)
    assert n_cases > 150
    # what the tables above were written for
    for M, steps in REG_STEPS.items():
        assert plan_single(M, 128, 256) == [2, 0, 0, 0, M, 1, steps * 64, 0]
    assert plan_single(1100, 256, 128, dbg=8) == [2, 0, 0, 0, 1100, 4, 320, 0] and parts_single(1100, 256, 128, dbg=8)[0][-1] == (960, 1100)
    for M, per_slice in DMA_M.items():
        v = plan_single(M, 128, 128)
        assert v[:4] == [3 if M % 64 else 1, M // 64 * 64, len(per_slice), per_slice[0]] and v[4] == M % 64
        assert [(hi - lo) // 64 for lo, hi in parts_single(M, 128, 128)[0][:len(per_slice)]] == per_slice
    assert plan_single(AIM_M, 128, 256)[2:4] == [33, 4] and plan_single(AIM_M, 128, 256, dbg=AIM_DBG)[2:4] == [27, 5]
    assert plan_batch(MIXED_M, [(n, k) for n, k, _ in MIXED]) == [6, 3, 10, 2, 1, 1, 1, 64]
    assert plan_batch(32, [(256, 256)] * 49) == [4, 1, 49, 1, 2, 0, 0, 0]
    # the DMA kernel keeps its own, tighter pitch condition
    assert plan_single(1024, 128, 128, lda=1 << 24)[0] == 2 and hook_plan(BF16, 1024, 128, 128, 1 << 24, 128, 0)[0] == 2
    assert hook_plan(BF16, 0, 128, 128, 128, 128, 0) == [0] * 8
    assert last() == before


REFUSALS = [
    ("dtype", dict(dt=F32), b"16-bit operands with N and K multiples of 128 only"),
    ("N", dict(n=192), b"16-bit operands with N and K multiples of 128 only"),
    ("K", dict(k=64), b"16-bit operands with N and K multiples of 128 only"),
    ("lda-8", dict(lda=132), b"16-bit operands with N and K multiples of 128 only"),
    ("lda-2^25", dict(lda=1 << 25), b"below 2^25"),
    ("ldb-2^25", dict(ldb=1 << 25), b"below 2^25"),
    ("ldb-huge", dict(ldb=1 << 40), b"below 2^25"),
]


@pytest.mark.parametrize("name,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_single_refusals_come_before_any_launch(name, kw, text):
    """through the plan hook and through om_gemm_tn_acc with made-up addresses (no device is touched: the refusal comes first)"""
    lib = N.lib()
    dt, n, k = kw.get("dt", BF16), kw.get("n", 128), kw.get("k", 128)
    lda, ldb = kw.get("lda", n), kw.get("ldb", k)
    p = lambda i: C.c_void_p(FAKE + 4096 * i)
    for M in (1, 64, 4096):
        got = hook_plan(dt, M, n, k, lda, ldb, 0)
        assert isinstance(got, bytes) and text in got, got
        assert lib.om_gemm_tn_acc(dt, p(1), lda, p(2), ldb, p(3), k, p(4), M, n, k, None) != 0 and text in lib.om_last_error()
        assert last() == [0] * 8


def test_pitch_limit_is_the_32_bit_offset_of_the_register_staged_kernel():
    """TN_FETCH1 adds a_lane + ua in 32 bits: row 63 of a step, column block 3, second half -> 63 * ld * 2 + 112 bytes.  The largest
    admitted pitch keeps that below 2^32, the first refused one (2^25) does not keep 64 rows below it; the wrap itself starts at
    ld = 34 087 042"""
    top = (1 << 25) - 8
    assert 126 * top + 112 < 1 << 32 and isinstance(hook_plan(BF16, 64, 128, 128, top, top, 0), list)
    assert hook_plan(F16, 64, 128, 128, top, 128, 0) == [2, 0, 0, 0, 64, 1, 64, 0]
    assert 126 * 34087041 + 112 < 1 << 32 <= 126 * 34087042 + 112 and 34087042 > 1 << 25
    assert isinstance(hook_plan(BF16, 64, 128, 128, 1 << 25, 128, 0), bytes)
    # the batch entry already refused such a pitch (32 rows below 2^31 bytes), with its own message
    assert b"multiples of 256" in hook_plan(BF16, 64, 256, 256, 1 << 25, 256, 1)
    assert hook_plan(BF16, 64, 256, 256, top, top, 1) == [4, 2, 1, 1, 1, 0, 0, 0]


def test_batch_refusals_come_before_any_launch():
    lib = N.lib()
    text = b"16-bit operands with N and K multiples of 256 and at least 32 tokens only"
    p = lambda i: FAKE + 4096 * i
    for M, n, k, lda in ((31, 256, 256, 256), (64, 128, 256, 128), (64, 256, 384, 256), (64, 256, 256, 260)):
        got = hook_plan(BF16, M, n, k, lda, k, 1)
        assert isinstance(got, bytes) and text in got, got
        prob = (N.OmTnProblem * 1)(N.OmTnProblem(A=p(1), B=p(2), C=p(3), bias=p(4), lda=lda, ldb=k, ldc=k, N=n, K=k))
        assert lib.om_gemm_tn_acc_batch(BF16, prob, 1, M, None) != 0 and text in lib.om_last_error()
        assert last() == [0] * 8
    prob = (N.OmTnProblem * 1)(N.OmTnProblem(A=p(1) + 8, B=p(2), C=p(3), bias=None, lda=256, ldb=256, ldc=256, N=256, K=256))
    assert lib.om_gemm_tn_acc_batch(F16, prob, 1, 64, None) != 0 and b"16-byte aligned" in lib.om_last_error()
    assert lib.om_gemm_tn_acc(F16, C.c_void_p(p(1) + 8), 128, C.c_void_p(p(2)), 128, C.c_void_p(p(3)), 128, None, 64, 128, 128, None) != 0
    assert b"16-byte aligned" in lib.om_last_error() and last() == [0] * 8
    assert isinstance(hook_plan(BF16, 64, 256, 256, 256, 256, -1), bytes)


def test_hooks_are_bound():
    lib = N.lib()
    for name in ("om_debug_gemm_tn_plan", "om_debug_gemm_tn_last", "om_gemm_tn_acc", "om_gemm_tn_acc_batch"):
        assert name in N.exported_symbols() and hasattr(lib, name)
    assert lib.om_debug_gemm_tn_plan(BF16, 64, 128, 128, 128, 128, 0, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_gemm_tn_last(None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_gemm_tn_acc(BF16, None, 128, None, 128, None, 128, None, 64, 128, 128, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_abi_version() == 6


# ---------------------------------------------------------------------------------------------------------------
# GPU harness
# ---------------------------------------------------------------------------------------------------------------
def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def make_problem(dt, M, Nn, K, seed, lda=None, ldb=None, ldc=None, off=0, A=None, B=None, C0=None):
    """operands and outputs of one contraction in guarded buffers; A / B / C0 given: reuse those values"""
    if A is None:
        A, B, C0 = operands(dt, M, Nn, K, seed, DEV)
    p = NS(M=M, N=Nn, K=K, C0=C0, b0=PREFILL)
    p.A = Buf(dt, M, Nn, lda or Nn, pre=1, post=1, off=off, fill=A)
    p.B = Buf(dt, M, K, ldb or K, pre=1, post=1, off=off, fill=B)
    p.frozen = Frozen(A=p.A.flat, B=p.B.flat)
    fresh(p, ldc)
    return p


def fresh(p, ldc=None):
    """new output buffers holding C0 and PREFILL"""
    p.C = Buf(F32, p.N, p.K, ldc or p.K, fill=p.C0)
    p.bias = Buf(F32, 1, p.N, p.N, fill=torch.full((1, p.N), p.b0, device=DEV))
    p.snaps = (p.C.snapshot(), p.bias.snapshot())


def launch_single(dt, p, use_bias=True):
    with torch.cuda.device(DEV):
        rc = N.lib().om_gemm_tn_acc(dt, p.A.ptr(), p.A.ld, p.B.ptr(), p.B.ld, p.C.ptr(), p.C.ld, p.bias.ptr() if use_bias else None,
                                    p.M, p.N, p.K, N.stream_ptr(torch.device(DEV)))
    sync()
    assert rc == 0, N.lib().om_last_error()
    return last()


def launch_batch(dt, probs, M, use_bias=None):
    use_bias = use_bias or [True] * len(probs)
    arr = (N.OmTnProblem * len(probs))()
    for i, p in enumerate(probs):
        arr[i] = N.OmTnProblem(A=p.A.ptr(), B=p.B.ptr(), C=p.C.ptr(), bias=p.bias.ptr() if use_bias[i] else None, lda=p.A.ld, ldb=p.B.ld,
                               ldc=p.C.ld, N=p.N, K=p.K)
    with torch.cuda.device(DEV):
        rc = N.lib().om_gemm_tn_acc_batch(dt, arr, len(probs), M, N.stream_ptr(torch.device(DEV)))
    sync()
    assert rc == 0, N.lib().om_last_error()
    return last()


def check(label, p, slices, use_bias=True, ref=None):
    """C and bias against float64, element by element; guards; operands unchanged.  Returns the reference for a second run."""
    ref = ref or tn_reference(p.A.window, p.B.window, p.C0, p.b0, slices)
    guards_ok(label, (p.C, p.snaps[0]), (p.bias, p.snaps[1]))
    assert_within(f"{label} C", p.C.window, ref[0], ref[1])
    if use_bias:
        assert_within(f"{label} bias", p.bias.window[0], ref[2], ref[3])
    else:
        assert p.bias.outside_changed(p.snaps[1]) == 0 and bool((p.bias.window == p.b0).all()), f"{label}: a NULL bias was written"
    p.frozen.check(label)
    return ref


def run_single_case(dt, label, M, Nn, K, dbg=0, lda=None, ldb=None, ldc=None, off=0, use_bias=True):
    want = plan_single(M, Nn, K, lda, ldb, dbg)
    slices = want[2] + want[5]
    p = make_problem(dt, M, Nn, K, 7 * M + Nn + K // 128, lda, ldb, ldc, off)
    outs = []
    with option(N.OPT_WGRAD_DEBUG, dbg):
        for _ in range(2):
            assert launch_single(dt, p, use_bias) == want, (label, want)
            ref = check(f"{label}/{NAME[dt]}/M{M}/{Nn}x{K}", p, slices, use_bias, outs[0][2] if outs else None)
            outs.append((p.C.window.clone(), p.bias.window[0].clone(), ref))
            fresh(p, ldc)
    (c1, b1, ref), (c2, b2, _) = outs
    if slices == 1:
        assert same_bits(c1, c2) and same_bits(b1, b2), f"{label}: one slice, yet two runs differ"
    else:
        assert bool(((c1.double() - c2.double()).abs() <= ref[1]).all()) and bool(((b1.double() - b2.double()).abs() <= ref[3]).all())
    return want


# ---------------------------------------------------------------------------------------------------------------
# GPU: om_gemm_tn_acc
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", REG_M + [1100])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_register_staged(dt, shape, M):
    want = run_single_case(dt, "regs", M, shape[0], shape[1], dbg=8 if M == 1100 else 0)
    assert want[0] == 2 and want[5] == (4 if M == 1100 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("M", list(DMA_M))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_dma_and_tail(dt, shape, M):
    want = run_single_case(dt, "dma", M, shape[0], shape[1])
    assert want[0] == (3 if M % 64 else 1) and want[2] == len(DMA_M[M]) and want[4] == M % 64


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_dma_grid_aim(dt):
    want = run_single_case(dt, "aim", AIM_M, 128, 256, dbg=AIM_DBG)
    assert want[:4] == [1, AIM_M, 27, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "null-bias"])
@pytest.mark.parametrize("M", STRIDE_M)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_strides_and_windows(dt, shape, M, use_bias):
    """A and B as column windows of wider tensors (pointers 8 elements in: still 16-byte aligned), C with a padded pitch"""
    n, k = shape
    want = run_single_case(dt, "strides", M, n, k, lda=n + 8, ldb=k + 72, ldc=k + 4, off=8, use_bias=use_bias)
    assert want[0] == (3 if M == 613 else 2)


# ---------------------------------------------------------------------------------------------------------------
# GPU: om_gemm_tn_acc_batch
# ---------------------------------------------------------------------------------------------------------------
def run_batch_case(dt, label, M, specs, shared=False):
    """specs: (N, K, bias?) per problem; shared: every problem reads the first one's A and B values"""
    want = plan_batch(M, [(n, k) for n, k, _ in specs])
    slices = 1 + (1 if M % 32 else 0)
    probs = []
    for i, (n, k, _) in enumerate(specs):
        src = probs[0] if shared and probs else None
        probs.append(make_problem(dt, M, n, k, 31 * M + 5 * i + n // 256 + k // 128, ldc=k + 4,
                                  A=src and src.A.window, B=src and src.B.window, C0=src and src.C0))
    use_bias = [b for _, _, b in specs]
    outs = []
    for _ in range(2):
        assert launch_batch(dt, probs, M, use_bias) == want, (label, want)
        refs = [None] * len(probs)
        for i, p in enumerate(probs):
            if not (shared and i):
                refs[i] = check(f"{label}/{NAME[dt]}/M{M}/{p.N}x{p.K}", p, slices, use_bias[i], outs[0][i][2] if outs else None)
        outs.append([(p.C.window.clone(), p.bias.window[0].clone(), r) for p, r in zip(probs, refs)])
        if shared:                                                # the same operands: the same bits in every problem
            for i, p in enumerate(probs[1:], 1):
                guards_ok(label, (p.C, p.snaps[0]), (p.bias, p.snaps[1]))
                assert same_bits(outs[-1][i][0], outs[-1][0][0]) and same_bits(outs[-1][i][1], outs[-1][0][1]), f"{label}: problem {i} differs"
        for p in probs:
            fresh(p, p.K + 4)
    for (c1, b1, _), (c2, b2, _) in zip(*outs):
        assert same_bits(c1, c2) and same_bits(b1, b2), f"{label}: a batch call is not bit-identical when repeated"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("M", WIDE_M)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_wide(dt, shape, M):
    want = run_batch_case(dt, "wide", M, [(shape[0], shape[1], True)])
    assert want[0] == (6 if M % 32 else 4) and want[1] == M // 32 and want[5] == M % 32


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_wide_mixed_batch(dt):
    """five problems, ten tiles on sixteen workgroups (the chunk walk, empty trailing workgroups), two without a bias, one tail row"""
    want = run_batch_case(dt, "mixed", MIXED_M, MIXED)
    assert want[2] % 8 != 0 and want[:6] == [6, 3, 10, 2, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_wide_two_launches(dt):
    want = run_batch_case(dt, "two-launches", 32, [(256, 256, True)] * 49, shared=True)
    assert want[4] == 2 and want[2] == 49


# ---------------------------------------------------------------------------------------------------------------
# GPU: non-finite values
# ---------------------------------------------------------------------------------------------------------------
NF_SINGLE = (613, 128, 256)      # DMA slices of 5 and 4 steps, a ragged tail of 37 rows from row 576
NF_BATCH = (63, 256, 512)        # one 32-token step of the 256 x 256 kernel, a ragged tail of 31 rows from row 32
NF_N, NF_K = 77, 200
NF_WHERE = [("dma", "single", 100), ("tail", "single", 600), ("tail-first-row", "single", 576), ("wide", "batch", 5),
            ("wide-tail", "batch", 40), ("wide-tail-first-row", "batch", 32)]


def run_non_finite(dt, kind, m, poison):
    """one poisoned element; the reference is built on the clean operands and the expected row / column marked by hand"""
    M, n, k = NF_SINGLE if kind == "single" else NF_BATCH
    A, B, C0 = operands(dt, M, n, k, 400 + m, DEV)
    Ap, Bp = A.clone(), B.clone()
    if poison == "nan":
        Ap[m, NF_N] = float("nan")
        A[m, NF_N] = 0
    else:
        Bp[m, NF_K] = float("inf")
        B[m, NF_K] = 0
    p = make_problem(dt, M, n, k, 0, ldc=k + 4, A=Ap, B=Bp, C0=C0)
    if kind == "single":
        want = plan_single(M, n, k)
        slices = want[2] + want[5]
        assert launch_single(dt, p) == want and want[0] == 3
    else:
        want, slices = plan_batch(M, [(n, k)]), 2
        assert launch_batch(dt, [p], M) == want and want[0] == 6
    ref, bound, ref_b, bound_b = tn_reference(A, B, C0, PREFILL, slices)
    guards_ok(poison, (p.C, p.snaps[0]), (p.bias, p.snaps[1]))
    p.frozen.check(poison)
    return p, ref, bound, ref_b, bound_b


@pytest.mark.gpu
@pytest.mark.parametrize("where,kind,m", NF_WHERE, ids=[w[0] for w in NF_WHERE])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_nan_in_a(dt, where, kind, m):
    """one NaN at A[m, n]: exactly row n of C and bias[n] are NaN, every other element inside its bound"""
    p, ref, bound, ref_b, bound_b = run_non_finite(dt, kind, m, "nan")
    ref[NF_N, :] = float("nan")
    ref_b[NF_N] = float("nan")
    assert bool(torch.isnan(p.C.window[NF_N]).all()) and bool(torch.isnan(p.bias.window[0, NF_N]))
    assert_within(f"nan/{where} C", p.C.window, ref, bound)
    assert_within(f"nan/{where} bias", p.bias.window[0], ref_b, bound_b)


@pytest.mark.gpu
@pytest.mark.parametrize("where,kind,m", NF_WHERE, ids=[w[0] for w in NF_WHERE])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_inf_in_b(dt, where, kind, m):
    """one +Inf at B[m, k]: column k of C is non-finite, every other column and the bias inside their bounds.  At the first row of a
    ragged step the row is also the stand-in the zero-filled rows load, where 0 x Inf arises: which non-finite value comes back is
    recorded (pytest -s), only that nothing finite turns non-finite and nothing non-finite finite is required"""
    p, ref, bound, ref_b, bound_b = run_non_finite(dt, kind, m, "inf")
    col = p.C.window[:, NF_K]
    print(f"inf/{where}/{NAME[dt]}: column {NF_K} holds {int(torch.isnan(col).sum())} NaN, {int(torch.isinf(col).sum())} Inf of {col.numel()}")
    assert not bool(torch.isfinite(col).any()), "a non-finite column came back finite"
    got = p.C.window.clone()
    got[:, NF_K] = 0
    ref[:, NF_K] = 0
    assert_within(f"inf/{where} C", got, ref, bound)
    assert_within(f"inf/{where} bias", p.bias.window[0], ref_b, bound_b)


# ---------------------------------------------------------------------------------------------------------------
# GPU: float16 subnormals in the bias column sum
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel,M,n,k", [("regs", 200, 128, 256), ("dma", 512, 128, 256), ("wide", 64, 256, 256)], ids=["regs", "dma", "wide"])
def test_f16_subnormal_bias_column(kernel, M, n, k):
    """a column of A that holds only positive float16 subnormals (1 .. 1023 times 2^-24): tn_sum8 converts each value, tw_sum2<f16_t>
    is a v_dot2_f32_f16 against (1, 1).  The float64 reference keeps the subnormals; so must the kernels: a flushed column is a bias
    gradient that is silently zero under a small loss scale"""
    col = 70
    A, B, C0 = operands(F16, M, n, k, 900 + M, DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    A[:, col] = (torch.randint(1, 1024, (M,), generator=gen, device=DEV).double() * 2.0 ** -24).to(torch.float16)
    assert bool((A[:, col] > 0).all()) and float(A[:, col].max()) < 2.0 ** -14
    p = make_problem(F16, M, n, k, 0, A=A, B=B, C0=C0)
    if kernel == "wide":
        got, slices = launch_batch(F16, [p], M), 1
        assert got == plan_batch(M, [(n, k)]) and got[0] == 4
    else:
        got = launch_single(F16, p)
        slices = got[2] + got[5]
        assert got == plan_single(M, n, k) and got[0] == (1 if kernel == "dma" else 2)
    ref = check(f"subnormal/{kernel}", p, slices)
    print(f"subnormal/{kernel}: bias[{col}] = {float(p.bias.window[0, col]):.6e}, float64 {float(ref[2][col]):.6e}")
    assert float(ref[2][col]) > 2.0 ** -126 * 2 ** 100             # a normal f32 by a wide margin


# ---------------------------------------------------------------------------------------------------------------
# GPU: the fallback path, omk_transpose x 2 + omk_gemm_splitk as train.hip composes them
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_transpose_splitk_fallback(dt):
    lib = N.lib()
    M, n, k = 200, 128, 256
    Mp = (M + 63) // 64 * 64                                       # train.hip: M rounded up to the split-K step of 64 tokens
    A, B, C0 = operands(dt, M, n, k, 77, DEV)
    slices = splitk_slices(n, k, Mp, 2)[0]
    ref, bound, _, _ = tn_reference(A, B, C0, 0.0, slices)
    frozen = Frozen(A=A, B=B)
    tl, tr = Buf(dt, n, Mp, Mp), Buf(dt, k, Mp, Mp)
    Cb = Buf(F32, n, k, k, fill=C0)
    snaps = (tl.snapshot(), tr.snapshot(), Cb.snapshot())
    s = N.stream_ptr(torch.device(DEV))
    with torch.cuda.device(DEV):
        assert lib.om_debug_transpose(dt, N.ptr(A), n, M, n, tl.ptr(), Mp, Mp, 0, s) == 0, lib.om_last_error()
        assert lib.om_debug_transpose(dt, N.ptr(B), k, M, k, tr.ptr(), Mp, Mp, 0, s) == 0, lib.om_last_error()
        assert lib.om_debug_gemm_splitk(dt, tl.ptr(), Mp, tr.ptr(), Mp, Cb.ptr(), k, n, k, Mp, s) == 0, lib.om_last_error()
    sync()
    guards_ok("fallback", (tl, snaps[0]), (tr, snaps[1]), (Cb, snaps[2]))
    frozen.check("fallback")
    assert torch.equal(tl.window[:, :M], A.t()) and bool((tl.window[:, M:].view(torch.int16) == 0).all())
    assert_within(f"fallback/{NAME[dt]}", Cb.window, ref, bound)
    assert rejected(ref, tn_reference(A, B, C0, 0.0, slices, ctl="last")[0], bound)
