"""om_gemm_nt kernel by kernel: every tile generation of csrc/gemm*.hip against a float64 reference of
act(A B^T + bias) (+|x) resid on the exact stored (rounded) inputs, element by element, within a bound derived from
the arithmetic -- output rounding, f32 accumulation, the activation's documented approximation, a subnormal floor.

Every GPU case names the kernel family it must reach and asserts it through om_debug_gemm_last(); every case also
carries a negative control on the reference side (the last K step dropped, the bias shifted by one column) that the
bound must reject, so the tolerance cannot quietly become vacuous.  Memory outside the M x N window of C (guard rows,
the ldc padding) and the inputs must come back bit-unchanged.
"""
import contextlib
import math

import pytest
import torch

from openmatch_amd import native as N

DEV = "cuda:0"
F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
BITS_DT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}        # half an ulp, relative
FLOOR = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -24}     # subnormal spacing (f16: 2^-24)
U_ACC = 2.0 ** -24
PHI_FIT = 7.4e-6               # |error| of the fitted Phi of the 16-bit erf-GELU (gemm_epilogue.h / gemm_epilogue6.h)
GELU_LIP = 1.13                # max |gelu'| (erf and tanh forms): how far an accumulation error can move the activation
FAM = N.GEMM_FAMILY
SENTINEL = {F32: 0x5A5A5A5A, BF16: 0x5A5A, F16: 0x5A5A}

# epilogue name -> (act code, bias?, resid mode None | "add" | "mul" | "inplace")
EPI = {
    "none": (N.ACT_NONE, False, None),
    "bias": (N.ACT_NONE, True, None),
    "erf": (N.ACT_GELU_ERF, True, None),
    "relu": (N.ACT_RELU, True, None),
    "tanh": (N.ACT_GELU_TANH, True, None),
    "add": (N.ACT_NONE, True, "add"),
    "mul": (N.ACT_GELU_TANH, True, "mul"),
    "none_mul": (N.ACT_NONE, True, "mul"),                    # the backward through GELU with a gelu' tape: (A B^T + bias) x resid
    "inplace": (N.ACT_NONE, True, "inplace"),
    # combinations of the ported self-test lists
    "erf_add": (N.ACT_GELU_ERF, True, "add"),
    "relu_add": (N.ACT_RELU, True, "add"),
    "mul_nobias": (N.ACT_GELU_TANH, False, "mul"),
}
MAIN_EPI = ["none", "bias", "erf", "relu", "tanh", "add", "mul", "none_mul", "inplace"]


# ---------------------------------------------------------------------------------------------------------------
# float64 reference and error bound (pure torch: the CPU tests below check them on emulated roundings)
# ---------------------------------------------------------------------------------------------------------------
def act64(act, x):
    if act == N.ACT_GELU_ERF:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == N.ACT_RELU:
        return torch.where(x < 0, torch.zeros_like(x), x)           # relu(NaN) = NaN, as torch.relu
    if act == N.ACT_GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return x


def gemm_reference(A, B, bias, resid, act, mul, k_used=None, bias_shift=0):
    """float64 act(A[:, :k] B[:, :k]^T + bias) (+|x) resid on the stored values; returns (out, acc, mag, y).
    k_used / bias_shift build the negative controls (a K step dropped, the bias one column off)."""
    a, b = A.double(), B.double()
    if k_used is not None:
        a, b = a[:, :k_used], b[:, :k_used]
    acc = a @ b.t()
    mag = a.abs() @ b.abs().t()                                # sum_k |a_ik| |b_jk|
    if bias is not None:
        bb = bias.double()
        if bias_shift:
            bb = torch.roll(bb, bias_shift)
        acc = acc + bb
        mag = mag + bb.abs()
    y = act64(act, acc)
    if resid is None:
        out = y
    else:
        r = resid.double()
        out = y * r if mul else y + r
    return out, acc, mag, y


def error_bound(acc, mag, y, resid, act, mul, K, out_dtype, fast_act=True):
    """Per-element bound on |kernel - float64 reference|: output rounding u_out (|act(acc)| + |r|), f32 accumulation
    (K + 2) 2^-24 sum|a||b| (through the activation's slope), the activation's approximation, and a subnormal floor."""
    u = U_OUT[out_dtype]
    acc_err = (K + 2) * U_ACC * mag
    if act in (N.ACT_GELU_ERF, N.ACT_GELU_TANH):
        acc_err = acc_err * GELU_LIP
    act_err = torch.zeros_like(acc)
    if act == N.ACT_GELU_ERF:
        act_err = acc.abs() * (PHI_FIT if fast_act else 8 * U_ACC)
    elif act == N.ACT_GELU_TANH:
        act_err = acc.abs() * 16 * U_ACC                      # tanhf and the cubic in f32
    prop = acc_err + act_err
    if resid is None:
        rnd = u * y.abs()
    else:
        r = resid.double().abs()
        if mul:
            rnd, prop = u * (y.abs() * r), prop * r
        else:
            rnd = u * (y.abs() + r)
    return rnd + prop * (1 + u) + FLOOR[out_dtype]          # (1 + u): the rounding of a value already off by `prop`


def round_to(x64, dtype_code):
    """float64 -> the stored format -> float64 (round to nearest even, overflow to inf: torch's own conversion)."""
    return x64.to(TORCH_DT[dtype_code]).double()


def violations(got, ref, bound, out_dtype=None):
    """Elements farther than `bound` from the EXACT float64 reference.  Which elements must be non-finite is decided by the
    reference converted to the output format (out_dtype; none: as given): a value that rounds past the format's range must
    come back as that same infinity, a NaN as a NaN, and nothing finite may turn non-finite."""
    got = got.double()
    stored = ref if out_dtype is None else round_to(ref, out_dtype)
    fin = torch.isfinite(stored)
    bad = fin & ~(torch.isfinite(got) & ((got - ref).abs() <= bound))
    bad |= ~fin & torch.isfinite(got)
    bad |= torch.isinf(stored) & (got != stored) & ~torch.isnan(got)
    return bad


def controls_rejected(A, B, bias, resid, act, mul, K, k_step, out_dtype, fast_act, bound_of_ref):
    """The negative controls: the reference with its last K step removed, and with the bias shifted by one column.
    Returns the names of the controls the bound FAILED to reject (must be empty)."""
    ref = gemm_reference(A, B, bias, resid, act, mul)[0]
    fin = torch.isfinite(ref) & torch.isfinite(bound_of_ref)
    missed = []
    ctl = {"k_step": gemm_reference(A, B, bias, resid, act, mul, k_used=K - k_step)[0]}
    if bias is not None and bias.numel() > 1:
        ctl["bias_shift"] = gemm_reference(A, B, bias, resid, act, mul, bias_shift=1)[0]
    for name, c in ctl.items():
        if not bool((((c - ref).abs() > bound_of_ref) & fin).any()):
            missed.append(name)
    return missed


# ---------------------------------------------------------------------------------------------------------------
# CPU tests of the helpers
# ---------------------------------------------------------------------------------------------------------------
def _emulated(A, B, bias, resid, act, mul, out_dtype):
    """A kernel emulated on the CPU: products summed in f32 in k order, the activation in f32, one rounding."""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    a, b = A.float(), B.float()
    for k in range(A.shape[1]):
        acc = acc + a[:, k:k + 1] * b[:, k][None, :]
    if bias is not None:
        acc = acc + bias.float()
    y = act64(act, acc.double()).float()
    if resid is not None:
        y = y * resid.float() if mul else y + resid.float()
    return y.to(TORCH_DT[out_dtype])


@pytest.mark.parametrize("in_dt,out_dt", [(BF16, BF16), (F16, F16), (F16, F32), (F32, F32), (F32, BF16)])
@pytest.mark.parametrize("epi", MAIN_EPI)
def test_bound_accepts_emulated_kernel_and_rejects_controls(in_dt, out_dt, epi):
    act, has_bias, rmode = EPI[epi]
    g = torch.Generator().manual_seed(3)
    M, Nn, K = 9, 24, 128
    A = torch.randn(M, K, generator=g).to(TORCH_DT[in_dt])
    B = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).to(TORCH_DT[in_dt])
    bias = torch.randn(Nn, generator=g) if has_bias else None
    resid = torch.randn(M, Nn, generator=g).to(TORCH_DT[out_dt]) if rmode else None
    mul = rmode == "mul"
    got = _emulated(A, B, bias, resid, act, mul, out_dt)
    ref, acc, mag, y = gemm_reference(A, B, bias, resid, act, mul)
    bound = error_bound(acc, mag, y, resid, act, mul, K, out_dt)
    assert not violations(got, ref, bound, out_dt).any()
    k_step = 128 // (4 if in_dt == F32 else 2)
    assert controls_rejected(A, B, bias, resid, act, mul, K, k_step, out_dt, True, bound) == []
    # one element off by two ulps of the output format is caught
    bad = got.clone()
    bad[4, 7] = (ref[4, 7] + 2 * bound[4, 7] + 4 * U_OUT[out_dt] * ref[4, 7].abs()).to(bad.dtype)
    assert violations(bad, ref, bound, out_dt)[4, 7]


def test_bound_requires_matching_non_finite_values():
    ref = torch.tensor([1.0, float("inf"), float("-inf"), float("nan"), 2.0], dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    ok = torch.tensor([1.0, float("inf"), float("-inf"), float("nan"), 2.0])
    assert not violations(ok, ref, bound).any()
    # a saturated overflow (65504 instead of inf), a NaN turned into 0, a spurious NaN: each is caught
    assert violations(torch.tensor([1.0, 65504.0, float("-inf"), float("nan"), 2.0]), ref, bound).tolist() == [0, 1, 0, 0, 0]
    assert violations(torch.tensor([1.0, float("inf"), float("-inf"), 0.0, 2.0]), ref, bound).tolist() == [0, 0, 0, 1, 0]
    assert violations(torch.tensor([1.0, float("inf"), float("-inf"), float("nan"), float("nan")]), ref, bound).tolist() == [0, 0, 0, 0, 1]
    assert violations(torch.tensor([1.0, float("-inf"), float("-inf"), float("nan"), 2.0]), ref, bound).tolist() == [0, 1, 0, 0, 0]


def test_float16_rounding_overflows_at_65520():
    x = torch.tensor([65504.0, 65519.0, 65520.0, -65520.0], dtype=torch.float64)
    assert round_to(x, F16).tolist() == [65504.0, 65504.0, float("inf"), float("-inf")]


def test_relu_reference_keeps_nan():
    x = torch.tensor([float("nan"), -1.0, 2.0, float("-inf")], dtype=torch.float64)
    y = act64(N.ACT_RELU, x)
    assert math.isnan(y[0]) and y[1:].tolist() == [0.0, 2.0, 0.0]
    assert math.isnan(torch.relu(torch.tensor([float("nan")]))[0])        # what the reference model does


def test_gemm_debug_hooks_are_bound():
    lib = N.lib()
    before = lib.om_debug_option_value(N.OPT_GEMM_GROUP_M)
    try:
        N.check(lib.om_debug_option(N.OPT_GEMM_GROUP_M, 13))
        assert lib.om_debug_option_value(N.OPT_GEMM_GROUP_M) == 13
    finally:
        N.check(lib.om_debug_option(N.OPT_GEMM_GROUP_M, before))
    assert lib.om_debug_option_value(N.OPT_GEMM_GROUP_M) == before
    assert lib.om_debug_option_value(10 ** 6) == -1
    # a refused call launches nothing and says so
    assert lib.om_gemm_nt(F32, 16, 33, 16, 33, F32, 16, 8, 4, 8, 33, None, None, 0, 0, None) != 0
    assert lib.om_debug_gemm_last() == 0


# ---------------------------------------------------------------------------------------------------------------
# GPU harness
# ---------------------------------------------------------------------------------------------------------------
_OPTS = {"variant": N.OPT_GEMM_VARIANT, "cont": N.OPT_GEMM_CONT, "skinny_m": N.OPT_GEMM_SKINNY_M,
         "group_m": N.OPT_GEMM_GROUP_M, "max_grid": N.OPT_GEMM_MAX_GRID}


@contextlib.contextmanager
def gemm_options(gen=None, **kw):
    """Set the GEMM run-time switches (and om_debug_gemm_gen) for a block; restore exactly the values read back before."""
    lib = N.lib()
    saved = {k: lib.om_debug_option_value(o) for k, o in _OPTS.items()}
    try:
        for k, v in kw.items():
            N.check(lib.om_debug_option(_OPTS[k], int(v)))
        if gen is not None:
            lib.om_debug_gemm_gen(int(gen))
        yield
    finally:
        for k, v in saved.items():
            N.check(lib.om_debug_option(_OPTS[k], v))
        if gen is not None:
            lib.om_debug_gemm_gen(0)


def _bits(t):
    return t.view(BITS_DT[{torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[t.dtype]])


def _start(ld, pre, off):
    """Element offset of a Buf's window inside its flat buffer."""
    return pre * ld + off


class Buf:
    """A strided matrix inside a flat buffer filled with a sentinel: rows * ld elements, `pre` guard rows before and
    `post` after, `off` extra elements of misalignment.  `window` is the [rows, cols] view the kernel may touch."""

    def __init__(self, dtype_code, rows, cols, ld, pre=1, post=2, off=0, fill=None):
        self.code, self.rows, self.cols, self.ld = dtype_code, rows, cols, ld
        self.start = _start(ld, pre, off)
        total = (pre + rows + post) * ld + off + 8
        self.flat = torch.empty(total, dtype=TORCH_DT[dtype_code], device=DEV)
        _bits(self.flat).fill_(SENTINEL[dtype_code] - (1 << 32 if dtype_code == F32 and SENTINEL[dtype_code] >= 1 << 31 else 0))
        self.window = self.flat.as_strided((rows, cols), (ld, 1), self.start)
        if fill is not None:
            self.window.copy_(fill)

    def ptr(self):
        return self.flat.data_ptr() + self.start * self.flat.element_size()

    def snapshot(self):
        return _bits(self.flat).clone()

    def outside_changed(self, snap):
        mask = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        mask.as_strided((self.rows, self.cols), (self.ld, 1), self.start).fill_(False)
        return int(((_bits(self.flat) != snap) & mask).sum().item())


def _rand(gen, shape, scale=1.0):
    return torch.randn(*shape, generator=gen, device=DEV, dtype=torch.float32) * scale


def k_step_of(in_dt):
    return 128 // (4 if in_dt == F32 else 2)


def run_gemm(in_dt, out_dt, A, B, C, bias, resid_ptr, ldr, act, stream=None):
    lib = N.lib()
    with torch.cuda.device(DEV):
        rc = lib.om_gemm_nt(in_dt, A.ptr(), A.ld, B.ptr(), B.ld, out_dt, C.ptr(), C.ld, C.rows, C.cols, A.cols,
                            N.c_void_p(bias) if bias else None, N.c_void_p(resid_ptr) if resid_ptr else None, ldr, act,
                            N.stream_ptr(torch.device(DEV)))
    N.check(rc)
    torch.cuda.synchronize()
    return lib.om_debug_gemm_last()


def make_case(in_dt, out_dt, M, Nn, K, epi, seed, lda=None, ldb=None, ldc=None, ldr=None, a_slice=False,
              bias_off=0, c_off=0, r_off=0):
    """Inputs of one case, stored exactly as the kernel will read them."""
    act, has_bias, rmode = EPI[epi]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    lda = lda or K
    ldb = ldb or K
    ldc = ldc or Nn
    if a_slice:                                               # a column slice of a [M, 3K] matrix
        full = Buf(in_dt, M, 3 * K, 3 * K, pre=0, post=0, fill=_rand(gen, (M, 3 * K)))
        A = Buf(in_dt, M, K, 3 * K, pre=0, post=0)
        A.flat, A.start = full.flat, K
        A.window = full.flat.as_strided((M, K), (3 * K, 1), K)
    else:
        A = Buf(in_dt, M, K, lda, pre=0, post=0, fill=_rand(gen, (M, K)))
    B = Buf(in_dt, Nn, K, ldb, pre=0, post=0, fill=_rand(gen, (Nn, K), 1.0 / math.sqrt(K)))
    bias = None
    if has_bias:
        bias_buf = torch.zeros(Nn + 4, dtype=torch.float32, device=DEV)
        bias_buf[bias_off:bias_off + Nn] = _rand(gen, (Nn,))
        bias = bias_buf[bias_off:bias_off + Nn]
    R = None
    if rmode in ("add", "mul"):
        ldr = ldr or Nn
        R = Buf(out_dt, M, Nn, ldr, pre=0, post=1, off=r_off, fill=_rand(gen, (M, Nn)))
    C = Buf(out_dt, M, Nn, ldc, off=c_off)
    if rmode == "inplace":
        C.window.copy_(_rand(gen, (M, Nn)))
        R = C
    return dict(A=A, B=B, C=C, bias=bias, R=R, act=act | (N.ACT_MUL_RESID if rmode == "mul" else 0),
                mul=rmode == "mul", base_act=act, in_dt=in_dt, out_dt=out_dt, K=K)


def launch(case):
    R = case["R"]
    return run_gemm(case["in_dt"], case["out_dt"], case["A"], case["B"], case["C"],
                    case["bias"].data_ptr() if case["bias"] is not None else 0,
                    R.ptr() if R is not None else 0, R.ld if R is not None else 0, case["act"])


def check_case(case, family, label, controls=True):
    """Launch once, assert the family, the float64 bound, the negative controls and the untouched memory.
    Returns C's window (for bit comparisons between runs)."""
    A, B, C, R = case["A"], case["B"], case["C"], case["R"]
    in_dt, out_dt, K = case["in_dt"], case["out_dt"], case["K"]
    resid_before = R.window.clone() if R is not None else None       # in place: the resid the kernel reads
    snaps = {"A": (A, A.snapshot()), "B": (B, B.snapshot()), "C": (C, C.snapshot())}
    if R is not None and R is not C:
        snaps["R"] = (R, R.snapshot())
    got_family = launch(case)
    assert got_family == FAM[family], f"{label}: ran family {got_family}, expected {family} ({FAM[family]})"
    for name, (buf, snap) in snaps.items():
        if name == "C":
            assert buf.outside_changed(snap) == 0, f"{label}: C written outside its M x N window"
        else:
            assert torch.equal(_bits(buf.flat), snap), f"{label}: input {name} modified"
    ref, acc, mag, y = gemm_reference(A.window, B.window, case["bias"], resid_before, case["base_act"], case["mul"])
    fast = out_dt != F32
    bound = error_bound(acc, mag, y, resid_before, case["base_act"], case["mul"], K, out_dt, fast_act=fast)
    bad = violations(C.window, ref, bound, out_dt)
    if bad.any():
        idx = bad.nonzero()[:4].tolist()
        detail = [(i, j, float(C.window[i, j]), float(ref[i, j]), float(bound[i, j])) for i, j in idx]
        raise AssertionError(f"{label}: {int(bad.sum())} elements outside the float64 bound, e.g. (m, n, got, ref, bound) {detail}")
    if controls:
        missed = controls_rejected(A.window, B.window, case["bias"], resid_before, case["base_act"], case["mul"], K,
                                   k_step_of(in_dt), out_dt, fast, bound)
        assert not missed, f"{label}: the bound accepts the negative control(s) {missed}: tolerance too loose"
    return C.window.clone()


# ---------------------------------------------------------------------------------------------------------------
# A. family x dtype x epilogue
# ---------------------------------------------------------------------------------------------------------------
def steps(in_dt, n):
    return n * k_step_of(in_dt)


# family -> (options, dtype pairs, epilogues, shapes (M, N, K steps))
ALL_EPI = MAIN_EPI
FAMILIES = {
    "skinny": (dict(), [(BF16, BF16), (F16, F16)], ALL_EPI,
               [(1, 208, 48), (7, 80, 4), (130, 16, 2), (511, 48, 6), (1000, 32, 16)]),
    "v1": (dict(variant=1), [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)], ALL_EPI,
           [(1, 8, 1), (7, 70, 3), (130, 200, 4), (513, 264, 48), (4099, 70, 1)]),
    "v2": (dict(variant=2), [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)], ALL_EPI,
           [(512, 200, 3), (513, 264, 1), (1000, 8, 4), (4099, 264, 48)]),
    "v6": (dict(variant=6), [(F32, F32), (BF16, BF16)], ALL_EPI,
           [(513, 264, 3), (1000, 520, 1), (4099, 264, 48)]),
    "v6-f32out": (dict(variant=6), [(BF16, F32), (F16, F32)], ["none", "bias"],
                  [(513, 264, 3), (1000, 520, 1), (4099, 264, 48)]),
    # generation 7 with the ring restarting per tile: bf16 sent there by bit 4 of OM_OPT_GEMM_CONT (bits 0 / 1 clear),
    # float16 by clearing bit 7 (every whole-tile f16 shape on the persistent kernel)
    "g7": (dict(cont=16, skinny_m=0), [(BF16, BF16)], ALL_EPI, [(512, 256, 3), (768, 512, 4), (512, 768, 48)]),
    "g7-f16": (dict(cont=0, skinny_m=0), [(F16, F16)], ["none", "bias", "erf", "relu", "add", "none_mul", "inplace"],
               [(512, 256, 1), (768, 512, 3), (512, 768, 48)]),
    "g7_one_tile": (dict(cont=511, skinny_m=0, gen=70), [(BF16, BF16)], ["none", "bias", "erf"],
                    [(512, 256, 3), (768, 512, 48)]),
    "7c16": (dict(cont=511, skinny_m=0), [(BF16, BF16)], ["none", "bias", "erf", "relu", "tanh"],
             [(512, 256, 3), (768, 512, 4), (512, 768, 48), (1024, 1024, 3)]),
    "7c16-f16": (dict(cont=495 & ~128, skinny_m=0), [(F16, F16)], ["none", "bias", "erf", "relu"],
                 [(512, 256, 3), (768, 512, 4), (512, 768, 48), (1024, 1024, 3)]),
    "7r16": (dict(cont=511, skinny_m=0), [(BF16, BF16)], ["add", "mul", "none_mul", "inplace"],
             [(512, 256, 3), (768, 512, 4), (512, 768, 48), (1024, 1024, 3)]),
    "7r16-f16": (dict(cont=495 & ~128, skinny_m=0), [(F16, F16)], ["add", "none_mul", "inplace"],
                 [(512, 256, 3), (768, 512, 4), (512, 768, 48), (1024, 1024, 3)]),
}


def _family_code(name):
    return name.split("-")[0]


def _opts(o):
    o = dict(o)
    return o.pop("gen", None), o


A_CASES = [pytest.param(fam, i, o, e, id=f"{_family_code(fam)}-{NAME[i]}->{NAME[o]}-{e}")
           for fam, (_, pairs, epis, _) in FAMILIES.items() for (i, o) in pairs for e in epis]


@pytest.mark.gpu
@pytest.mark.parametrize("fam,in_dt,out_dt,epi", A_CASES)
def test_family_dtype_epilogue(fam, in_dt, out_dt, epi):
    opts, _, _, shapes = FAMILIES[fam]
    gen, opts = _opts(opts)
    family = _family_code(fam)
    with gemm_options(gen=gen, **opts):
        for si, (M, Nn, ks) in enumerate(shapes):
            K = steps(in_dt, ks)
            case = make_case(in_dt, out_dt, M, Nn, K, epi, seed=1000 * si + 7)
            check_case(case, family, f"{fam} {NAME[in_dt]}->{NAME[out_dt]} {epi} M={M} N={Nn} K={K}")


FEW_K_STEPS = ((1, "erf"), (2, "bias"), (1, "relu"))      # (K steps, epilogue)


def _few_k_opts(dt):
    return dict(skinny_m=0) if dt == BF16 else dict(skinny_m=0, cont=495 & ~128)


def _few_k_size(dt):
    return 4096 if dt == BF16 else 512


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_restart_per_tile_kernel_at_one_and_two_k_steps(dt):
    """Fewer than three K steps: whole-tile 16-bit shapes the cost model sends to generation 7 take its restart-per-tile
    kernel (the continuous ring needs three).  bf16 at default options (256 tiles), f16 with bit 7 cleared."""
    with gemm_options(**_few_k_opts(dt)):
        for ks, epi in FEW_K_STEPS:
            M = Nn = _few_k_size(dt)
            case = make_case(dt, dt, M, Nn, steps(dt, ks), epi, seed=ks)
            check_case(case, "g7", f"g7 {NAME[dt]} K steps={ks} {epi}")


# the self-test's quick GEMM list (tests/native/selftest.cpp), ported with the family each shape reaches at default options
SELFTEST_QUICK = [
    (F32, F32, 128, 128, 32, "none", "v1"), (BF16, F32, 128, 128, 64, "none", "v1"), (F32, F32, 256, 384, 256, "bias", "v1"),
    (BF16, F32, 256, 384, 256, "bias", "v1"), (F32, F32, 130, 200, 96, "erf_add", "v1"), (BF16, BF16, 130, 200, 192, "erf_add", "v1"),
    (BF16, F32, 1000, 70, 128, "relu_add", "v1"), (F32, F32, 77, 300, 64, "mul_nobias", "v1"),
    (BF16, BF16, 4099, 768, 768, "erf", "v2"), (F32, F32, 1030, 768, 768, "add", "v2"), (BF16, BF16, 1000, 200, 128, "relu_add", "v2"),
    (BF16, BF16, 513, 2304, 768, "bias", "skinny"), (BF16, BF16, 2048, 768, 3072, "add", "v2"),
    (F32, F32, 777, 132, 64, "mul_nobias", "v2"), (BF16, F32, 600, 128, 64, "none", "v2"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("in_dt,out_dt,M,Nn,K,epi,fam", [pytest.param(*c, id=f"{c[6]}-{NAME[c[0]]}->{NAME[c[1]]}-{c[2]}x{c[3]}x{c[4]}-{c[5]}")
                                                         for c in SELFTEST_QUICK])
def test_selftest_quick_list(in_dt, out_dt, M, Nn, K, epi, fam):
    with gemm_options():
        check_case(make_case(in_dt, out_dt, M, Nn, K, epi, seed=M + Nn), fam, f"quick {fam} {M}x{Nn}x{K} {epi}")


# the self-test's gen7 list (bf16 -> bf16), with bit 4 of OM_OPT_GEMM_CONT set so that whole-tile shapes of three or more K steps
# go to generation 7 whatever the cost model says, and the few-rows kernel off; debug generation 0 and 70
SELFTEST_GEN7 = [
    (512, 256, 128, "none", "v2", "v2"), (512, 256, 64, "bias", "v2", "v2"), (1024, 512, 192, "add", "7r16", "7r16"),
    (4096, 768, 768, "erf", "7c16", "g7_one_tile"), (2048, 768, 3072, "add", "7r16", "7r16"),
    (70 * 256, 1024, 256, "add", "7r16", "7r16"), (70 * 256, 768, 128, "relu", "g7", "g7"),
    (70 * 256, 1024, 192, "erf", "7c16", None), (70 * 256, 768, 768, "bias", "7c16", None), (70 * 256, 768, 256, "none", "7c16", None),
    (2048, 768, 3072, "relu", "7c16", None), (256, 256, 448, "bias", "v1", None),
]


GEN7_CASES = [pytest.param(gen, M, Nn, K, epi, fam, id=f"gen{gen}-{fam}-{M}x{Nn}x{K}-{epi}")
              for gen in (0, 70) for (M, Nn, K, epi, fam0, fam70) in SELFTEST_GEN7
              for fam in [fam0 if gen == 0 else fam70] if fam is not None]      # the self-test runs the last five at generation 0 only


@pytest.mark.gpu
@pytest.mark.parametrize("gen,M,Nn,K,epi,fam", GEN7_CASES)
def test_selftest_gen7_list(gen, M, Nn, K, epi, fam):
    with gemm_options(gen=gen, cont=495 | 16, skinny_m=0):
        check_case(make_case(BF16, BF16, M, Nn, K, epi, seed=M + K), fam, f"gen7 list gen={gen} {fam} {M}x{Nn}x{K} {epi}")


# ---------------------------------------------------------------------------------------------------------------
# B. tile walk and persistence of generation 7
# ---------------------------------------------------------------------------------------------------------------
# tile counts (M / 256) x (N / 256): 2, 6, 9, 39 = 13 x 3 (group_m 8 leaves a group of 5), 255, 256, 257 (one more than the
# 256 CUs), 840; plus 101 (one more than a grid capped at 100).  A single 256 x 256 tile cannot reach generation 7 through
# om_gemm_nt (fewer than 512 rows go to generation 1: wide_ok), so the smallest walk is 2 x 1.
TILE_GRIDS = [(2, 1), (2, 3), (3, 3), (13, 3), (17, 15), (16, 16), (257, 1), (28, 30), (101, 1)]
WALKS = [(g, m) for g in (0, 1, 7, 8, 100, 128) for m in (1, 3, 8, 13)]
WALK_KERNELS = {
    "7c16-bf16": (BF16, "bias", dict(cont=511), "7c16"),
    "7c16-f16": (F16, "erf", dict(cont=495 & ~128), "7c16"),
    "7r16-bf16": (BF16, "add", dict(cont=511), "7r16"),
    "7r16-f16": (F16, "inplace", dict(cont=495 & ~128), "7r16"),
    "g7-bf16": (BF16, "relu", dict(cont=16), "g7"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kern", list(WALK_KERNELS))
@pytest.mark.parametrize("tm,tn", TILE_GRIDS, ids=[f"{a * b}tiles" for a, b in TILE_GRIDS])
def test_tile_walk_is_bit_identical_across_grid_caps_and_groups(kern, tm, tn):
    """Every (OM_OPT_GEMM_MAX_GRID, OM_OPT_GEMM_GROUP_M) gives the same bits (the walk must not change any tile's
    arithmetic); the default walk is inside the float64 bound; two identical calls are bit-identical.  Before every
    launch C's whole buffer goes back to the sentinel (and, in place, the window to the residual), so a tile a walk skips
    keeps the sentinel and fails the comparison; after every launch nothing outside the M x N window may have changed."""
    dt, epi, opts, family = WALK_KERNELS[kern]
    M, Nn = 256 * tm, 256 * tn
    ks = 4 if (tm, tn) == (13, 3) else 3                       # the continuous ring at its minimum (3) and 4 K steps
    case = make_case(dt, dt, M, Nn, steps(dt, ks), epi, seed=tm * 1000 + tn)
    C = case["C"]
    pristine = C.snapshot()                                    # sentinel everywhere (+ the residual in the window, in place)

    def relaunch(label, **walk):
        _bits(C.flat).copy_(pristine)
        with gemm_options(**walk):
            code = launch(case)
        assert code == FAM[family], (label, code)
        assert C.outside_changed(pristine) == 0, f"{label}: C written outside its M x N window"
        return C.window

    with gemm_options(skinny_m=0, **opts):
        first = check_case(case, family, f"{kern} {tm}x{tn} tiles default walk")
        for cap, gm in WALKS:
            got = relaunch(f"{kern} {tm}x{tn} max_grid={cap} group_m={gm}", max_grid=cap, group_m=gm)
            diff = int((_bits(got) != _bits(first)).sum())
            assert diff == 0, f"{kern} {tm}x{tn} tiles: max_grid={cap} group_m={gm} changes {diff} elements"
        got = relaunch(f"{kern} {tm}x{tn} repeat")
        assert torch.equal(_bits(got), _bits(first)), f"{kern}: two identical calls differ"


# ---------------------------------------------------------------------------------------------------------------
# C. strides and untouched memory (every case above already keeps guard rows; here lda / ldb / ldc / ldr > the row)
# ---------------------------------------------------------------------------------------------------------------
# family -> (options, in, out, epilogue, M, N, K steps, ldr multiple): generation 7 reads resid rows in 128-byte units
STRIDE_CASES = {
    "skinny": (dict(), BF16, BF16, "add", 130, 208, 4, 8),
    "v1": (dict(variant=1), F16, F16, "mul", 130, 70, 3, 1),
    "v1-f32": (dict(variant=1), F32, F32, "add", 513, 70, 3, 1),
    "v2": (dict(variant=2), BF16, BF16, "add", 1000, 200, 4, 8),
    "v2-f16": (dict(variant=2), F16, F32, "bias", 513, 264, 3, 4),
    "v6": (dict(variant=6), BF16, BF16, "mul", 1000, 520, 4, 8),
    "v6-f32": (dict(variant=6), F32, F32, "add", 513, 264, 3, 4),
    "g7": (dict(cont=16, skinny_m=0), BF16, BF16, "add", 512, 512, 3, 64),
    "7c16": (dict(cont=511, skinny_m=0), BF16, BF16, "erf", 768, 512, 4, 64),
    "7c16-f16": (dict(cont=495 & ~128, skinny_m=0), F16, F16, "relu", 768, 512, 3, 64),
    "7r16": (dict(cont=511, skinny_m=0), BF16, BF16, "mul", 512, 768, 4, 64),
    "7r16-f16": (dict(cont=495 & ~128, skinny_m=0), F16, F16, "add", 512, 768, 3, 64),
}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["padded", "slice"])
@pytest.mark.parametrize("fam", list(STRIDE_CASES))
def test_strides_and_guard_memory(fam, layout):
    opts, in_dt, out_dt, epi, M, Nn, ks, rmult = STRIDE_CASES[fam]
    K = steps(in_dt, ks)
    kpad = k_step_of(in_dt)                                     # lda = K + 64 (16-bit) / K + 32 (f32): 128 bytes more
    cpad = 24 if out_dt != F32 else 12
    ldr = Nn + 64 if rmult == 64 else Nn + 40
    if layout == "padded":
        kw = dict(lda=K + kpad, ldb=K + 2 * kpad, ldc=Nn + cpad, ldr=ldr)
    else:
        kw = dict(a_slice=True, ldb=2 * K, ldc=Nn + 2 * cpad, ldr=ldr + 64)
    with gemm_options(**opts):
        check_case(make_case(in_dt, out_dt, M, Nn, K, epi, seed=M, **kw), _family_code(fam), f"{fam} {layout} strides {kw}")


# ---------------------------------------------------------------------------------------------------------------
# D. alignment fallbacks the ABI allows
# ---------------------------------------------------------------------------------------------------------------
# (name, options, dtype, epilogue, M, N, K steps, make_case kwargs, family that must serve it)
ALIGN_CASES = [
    ("bias+4 v6 bf16", dict(variant=6), BF16, "bias", 1000, 520, 3, dict(bias_off=1), "v2"),
    ("bias+4 v6 f32", dict(variant=6), F32, "erf", 1000, 520, 3, dict(bias_off=1), "v2"),
    ("bias+4 g7 bf16", dict(cont=511, skinny_m=0), BF16, "erf", 512, 768, 3, dict(bias_off=1), "v2"),
    ("bias+4 g7 f16", dict(cont=495 & ~128, skinny_m=0), F16, "bias", 512, 768, 3, dict(bias_off=1), "v2"),
    ("bias+4 skinny", dict(), F16, "erf", 100, 208, 4, dict(bias_off=1), "skinny"),
    ("C+2 bf16", dict(skinny_m=0), BF16, "bias", 1024, 512, 4, dict(c_off=1), "v1"),
    ("C+2 f16", dict(cont=495 & ~128, skinny_m=0), F16, "relu", 512, 512, 3, dict(c_off=1), "v1"),
    ("C+2 skinny", dict(), F16, "bias", 100, 208, 4, dict(c_off=1), "skinny"),
    ("resid+2 bf16", dict(cont=511, skinny_m=0), BF16, "add", 512, 512, 3, dict(r_off=1), "v1"),
    ("resid+2 f16", dict(cont=495 & ~128, skinny_m=0), F16, "add", 512, 512, 3, dict(r_off=1), "v1"),
    ("resid+2 skinny", dict(), BF16, "mul", 100, 208, 4, dict(r_off=1), "skinny"),
    ("ldc%8 bf16", dict(cont=511, skinny_m=0), BF16, "erf", 512, 512, 3, dict(ldc=517), "v1"),
    ("ldc%8 f16", dict(cont=495 & ~128, skinny_m=0), F16, "add", 512, 512, 3, dict(ldc=515), "v1"),
    ("ldc%4 f32", dict(variant=6), F32, "bias", 1000, 520, 3, dict(ldc=523), "v1"),
    ("ldr%64 bf16 residual", dict(cont=511, skinny_m=0), BF16, "add", 512, 512, 3, dict(ldr=520), "v6"),
    ("ldr%64 f16 residual", dict(cont=495 & ~128, skinny_m=0), F16, "add", 512, 512, 3, dict(ldr=520), "v2"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts,dt,epi,M,Nn,ks,kw,fam", ALIGN_CASES, ids=[c[0] + "->" + c[8] for c in ALIGN_CASES])
def test_alignment_fallbacks(name, opts, dt, epi, M, Nn, ks, kw, fam):
    with gemm_options(**opts):
        check_case(make_case(dt, dt, M, Nn, steps(dt, ks), epi, seed=M + Nn, **kw), fam, name)


# ---------------------------------------------------------------------------------------------------------------
# D'. the decision table without a GPU: om_debug_gemm_plan on the addresses the GPU cases above would pass
# ---------------------------------------------------------------------------------------------------------------
_ES = {F32: 4, BF16: 2, F16: 2}


def planned_family(in_dt, out_dt, M, Nn, K, epi, lda=None, ldb=None, ldc=None, ldr=None, a_slice=False,
                   bias_off=0, c_off=0, r_off=0):
    """om_debug_gemm_plan for the call make_case(the same arguments) + launch would make.  Every buffer make_case allocates
    gets a made-up base address of its own, 512-byte aligned as the device allocator's are, plus the byte offset of its
    window (Buf: guard rows, misalignment; the bias slice); the leading dimensions are make_case's."""
    act, has_bias, rmode = EPI[epi]
    lda, ldb, ldc = (3 * K if a_slice else lda or K), ldb or K, ldc or Nn
    bases = iter(range(1 << 30, 1 << 40, 1 << 30))
    a = next(bases) + (K if a_slice else 0) * _ES[in_dt]
    b = next(bases)
    bias = next(bases) + 4 * bias_off if has_bias else None
    r = None
    if rmode in ("add", "mul"):
        ldr = ldr or Nn
        r = next(bases) + _start(ldr, 0, r_off) * _ES[out_dt]
    c = next(bases) + _start(ldc, 1, c_off) * _ES[out_dt]
    if rmode == "inplace":
        r, ldr = c, ldc
    return N.lib().om_debug_gemm_plan(in_dt, a, lda, b, ldb, out_dt, c, ldc, M, Nn, K, bias, r, ldr if r else 0,
                                      act | (N.ACT_MUL_RESID if rmode == "mul" else 0))


def _decision_table():
    """(label, options, in, out, M, N, K, epilogue, make_case kwargs, family) of every case of the GPU tables above, with the
    family the GPU test asserts through om_debug_gemm_last."""
    for fam, (opts, pairs, epis, shapes) in FAMILIES.items():
        for i, o in pairs:
            for e in epis:
                for M, Nn, ks in shapes:
                    yield f"A {fam}", opts, i, o, M, Nn, steps(i, ks), e, {}, _family_code(fam)
    for i, o, M, Nn, K, e, fam in SELFTEST_QUICK:
        yield "quick", {}, i, o, M, Nn, K, e, {}, fam
    for c in GEN7_CASES:
        gen, M, Nn, K, e, fam = c.values
        yield "gen7 list", dict(gen=gen, cont=495 | 16, skinny_m=0), BF16, BF16, M, Nn, K, e, {}, fam
    for name, opts, dt, e, M, Nn, ks, kw, fam in ALIGN_CASES:
        yield name, opts, dt, dt, M, Nn, steps(dt, ks), e, kw, fam
    for dt in (BF16, F16):
        for ks, e in FEW_K_STEPS:
            yield "few K steps", _few_k_opts(dt), dt, dt, _few_k_size(dt), _few_k_size(dt), steps(dt, ks), e, {}, "g7"


def test_decision_table_without_a_gpu():
    """The planner alone (no launch, no GPU) names, for every case of FAMILIES, the quick list, the gen7 list, ALIGN_CASES and
    the one- and two-K-step cases, the family the GPU test of that case asserts."""
    wrong, n = [], 0
    for label, opts, i, o, M, Nn, K, e, kw, fam in _decision_table():
        gen, opts = _opts(opts)
        with gemm_options(gen=gen, **opts):
            got = planned_family(i, o, M, Nn, K, e, **kw)
        n += 1
        if got != FAM[fam]:
            wrong.append((label, opts, gen, NAME[i], NAME[o], M, Nn, K, e, kw, fam, got))
    assert n == (sum(len(p) * len(e) * len(sh) for _, p, e, sh in FAMILIES.values()) + len(SELFTEST_QUICK) + len(GEN7_CASES) +
                 len(ALIGN_CASES) + 2 * len(FEW_K_STEPS)), n
    assert not wrong, f"{len(wrong)} of {n} cases planned another family, e.g. {wrong[:5]}"
    # refusals and empty problems: what om_gemm_nt answers with an error is negative, what it skips is 0
    assert N.lib().om_debug_gemm_plan(F32, 16, 33, 16, 33, F32, 16, 8, 4, 8, 33, None, None, 0, 0) < 0
    assert N.lib().om_debug_gemm_plan(BF16, 1 << 30, 64, 2 << 30, 64, BF16, 3 << 30, 8, 0, 8, 64, None, None, 0, 0) == 0


def test_plan_hook_leaves_the_last_family_alone():
    lib = N.lib()
    assert lib.om_gemm_nt(F32, 16, 33, 16, 33, F32, 16, 8, 4, 8, 33, None, None, 0, 0, None) != 0      # refused: last = 0
    assert planned_family(BF16, BF16, 4096, 768, 768, "erf") in FAM.values()
    assert lib.om_debug_gemm_last() == 0


# ---------------------------------------------------------------------------------------------------------------
# E. non-finite values on every family with a 16-bit output
# ---------------------------------------------------------------------------------------------------------------
NF_FAMILIES = {      # family -> (options, dtypes, shape (M, N, K steps), activations served)
    "skinny": (dict(), (BF16, F16), (100, 208, 4), ("none", "erf", "relu", "tanh")),
    "v1": (dict(variant=1), (BF16, F16), (130, 200, 4), ("none", "erf", "relu", "tanh")),
    "v2": (dict(variant=2), (BF16, F16), (1000, 264, 4), ("none", "erf", "relu", "tanh")),
    "v6": (dict(variant=6), (BF16,), (1000, 520, 4), ("none", "erf", "relu", "tanh")),
    "g7": (dict(cont=16, skinny_m=0), (BF16,), (512, 512, 4), ("none", "erf", "relu", "tanh")),
    "g7-f16": (dict(cont=0, skinny_m=0), (F16,), (512, 512, 4), ("none", "erf", "relu")),
    "7c16": (dict(cont=511, skinny_m=0), (BF16,), (512, 512, 4), ("none", "erf", "relu", "tanh")),
    "7c16-f16": (dict(cont=495 & ~128, skinny_m=0), (F16,), (512, 512, 4), ("none", "erf", "relu")),
    "g7_one_tile": (dict(cont=511, skinny_m=0, gen=70), (BF16,), (512, 512, 4), ("none", "erf")),
    # the residual kernels: the one-plane residual is added in f32 before the single rounding
    "7r16": (dict(cont=511, skinny_m=0), (BF16,), (512, 512, 4), ("none", "tanh")),
    "7r16-f16": (dict(cont=495 & ~128, skinny_m=0), (F16,), (512, 512, 4), ("none",)),
}
NF_RESID = {"7r16", "7r16-f16"}
NF_CASES = [pytest.param(f, dt, a, id=f"{_family_code(f)}-{NAME[dt]}-{a}{'-add' if f in NF_RESID else ''}")
            for f, (_, dts, _, acts) in NF_FAMILIES.items() for dt in dts for a in acts]
NF_ACT = {"none": N.ACT_NONE, "erf": N.ACT_GELU_ERF, "relu": N.ACT_RELU, "tanh": N.ACT_GELU_TANH}


@pytest.mark.gpu
@pytest.mark.parametrize("fam,dt,actname", NF_CASES)
def test_non_finite_values_propagate(fam, dt, actname):
    """A row of A holding a NaN, and one holding an inf, give non-finite outputs in those rows only (where the float64
    reference is non-finite; relu(-inf) = 0 stays 0) -- an activation must not turn a NaN into a number (torch.relu(NaN) is
    NaN: the float16 loss scaler skips a step only if an overflow stays non-finite).  float16 outputs whose magnitude rounds
    past 65504 are +-inf, exactly where torch's conversion of the float64 value gives inf, not saturated."""
    gen, opts = _opts(NF_FAMILIES[fam][0])
    _, _, (M, Nn, ks), _ = NF_FAMILIES[fam]
    family = _family_code(fam)
    K = steps(dt, ks)
    case = make_case(dt, dt, M, Nn, K, "add" if fam in NF_RESID else "bias", seed=99)
    case["act"] = case["base_act"] = NF_ACT[actname]
    A, B = case["A"].window, case["B"].window
    if dt == F16:
        # integer data: every f32 sum is exact, so which side of 65520 a value lands on is decided by the arithmetic alone.
        # Rows 0-3 of A are 1, 1, 2, 2; every 7th column of B is v in (255, -255, 256, -256) over the first K / 2 entries, 0 after:
        # rows 2, 3 reach 2 (K / 2) v = 65280 | -65280 | 65536 | -65536 at K = 256, and the bias moves the first two onto the edge:
        # 65280 + 239 = 65519 (rounds to 65504), -65280 - 240 = -65520 (rounds to -inf); 65536 is inf
        g = torch.Generator(device=DEV).manual_seed(5)
        A.copy_(torch.randint(-2, 3, A.shape, generator=g, device=DEV))
        B.copy_(torch.randint(-2, 3, B.shape, generator=g, device=DEV))
        bias = case["bias"]
        bias.copy_(torch.randint(-3, 4, (Nn,), generator=g, device=DEV).float())
        A[0:2] = 1.0
        A[2:4] = 2.0
        cols = torch.arange(0, Nn, 7, device=DEV)
        vals = torch.tensor([255.0, -255.0, 256.0, -256.0], device=DEV).repeat(len(cols))[:len(cols)]
        B[cols] = 0.0
        B[cols, :K // 2] = vals[:, None].to(B.dtype)
        edge = {255.0: 239.0, -255.0: -240.0, 256.0: 0.0, -256.0: 0.0}
        bias[cols] = torch.tensor([edge[float(v)] for v in vals], device=DEV)
        if case["R"] is not None:
            # integer residual; at the edge columns row 2 gets +1 (65519 + 1 = 65520: the residual add overflows) and
            # row 3 gets 0 (65519 stays 65504)
            R = case["R"].window
            R.copy_(torch.randint(-2, 3, R.shape, generator=g, device=DEV))
            R[2, cols] = torch.where(vals.abs() == 255.0, torch.sign(vals), torch.zeros_like(vals)).to(R.dtype)
            R[3, cols] = 0.0
    nan_row, inf_row = 5, 9
    A[nan_row, 3] = float("nan")
    A[inf_row, K - 1] = float("inf")
    with gemm_options(gen=gen, **opts):
        check_case(case, family, f"{fam} {NAME[dt]} {actname} non-finite", controls=False)
    C = case["C"].window.double()
    assert (~torch.isfinite(C[nan_row])).all(), f"{fam} {actname}: a NaN in row {nan_row} of A gave finite outputs"
    if dt == F16:
        assert torch.isinf(C[2:4]).any(), f"{fam} {actname}: no float16 overflow reached inf"
        if fam in NF_RESID:
            edge = cols[vals == 255.0]
            assert torch.isinf(C[2, edge]).all() and (C[3, edge] == 65504.0).all(), f"{fam}: residual add at the edge of 65504"
