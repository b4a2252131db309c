"""The last training kernels without a kernel-level test, each called alone through its om_debug_* hook and compared with a plain float64
(or bit-exact) statement of what it computes: the operand transposes of the fallback weight-gradient path (transpose_kernel,
transpose_batch_kernel), zero_rows_from_kernel, and the T5 kernels (t5_act_fwd / t5_act_bwd, t5_embed_bwd, t5_bias / t5_bias_bwd).  All
shapes are tiny; every written tensor is followed by sentinel guards, every accumulated-into buffer starts from PREFILL.

    transpose        out[c][r] = op(in[r][c]) for r < R, bit-zero for R <= r < Rp, nothing beyond Rp or beyond column C.  op 0 is a bit
                     copy; op 1 is erf-GELU: float64 of the stored input, one rounding U to the storage type, 8 u |x| for erff and the
                     three f32 products (the allowance tests/test_gemm_kernels.py gives the libm form)
    zero_rows_from   rows [first, M) of a row-major tensor are zero, rows before keep their bits; `first` is read on the device
    T5 activation    kind 0: g = relu(f), df = dg [f > 0] (so relu'(+-0) = 0): exact.  kind 1 (u = 2^-24, U the storage rounding):
                       z = c (x + a x^3), t = tanh(z), c = sqrt(2 / pi), a = 0.044715
                       gelu_new(x)  = x (1 + t) / 2                          g   = gelu_new(f) f2
                       gelu_new'(x) = (1 + t) / 2 + x (1 - t^2) c (1 + 3 a x^2) / 2
                       df = dg f2 gelu_new'(f),  df2 = dg gelu_new(f)
                     tanhf with the cubic in f32 is given e_t = 16 u on t, as tests/test_gemm_kernels.py gives it.  Propagated:
                       |d gelu_new|  <= |x| e_t / 2 + 4 u |gelu_new|
                       |d gelu_new'| <= e_t (1/2 + |t| |x| c (1 + 3 a x^2)) + 2 u |x| c (1 + 3 a x^2) / 2 + 8 u (|1 + t| / 2 + |second term|)
                     (1 - t^2 is formed from a rounded t^2: 2 u absolute; each product and sum one rounding), then the products with
                     f2 and dg (3 u relative) and one output rounding U
    T5 embedding     dword[clamp(ids[tok], 0, vocab - 1)] += dy[row], tok = row_map[row] (rows with tok < 0 skipped): f32 atomics in
                     any order, (count + 2) u (sum|dy| + |prefill|) per element, count = rows that hit the id.  The prefill is a term of
                     the sum like any other: each of the `count` atomic additions rounds a running value that holds it, so it enters
                     `count` times and not once ((count + 2) u sum|dy| + u |prefill| is below the half ulp of 0.25 + x that two
                     additions may each lose).  Rows nobody hits keep their bits
    T5 bias          out[h][q][k] = table[lut[k - q + L - 1]][h]: a bit-exact gather; backward dtable[lut[r]][h] += drel[h][r] within
                     (count + 2) u (sum|drel| + |prefill|); with drel = 1 and a zeroed table it counts the offsets per bucket exactly
"""
import ctypes as C
import math

import pytest
import torch

from openmatch_amd import native as N
from tests.test_gemm_epilogues import assert_within, guards_ok, sync
from tests.test_gemm_kernels import BF16, DEV, F16, F32, FLOOR, NAME, SENTINEL, TORCH_DT, U_ACC, U_OUT, Buf, _bits
from tests.test_row_kernels import FAKE, PREFILL

u = U_ACC
ALL_DT = [F32, BF16, F16]
GELU_C, GELU_A = math.sqrt(2.0 / math.pi), 0.044715
E_T = 16 * u
GUARD_F = 7.5


def stream():
    return N.stream_ptr(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------
# float64 references (device-agnostic)
# ---------------------------------------------------------------------------------------------------------------
def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_new64(x):
    return 0.5 * x * (1.0 + torch.tanh(GELU_C * (x + GELU_A * x ** 3)))


def gelu_new_grad64(x):
    t = torch.tanh(GELU_C * (x + GELU_A * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_C * (1.0 + 3.0 * GELU_A * x * x)


def gelu_new_err(x):
    """bounds of the f32 evaluation of gelu_new(x) and gelu_new'(x) (docstring)"""
    t = torch.tanh(GELU_C * (x + GELU_A * x ** 3))
    poly = x.abs() * GELU_C * (1.0 + 3.0 * GELU_A * x * x)
    second = 0.5 * poly * (1.0 - t * t)
    e_f = 0.5 * x.abs() * E_T + 4 * u * gelu_new64(x).abs()
    e_g = E_T * (0.5 + t.abs() * poly) + 2 * u * 0.5 * poly + 8 * u * (0.5 * (1.0 + t) + second)
    return e_f, e_g


def act_reference(f, f2, dg, kind, dt):
    """(g, bound), (df, bound), (df2, bound) of the T5 activation in float64 on the stored values"""
    x, U, fl = f.double(), U_OUT[dt], FLOOR[dt]
    if kind == 0:
        zero = torch.zeros_like(x)
        return (torch.where(x > 0, x, zero), zero), (torch.where(x > 0, dg.double(), zero), zero), None
    y, d = f2.double(), dg.double()
    e_f, e_g = gelu_new_err(x)
    g = gelu_new64(x) * y
    df = d * y * gelu_new_grad64(x)
    df2 = d * gelu_new64(x)
    stored = lambda v, e: U * v.abs() + e * (1 + U) + fl
    return ((g, stored(g, y.abs() * e_f + 2 * u * g.abs())),
            (df, stored(df, (d * y).abs() * e_g + 3 * u * df.abs())),
            (df2, stored(df2, d.abs() * e_f + 2 * u * df2.abs())))


def act_inputs(n, dt, device):
    gen = torch.Generator(device=device).manual_seed(n)
    f = torch.linspace(-8.0, 8.0, n, device=device) if n > 1 else torch.zeros(1, device=device)
    if n >= 255:
        f[n // 2], f[n // 3] = 0.0, -0.0
        assert math.copysign(1.0, float(f[n // 3])) < 0
    f2 = torch.randn(n, generator=gen, device=device) * 1.5
    dg = torch.randn(n, generator=gen, device=device)
    return f.to(TORCH_DT[dt]), f2.to(TORCH_DT[dt]), dg.to(TORCH_DT[dt])


def scatter_reference(values, index, rows, prefill):
    """prefill + sum of values[i] into row index[i] (index < 0: skipped), the bound (count + 2) u (sum|v| + |prefill|), and the hit mask"""
    v = values.double()
    live = index >= 0
    ref = torch.full((rows, v.shape[1]), float(prefill), dtype=torch.float64, device=v.device)
    mag = torch.zeros_like(ref)
    cnt = torch.zeros(rows, dtype=torch.float64, device=v.device)
    ref.index_add_(0, index[live], v[live])
    mag.index_add_(0, index[live], v[live].abs())
    cnt.index_add_(0, index[live], torch.ones(int(live.sum()), dtype=torch.float64, device=v.device))
    return ref, (cnt[:, None] + 2) * u * (mag + abs(prefill)), cnt > 0


def t5_lut(L, buckets=32, max_dist=128):
    lib = N.lib()
    return torch.tensor([lib.om_t5_relative_bucket(rel, buckets, max_dist) for rel in range(-(L - 1), L)], dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_activation_references_are_the_autograd_of_the_forward():
    x = torch.linspace(-8.0, 8.0, 4001, dtype=torch.float64).requires_grad_()
    gelu_new64(x).sum().backward()
    assert torch.allclose(gelu_new_grad64(x.detach()), x.grad, rtol=1e-12, atol=1e-14)
    want = torch.nn.functional.gelu(x.detach(), approximate="tanh")
    assert torch.allclose(gelu_new64(x.detach()), want, rtol=1e-12, atol=1e-14)
    assert torch.allclose(gelu_erf64(x.detach()), torch.nn.functional.gelu(x.detach()), rtol=1e-12, atol=1e-14)
    # the gated form through both inputs, and relu with relu'(+-0) = 0 as torch has it
    f = torch.tensor([-3.0, -0.0, 0.0, 0.4, 2.5], dtype=torch.float64, requires_grad=True)
    f2 = torch.tensor([0.7, -1.1, 2.0, -0.3, 1.9], dtype=torch.float64, requires_grad=True)
    dg = torch.tensor([1.3, 0.2, -0.8, 0.5, -2.0], dtype=torch.float64)
    ((gelu_new64(f) * f2) * dg).sum().backward()
    (g, _), (df, _), (df2, _) = act_reference(f.detach(), f2.detach(), dg, 1, F32)
    assert torch.allclose(df, f.grad, rtol=1e-12, atol=1e-14) and torch.allclose(df2, f2.grad, rtol=1e-12, atol=1e-14)
    f.grad = None
    (torch.relu(f) * dg).sum().backward()
    (g, _), (df, _), _ = act_reference(f.detach(), None, dg, 0, F32)
    assert torch.equal(df, f.grad) and torch.equal(g, torch.relu(f.detach())) and df[1] == 0 and df[2] == 0


@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: NAME[d])
def test_activation_bounds_admit_an_f32_evaluation_and_reject_controls(dt):
    """the emulated kernel is the two formulas in float32, rounded to the storage type; the controls are gelu_new' without its second
    term and the erf form in place of the tanh form"""
    f, f2, dg = act_inputs(1000, dt, "cpu")
    (g, eg), (df, edf), (df2, edf2) = act_reference(f, f2, dg, 1, dt)
    x, y, d = f.float(), f2.float(), dg.float()
    t = torch.tanh(np32(GELU_C) * (x + np32(GELU_A) * x * x * x))
    gel = 0.5 * x * (1.0 + t)
    grad = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * np32(GELU_C) * (1.0 + 3.0 * np32(GELU_A) * x * x)
    for got, ref, e in ((gel * y, g, eg), (d * y * grad, df, edf), (d * gel, df2, edf2)):
        assert bool(((got.to(TORCH_DT[dt]).double() - ref).abs() <= e).all())
    t64 = torch.tanh(GELU_C * (f.double() + GELU_A * f.double() ** 3))
    assert bool((((dg.double() * f2.double() * 0.5 * (1.0 + t64)) - df).abs() > edf).any())
    assert bool((((gelu_erf64(f.double()) * f2.double()) - g).abs() > eg).any())


def np32(v):
    return torch.tensor(v, dtype=torch.float32)


def test_hooks_check_their_arguments():
    lib = N.lib()
    names = ["om_debug_transpose", "om_debug_transpose_batch", "om_debug_zero_rows_from", "om_debug_t5_act_fwd", "om_debug_t5_act_bwd",
             "om_debug_t5_embed_bwd", "om_debug_t5_bias", "om_debug_t5_bias_bwd"]
    for name in names:
        assert name in N.exported_symbols() and hasattr(lib, name)
    p, z, s = C.c_void_p(FAKE), C.c_void_p(0), C.c_void_p(0)
    with_dtype = {
        "om_debug_transpose": lambda dt, a: lib.om_debug_transpose(dt, a, 8, 4, 8, p, 8, 8, 0, s),
        "om_debug_t5_act_fwd": lambda dt, a: lib.om_debug_t5_act_fwd(dt, a, z, p, 16, 0, s),
        "om_debug_t5_act_bwd": lambda dt, a: lib.om_debug_t5_act_bwd(dt, a, p, z, p, z, 16, 0, s),
        "om_debug_t5_embed_bwd": lambda dt, a: lib.om_debug_t5_embed_bwd(dt, a, p, p, 4, 8, 5, z, s),
    }
    for name, f in with_dtype.items():
        assert f(BF16, z) != 0 and b"null argument" in lib.om_last_error() and name.encode() in lib.om_last_error(), name
        assert f(7, p) != 0 and b"dtype must be" in lib.om_last_error(), name
    # the gated form needs its second input and second output
    assert lib.om_debug_t5_act_fwd(F32, p, z, p, 16, 1, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_t5_act_bwd(F32, p, p, p, p, z, 16, 1, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_t5_embed_bwd(F32, p, p, p, 4, 8, 0, z, s) != 0 and b"at least 1" in lib.om_last_error()
    for fn in (lib.om_debug_t5_bias, lib.om_debug_t5_bias_bwd):
        assert fn(z, p, p, 4, 2, s) != 0 and b"null" in lib.om_last_error()
        assert fn(p, p, p, 0, 2, s) != 0 and b"at least 1" in lib.om_last_error()
        assert fn(p, p, p, 4, 0, s) != 0 and b"at least 1" in lib.om_last_error()
    arr, cnt = (C.c_void_p * 1)(FAKE), (C.c_int * 1)(4)
    assert lib.om_debug_transpose_batch(BF16, None, arr, cnt, cnt, 1, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_transpose_batch(7, arr, arr, cnt, cnt, 1, s) != 0 and b"dtype must be" in lib.om_last_error()
    assert lib.om_debug_transpose_batch(F16, (C.c_void_p * 1)(None), arr, cnt, cnt, 1, s) != 0 and b"null" in lib.om_last_error()
    # nothing to do: no launch, no device
    assert lib.om_debug_transpose_batch(F16, None, None, None, None, 0, s) == 0
    assert lib.om_debug_transpose(F32, p, 8, 0, 8, p, 8, 8, 0, s) == 0 and lib.om_debug_transpose(F32, p, 8, 4, 0, p, 8, 8, 0, s) == 0
    assert lib.om_debug_t5_act_fwd(F32, p, z, p, 0, 0, s) == 0 and lib.om_debug_t5_act_bwd(F32, p, p, z, p, z, 0, 0, s) == 0
    assert lib.om_debug_t5_embed_bwd(F32, p, p, p, 0, 8, 5, z, s) == 0 and lib.om_debug_zero_rows_from(p, 16, p, 0, s) == 0
    assert lib.om_abi_version() == 6


def test_zero_rows_from_refusals():
    """unaligned p and a row that is not whole 16-byte vectors are refused before any launch (made-up addresses)"""
    lib = N.lib()
    p, s = C.c_void_p(FAKE), C.c_void_p(0)
    text = b"rows of whole 16-byte vectors"
    assert lib.om_debug_zero_rows_from(C.c_void_p(FAKE + 8), 16, p, 4, s) != 0 and text in lib.om_last_error()
    for rb in (8, 24, 1540):
        assert lib.om_debug_zero_rows_from(p, rb, p, 4, s) != 0 and text in lib.om_last_error()
    assert lib.om_debug_zero_rows_from(C.c_void_p(0), 16, p, 4, s) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_zero_rows_from(p, 16, C.c_void_p(0), 4, s) != 0 and b"null" in lib.om_last_error()


# ---------------------------------------------------------------------------------------------------------------
# GPU: transposes
# ---------------------------------------------------------------------------------------------------------------
TR_R = [1, 63, 64, 65, 130]
TR_C = [1, 64, 65, 200]


def values(dt, R, Cc, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(R, Cc, generator=gen, device=DEV) * 2).to(TORCH_DT[dt])
    if R * Cc >= 4:
        x.view(-1)[1], x.view(-1)[2] = 0.0, -0.0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("op", [0, 1], ids=["copy", "gelu"])
@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: NAME[d])
def test_transpose(dt, op):
    lib = N.lib()
    for R in TR_R:
        for Cc in TR_C:
            Rp, ldi = R + 3, Cc + 5
            src = Buf(dt, R, Cc, ldi, fill=values(dt, R, Cc, 100 * R + Cc))
            out = Buf(dt, Cc, Rp, Rp + 2)
            snaps = (src.snapshot(), out.snapshot())
            with torch.cuda.device(DEV):
                rc = lib.om_debug_transpose(dt, src.ptr(), ldi, R, Cc, out.ptr(), out.ld, Rp, op, stream())
            sync()
            label = f"transpose/{NAME[dt]}/op{op}/{R}x{Cc}"
            assert rc == 0, lib.om_last_error()
            guards_ok(label, (out, snaps[1]))
            assert torch.equal(_bits(src.flat), snaps[0]), f"{label}: input modified"
            assert bool((_bits(out.window[:, R:]) == 0).all()), f"{label}: rows R .. Rp - 1 are not bit-zero"
            got = out.window[:, :R]
            if op == 0:
                assert torch.equal(_bits(got), _bits(src.window.t())), f"{label}: not a bit copy"
            else:
                x = src.window.t().double()
                ref = gelu_erf64(x)
                assert_within(label, got, ref, U_OUT[dt] * ref.abs() + 8 * u * x.abs() * (1 + U_OUT[dt]) + FLOOR[dt], dt)


@pytest.mark.gpu
def test_transpose_of_no_rows_launches_nothing():
    out = Buf(BF16, 8, 8, 8)
    snap = out.snapshot()
    src = torch.ones(8, 8, dtype=torch.bfloat16, device=DEV)
    with torch.cuda.device(DEV):
        assert N.lib().om_debug_transpose(BF16, N.ptr(src), 8, 0, 8, out.ptr(), 8, 8, 0, stream()) == 0
    sync()
    assert torch.equal(_bits(out.flat), snap)


BATCH_SHAPES = [(1, 1), (5, 70), (64, 64), (65, 3), (130, 2), (3, 129), (0, 7), (64, 65), (7, 0), (2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("jobs", [1, 3, 41], ids=lambda j: f"{j}-jobs")
@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: NAME[d])
def test_transpose_batch(dt, jobs):
    """dense transposes, 40 to a launch (41 jobs: two launches), zero-sized jobs among them; bit-exact, a guard behind every output"""
    lib = N.lib()
    shapes = [(64, 65)] if jobs == 1 else [BATCH_SHAPES[(i + (5 if jobs == 3 else 0)) % len(BATCH_SHAPES)] for i in range(jobs)]
    if jobs == 41:
        shapes[39], shapes[40] = (0, 7), (65, 3)                   # the first launch ends in an empty job, the second holds one job
    assert any(r * c == 0 for r, c in shapes) or jobs == 1
    guard = 16
    ins = [values(dt, r, c, 7 * i + r + c) if r * c else torch.empty(0, dtype=TORCH_DT[dt], device=DEV) for i, (r, c) in enumerate(shapes)]
    outs = []
    for r, c in shapes:
        o = torch.empty(r * c + guard, dtype=TORCH_DT[dt], device=DEV)
        _bits(o).fill_(SENTINEL[dt] - (1 << 32 if dt == F32 and SENTINEL[dt] >= 1 << 31 else 0))
        outs.append(o)
    snaps = [_bits(o).clone() for o in outs]
    n = len(shapes)
    in_p = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in ins])
    out_p = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    Rs, Cs = (C.c_int * n)(*[r for r, _ in shapes]), (C.c_int * n)(*[c for _, c in shapes])
    with torch.cuda.device(DEV):
        rc = lib.om_debug_transpose_batch(dt, in_p, out_p, Rs, Cs, n, stream())
    sync()
    assert rc == 0, lib.om_last_error()
    for i, ((r, c), x, o, snap) in enumerate(zip(shapes, ins, outs, snaps)):
        assert torch.equal(_bits(o)[r * c:], snap[r * c:]), f"job {i} {r}x{c}: written behind the output"
        if r * c:
            assert torch.equal(_bits(o[:r * c].view(c, r)), _bits(x.t().contiguous())), f"job {i} {r}x{c}: not a bit copy"


# ---------------------------------------------------------------------------------------------------------------
# GPU: zero_rows_from
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 600])
def test_zero_rows_from(M):
    lib = N.lib()
    for row_bytes in (16, 48, 1536):
        gen = torch.Generator(device=DEV).manual_seed(M + row_bytes)
        for first in sorted({0, 1, M - 1, M, M + 3}):
            flat = torch.randint(1, 256, (256 + M * row_bytes + 256,), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
            assert flat.data_ptr() % 16 == 0
            before = flat.clone()
            fdev = torch.tensor([first], dtype=torch.int32, device=DEV)
            with torch.cuda.device(DEV):
                rc = lib.om_debug_zero_rows_from(flat.data_ptr() + 256, row_bytes, N.ptr(fdev), M, stream())
            sync()
            assert rc == 0, lib.om_last_error()
            label = f"zero_rows_from M {M} row_bytes {row_bytes} first {first}"
            body, was = flat[256:256 + M * row_bytes].view(M, row_bytes), before[256:256 + M * row_bytes].view(M, row_bytes)
            cut = min(first, M)
            assert torch.equal(body[:cut], was[:cut]), f"{label}: a row before `first` changed"
            assert bool((body[cut:] == 0).all()), f"{label}: a row from `first` on is not zero"
            assert torch.equal(flat[:256], before[:256]) and torch.equal(flat[256 + M * row_bytes:], before[256 + M * row_bytes:]), f"{label}: guards"
            assert int(fdev[0]) == first


# ---------------------------------------------------------------------------------------------------------------
# GPU: T5 activation
# ---------------------------------------------------------------------------------------------------------------
def guarded(n, dt):
    t = torch.full((n + 8,), GUARD_F, dtype=TORCH_DT[dt], device=DEV)
    return t


def guard_kept(t, n):
    return bool((t[n:] == GUARD_F).all())


ACT_N = [1, 255, 256, 257, 1000]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["relu", "gated-gelu"])
@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: NAME[d])
def test_t5_activation(dt, kind):
    lib = N.lib()
    for n in ACT_N:
        f, f2, dg = act_inputs(n, dt, DEV)
        keep = [t.clone() for t in (f, f2, dg)]
        (g_ref, g_e), (df_ref, df_e), second = act_reference(f, f2, dg, kind, dt)
        g, df, df2 = guarded(n, dt), guarded(n, dt), guarded(n, dt)
        with torch.cuda.device(DEV):
            rc = lib.om_debug_t5_act_fwd(dt, N.ptr(f), N.ptr(f2) if kind else None, N.ptr(g), n, kind, stream())
            rc |= lib.om_debug_t5_act_bwd(dt, N.ptr(dg), N.ptr(f), N.ptr(f2) if kind else None, N.ptr(df), N.ptr(df2) if kind else None, n, kind, stream())
        sync()
        assert rc == 0, lib.om_last_error()
        label = f"t5_act/{NAME[dt]}/kind{kind}/n{n}"
        assert guard_kept(g, n) and guard_kept(df, n) and guard_kept(df2, n), f"{label}: written behind an output"
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((f, f2, dg), keep)), f"{label}: input modified"
        assert_within(f"{label} g", g[:n], g_ref, g_e, dt)
        assert_within(f"{label} df", df[:n], df_ref, df_e, dt)
        if kind:
            assert_within(f"{label} df2", df2[:n], second[0], second[1], dt)
        else:
            assert bool((df2 == GUARD_F).all()), f"{label}: relu wrote a second gradient"
        # in place, as train.hip calls it: df == dg
        dg2 = guarded(n, dt)
        dg2[:n] = dg
        with torch.cuda.device(DEV):
            rc = lib.om_debug_t5_act_bwd(dt, N.ptr(dg2), N.ptr(f), N.ptr(f2) if kind else None, N.ptr(dg2), N.ptr(df2) if kind else None, n, kind, stream())
        sync()
        assert rc == 0, lib.om_last_error()
        assert torch.equal(_bits(dg2), _bits(df)), f"{label}: the in-place call differs from the out-of-place one"


# ---------------------------------------------------------------------------------------------------------------
# GPU: T5 embedding backward
# ---------------------------------------------------------------------------------------------------------------
def acc_buffer(rows, cols):
    t = torch.full((rows * cols + 8,), GUARD_F, device=DEV)
    t[:rows * cols] = PREFILL
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [False, True], ids=["rows", "row_map"])
@pytest.mark.parametrize("H", [8, 300])
@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: NAME[d])
def test_t5_embed_bwd(dt, H, mapped):
    lib = N.lib()
    M, vocab, tokens = 37, 11, 50
    gen = torch.Generator(device=DEV).manual_seed(H + mapped)
    dy = torch.randn(M, H, generator=gen, device=DEV).to(TORCH_DT[dt])
    ids = torch.randint(-3, vocab + 4, (tokens,), generator=gen, device=DEV)
    ids[:6] = torch.tensor([4, 4, 4, -7, vocab + 9, 4], device=DEV)      # repeats and both clamps among the first rows
    ids[ids == 7] = 8                                                    # a row nobody hits
    if mapped:
        row_map = torch.randperm(tokens, generator=gen, device=DEV)[:M].to(torch.int32)
        row_map[0], row_map[1] = 3, 4                                    # the two clamped tokens
        row_map[3], row_map[20] = -1, -1
        row_map[5] = row_map[4]                                          # two rows of dy for one token
        tok = row_map.long()
    else:
        row_map, tok = None, torch.arange(M, device=DEV)
    hit = torch.where(tok >= 0, ids[tok.clamp(min=0)].clamp(0, vocab - 1), torch.full_like(tok, -1))
    ref, bound, touched = scatter_reference(dy, hit, vocab, PREFILL)
    assert not bool(touched[7]) and bool(touched[0]) and bool(touched[vocab - 1])
    dword = acc_buffer(vocab, H)
    keep = (dy.clone(), ids.clone())
    with torch.cuda.device(DEV):
        rc = lib.om_debug_t5_embed_bwd(dt, N.ptr(dy), N.ptr(ids), N.ptr(dword), M, H, vocab, N.ptr(row_map), stream())
    sync()
    assert rc == 0, lib.om_last_error()
    label = f"t5_embed_bwd/{NAME[dt]}/H{H}/{'map' if mapped else 'rows'}"
    got = dword[:vocab * H].view(vocab, H)
    assert bool((dword[vocab * H:] == GUARD_F).all()), f"{label}: written behind dword"
    assert torch.equal(_bits(dy), _bits(keep[0])) and torch.equal(ids, keep[1])
    assert_within(label, got, ref, bound)
    assert bool((got[~touched] == PREFILL).all()), f"{label}: a row nobody hits changed"
    # control: without the clamp the out-of-range rows would be lost
    lost = torch.where((hit >= 0) & ((ids[tok.clamp(min=0)] < 0) | (ids[tok.clamp(min=0)] >= vocab)), torch.full_like(hit, -1), hit)
    ctl = scatter_reference(dy, lost, vocab, PREFILL)[0]
    assert bool(((ctl - ref).abs() > bound).any())


# ---------------------------------------------------------------------------------------------------------------
# GPU: T5 relative-position bias
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("heads", [1, 12])
@pytest.mark.parametrize("L", [1, 2, 33])
def test_t5_bias_and_backward(L, heads):
    lib = N.lib()
    buckets = 32
    lut_h = t5_lut(L, buckets)
    lut = lut_h.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(L + heads)
    table = torch.randn(buckets, heads, generator=gen, device=DEV)
    out = torch.full((heads * L * L + 8,), GUARD_F, device=DEV)
    drel = torch.randn(heads, 2 * L - 1, generator=gen, device=DEV)
    dtable = acc_buffer(buckets, heads)
    counts = torch.zeros(buckets * heads + 8, device=DEV)
    ones = torch.ones(heads, 2 * L - 1, device=DEV)
    keep = (table.clone(), drel.clone(), lut.clone())
    with torch.cuda.device(DEV):
        rc = lib.om_debug_t5_bias(N.ptr(table), N.ptr(lut), N.ptr(out), L, heads, stream())
        rc |= lib.om_debug_t5_bias_bwd(N.ptr(drel), N.ptr(lut), N.ptr(dtable), L, heads, stream())
        rc |= lib.om_debug_t5_bias_bwd(N.ptr(ones), N.ptr(lut), N.ptr(counts), L, heads, stream())
    sync()
    assert rc == 0, lib.om_last_error()
    label = f"t5_bias/L{L}/heads{heads}"
    assert torch.equal(table, keep[0]) and torch.equal(drel, keep[1]) and torch.equal(lut, keep[2])
    # forward: a bit-exact gather
    q, k = torch.meshgrid(torch.arange(L, device=DEV), torch.arange(L, device=DEV), indexing="ij")
    want = table[lut.long()[k - q + (L - 1)]].permute(2, 0, 1).contiguous()              # [heads, L, L]
    assert torch.equal(out[:heads * L * L].view(heads, L, L).view(torch.int32), want.view(torch.int32)), f"{label}: not a bit-exact gather"
    assert bool((out[heads * L * L:] == GUARD_F).all())
    # backward: the offsets that share a bucket summed into the pre-filled table
    index = lut.long().repeat(heads) * heads + torch.arange(heads, device=DEV).repeat_interleave(2 * L - 1)      # flat [bucket][head]
    ref, bound, touched = scatter_reference(drel.reshape(-1, 1), index, buckets * heads, PREFILL)
    got = dtable[:buckets * heads].view(-1, 1)
    assert_within(f"{label} dtable", got, ref, bound)
    assert bool((got[~touched] == PREFILL).all()) and bool((dtable[buckets * heads:] == GUARD_F).all())
    if L == 33:
        assert float(torch.bincount(lut.long()).max()) > 1                       # log-spaced buckets shared by several offsets
    # drel = 1 on a zeroed table counts the offsets per bucket exactly
    per_bucket = torch.bincount(lut.long(), minlength=buckets).float()
    assert torch.equal(counts[:buckets * heads].view(buckets, heads), per_bucket[:, None].expand(buckets, heads)), f"{label}: counts"
    assert bool((counts[buckets * heads:] == 0).all())
