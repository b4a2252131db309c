"""The float16-only index (OM_SEARCH_F16_ONLY, FlatIPIndex(precision="f16"); DESIGN.md 4f "Float16-only index"): rows stored in float16,
2 bytes per element, searched exactly with float32 queries.

  CPU   the symbols; mode 2 schedules like mode 1; the refusals of both entries in the new mode, before any launch; what modes 0 and 1
        refuse is what they refused
  GPU   1 the bits of an f16_rescore index built from the widened rows, through both entries, at every branch of the scan and the
          re-score; each result also judged against oracle/flatip.py with fp64 adjudication
        2 the row-typed kernels alone (om_debug_rescore_rows): float16 rows and float32 rows holding the same values give the same bits
        3 add: the stored plane, growth, reserve, the statistics, the resident bytes, values beyond float16
        4 a 10 000-way tie: redone on the device, the other queries of the batch untouched
        5 a margin nothing certifies: every query redone
        6 a search captured in a graph;  7 search(), id_offset, reset, merge_topk over two float16-only shards"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from oracle import flatip

DEV = "cuda:0"
FLT_MIN = np.float32(-3.4028235e38)


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_new_symbols_exist():
    lib = N.lib()
    for name in ("om_index_add_f16", "om_debug_rescore_rows"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None
    assert N.SEARCH_F16_ONLY == 2 and (N.SEARCH_F32, N.SEARCH_F16_RESCORE) == (0, 1)


def schedule(mode, nq, n, k):
    cap = 1024
    chunks, cnt = (C.c_int64 * cap)(), C.c_int(-1)
    N.check(N.lib().om_debug_search_schedule(mode, nq, n, k, chunks, cap, C.byref(cnt)))
    assert 0 <= cnt.value <= cap
    return list(chunks[:cnt.value])


@pytest.mark.parametrize("k", [10, 1000])
@pytest.mark.parametrize("nq", [1, 64, 300, 6980])
@pytest.mark.parametrize("n", [0, 4096, 4097, 50000, 8841823])
def test_mode_2_schedules_like_mode_1(k, nq, n):
    assert schedule(N.SEARCH_F16_ONLY, nq, n, k) == schedule(N.SEARCH_F16_RESCORE, nq, n, k)


def test_mode_2_is_not_the_float32_schedule():
    assert schedule(N.SEARCH_F16_ONLY, 1, 8841823, 1000) != schedule(N.SEARCH_F32, 1, 8841823, 1000)


def test_scan_plan_and_round_take_half_as_before():
    """the planner knows no modes: half = 1 is what both 16-bit modes ask for"""
    lib = N.lib()
    out = (C.c_int * 4)()
    N.check(lib.om_debug_scan_plan(1, 1, 768, out))
    assert list(out) == [N.SCAN_FAMILY["stream32"], 32, 1, 12]
    N.check(lib.om_debug_scan_plan(0, 1, 768, out))
    assert out[0] == N.SCAN_FAMILY["generic"]
    rnd = (C.c_int64 * 8)()
    N.check(lib.om_debug_scan_round(1, 300, 256, 25915, 256, rnd))
    assert rnd[0] == N.SCAN_KERNEL["wide7c"] and rnd[1] == 25915 // 256 * 256 and rnd[4] == N.SCAN_KERNEL["tile6"] and rnd[5] == 25915 % 256


FAKE = 0x1000


def _sync_refused(mode=2, idx32=0, idx16=FAKE, stats=FAKE, d=64, k=10, ws_bytes=1 << 40):
    """one om_sim_topk call with pointers that are never followed: every refusal comes before the first launch"""
    p = N.c_void_p
    return N.lib().om_sim_topk(mode, p(FAKE), 3, p(idx32), p(idx16), p(stats), 5000, d, k, 0, p(FAKE), p(FAKE), p(FAKE), ws_bytes, p(0))


def _async_refused(mode=2, idx32=0, idx16=FAKE, stats=FAKE, d=64, k=10, ws_bytes=1 << 40):
    p = N.c_void_p
    return N.lib().om_sim_topk_async(mode, p(FAKE), 3, p(idx32), p(idx16), p(stats), 5000, d, k, 0, p(FAKE), p(FAKE), p(0x2000), p(FAKE),
                                     ws_bytes, p(0))


@pytest.mark.parametrize("entry", [_sync_refused, _async_refused], ids=["sync", "async"])
def test_mode_2_refusals(entry):
    err = N.lib().om_last_error
    assert entry(idx16=0) == 1
    assert b"OM_SEARCH_F16_ONLY" in err() and b"index_f16" in err()
    assert entry(stats=0) == 1
    assert b"OM_SEARCH_F16_ONLY" in err() and b"stats" in err()
    assert entry(d=16448) == 1
    assert b"OM_SEARCH_F16_ONLY" in err() and b"16384" in err()
    with switched(N.OPT_SCAN_GEN7, 0):
        assert entry() == 1
        assert b"OM_SEARCH_F16_ONLY" in err() and b"OM_OPT_SCAN_GEN7" in err()
    assert entry(k=2049) == 1
    assert b"2048" in err()


def test_mode_2_needs_the_async_workspace_in_the_sync_entry():
    lib = N.lib()
    small, big = lib.om_sim_topk_workspace_bytes(3, 64, 10), lib.om_sim_topk_async_workspace_bytes(3, 64, 10)
    assert small < big
    assert _sync_refused(ws_bytes=small) == 1
    assert b"OM_SEARCH_F16_ONLY" in lib.om_last_error() and b"om_sim_topk_async_workspace_bytes" in lib.om_last_error()
    assert _sync_refused(ws_bytes=big - 1) == 1
    assert _async_refused(ws_bytes=big - 1) == 1
    assert b"workspace too small" in lib.om_last_error()


@pytest.mark.parametrize("entry", [_sync_refused, _async_refused], ids=["sync", "async"])
@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_still_need_index_f32(entry, mode):
    assert entry(mode=mode, idx32=0) == 1
    assert N.lib().om_last_error() == b"index_f32 is null" or N.lib().om_last_error().endswith(b"index_f32 is null")


def test_mode_1_still_names_its_missing_planes():
    assert _sync_refused(mode=1, idx32=FAKE, idx16=0) == 1
    assert b"f16 mode needs index_f16 and stats" in N.lib().om_last_error()


def test_index_add_f16_refuses_other_dtypes():
    p = N.c_void_p
    lib = N.lib()
    for dt in (N.OM_BF16, 7, -1):
        assert lib.om_index_add_f16(dt, p(FAKE), 4, 64, p(FAKE), p(FAKE), p(FAKE), p(0)) == 1
        assert b"OM_F32 or OM_F16" in lib.om_last_error()
    assert lib.om_index_add_f16(N.OM_F32, p(FAKE), 4, 64, p(FAKE), p(FAKE), p(0), p(0)) == 1      # the counter is not optional


def test_unknown_precision_is_still_a_value_error():
    from openmatch_amd.index import FlatIPIndex
    with pytest.raises(ValueError, match="precision"):
        FlatIPIndex(8, device=DEV, precision="nonsense")


# ------------------------------------------------------------------------------------------------------------- GPU
def _pair(P):
    """index A: float16-only, from P;  index B: today's two-copy index, from the widened float16 rows"""
    from openmatch_amd.index import FlatIPIndex
    d = P.shape[1]
    A = FlatIPIndex(d, device=DEV, precision="f16"); A.add(P)
    W = torch.from_numpy(P).half().float().numpy()
    B = FlatIPIndex(d, device=DEV, precision="f16_rescore"); B.add(W)
    return A, B, W


def judge(D, I, W, Q, k):
    """as tests/test_search_async.py::test_margin_too_wide judges a search, over the rows the index holds (W, widened)"""
    ref = flatip.IndexFlatIP(W.shape[1]); ref.add(W)
    _, Ir = ref.search(Q, k)
    n = min(k, W.shape[0])
    assert (np.diff(D[:, :n], axis=1) <= 0).all()
    lazy = {}

    def full(q, disputed):
        if "W" not in lazy:
            lazy["W"], lazy["Q"] = torch.from_numpy(W).double(), torch.from_numpy(Q).double()
        sc = lazy["W"] @ lazy["Q"][q]
        return sc[torch.tensor(disputed)].numpy(), torch.topk(sc, n).values[-1].item()
    n_exact, n_tie, n_bad, detail = flatip.topk_sets_equal(I, Ir, full, rel_tol=2e-6)
    assert n_bad == 0, detail
    exact = np.einsum("qd,qkd->qk", Q.astype(np.float64), W[I[:, :n]].astype(np.float64))
    assert np.abs(D[:, :n] - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())
    return n_exact, n_tie


@pytest.mark.gpu
@pytest.mark.parametrize("n,nq,k,d", [(300, 5, 1000, 64), (4096, 7, 10, 64), (4097, 7, 10, 64), (20011, 1, 10, 256), (20011, 33, 100, 768),
                                      (20011, 33, 100, 1024), (20011, 16, 100, 2048), (30011, 130, 100, 320), (30011, 300, 1000, 256)])
def test_bits_of_the_two_copy_index(n, nq, k, d):
    rng = np.random.default_rng(n + nq + k + d)
    P = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    A, B, W = _pair(P)
    assert A._f32 is None
    q = torch.from_numpy(Q).to(DEV)
    ha, hb = A.search_device_async(q, k), B.search_device_async(q, k)
    ia, ib = ha.info(), hb.info()
    print(f"n={n} nq={nq} k={k} d={d}: async f16 {ia}; two-copy {ib}")
    assert torch.equal(ha.D, hb.D) and torch.equal(ha.I, hb.I)
    assert ia["kernel"] == ib["kernel"] and ia["rounds"] == ib["rounds"] and ia["redone"] == ib["redone"] == 0
    Db, Ib = B.search_device(q, k)
    Db, Ib, sb = Db.clone(), Ib.clone(), dict(B.last_search_info)
    Da, Ia = A.search_device(q, k)
    sa = dict(A.last_search_info)
    print(f"    sync f16 {sa}; two-copy {sb}")
    assert sb["scan"] == "f16+rescore" and not sb["margin_too_wide"]           # B took no float32 retry
    assert torch.equal(Da, Db) and torch.equal(Ia, Ib)
    assert torch.equal(Da, ha.D) and torch.equal(Ia, ha.I)
    assert sa["scan"] == "f16+rescore" and sa["kernel"] == sb["kernel"] and sa["redone"] == 0 and sa["overflow_fallbacks"] == 0
    D, I = Da.cpu().numpy(), Ia.cpu().numpy()
    if n < k:
        assert (I[:, n:] == -1).all() and (D[:, n:] == FLT_MIN).all()
    n_exact, n_tie = judge(D, I, W, Q, k)
    print(f"    id sets identical to the oracle's for {n_exact}/{nq}, fp64 near-tie only {n_tie}")


def rescore_rows(kernel, rows, Q, cand):
    """om_debug_rescore_rows over device tensors: rows [N, d] float32 or float16, Q [nq, d] f32, cand [nq, m] int32 (None: kernel 2)"""
    lib = N.lib()
    n, d = rows.shape
    nq = Q.shape[0]
    m = n if cand is None else cand.shape[1]
    out = torch.full((nq, m), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = lib.om_sim_topk_async_workspace_bytes(nq, d, 1)
    _buf, ws = N.Workspace.get(torch.device(DEV), nbytes, "test-rescore")
    N.check(lib.om_debug_rescore_rows(kernel, N.OM_F16 if rows.dtype == torch.float16 else N.OM_F32, N.ptr(rows), n, d, N.ptr(Q), nq,
                                      N.ptr(cand), m, N.ptr(out), N.c_void_p(ws), nbytes, N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 192, 256, 768, 2048])
def test_rescore_kernels_give_the_same_bits_on_float16_rows(d):
    rng = np.random.default_rng(d)
    n, nq, m = 301, 5, 40
    R16 = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).half()
    R16[7, :8] = torch.tensor([6.1e-5, 3e-6, -6e-8, 0.0, -0.0, 65504.0, -65504.0, 1.0]).half()      # subnormals, zeros, the largest values
    Qh = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(0, n, size=(nq, m)).astype(np.int32)
    cand[:, 0], cand[:, 1], cand[:, 2], cand[:, 3] = 0, n - 1, 7, 7                              # both ends of the buffer; a repeated row
    cand[:, 4:8] = cand[:, 8:12]
    r16 = R16.to(DEV).contiguous()
    r32 = r16.float().contiguous()
    Q, c = torch.from_numpy(Qh).to(DEV), torch.from_numpy(cand).to(DEV)
    exact = Qh.astype(np.float64) @ R16.double().numpy().T                                       # [nq, n]
    # |error| of a float32 dot product of d terms, any order: d * 2^-24 * sum |q_i p_i| bounds it
    bound = d * 2.0 ** -24 * (np.abs(Qh).astype(np.float64) @ np.abs(R16.double().numpy()).T) + 1e-30
    for kernel in (0, 1):
        a, b = rescore_rows(kernel, r16, Q, c), rescore_rows(kernel, r32, Q, c)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kernel
        want = np.take_along_axis(exact, cand.astype(np.int64), 1)
        assert (np.abs(a.cpu().numpy() - want) <= np.take_along_axis(bound, cand.astype(np.int64), 1)).all(), kernel
    a, b = rescore_rows(2, r16, Q, None), rescore_rows(2, r32, Q, None)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (np.abs(a.cpu().numpy() - exact) <= bound).all()
    # the redo's bits are the re-score's: the same (query, row) gives the same bits wherever it is computed
    every = torch.arange(n, dtype=torch.int32, device=DEV).repeat(nq, 1).contiguous()
    assert torch.equal(rescore_rows(0, r16, Q, every).view(torch.int32), a.view(torch.int32))


def _stats_of_two_copy(W):
    """what om_index_to_f16 leaves on the widened rows W [n, dpad] (device, f32)"""
    st = torch.zeros(2, dtype=torch.float32, device=DEV)
    tmp = torch.empty(W.shape, dtype=torch.float16, device=DEV)
    N.check(N.lib().om_index_to_f16(N.ptr(W), W.shape[0], W.shape[1], N.ptr(tmp), N.ptr(st), N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return st, tmp


@pytest.mark.gpu
@pytest.mark.parametrize("d", [100, 256])
def test_add_stores_the_float16_rows(d):
    from openmatch_amd.index import FlatIPIndex
    rng = np.random.default_rng(d)
    P = rng.standard_normal((4000, d)).astype(np.float32)
    P[5, :3] = [6.1e-5, 3e-6, 65504.0]
    want = torch.from_numpy(P).half()
    one = FlatIPIndex(d, device=DEV, precision="f16"); one.add(P)
    dpad = (d + 63) // 64 * 64
    assert one._f32 is None and one.ntotal == 4000 and one._f16.dtype == torch.float16
    assert one._f16.numel() * one._f16.element_size() == one.capacity * dpad * 2
    got = one._f16[:4000].cpu()
    assert torch.equal(got[:, :d].view(torch.int16), want.view(torch.int16))
    assert (got[:, d:] == 0).all() and got.shape[1] == dpad
    # two adds across a growth (1 000 rows fit the first 1 024, 3 000 more do not) leave the same index
    two = FlatIPIndex(d, device=DEV, precision="f16"); two.add(P[:1000])
    first = two._f16.data_ptr()
    two.add(torch.from_numpy(P[1000:]))
    assert two._f16.data_ptr() != first and two.ntotal == 4000
    assert torch.equal(two._f16[:4000].view(torch.int16), one._f16[:4000].view(torch.int16))
    assert torch.equal(two._stats, one._stats)
    # a device float16 tensor (and a numpy float16 array, and bfloat16 through float32) bit for bit
    h = FlatIPIndex(d, device=DEV, precision="f16"); h.add(want.to(DEV)); h.add(want.numpy())
    assert torch.equal(h._f16[:4000].view(torch.int16), one._f16[:4000].view(torch.int16))
    assert torch.equal(h._f16[4000:8000].view(torch.int16), one._f16[:4000].view(torch.int16))
    assert torch.equal(h._stats, one._stats)
    bf = torch.from_numpy(P[100:164]).bfloat16()                    # (rows without the 65504 above: bfloat16 rounds it to 65536)
    b = FlatIPIndex(d, device=DEV, precision="f16"); b.add(bf)
    assert torch.equal(b._f16[:64, :d].cpu().view(torch.int16), bf.float().half().view(torch.int16))
    # the statistics: no row error, and the norm word om_index_to_f16 leaves on the same values
    st, _ = _stats_of_two_copy(one._f16[:4000].float().contiguous())
    assert st[0].item() == 0.0
    assert one._stats[0].item() == 0.0 and torch.equal(one._stats.view(torch.int32), st.view(torch.int32))
    norm = one._f16[:4000].double().norm(dim=1).max().item()
    assert norm <= one._stats[1].item() <= norm * 1.001


@pytest.mark.gpu
def test_reserve_allocates_once():
    from openmatch_amd.index import FlatIPIndex
    rng = np.random.default_rng(1)
    P = rng.standard_normal((3000, 64)).astype(np.float32)
    for precision in ("f16", "f16_rescore", "f32"):
        idx = FlatIPIndex(64, device=DEV, precision=precision)
        idx.reserve(3000)
        assert idx.capacity == 3000
        ptr = idx._f16.data_ptr()
        for s in range(0, 3000, 700):
            idx.add(P[s:s + 700])
            assert idx._f16.data_ptr() == ptr
        assert idx.ntotal == 3000 and idx.capacity == 3000
        assert (idx._f32 is None) == (precision == "f16")
        idx.reserve(10)                                                  # never shrinks
        assert idx.capacity == 3000 and idx._f16.data_ptr() == ptr
        D, I = idx.search(P[:4], 1)
        assert (I[:, 0] == np.arange(4)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [1e6, float("nan"), float("inf")])
def test_values_beyond_float16_are_refused(poison):
    from openmatch_amd.index import FlatIPIndex
    rng = np.random.default_rng(2)
    P = rng.standard_normal((5000, 64)).astype(np.float32)
    Q = rng.standard_normal((3, 64)).astype(np.float32)
    idx = FlatIPIndex(64, device=DEV, precision="f16"); idx.add(P[:4500])
    before, stats = idx._f16[:4500].clone(), idx._stats.clone()
    bad = P[4500:].copy()
    bad[17, 5] = poison
    with pytest.raises(ValueError, match="65504"):
        idx.add(bad)
    assert idx.ntotal == 4500 and torch.equal(idx._f16[:4500], before) and torch.equal(idx._stats, stats)
    idx.add(P[4500:])
    h = idx.search_device_async(torch.from_numpy(Q).to(DEV), 10)
    assert h.info()["redone"] == 0
    judge(h.D.cpu().numpy(), h.I.cpu().numpy(), torch.from_numpy(P).half().float().numpy(), Q, 10)


_CACHE = {}


def tie_case():
    """tests/test_search_async.py's tie_case with the tied vector and the gaussian rows rounded to float16 FIRST, so that a float16-only
    index and a two-copy index hold the same values: 30 000 gaussian rows and 10 000 copies of v at shuffled positions, d = 256"""
    if "tie" not in _CACHE:
        rng = np.random.default_rng(30)
        d, k = 256, 100
        G = torch.from_numpy(rng.standard_normal((30000, d)).astype(np.float32)).half().float().numpy()
        v = torch.from_numpy(rng.standard_normal(d).astype(np.float32)).half().float().numpy()
        P = np.concatenate([G, np.tile(v, (10000, 1))])
        perm = rng.permutation(40000)
        P = np.ascontiguousarray(P[perm])
        copies = np.sort(np.nonzero(perm >= 30000)[0])                   # rows of P that hold v, ascending
        QG = rng.standard_normal((100, d)).astype(np.float32)
        along = (np.linspace(0.5, 1.5, 100, dtype=np.float32)[:, None] * v).astype(np.float32)
        ref = flatip.IndexFlatIP(d); ref.add(P)
        Dg, _ = ref.search(QG, k)
        assert ((QG.astype(np.float64) @ v.astype(np.float64)) < Dg[:, -1] - 5.0).all()      # no gaussian query reaches the tie
        A, B, W = _pair(P)
        assert np.array_equal(W, P)
        _CACHE["tie"] = dict(P=P, v=v, copies=copies, QG=QG, along=along, d=d, k=k, A=A, B=B)
    return _CACHE["tie"]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [4, 200])
def test_redo_on_ties(nq):
    c = tie_case()
    k, half = c["k"], nq // 2
    Q = np.empty((nq, c["d"]), np.float32)
    Q[0::2], Q[1::2] = c["along"][:half], c["QG"][:half]                 # tied and gaussian queries interleaved
    A, B = c["A"], c["B"]
    Dg, Ig = A.search_device(torch.from_numpy(np.ascontiguousarray(Q[1::2])).to(DEV), k)      # the gaussian queries alone
    Dg, Ig = Dg.clone(), Ig.clone()
    assert A.last_search_info["redone"] == 0
    q = torch.from_numpy(Q).to(DEV)
    ha, hb = A.search_device_async(q, k), B.search_device_async(q, k)
    got = ha.info()
    print(f"nq={nq}: {got}")
    assert got["redone"] >= half, got
    assert np.array_equal(ha.I.cpu().numpy()[0::2], np.tile(c["copies"][:k], (half, 1)))      # the k lowest rows of the tie, ascending
    want = (c["along"][:half].astype(np.float64) @ c["v"].astype(np.float64))[:, None]
    assert np.abs(ha.D.cpu().numpy()[0::2] - want).max() <= 1e-4 * np.abs(want).max()
    assert torch.equal(ha.D[1::2], Dg) and torch.equal(ha.I[1::2], Ig)
    assert torch.equal(ha.D, hb.D) and torch.equal(ha.I, hb.I)
    Ds, Is = A.search_device(q, k)                                       # the synchronous entry runs the same chain
    assert torch.equal(Ds, ha.D) and torch.equal(Is, ha.I)
    assert A.last_search_info["redone"] == got["redone"] and A.last_search_info["overflow_fallbacks"] == 0


@pytest.mark.gpu
def test_a_margin_nothing_certifies():
    """one row of 60 000 in every column -- finite in float16 -- makes max ||row|| ~ 1e6: the query-rounding term of the margin (~1e3)
    dwarfs the spread of the scores (~50), every list overflows, every query is redone"""
    n, nq, k, d = 20000, 3, 10, 256
    rng = np.random.default_rng(20000)
    P = rng.standard_normal((n, d)).astype(np.float32)
    P[777] = 60000.0
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    A, B, W = _pair(P)
    q = torch.from_numpy(Q).to(DEV)
    ha, hb = A.search_device_async(q, k), B.search_device_async(q, k)
    got = ha.info()
    print(got, hb.info())
    assert got["redone"] == 3, got
    assert torch.equal(ha.D, hb.D) and torch.equal(ha.I, hb.I)
    judge(ha.D.cpu().numpy(), ha.I.cpu().numpy(), W, Q, k)
    Ds, Is = A.search_device(q, k)
    info = A.last_search_info
    print(info)
    assert torch.equal(Ds, ha.D) and torch.equal(Is, ha.I)
    assert info["redone"] == 3 and info["margin_too_wide_queries"] == got["margin_too_wide_queries"]
    assert info["margin_too_wide"] == got["margin_too_wide"] and info["scan"] == "f16+rescore"


@pytest.mark.gpu
def test_capture():
    """one search captured with torch.cuda.graph on a side stream after an eager warm call; replayed with gaussian queries (the eager
    bits), then with the tied vector (all four redone, inside the replay)"""
    c = tie_case()
    idx, k = c["A"], 10
    QG = torch.from_numpy(c["QG"][:4]).to(DEV)
    Dg, Ig = idx.search_device(QG, k)
    Dg, Ig = Dg.clone(), Ig.clone()
    static_q = QG.clone()
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        warm = idx.search_device_async(static_q, k)                      # sets the kernels' function attributes
    stream.synchronize()
    assert torch.equal(warm.D, Dg) and torch.equal(warm.I, Ig)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        h = idx.search_device_async(static_q, k)
    h.D.zero_(); h.I.zero_()
    graph.replay()
    got = h.info()
    assert got["redone"] == 0 and torch.equal(h.D, Dg) and torch.equal(h.I, Ig), got
    static_q.copy_(torch.from_numpy(np.tile(c["v"], (4, 1))))
    graph.replay()
    got = h.info()
    assert got["redone"] == 4, got
    assert np.array_equal(h.I.cpu().numpy(), np.tile(c["copies"][:k], (4, 1)))


@pytest.mark.gpu
def test_search_offsets_reset_and_shards():
    from openmatch_amd.index import FlatIPIndex, merge_topk
    rng = np.random.default_rng(9)
    n, d, k = 9000, 128, 20
    P = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((6, d)).astype(np.float32)
    W = torch.from_numpy(P).half().float().numpy()
    idx = FlatIPIndex(d, device=DEV, precision="f16_only"); idx.add(P)      # (the alias)
    assert idx.precision == "f16"
    D, I = idx.search(Q, k)                                              # numpy in, numpy out
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (6, k)
    judge(D, I, W, Q, k)
    q = torch.from_numpy(Q).to(DEV)
    Do, Io = idx.search_device(q, k, id_offset=12345)
    assert np.array_equal(Io.cpu().numpy(), I + 12345) and np.array_equal(Do.cpu().numpy(), D)
    ho = idx.search_device_async(q, k, id_offset=12345)
    assert torch.equal(ho.I, Io) and torch.equal(ho.D, Do)
    # two float16-only shards, searched with their offsets and merged, are the whole index
    cut = 5000
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        sh = FlatIPIndex(d, device=DEV, precision="f16"); sh.add(P[lo:hi])
        parts.append(sh.search_device(q, k, id_offset=lo))
    Dm, Im = merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
    assert np.array_equal(Im.cpu().numpy(), I) and np.array_equal(Dm.cpu().numpy(), D)
    # reset, then reuse with other rows
    idx.reset()
    assert idx.ntotal == 0 and idx._f16 is None and idx._f32 is None and (idx._stats == 0).all()
    De, Ie = idx.search(Q, 3)
    assert (Ie == -1).all() and (De == FLT_MIN).all()
    idx.add(P[cut:])
    D2, I2 = idx.search(Q, k)
    assert np.array_equal(I2 + cut, parts[1][1].cpu().numpy()) and np.array_equal(D2, parts[1][0].cpu().numpy())
