"""The stream-ordered search (om_sim_topk_async, FlatIPIndex.search_device_async; DESIGN.md 4f "Stream-ordered search").

  CPU   the symbols, the workspace size, the refusals; the fast schedule both entries run (csrc/search_plan.h search_schedule through
        om_debug_search_schedule) by its properties: starts behind the 4 096 dense rows, contiguous to N, whole tiles, no sliver
  GPU   nothing to redo: the bits of search_device, and its `scan` / `kernel`
  GPU   a 10 000-way exact tie (longer than the 8 192-key list whatever the chunking): the tied queries are redone on the device -- the
        lowest rows of the tie, in order -- and the other queries of the batch keep the bits of a synchronous search
  GPU   a certified margin that is not finite; a search captured in a graph (a synchronisation inside the entry would fail the capture);
        two searches in flight on one stream and on two"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from oracle import flatip

DEV = "cuda:0"
DENSE_CHUNK = 4096
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
def test_the_three_symbols_exist():
    lib = N.lib()
    for name in ("om_sim_topk_async_workspace_bytes", "om_sim_topk_async", "om_debug_search_schedule"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None


@pytest.mark.parametrize("n,d,k", [(1, 64, 1), (7, 256, 10), (128, 768, 1000), (300, 768, 100), (6980, 768, 1000), (32768, 64, 2048)])
def test_workspace_covers_the_synchronous_one(n, d, k):
    lib = N.lib()
    assert lib.om_sim_topk_async_workspace_bytes(n, d, k) >= lib.om_sim_topk_workspace_bytes(n, d, k) > 0
    assert lib.om_sim_topk_async_workspace_bytes(0, d, k) == 0 and lib.om_sim_topk_async_workspace_bytes(-3, d, k) == 0


def _refused(k=10, status=0x2000, **kw):
    """one call with pointers that are never followed: every refusal comes before the first launch"""
    fake = N.c_void_p(0x1000)
    return N.lib().om_sim_topk_async(N.SEARCH_F16_RESCORE, fake, 3, fake, fake, fake, 5000, 64, k, 0, fake, fake,
                                     N.c_void_p(status) if status else N.c_void_p(0), fake, 1 << 40, N.c_void_p(0))


def test_k_above_2048_is_refused():
    assert _refused(k=2049) == 1
    assert b"2048" in N.lib().om_last_error()


def test_a_null_status_is_refused():
    assert _refused(status=0) == 1
    assert b"status" in N.lib().om_last_error()


def test_refuses_when_the_fast_schedule_is_switched_off():
    with switched(N.OPT_SCAN_GEN7, 0):
        assert _refused() == 1
        assert b"OM_OPT_SCAN_GEN7" in N.lib().om_last_error()


def schedule(mode, nq, n, k):
    cap = 1024
    chunks, cnt = (C.c_int64 * cap)(), C.c_int(-1)
    N.check(N.lib().om_debug_search_schedule(mode, nq, n, k, chunks, cap, C.byref(cnt)))
    assert 0 <= cnt.value <= cap
    return list(chunks[:cnt.value])


@pytest.mark.parametrize("mode", [N.SEARCH_F32, N.SEARCH_F16_RESCORE], ids=["f32", "f16"])
@pytest.mark.parametrize("k", [10, 1000])
@pytest.mark.parametrize("nq", [1, 64, 300, 6980])
@pytest.mark.parametrize("n", [4097, 50000, 8841823])
def test_schedule_properties(mode, k, nq, n):
    """chunks[i] is the number of rows of round i; round 0 starts at row DENSE_CHUNK and round i + 1 where round i ended"""
    chunks = schedule(mode, nq, n, k)
    assert chunks and all(c > 0 for c in chunks)
    starts = np.concatenate([[DENSE_CHUNK], DENSE_CHUNK + np.cumsum(chunks)])
    assert starts[0] == DENSE_CHUNK and starts[-1] == n                  # contiguous by construction of `starts`, and they end at N
    assert all(c % 256 == 0 for c in chunks[:-1])
    assert all(4 * b >= a for a, b in zip(chunks, chunks[1:])), chunks  # no chunk smaller than a quarter of its predecessor ...
    if len(chunks) > 1:
        assert 4 * chunks[-1] >= chunks[-2]                              # ... the last one in particular


@pytest.mark.parametrize("n", [0, 1, 300, 4095, 4096])
def test_a_shard_of_at_most_one_dense_chunk_has_no_rounds(n):
    for mode in (N.SEARCH_F32, N.SEARCH_F16_RESCORE):
        assert schedule(mode, 7, n, 10) == []


def test_schedule_counts_rounds_beyond_the_callers_array():
    full = schedule(N.SEARCH_F16_RESCORE, 6980, 8841823, 1000)
    assert len(full) > 3
    chunks, cnt = (C.c_int64 * 4)(-1, -1, -1, -1), C.c_int(0)
    N.check(N.lib().om_debug_search_schedule(N.SEARCH_F16_RESCORE, 6980, 8841823, 1000, chunks, 3, C.byref(cnt)))
    assert cnt.value == len(full) and list(chunks) == full[:3] + [-1]


# ------------------------------------------------------------------------------------------------------------- GPU
PRECISIONS = ["f16_rescore", "f32"]
_CACHE = {}


def _index(P, precision):
    from openmatch_amd.index import FlatIPIndex
    idx = FlatIPIndex(P.shape[1], device=DEV, precision=precision)
    idx.add(P)
    return idx


def _sync(idx, Q, k):
    D, I = idx.search_device(torch.from_numpy(Q).to(DEV), k)
    return D.clone(), I.clone(), dict(idx.last_search_info)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", [(20000, 1, 10, 256), (20000, 33, 100, 768), (30011, 300, 100, 256), (300, 5, 1000, 64),
                                      (4096, 7, 10, 64), (4097, 7, 10, 64)])
def test_same_bits_as_the_sync_entry_when_nothing_is_redone(precision, n, nq, k, d):
    rng = np.random.default_rng(n + nq + k)
    P = rng.standard_normal((n, d)).astype(np.float32)                   # gaussian: no exact ties
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = _index(P, precision)
    D, I, info = _sync(idx, Q, k)
    h = idx.search_device_async(torch.from_numpy(Q).to(DEV), k)
    got = h.info()
    print(f"[{precision}] n={n} nq={nq} k={k} d={d}: sync {info}; async {got}")
    assert got["redone"] == 0, got
    assert torch.equal(h.D, D) and torch.equal(h.I, I)
    assert got["scan"] == info["scan"] and got["kernel"] == info["kernel"], (got, info)
    if n < k:
        assert (h.I[:, n:] == -1).all() and (h.D[:, n:] == float(FLT_MIN)).all()


def tie_case():
    """30 000 gaussian rows and 10 000 copies of one vector v at shuffled positions, d = 256; 100 gaussian queries none of which scores
    the tie into its top 100 (checked here: such a query would be redone too, and an f32-mode redo returns the re-score's bits, not the
    scan's); the oracle's answers, computed once"""
    if "tie" not in _CACHE:
        rng = np.random.default_rng(30)                                  # (a seed at which the check below holds)
        d, k = 256, 100
        G = rng.standard_normal((30000, d)).astype(np.float32)
        v = rng.standard_normal(d).astype(np.float32)
        P = np.concatenate([G, np.tile(v, (10000, 1))])
        perm = rng.permutation(40000)
        P = np.ascontiguousarray(P[perm])
        copies = np.sort(np.nonzero(perm >= 30000)[0])                   # rows of P that hold v, ascending
        QG = rng.standard_normal((100, d)).astype(np.float32)
        along = (np.linspace(0.5, 1.5, 100, dtype=np.float32)[:, None] * v).astype(np.float32)
        ref = flatip.IndexFlatIP(d); ref.add(P)
        Dg, _ = ref.search(QG, k)
        assert ((QG.astype(np.float64) @ v.astype(np.float64)) < Dg[:, -1] - 5.0).all()
        Da, _ = ref.search(along, k)
        _CACHE["tie"] = dict(P=P, v=v, copies=copies, QG=QG, along=along, Da=np.asarray(Da), d=d, k=k)
    return _CACHE["tie"]


def tie_index(precision):
    key = ("tie-index", precision)
    if key not in _CACHE:
        _CACHE[key] = _index(tie_case()["P"], precision)
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nq", [4, 200])
def test_redo_on_ties(precision, nq):
    c = tie_case()
    k, half = c["k"], nq // 2
    Q = np.empty((nq, c["d"]), np.float32)
    Q[0::2], Q[1::2] = c["along"][:half], c["QG"][:half]                 # tied and gaussian queries interleaved
    idx = tie_index(precision)
    Dg, Ig, _ = _sync(idx, np.ascontiguousarray(Q[1::2]), k)              # the gaussian queries alone
    h = idx.search_device_async(torch.from_numpy(Q).to(DEV), k)
    got = h.info()
    D, I = h.D.cpu().numpy(), h.I.cpu().numpy()
    rel = np.abs(D[0::2] - c["Da"][:half]).max() / np.abs(c["Da"][:half]).max()
    print(f"[{precision}] nq={nq}: {got}; tied scores off the oracle's by {rel:.3g} relative")
    assert got["redone"] >= half, got
    assert np.abs(D[0::2] - c["Da"][:half]).max() <= 1e-4 * np.abs(c["Da"][:half]).max()
    assert np.array_equal(I[0::2], np.tile(c["copies"][:k], (half, 1)))  # the k lowest rows of the tie, ascending
    assert torch.equal(h.D[1::2], Dg) and torch.equal(h.I[1::2], Ig)


@pytest.mark.gpu
def test_margin_too_wide():
    """one row beyond f16: the rounding statistics are +inf, no margin certifies anything, every query is redone -- judged as
    tests/test_gpu_parity.py::test_flat_ip_search_matches_oracle judges a search"""
    n, nq, k, d = 5000, 3, 10, 256
    rng = np.random.default_rng(5000)
    P = rng.standard_normal((n, d)).astype(np.float32)
    P[100] = 1e6
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = _index(P, "f16_rescore")
    h = idx.search_device_async(torch.from_numpy(Q).to(DEV), k)
    got = h.info()
    print(got)
    assert got["margin_too_wide_queries"] == 3 and got["margin_too_wide"] and got["redone"] == 3, got
    D, I = h.D.cpu().numpy(), h.I.cpu().numpy()
    ref = flatip.IndexFlatIP(d); ref.add(P)
    _, Ir = ref.search(Q, k)
    assert (np.diff(D, axis=1) <= 0).all()
    P64, Q64 = torch.from_numpy(P).double(), torch.from_numpy(Q).double()

    def full(q, disputed):
        sc = P64 @ Q64[q]
        return sc[torch.tensor(disputed)].numpy(), torch.topk(sc, k).values[-1].item()
    n_exact, n_tie, n_bad, detail = flatip.topk_sets_equal(I, Ir, full, rel_tol=2e-6)
    assert n_bad == 0, detail
    exact = np.einsum("qd,qkd->qk", Q.astype(np.float64), P[I].astype(np.float64))
    assert np.abs(D - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())


@pytest.mark.gpu
def test_capture():
    """one search captured with torch.cuda.graph on a side stream after an eager warm call; replayed with gaussian queries (the bits of
    the synchronous search), then with the tied vector (all four redone, inside the replay)"""
    c = tie_case()
    idx, k = tie_index("f16_rescore"), 10
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
def test_searches_in_flight():
    """two handles back to back on one stream with nothing between, then two indexes on two streams: four correct results, so every
    handle has a workspace of its own"""
    c = tie_case()
    rng = np.random.default_rng(77)
    k = 100
    A = _index(rng.standard_normal((20000, 256)).astype(np.float32), "f16_rescore")
    B = tie_index("f16_rescore")
    Q1 = rng.standard_normal((33, 256)).astype(np.float32)
    Q2 = rng.standard_normal((7, 256)).astype(np.float32)
    QB = np.ascontiguousarray(c["QG"][:40])
    want = {"a1": _sync(A, Q1, k), "a2": _sync(A, Q2, k), "b": _sync(B, QB, k)}
    q1, q2, qb = (torch.from_numpy(x).to(DEV) for x in (Q1, Q2, QB))
    torch.cuda.synchronize()
    h1 = A.search_device_async(q1, k)
    h2 = A.search_device_async(q2, k)
    torch.cuda.synchronize()
    for h, key in ((h1, "a1"), (h2, "a2")):
        assert torch.equal(h.D, want[key][0]) and torch.equal(h.I, want[key][1]), key
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(s1):
        g1 = A.search_device_async(q1, k)
    with torch.cuda.stream(s2):
        g2 = B.search_device_async(qb, k)
    torch.cuda.synchronize()
    assert torch.equal(g1.D, want["a1"][0]) and torch.equal(g1.I, want["a1"][1])
    assert torch.equal(g2.D, want["b"][0]) and torch.equal(g2.I, want["b"][1])
    assert g1.info()["redone"] == 0 and g2.info()["redone"] == 0
