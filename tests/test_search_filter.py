"""Filtered exact search on the GPU (om_sim_topk_filtered, FlatIPIndex.search_device_filtered*, RowFilter; DESIGN.md 4f "Filtered search").

The oracle of a filtered search is an unfiltered one: a fresh FlatIPIndex of the same precision built from the allowed rows in their
order, searched with search_device_async, its `I` mapped back through the id list.  In the two 16-bit modes every returned score is a
rescore_dot, so D and I must be EQUAL.  In 'f32' mode the dense bootstrap and the tile scan accumulate in different orders and which
of them scores a row depends on where it lies, so that mode is judged as tests/test_search_async.py::test_margin_too_wide judges a
search: oracle/flatip.py over the allowed rows, disputed ids adjudicated in float64.  Gaussian data throughout: no exact ties."""
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import flatip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLT_MIN = float(np.float32(-3.4028235e38))
PRECISIONS = ["f16_rescore", "f32", "f16"]
#         N     nq    k    d       family
SHAPES = [(20000, 1, 10, 256),     # stream32
          (20000, 33, 100, 768),   # stream32
          (20000, 16, 10, 1536),   # stream16
          (30011, 300, 100, 256),  # wide, strided re-score
          (4097, 7, 10, 64),       # generic
          (300, 5, 1000, 64)]      # one dense step, N < k
SHAPE_IDS = ["-".join(map(str, s)) for s in SHAPES]
_CACHE = {}


def data(n, nq, d):
    key = ("data", n, nq, d)
    if key not in _CACHE:
        rng = np.random.default_rng(n + nq + d)
        _CACHE[key] = (rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32))
    return _CACHE[key]


def index_of(n, nq, d, precision):
    from openmatch_amd.index import FlatIPIndex
    key = ("index", n, nq, d, precision)
    if key not in _CACHE:
        idx = FlatIPIndex(d, device=DEV, precision=precision)
        idx.add(data(n, nq, d)[0])
        _CACHE[key] = idx
    return _CACHE[key]


def uniform_mask(n, p, seed=0):
    return np.random.default_rng(1000 * n + int(p * 1000) + seed).random(n) < p


def check(precision, P, Q, k, mask, D, I, id_offset=0):
    """(D, I) device tensors of a filtered search of Q over the rows of P that `mask` allows, against the oracle"""
    from openmatch_amd.index import FlatIPIndex
    ids = np.nonzero(mask)[0]
    m = min(k, len(ids))
    Dn, In = D.cpu().numpy(), I.cpu().numpy()
    assert (In[:, m:] == -1).all() and (Dn[:, m:] == np.float32(FLT_MIN)).all()           # padding, and only there
    assert (In[:, :m] >= 0).all()
    if len(ids) == 0:
        return
    if precision != "f32":
        ref = FlatIPIndex(P.shape[1], device=DEV, precision=precision)
        ref.add(P[ids])
        h = ref.search_device_async(torch.from_numpy(Q).to(DEV), k)
        assert h.info()["redone"] == 0
        t = torch.from_numpy(ids).to(DEV)
        Io = torch.where(h.I >= 0, t[h.I.clamp(min=0)] + id_offset, h.I)
        assert torch.equal(D, h.D), f"scores differ from the oracle's in {(D != h.D).sum().item()} places"
        assert torch.equal(I, Io), f"ids differ from the oracle's in {(I != Io).sum().item()} places"
        return
    In = In - id_offset * (In >= 0)
    assert mask[In[:, :m]].all(), "a row the filter does not allow was returned"
    ref = flatip.IndexFlatIP(P.shape[1]); ref.add(P[ids])
    _, Ir = ref.search(Q, k)
    Ir = np.where(Ir >= 0, ids[np.maximum(Ir, 0)], -1)
    assert (np.diff(Dn[:, :m], axis=1) <= 0).all()
    A64, Q64 = torch.from_numpy(P[ids]).double(), torch.from_numpy(Q).double()
    pos = {int(r): j for j, r in enumerate(ids)}

    def full(q, disputed):
        sc = A64 @ Q64[q]
        return sc[torch.tensor([pos[r] for r in disputed])].numpy(), torch.topk(sc, m).values[-1].item()
    _, _, n_bad, detail = flatip.topk_sets_equal(In, Ir, full, rel_tol=2e-6)
    assert n_bad == 0, detail
    exact = np.einsum("qd,qkd->qk", Q.astype(np.float64), P[In[:, :m]].astype(np.float64))
    assert np.abs(Dn[:, :m] - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())


def run(idx, Q, k, rf, route=None, id_offset=0):
    h = idx.search_device_filtered_async(torch.from_numpy(Q).to(DEV), k, rf, id_offset=id_offset, route=route)
    info = h.info()
    return h.D, h.I, info


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", SHAPES, ids=SHAPE_IDS)
def test_all_ones_scan_is_the_unfiltered_search(precision, n, nq, k, d):
    from openmatch_amd.index import RowFilter
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    h = idx.search_device_async(torch.from_numpy(Q).to(DEV), k)
    want = h.info()
    rf = RowFilter(idx, torch.ones(n, dtype=torch.bool))
    assert (rf.n_allowed, rf.first, rf.last) == (n, 0, n - 1)
    D, I, got = run(idx, Q, k, rf, route="scan")
    print(f"[{precision}] {n} {nq} {k} {d}: unfiltered {want}; all-ones scan {got}")
    assert got["route"] == "scan" and got["n_allowed"] == n and got["redone"] == 0 and want["redone"] == 0
    assert torch.equal(D, h.D) and torch.equal(I, h.I)
    assert got["rounds"] == want["rounds"] and got["kernel"] == want["kernel"] and got["scan"] == want["scan"]


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("p", [0.9, 0.5])
@pytest.mark.parametrize("n,nq,k,d", SHAPES, ids=SHAPE_IDS)
def test_uniform_filters_on_every_route(precision, p, n, nq, k, d):
    from openmatch_amd.index import RowFilter
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    mask = uniform_mask(n, p)
    rf = RowFilter(idx, torch.from_numpy(mask))
    assert rf.n_allowed == int(mask.sum())
    for route in (None, "scan", "gather"):
        D, I, info = run(idx, Q, k, rf, route=route)
        print(f"[{precision}] {n} {nq} {k} {d} p={p} route={route}: {info}")
        assert info["route"] == (route or "scan") and info["n_allowed"] == rf.n_allowed
        if route is None:
            assert info["redone"] == 0, info
        check(precision, P, Q, k, mask, D, I)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_filter_that_defeats_the_bootstrap_is_redone(precision):
    """one allowed row among the first 12 000: no threshold exists when the first round starts, its lists overflow, all four are redone"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 4, 100, 256
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    r = np.arange(n)
    mask = (r == 0) | ((r >= 12000) & (r % 3 != 0))
    D, I, info = run(idx, Q, k, RowFilter(idx, torch.from_numpy(mask)), route="scan")
    print(f"[{precision}] {info}")
    check(precision, P, Q, k, mask, D, I)
    assert info["redone"] == 4, info


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("route", ["scan", "gather"])
def test_fewer_allowed_rows_than_k(precision, route):
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 33, 100, 768
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    ids = np.sort(np.random.default_rng(37).choice(n, 37, replace=False))
    mask = np.zeros(n, bool); mask[ids] = True
    D, I, info = run(idx, Q, k, RowFilter(idx, ids), route=route)
    print(f"[{precision}] {route}: {info}")
    assert info["n_allowed"] == 37 and info["route"] == route
    assert (I[:, :37] >= 0).all() and (I[:, 37:] == -1).all() and (D[:, 37:] == FLT_MIN).all()
    check(precision, P, Q, k, mask, D, I)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_redo_rank_is_counted_on_the_device(precision):
    """the same 37 rows, but the host's count is stale (every row of the scanned range): the schedule is the unfiltered one, no
    threshold ever forms, the lists overflow -- and the redo selects rank min(k, 37) from the count the device took"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 4, 100, 256
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    ids = np.sort(np.random.default_rng(38).choice(n, 37, replace=False))
    mask = np.zeros(n, bool); mask[ids] = True
    rf = RowFilter(idx, ids)
    rf.n_allowed = rf.last + 1 - rf.first // 256 * 256
    D, I, info = run(idx, Q, k, rf, route="scan")
    print(f"[{precision}] {info}")
    assert info["redone"] == nq, info
    assert (I[:, :37] >= 0).all() and (I[:, 37:] == -1).all() and (D[:, 37:] == FLT_MIN).all()
    check(precision, P, Q, k, mask, D, I)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("route", [None, "scan", "gather"])
def test_nothing_allowed_is_padding(precision, route):
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 4097, 7, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    D, I, info = run(idx, Q, k, RowFilter(idx, torch.zeros(n, dtype=torch.bool)), route=route)
    assert info["route"] == "empty" and info["n_allowed"] == 0 and info["redone"] == 0
    assert D.shape == (nq, k) and (D == FLT_MIN).all() and (I == -1).all()


def test_native_entry_with_an_empty_bitmap():
    """the route never sends an empty filter to the device; the entry itself must still answer it: padding"""
    from openmatch_amd import native as N
    n, nq, k, d = 20000, 4, 10, 256
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, "f16_rescore")
    q = torch.from_numpy(Q).to(DEV)
    words = torch.zeros((n + 31) // 32, dtype=torch.int32, device=DEV)
    D = torch.zeros(nq, k, dtype=torch.float32, device=DEV)
    I = torch.zeros(nq, k, dtype=torch.int64, device=DEV)
    lib = N.lib()
    nbytes = lib.om_sim_topk_filtered_workspace_bytes(nq, d, k)
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=DEV)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    with torch.cuda.device(DEV):
        N.check(lib.om_sim_topk_filtered(N.SEARCH_F16_RESCORE, N.ptr(q), nq, N.ptr(idx._f32), N.ptr(idx._f16), N.ptr(idx._stats), n, d, k, 0,
                                         N.ptr(words), 0, N.ptr(D), N.ptr(I), N.c_void_p(0), N.c_void_p(ws), nbytes, N.stream_ptr(idx.device)))
    torch.cuda.synchronize()
    assert (D == FLT_MIN).all() and (I == -1).all()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", SHAPES, ids=SHAPE_IDS)
def test_a_sparse_filter_gathers_and_caches_its_planes(precision, n, nq, k, d):
    from openmatch_amd.index import RowFilter, filter_route
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    mask = uniform_mask(n, 0.01)
    rf = RowFilter(idx, torch.from_numpy(mask))
    D, I, info = run(idx, Q, k, rf)
    print(f"[{precision}] {n} {nq} {k} {d} p=0.01: {info}")
    assert info["route"] == filter_route(precision, k, rf.first, rf.last, rf.n_allowed)
    if k >= 100 and n >= 20000:                    # (k = 10: k_eff is about 1000, whose list a scan still holds; 300 rows: the
        assert info["route"] == "gather"           # filter passes one row, which is a range)
    assert info["redone"] == 0
    check(precision, P, Q, k, mask, D, I)
    if info["route"] == "gather":
        planes = rf._gathered[3]
        assert planes.ntotal == rf.n_allowed and planes._f16.shape[0] == rf.n_allowed
        assert (planes._f32 is None) == (precision == "f16")
        before = (planes._f16.data_ptr(), rf._gathered[2].data_ptr())
        D2, I2, _ = run(idx, Q, k, rf)
        assert rf._gathered[3] is planes and (planes._f16.data_ptr(), rf._gathered[2].data_ptr()) == before
        assert torch.equal(D2, D) and torch.equal(I2, I)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cached_planes_do_not_outlive_the_index_contents(precision):
    """a filter names row numbers: after the index is reset and filled with as many OTHER rows, the same filter searches those (the
    gather route builds its planes anew instead of searching the ones it cached), and so after an `add` to the index"""
    from openmatch_amd.index import FlatIPIndex, RowFilter
    n, nq, k, d = 20000, 33, 100, 768
    P, Q = data(n, nq, d)
    P2 = np.ascontiguousarray(P[::-1])
    idx = FlatIPIndex(d, device=DEV, precision=precision)
    idx.add(P)
    mask = uniform_mask(n, 0.01)
    rf = RowFilter(idx, torch.from_numpy(mask))
    D, I, info = run(idx, Q, k, rf)
    assert info["route"] == "gather"
    check(precision, P, Q, k, mask, D, I)
    planes = rf._gathered[3]
    idx.reset()
    idx.add(P2[:n // 2]); idx.add(P2[n // 2:])
    D, I, info = run(idx, Q, k, rf)
    assert info["route"] == "gather" and rf._gathered[3] is not planes
    check(precision, P2, Q, k, mask, D, I)
    idx.add(P[:7])                                  # the index has grown: the filter is for another ntotal
    with pytest.raises(ValueError, match=str(n)):
        run(idx, Q, k, rf)


# ---------------------------------------------------------------------------------------------------------------- 7, 8
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_contiguous_run_is_a_range(precision):
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 33, 100, 768
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    mask = np.zeros(n, bool); mask[5000:17000] = True
    rf = RowFilter(idx, np.arange(5000, 17000))
    assert (rf.n_allowed, rf.first, rf.last) == (12000, 5000, 16999)
    D, I, info = run(idx, Q, k, rf, id_offset=1 << 33)
    assert info["route"] == "range" and info["redone"] == 0
    check(precision, P, Q, k, mask, D, I, id_offset=1 << 33)
    Ds, Is, _ = run(idx, Q, k, rf, route="scan", id_offset=1 << 33)      # the same rows through the bitmap
    check(precision, P, Q, k, mask, Ds, Is, id_offset=1 << 33)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_exclusion_list(precision):
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 30011, 300, 100, 256
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    gone = np.random.default_rng(8).choice(n, 3000, replace=False)
    mask = np.ones(n, bool); mask[gone] = False
    a = RowFilter(idx, torch.from_numpy(gone).to(DEV), invert=True)
    b = RowFilter(idx, torch.from_numpy(mask))
    assert torch.equal(a.words, b.words) and (a.n_allowed, a.first, a.last) == (b.n_allowed, b.first, b.last)
    Da, Ia, info = run(idx, Q, k, a)
    Db, Ib, _ = run(idx, Q, k, b)
    assert info["route"] == "scan" and torch.equal(Da, Db) and torch.equal(Ia, Ib)
    assert not np.isin(Ia.cpu().numpy(), gone).any()
    check(precision, P, Q, k, mask, Da, Ia)


def test_a_filter_for_another_index_is_refused():
    from openmatch_amd.index import RowFilter
    idx, other = index_of(4097, 7, 64, "f32"), index_of(300, 5, 64, "f32")
    rf = RowFilter(other, torch.ones(300, dtype=torch.bool))
    with pytest.raises(ValueError, match="300"):
        idx.search_device_filtered(torch.from_numpy(data(4097, 7, 64)[1]).to(DEV), 10, rf)


def test_numpy_form_and_last_search_info():
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 4097, 7, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, "f16_rescore")
    mask = uniform_mask(n, 0.5, seed=3)
    D, I = idx.search_filtered(Q, k, RowFilter(idx, mask))
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
    info = idx.last_search_info
    assert info["route"] == "scan" and info["n_allowed"] == int(mask.sum()) and info["redone"] == 0
    check("f16_rescore", P, Q, k, mask, torch.from_numpy(D).to(DEV), torch.from_numpy(I).to(DEV))


# ---------------------------------------------------------------------------------------------------------------- 9
def test_capture():
    """one scan-route search captured on a side stream after an eager warm call, replayed with the queries it was captured with and
    then with others; the handle (workspace, status, bitmap) stays alive"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 33, 100, 768
    P, Q = data(n, nq, d)
    Q2 = np.random.default_rng(99).standard_normal((nq, d)).astype(np.float32)
    idx = index_of(n, nq, d, "f16_rescore")
    mask = uniform_mask(n, 0.5, seed=9)
    rf = RowFilter(idx, torch.from_numpy(mask))
    static_q = torch.from_numpy(Q).to(DEV)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        warm = idx.search_device_filtered_async(static_q, k, rf)          # sets the kernels' function attributes
    stream.synchronize()
    check("f16_rescore", P, Q, k, mask, warm.D, warm.I)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        h = idx.search_device_filtered_async(static_q, k, rf)
    del rf
    h.D.zero_(); h.I.zero_()
    graph.replay()
    got = h.info()
    assert got["route"] == "scan" and got["redone"] == 0, got
    assert torch.equal(h.D, warm.D) and torch.equal(h.I, warm.I)
    static_q.copy_(torch.from_numpy(Q2))
    graph.replay()
    assert h.info()["redone"] == 0
    check("f16_rescore", P, Q2, k, mask, h.D, h.I)


# ---------------------------------------------------------------------------------------------------------------- 10
def tiny_retriever(tmp_path, P, Q):
    from types import SimpleNamespace as NS
    from openmatch_amd.retriever import Retriever
    docs, queries = [f"d{i}" for i in range(len(P))], [f"q{i}" for i in range(len(Q))]
    for kind, rows, ids in (("corpus", P, docs), ("query", Q, queries)):
        with open(os.path.join(tmp_path, f"embeddings.{kind}.rank.0"), "wb") as f:
            pickle.dump((rows, ids), f, protocol=4)
    args = NS(device=DEV, output_dir=str(tmp_path), world_size=1, process_index=0, local_process_index=0, fp16=False)
    return Retriever.from_embeddings(torch.nn.Identity(), args)


@pytest.mark.parametrize("last_kept", [True, False], ids=["last-doc-kept", "last-doc-not-kept"])
def test_retriever_doc_filter_keeps_fewer_than_topk(tmp_path, last_kept):
    """12 kept documents, topk = 20: every query gets exactly the 12, in the oracle's order with the search's scores -- the padding names
    no document (it would name the corpus's last one: a document the filter does not keep, or a real hit whose score it would overwrite)"""
    n, nq, k, d = 300, 5, 20, 64
    P, Q = data(n, nq, d)
    r = tiny_retriever(tmp_path, P, Q)
    rows = [int(i) for i in np.random.default_rng(11).choice(n - 1, 11, replace=False)] + [n - 1 if last_kept else n - 2]
    keep = {f"d{i}" for i in rows}
    got = r.search(k, doc_filter=keep)
    ref = flatip.IndexFlatIP(d); ref.add(P)
    Dr, Ir = ref.search(Q, n)                                             # the oracle's full ranking, filtered
    for q in range(nq):
        want = [(f"d{i}", s) for i, s in zip(Ir[q], Dr[q]) if f"d{i}" in keep]
        assert len(want) == 12 and list(got[f"q{q}"]) == [doc for doc, _ in want]
        exact = np.array([s for _, s in want], dtype=np.float64)          # the bound `check` puts on a float32 score
        assert np.abs(np.array(list(got[f"q{q}"].values())) - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())
    r.query_lookup = []
    assert r.search(k, doc_filter=["not-a-doc"]) == {f"q{q}": {} for q in range(nq)}      # nothing kept: no hit


def test_retriever_doc_filter(tmp_path):
    n, nq, k, d = 300, 5, 20, 64
    P, Q = data(n, nq, d)
    r = tiny_retriever(tmp_path, P, Q)
    keep = {f"d{i}" for i in np.random.default_rng(10).choice(n, 120, replace=False)} | {"not-a-doc"}
    got = r.search(k, doc_filter=keep)
    ref = flatip.IndexFlatIP(d); ref.add(P)
    _, Ir = ref.search(Q, n)                                              # the oracle's full ranking, filtered
    for q in range(nq):
        want = [f"d{i}" for i in Ir[q] if f"d{i}" in keep][:k]
        assert list(got[f"q{q}"]) == want
    r.query_lookup = []
    assert r.search(k) != got and len(r.search(k)) == nq                 # (unfiltered: other documents)
    r.args.world_size = 2
    with pytest.raises(NotImplementedError, match="shard"):
        r.search(k, doc_filter=keep)
