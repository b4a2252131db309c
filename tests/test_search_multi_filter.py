"""Exact search with a filter per query on the GPU (om_sim_topk_filtered_multi, om_sim_topk_candidates, om_debug_drop_lists_multi,
FlatIPIndex.search_device_filtered_multi* / search_device_candidates*, Retriever.search(doc_filters=...); DESIGN.md 4f "A filter per query").

The oracle is the existing single-filter search, per group of queries that share a filter, and search_device_async for unfiltered
queries.  In the two 16-bit precisions every returned score is a rescore_dot: D and I must be EQUAL.  In 'f32' the batch and the group
plan different scan kernels, so that precision is judged as tests/test_search_filter.py::check judges a search (oracle/flatip.py over the
allowed rows, disputed ids in float64 at rel_tol 2e-6, scores within 1e-4 * max(1, |exact|): that file's own tolerances).  Gaussian data
throughout: no exact ties."""
import numpy as np
import pytest
import torch

from tests.test_search_filter import DEV, FLT_MIN, PRECISIONS, check, data, index_of, tiny_retriever, uniform_mask

pytestmark = pytest.mark.gpu

SORT_CAP = 8192
QSTAT_OVERFLOW = 1
STALE_ROW = 0xf0000000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def judge(precision, idx, P, Q, k, masks, filter_of, D, I, id_offset=0):
    """(D, I) of a multi-filter search against the oracle: per bitmap the single-filter search of its queries, search_device_async for
    the queries at -1.  filter_of: host ints per query; masks: bool [N] per bitmap."""
    from openmatch_amd.index import RowFilter
    filter_of = np.asarray(filter_of)
    for f in sorted(set(filter_of.tolist())):
        sel = np.nonzero(filter_of == f)[0]
        t = torch.from_numpy(sel).to(DEV)
        Dg, Ig = D.index_select(0, t), I.index_select(0, t)
        if f < 0:
            h = idx.search_device_async(dev(Q[sel]), k, id_offset=id_offset)
            if precision != "f32":
                assert h.info()["redone"] == 0
                assert torch.equal(Dg, h.D) and torch.equal(Ig, h.I), f"unfiltered queries differ from search_device_async"
            else:
                check(precision, P, Q[sel], k, np.ones(len(P), bool), Dg, Ig, id_offset=id_offset)
        elif precision != "f32":
            h = idx.search_device_filtered_async(dev(Q[sel]), k, RowFilter(idx, torch.from_numpy(masks[f])), id_offset=id_offset)
            h.info()
            assert torch.equal(Dg, h.D), f"bitmap {f}: scores differ from the single-filter search in {(Dg != h.D).sum().item()} places"
            assert torch.equal(Ig, h.I), f"bitmap {f}: ids differ from the single-filter search in {(Ig != h.I).sum().item()} places"
        else:
            check(precision, P, Q[sel], k, masks[f], Dg, Ig, id_offset=id_offset)


def native_multi(idx, Q, k, words, filter_of, n_allowed_min, id_offset=0):
    """om_sim_topk_filtered_multi over all rows of idx through FlatIPIndex._enqueue_multi: words [F, pitch] int32 on the device"""
    from openmatch_amd.index import SearchHandle
    q, D, I, mode = idx._search_args(dev(Q), k)
    fo = None if filter_of is None else dev(np.asarray(filter_of, np.int32))
    chunks = idx._enqueue_multi(q, D, I, mode, k, idx._f32, idx._f16, idx.ntotal, id_offset, words, fo, n_allowed_min)
    h = SearchHandle(D, I, q, chunks, idx.device)
    return D, I, h.info()


# ---------------------------------------------------------------------------------------------------------------- 1
#         N     nq    k    d       family
MIXED = [(20011, 33, 100, 768),    # stream32; N no multiple of 32
         (20000, 16, 10, 1536),    # stream16
         (30011, 300, 100, 256),   # wide, strided re-score
         (4097, 7, 10, 64)]        # generic


def four_masks(n):
    # the run starts at row 0: a filter with no allowed row in the bootstrap's chunk has no threshold when the rounds begin and is redone,
    # alone (the single form's test_a_filter_that_defeats_the_bootstrap_is_redone) as in a batch (test_the_redo_is_per_query below)
    run = np.zeros(n, bool)
    run[:n // 2 + 3] = True
    return [uniform_mask(n, 0.9), uniform_mask(n, 0.5), np.ones(n, bool), run]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", MIXED, ids=["-".join(map(str, s)) for s in MIXED])
def test_mixed_batch(precision, n, nq, k, d):
    """four bitmaps and unfiltered queries in one call; then the same call through the native entry with a pitch 8 words larger than
    needed, bits set beyond N in a last word and in the pitch padding: the same bits"""
    from openmatch_amd.index import RowFilter
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    masks = four_masks(n)
    filters = [RowFilter(idx, torch.from_numpy(m)) for m in masks]
    filter_of = [-1 if q % 5 == 4 else q % 4 for q in range(nq)]
    h = idx.search_device_filtered_multi_async(dev(Q), k, filters, filter_of=filter_of)
    info = h.info()
    print(f"[{precision}] {n} {nq} {k} {d}: {info}")
    assert info["parts"] == [{"route": "scan", "queries": nq, "n_filters": 4}]
    assert info["redone"] == 0, info              # the schedule is the single-filter one of p = 0.5
    judge(precision, idx, P, Q, k, masks, filter_of, h.D, h.I)
    words_needed = (n + 31) // 32
    pitch = words_needed + 8
    words = np.zeros((4, pitch), np.uint32)
    for f, m in enumerate(masks):
        words[f, :words_needed] = np.packbits(np.concatenate([m, np.zeros(-n % 32, bool)]), bitorder="little").view(np.uint32)
    words[:, words_needed:] = 0xffffffff                                  # the pitch padding
    if n % 32:
        words[1, words_needed - 1] |= np.uint32(0xffffffff) << np.uint32(n % 32)      # bits at and beyond N in the last word
    n_min = min(int(m.sum()) for m in masks)
    D, I, info2 = native_multi(idx, Q, k, dev(words.view(np.int32)), filter_of, n_min)
    assert info2["redone"] == 0 and info2["rounds"] == info["rounds"] and info2["kernel"] == info["kernel"]
    if precision != "f32":
        assert torch.equal(D, h.D) and torch.equal(I, h.I)
    else:
        judge(precision, idx, P, Q, k, masks, filter_of, D, I)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_bitmap_per_query_without_filter_of(precision):
    """filter_of = NULL: query q under bitmap q"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 4097, 7, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    masks = [uniform_mask(n, p, seed=s) for s, p in enumerate([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3])]
    filters = [RowFilter(idx, torch.from_numpy(m)) for m in masks]
    h = idx.search_device_filtered_multi_async(dev(Q), k, filters)
    info = h.info()
    assert info["parts"] == [{"route": "scan", "queries": nq, "n_filters": nq}]
    assert idx._multi_last["parts"][0]["filter_of"] is None               # the native entry got a NULL filter_of
    judge(precision, idx, P, Q, k, masks, list(range(nq)), h.D, h.I)
    words = torch.stack([f.words for f in filters]).contiguous()
    D, I, _ = native_multi(idx, Q, k, words, None, min(f.n_allowed for f in filters), id_offset=1 << 33)
    judge(precision, idx, P, Q, k, masks, list(range(nq)), D, I, id_offset=1 << 33)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_redo_is_per_query(precision):
    """query 0 under the mask that defeats the bootstrap, query 1 under 37 rows, queries 2 and 3 under p = 0.9 -- and the host's count
    stale (n_allowed_min = N: the unfiltered schedule).  The first two overflow and are redone, each to the rank min(k, rows of ITS
    bitmap) counted on the device; the other two keep the bits of their single-filter search."""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20000, 4, 100, 256
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    r = np.arange(n)
    few = np.zeros(n, bool)
    few[np.sort(np.random.default_rng(37).choice(n, 37, replace=False))] = True
    masks = [(r == 0) | ((r >= 12000) & (r % 3 != 0)), few, uniform_mask(n, 0.9)]
    filter_of = [0, 1, 2, 2]
    words = torch.stack([RowFilter(idx, torch.from_numpy(m)).words for m in masks]).contiguous()
    D, I, info = native_multi(idx, Q, k, words, filter_of, n)
    print(f"[{precision}] {info}")
    assert info["redone"] >= 1, info
    assert (I[1, :37] >= 0).all() and (I[1, 37:] == -1).all() and (D[1, 37:] == FLT_MIN).all()
    judge(precision, idx, P, Q, k, masks, filter_of, D, I)
    # the forced scan route of the Python form plans for the sparsest bitmap (37 rows: everything is scored densely): exact as well
    filters = [RowFilter(idx, torch.from_numpy(m)) for m in masks]
    h = idx.search_device_filtered_multi_async(dev(Q), k, filters, filter_of=filter_of, route="scan")
    assert h.info()["parts"] == [{"route": "scan", "queries": nq, "n_filters": 3}]
    judge(precision, idx, P, Q, k, masks, filter_of, h.D, h.I)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", MIXED, ids=["-".join(map(str, s)) for s in MIXED])
def test_all_queries_unfiltered_is_the_unfiltered_search(precision, n, nq, k, d):
    from openmatch_amd.index import RowFilter
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    want_h = idx.search_device_async(dev(Q), k)
    want = want_h.info()
    rf = RowFilter(idx, torch.from_numpy(uniform_mask(n, 0.5)))
    h = idx.search_device_filtered_multi_async(dev(Q), k, [rf, None], filter_of=[-1 if q % 2 else 1 for q in range(nq)])
    got = h.info()
    assert got["parts"] == [{"route": "scan", "queries": nq, "n_filters": 0}] and got["redone"] == 0 and want["redone"] == 0
    assert torch.equal(h.D, want_h.D) and torch.equal(h.I, want_h.I)
    assert got["rounds"] == want["rounds"] and got["kernel"] == want["kernel"] and got["scan"] == want["scan"]


# ---------------------------------------------------------------------------------------------------------------- 5
CAND_N, CAND_PITCH = 20011, 5000


def candidate_lists(n, k, seed):
    """per query 0, 1, k - 1, 4096, 4097 and 5000 distinct candidates at pitch 5000: rows 0 and N - 1 among them, a repeated row wherever a
    column is free, the columns shuffled"""
    rng = np.random.default_rng(seed)
    cand = np.full((6, CAND_PITCH), -1, np.int64)
    rows = []
    for q, c in enumerate([0, 1, k - 1, 4096, 4097, 5000]):
        ids = rng.choice(np.arange(1, n - 1), max(c - 2, 0), replace=False)
        ids = np.concatenate([ids, [0, n - 1]])[-c:] if c else ids[:0]
        rows.append(np.sort(ids))
        line = list(ids)
        if 0 < c < CAND_PITCH:
            line += [int(ids[0])] * min(3, CAND_PITCH - c)                # repeats of one row
        line += [-1] * (CAND_PITCH - len(line))
        cand[q] = rng.permutation(np.array(line))
    return cand, rows


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("k", [10, 1000])
def test_candidates(precision, d, k):
    from openmatch_amd.index import RowFilter
    n, nq = CAND_N, 6
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    cand, rows = candidate_lists(n, k, seed=k + d)
    D, I = idx.search_device_candidates(dev(Q), k, dev(cand), id_offset=7)
    info = idx.last_search_info
    assert info["route"] == "candidates" and info["redone"] == 0
    Dh, Ih = idx.search_candidates(Q, k, cand)                            # candidates on the host, id_offset 0
    assert np.array_equal(Dh, D.cpu().numpy()) and np.array_equal(np.where(Ih >= 0, Ih + 7, Ih), I.cpu().numpy())
    In = I.cpu().numpy()
    for q in range(nq):
        m = min(k, len(rows[q]))
        got = In[q, :m] - 7
        assert len(set(got.tolist())) == m and np.isin(got, rows[q]).all(), f"query {q}: a repeated or foreign id"
        assert (In[q, m:] == -1).all() and (D[q, m:] == FLT_MIN).all()    # padding exactly where fewer than k candidates exist
        mask = np.zeros(n, bool)
        mask[rows[q]] = True
        if precision != "f32":
            h = idx.search_device_filtered_async(dev(Q[q:q + 1]), k, RowFilter(idx, rows[q]), id_offset=7)
            h.info()
            assert torch.equal(D[q:q + 1], h.D) and torch.equal(I[q:q + 1], h.I), f"query {q} ({len(rows[q])} candidates)"
        else:
            check(precision, P, Q[q:q + 1], k, mask, D[q:q + 1], I[q:q + 1], id_offset=7)


def test_candidate_holes_are_never_followed():
    """the native entry with unsorted lists: -1, N, 2^31 - 1 and -5 are holes wherever they stand"""
    from openmatch_amd.index import SearchHandle
    n, nq, k, d = CAND_N, 6, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, "f16_rescore")
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(n)[:300] for _ in range(nq)]).astype(np.int64)
    want = idx.search_device_candidates(dev(Q), k, dev(cand))
    holes = np.array([-1, n, 2 ** 31 - 1, -5, n + 12345])
    wide = np.concatenate([cand, np.tile(holes, (nq, 20))], axis=1)
    wide = np.stack([rng.permutation(row) for row in wide]).astype(np.int32)
    q, D, I, mode = idx._search_args(dev(Q), k)
    keep = idx._enqueue_candidates(q, D, I, mode, k, dev(wide), 0)
    SearchHandle(D, I, q, [], idx.device, {"_keep": keep}).info()
    assert torch.equal(D, want[0]) and torch.equal(I, want[1])
    with pytest.raises(ValueError, match="outside"):
        idx.search_device_candidates(dev(Q), k, dev(wide.astype(np.int64)))
    with pytest.raises(ValueError, match="outside"):
        idx.search_device_candidates(dev(Q), k, wide.astype(np.int64))     # on the host: checked there


# ---------------------------------------------------------------------------------------------------------------- 6
def run_drop(lists, counts, words, nrows, filter_of, use_qstat=True):
    """om_debug_drop_lists_multi over lists [(scores, rows)]; returns (scores, rows [nq][8192], cnt, qstat, flag)"""
    from openmatch_amd import native as N
    lib = N.lib()
    nq = len(lists)
    m = max(1, max(len(s) for s, _ in lists))
    sc = np.zeros((nq, m), np.float32)
    ro = np.zeros((nq, m), np.uint32)
    for q, (s, r) in enumerate(lists):
        sc[q, :len(s)], ro[q, :len(s)] = s, r
    d_sc, d_ro, d_cnt = dev(sc), dev(ro.view(np.int32)), dev(np.asarray(counts, np.uint32).view(np.int32))
    d_words = dev(np.ascontiguousarray(words, np.uint32).view(np.int32))
    d_of = None if filter_of is None else dev(np.asarray(filter_of, np.int32))
    o_sc = torch.empty((nq, SORT_CAP), dtype=torch.float32, device=DEV)
    o_ro = torch.empty((nq, SORT_CAP), dtype=torch.int32, device=DEV)
    o_st = torch.full((nq * 4 + 4,), -1, dtype=torch.int32, device=DEV)
    nbytes = lib.om_sim_topk_async_workspace_bytes(nq, 64, 1)
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=DEV)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    with torch.cuda.device(DEV):
        N.check(lib.om_debug_drop_lists_multi(nq, m, N.ptr(d_sc), N.ptr(d_ro), N.ptr(d_cnt), int(use_qstat), N.ptr(d_words), nrows,
                                              words.shape[1], words.shape[0], N.ptr(d_of), N.ptr(o_sc), N.ptr(o_ro), N.ptr(o_st),
                                              N.c_void_p(ws), nbytes, N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    st = o_st.cpu().numpy().view(np.uint32)
    per = st[:nq * 4].reshape(nq, 4)
    return o_sc.cpu().numpy(), o_ro.cpu().numpy().view(np.uint32), per[:, 0], per[:, 3], st[nq * 4:], m


def drop_reference(scores, rows, count, m, bits, nrows):
    """what list q holds after the drop: (scores, rows, cnt, overflow).  scores / rows: the m slots handed in (slots m .. 8191 hold stale
    keys: score +inf, row 0xf0000000 + slot).  bits: bool [>= nrows] of the query's bitmap, None for a query under no filter, False for
    one with nothing allowed."""
    s = np.concatenate([np.asarray(scores, np.float32), np.zeros(m - len(scores), np.float32), np.full(SORT_CAP - m, np.inf, np.float32)])
    r = np.concatenate([np.asarray(rows, np.uint32), np.zeros(m - len(rows), np.uint32), STALE_ROW + np.arange(m, SORT_CAP, dtype=np.uint32)])
    n = min(int(count), SORT_CAP)
    if bits is None:
        return s[:n], r[:n], n, count > SORT_CAP
    if bits is False:
        return s[:0], r[:0], 0, count > SORT_CAP
    ok = np.array([row < nrows and bits[row] for row in r[:n]], bool)
    return s[:n][ok], r[:n][ok], int(ok.sum()), count > SORT_CAP


DROP_NROWS = 1000


def drop_fixture(length, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2 ** 32, size=(2, (DROP_NROWS + 31) // 32 + 3), dtype=np.uint64).astype(np.uint32)      # pitch 3 words wider
    bits = [np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool) for w in words]
    # rows: mostly inside [0, nrows), some at and beyond it (their bit, where the padded bitmap has one, is not to be read)
    lists = [(rng.standard_normal(length).astype(np.float32), rng.integers(0, DROP_NROWS + 40, length).astype(np.uint32)) for _ in range(3)]
    return words, bits, lists


@pytest.mark.parametrize("length", [0, 255, 256, 257, 8192])
def test_drop_per_query_against_numpy(length):
    words, bits, lists = drop_fixture(length, seed=length)
    filter_of = [1, 0, -1]
    sc, ro, cnt, qstat, flag, m = run_drop(lists, [length] * 3, words, DROP_NROWS, filter_of)
    for q, f in enumerate(filter_of):
        ws, wr, wn, _ = drop_reference(lists[q][0], lists[q][1], length, m, None if f < 0 else bits[f], DROP_NROWS)
        assert cnt[q] == wn, (q, cnt[q], wn)
        assert np.array_equal(sc[q, :wn].view(np.uint32), ws.view(np.uint32)) and np.array_equal(ro[q, :wn], wr), f"query {q}"
        assert qstat[q] == 0
    assert flag[0] == 0
    if length:
        assert 0 < cnt[0] < length and 0 < cnt[1] < length and cnt[2] == length


@pytest.mark.parametrize("over", [0, 2], ids=["filtered-query", "unfiltered-query"])
def test_drop_clamps_and_marks_one_query(over):
    """one count above SORT_CAP (a round whose appends were dropped): clamped, flag[0] set, QSTAT_OVERFLOW for that query alone"""
    words, bits, lists = drop_fixture(SORT_CAP, seed=77 + over)
    counts = [300, 257, 300]
    counts[over] = 9000
    filter_of = [1, 0, -1]
    sc, ro, cnt, qstat, flag, m = run_drop(lists, counts, words, DROP_NROWS, filter_of)
    for q, f in enumerate(filter_of):
        ws, wr, wn, overflow = drop_reference(lists[q][0], lists[q][1], counts[q], m, None if f < 0 else bits[f], DROP_NROWS)
        assert overflow == (q == over)
        assert cnt[q] == wn and cnt[q] <= SORT_CAP
        assert np.array_equal(sc[q, :wn].view(np.uint32), ws.view(np.uint32)) and np.array_equal(ro[q, :wn], wr), f"query {q}"
        assert qstat[q] == (QSTAT_OVERFLOW if q == over else 0)
    assert flag[0] == 1
    if over == 2:
        assert cnt[2] == SORT_CAP
    # without qstat (the chain's last selection): clamped and flagged, no query marked
    *_, cnt2, qstat2, flag2, _ = run_drop(lists, counts, words, DROP_NROWS, filter_of, use_qstat=False)
    assert np.array_equal(cnt2, cnt) and (qstat2 == 0).all() and flag2[0] == 1


def test_drop_without_filter_of_and_with_nothing_allowed():
    words, bits, lists = drop_fixture(300, seed=5)
    sc, ro, cnt, qstat, flag, m = run_drop(lists, [300] * 3, words, DROP_NROWS, [7, 0, 2])      # 7, 2 >= n_filters: nothing allowed
    assert cnt[0] == 0 and cnt[2] == 0 and 0 < cnt[1] < 300
    words3 = np.concatenate([words, words[:1] ^ np.uint32(0xffffffff)])
    bits3 = bits + [~bits[0]]
    sc, ro, cnt, qstat, flag, m = run_drop(lists, [300] * 3, words3, DROP_NROWS, None)           # query q under bitmap q
    for q in range(3):
        ws, wr, wn, _ = drop_reference(lists[q][0], lists[q][1], 300, m, bits3[q], DROP_NROWS)
        assert cnt[q] == wn and np.array_equal(ro[q, :wn], wr) and np.array_equal(sc[q, :wn].view(np.uint32), ws.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("precision", PRECISIONS)
def test_router_end_to_end(precision):
    """one call: a dense group (scan), a 2-query sparse group (candidates), a 9-query sparse group (gather: one query beyond the measured
    crossover of 8), an empty filter (candidates) -- interleaved, so the permutation is no identity"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20011, 33, 100, 768
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    masks = [uniform_mask(n, 0.5, seed=1), uniform_mask(n, 0.01, seed=2), uniform_mask(n, 0.01, seed=3), np.zeros(n, bool)]
    filters = [RowFilter(idx, torch.from_numpy(m)) for m in masks]
    filter_of = [0] * nq
    for q in (3, 20):
        filter_of[q] = 1
    for q in (0, 1, 5, 7, 8, 13, 19, 27, 32):
        filter_of[q] = 2
    filter_of[11] = 3
    h = idx.search_device_filtered_multi_async(dev(Q), k, filters, filter_of=filter_of, id_offset=5)
    info = h.info()
    print(f"[{precision}] {info}")
    assert info["parts"] == [{"route": "scan", "queries": nq - 12, "n_filters": 1}, {"route": "gather", "queries": 9, "n_filters": 1},
                             {"route": "candidates", "queries": 3, "n_filters": 2}]
    assert info["redone"] == 0
    assert (h.I[11] == -1).all() and (h.D[11] == FLT_MIN).all()
    judge(precision, idx, P, Q, k, masks, filter_of, h.D, h.I, id_offset=5)
    planes = filters[2]._gathered[3]
    assert planes.ntotal == filters[2].n_allowed and filters[1]._gathered is None      # the 2-query group gathered nothing
    before = planes._f16.data_ptr()
    plan = idx._multi_last
    h2 = idx.search_device_filtered_multi_async(dev(Q), k, filters, filter_of=filter_of, id_offset=5)
    h2.info()
    assert idx._multi_last is plan and filters[2]._gathered[3] is planes and planes._f16.data_ptr() == before
    assert torch.equal(h2.D, h.D) and torch.equal(h2.I, h.I)
    # forced routes: one part each, the same answer (16-bit: the same bits)
    live = [0 if f == 3 else f for f in filter_of]
    ha = idx.search_device_filtered_multi_async(dev(Q), k, filters, filter_of=live, id_offset=5)
    ha.info()
    for route in ("scan", "candidates"):
        if route == "candidates" and precision == "f32":
            continue                                  # (f32 lists are scored by the re-score, scans by the MFMA: judged in test_candidates)
        hf = idx.search_device_filtered_multi_async(dev(Q[:12]), k, filters, filter_of=live[:12], id_offset=5, route=route)
        got = hf.info()
        assert [p["route"] for p in got["parts"]] == [route]
        if precision != "f32":
            assert torch.equal(hf.D, ha.D[:12]) and torch.equal(hf.I, ha.I[:12]), route
        else:
            judge(precision, idx, P, Q[:12], k, masks, live[:12], hf.D, hf.I, id_offset=5)


def test_one_filter_for_every_query_is_the_single_form():
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 4097, 7, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, "f16_rescore")
    rf = RowFilter(idx, torch.from_numpy(uniform_mask(n, 0.5)))
    want = idx.search_device_filtered_async(dev(Q), k, rf)
    wi = want.info()
    for filters, filter_of in (([rf] * nq, None), ([None, rf], [1] * nq)):
        D, I = idx.search_device_filtered_multi(dev(Q), k, filters, filter_of=filter_of)
        got = idx.last_search_info
        assert got["parts"] == [{"route": "scan", "queries": nq, "n_filters": 1}] and got["route"] == "scan"
        assert torch.equal(D, want.D) and torch.equal(I, want.I) and got["rounds"] == wi["rounds"] and got["n_allowed"] == rf.n_allowed
    Dn, In = idx.search_filtered_multi(Q, k, [rf] * nq)
    assert np.array_equal(Dn, want.D.cpu().numpy()) and np.array_equal(In, want.I.cpu().numpy())
    other = index_of(300, 5, 64, "f16_rescore")
    with pytest.raises(ValueError, match="300"):
        idx.search_device_filtered_multi(dev(Q), k, [RowFilter(other, torch.ones(300, dtype=torch.bool))] * nq)
    with pytest.raises(ValueError, match="filter"):
        idx.search_device_filtered_multi(dev(Q), k, [rf], filter_of=[0] * (nq - 1) + [1])


# ---------------------------------------------------------------------------------------------------------------- 8
def test_capture():
    """the multi-filter search and the candidate search, each captured on a side stream after one eager call, replayed with the queries
    they were captured with and then with others in place"""
    from openmatch_amd.index import RowFilter
    n, nq, k, d = 20011, 33, 100, 768
    P, Q = data(n, nq, d)
    Q2 = np.random.default_rng(99).standard_normal((nq, d)).astype(np.float32)
    idx = index_of(n, nq, d, "f16_rescore")
    masks = [uniform_mask(n, 0.5, seed=9), uniform_mask(n, 0.9, seed=9), uniform_mask(n, 0.01, seed=9)]
    filters = [RowFilter(idx, torch.from_numpy(m)) for m in masks]
    filter_of = [(-1 if q % 7 == 6 else q % 2) for q in range(nq)]
    filter_of[5] = filter_of[6] = 2                                        # a candidates part beside the scan part
    cand = dev(np.stack([np.random.default_rng(q).permutation(n)[:300] for q in range(nq)]))
    static_q = dev(Q)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        warm = idx.search_device_filtered_multi_async(static_q, k, filters, filter_of=filter_of)
        warm_c = idx.search_device_candidates_async(static_q, k, cand)
    stream.synchronize()
    assert [p["route"] for p in warm.info()["parts"]] == ["scan", "candidates"]
    judge("f16_rescore", idx, P, Q, k, masks, filter_of, warm.D, warm.I)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        h = idx.search_device_filtered_multi_async(static_q, k, filters, filter_of=filter_of)
        hc = idx.search_device_candidates_async(static_q, k, cand)
    h.D.zero_(); h.I.zero_(); hc.D.zero_(); hc.I.zero_()
    graph.replay()
    assert h.info()["redone"] == 0
    assert torch.equal(h.D, warm.D) and torch.equal(h.I, warm.I)
    assert torch.equal(hc.D, warm_c.D) and torch.equal(hc.I, warm_c.I)
    static_q.copy_(torch.from_numpy(Q2))
    graph.replay()
    torch.cuda.synchronize()
    eager = idx.search_device_filtered_multi_async(dev(Q2), k, filters, filter_of=filter_of)
    eager_c = idx.search_device_candidates_async(dev(Q2), k, cand)
    torch.cuda.synchronize()
    assert torch.equal(h.D, eager.D) and torch.equal(h.I, eager.I)
    assert torch.equal(hc.D, eager_c.D) and torch.equal(hc.I, eager_c.I)
    judge("f16_rescore", idx, P, Q2, k, masks, filter_of, h.D, h.I)


# ---------------------------------------------------------------------------------------------------------------- 9
def test_retriever_doc_filters(tmp_path):
    """a run dict {qid: {docid: score}}: per query the documents and scores of doc_filter=<that query's docs> searched alone"""
    n, nq, k, d = 300, 5, 20, 64
    P, Q = data(n, nq, d)
    r = tiny_retriever(tmp_path, P, Q)
    rng = np.random.default_rng(12)
    run = {f"q{q}": {f"d{i}": float(s) for i, s in zip(rng.choice(n, c, replace=False), rng.random(c))}
           for q, c in zip(range(4), [120, 12, 1, 0])}                    # q3: an empty collection; q4: absent
    run["q1"]["not-a-doc"] = 1.0
    got = r.search(k, doc_filters=run)
    assert set(got) == {f"q{q}" for q in range(nq)}
    for q in range(4):
        r.query_lookup = []
        alone = r.search(k, doc_filter=list(run[f"q{q}"]))[f"q{q}"]
        assert list(got[f"q{q}"]) == list(alone), f"q{q}"
        if r.index.precision != "f32":
            assert got[f"q{q}"] == alone
        else:
            for doc, s in alone.items():
                assert abs(got[f"q{q}"][doc] - s) < 1e-4 * max(1.0, abs(s))
    assert len(got["q0"]) == k and len(got["q1"]) == 12 and len(got["q2"]) == 1 and got["q3"] == {}
    r.query_lookup = []
    assert got["q4"] == r.search(k)["q4"]                                  # absent from the mapping: searched unfiltered
    r.query_lookup = []
    with pytest.raises(ValueError, match="doc_filter"):
        r.search(k, doc_filter=["d1"], doc_filters=run)
