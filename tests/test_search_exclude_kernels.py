"""drop_excluded_kernel alone (om_debug_drop_lists_excluding: the drop of om_sim_topk_excluding launched as that entry launches it, over
lists handed in) against a numpy compaction: a key stays, in its order, when its row is below nrows and not in the query's exclusion
list; a query whose list is empty keeps its keys as they are; a count above SORT_CAP is clamped and marked.  Bit-exact: the kernel moves
keys, it computes nothing.  DESIGN.md 4f "Exclusion lists"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SORT_CAP = 8192
EXCLUDE_MAX = 4096
QSTAT_OVERFLOW = 1
STALE_ROW = 0xf0000000
NROWS = 3000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table_of(excl):
    """per-query id lists, each ascending without repeats -> int32 [nq, pitch >= 1] padded with -1, as the entry takes it"""
    pitch = max(1, max(len(e) for e in excl))
    t = np.full((len(excl), pitch), -1, np.int32)
    for q, e in enumerate(excl):
        e = np.asarray(e, np.int64)
        assert (np.diff(e) > 0).all() and (e >= 0).all() and (e < 2 ** 31).all()
        t[q, :len(e)] = e
    return t


def run_drop(lists, counts, excl, nrows=NROWS, use_qstat=True):
    """om_debug_drop_lists_excluding over lists [(scores, rows)]; returns (scores, rows [nq][8192], cnt, qstat, flag, m)"""
    from openmatch_amd import native as N
    lib = N.lib()
    nq = len(lists)
    m = max(1, max(len(s) for s, _ in lists))
    sc = np.zeros((nq, m), np.float32)
    ro = np.zeros((nq, m), np.uint32)
    for q, (s, r) in enumerate(lists):
        sc[q, :len(s)], ro[q, :len(s)] = s, r
    table = table_of(excl)
    d_sc, d_ro, d_cnt, d_ex = dev(sc), dev(ro.view(np.int32)), dev(np.asarray(counts, np.uint32).view(np.int32)), dev(table)
    o_sc = torch.empty((nq, SORT_CAP), dtype=torch.float32, device=DEV)
    o_ro = torch.empty((nq, SORT_CAP), dtype=torch.int32, device=DEV)
    o_st = torch.full((nq * 4 + 4,), -1, dtype=torch.int32, device=DEV)
    nbytes = lib.om_sim_topk_async_workspace_bytes(nq, 64, 1)
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=DEV)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    with torch.cuda.device(DEV):
        N.check(lib.om_debug_drop_lists_excluding(nq, m, N.ptr(d_sc), N.ptr(d_ro), N.ptr(d_cnt), int(use_qstat), N.ptr(d_ex), table.shape[1], nrows,
                                                  N.ptr(o_sc), N.ptr(o_ro), N.ptr(o_st), N.c_void_p(ws), nbytes,
                                                  N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    st = o_st.cpu().numpy().view(np.uint32)
    per = st[:nq * 4].reshape(nq, 4)
    return o_sc.cpu().numpy(), o_ro.cpu().numpy().view(np.uint32), per[:, 0], per[:, 3], st[nq * 4:], m


def drop_reference(scores, rows, count, m, excluded, nrows=NROWS):
    """what list q holds after the drop: (scores, rows, cnt, overflow).  scores / rows: the slots handed in, padded to m with (0, row 0);
    slots m .. 8191 hold stale keys (score +inf, row 0xf0000000 + slot).  excluded: the query's list; empty: the keys stay as they are."""
    s = np.concatenate([np.asarray(scores, np.float32), np.zeros(m - len(scores), np.float32), np.full(SORT_CAP - m, np.inf, np.float32)])
    r = np.concatenate([np.asarray(rows, np.uint32), np.zeros(m - len(rows), np.uint32), STALE_ROW + np.arange(m, SORT_CAP, dtype=np.uint32)])
    n = min(int(count), SORT_CAP)
    if len(excluded) == 0:
        return s[:n], r[:n], n, count > SORT_CAP
    ok = (r[:n] < nrows) & ~np.isin(r[:n], np.asarray(excluded, np.int64).astype(np.uint32))
    return s[:n][ok], r[:n][ok], int(ok.sum()), count > SORT_CAP


def compare(lists, counts, excl, got, marked=()):
    sc, ro, cnt, qstat, flag, m = got
    for q, (s, r) in enumerate(lists):
        ws, wr, wn, overflow = drop_reference(s, r, counts[q], m, excl[q])
        assert cnt[q] == wn, (q, cnt[q], wn)
        assert np.array_equal(ro[q, :wn], wr), f"query {q}: rows or their order differ"
        assert np.array_equal(sc[q, :wn].view(np.uint32), ws.view(np.uint32)), f"query {q}: a score left its row"
        assert overflow == (q in marked) and qstat[q] == (QSTAT_OVERFLOW if q in marked else 0)
    assert flag[0] == (1 if marked else 0)


def fixture(length, seed):
    """four queries: an empty list, one id, EXCLUDE_MAX ids reaching far beyond nrows, 300 ids; key rows mostly inside [0, nrows), some
    at and beyond it, repeats allowed (the scan never appends one, the kernel does not care)"""
    rng = np.random.default_rng(seed)
    lists = [(rng.standard_normal(length).astype(np.float32), rng.integers(0, NROWS + 40, length).astype(np.uint32)) for _ in range(4)]
    one = [int(lists[1][1][length // 2])] if length else [5]
    excl = [[], one, np.sort(rng.choice(NROWS + 4000, EXCLUDE_MAX, replace=False)), np.sort(rng.choice(NROWS, 300, replace=False))]
    return lists, excl


@pytest.mark.parametrize("length", [0, 1, 255, 256, 257, SORT_CAP])
def test_drop_against_numpy(length):
    lists, excl = fixture(length, seed=length)
    got = run_drop(lists, [length] * 4, excl)
    compare(lists, [length] * 4, excl, got)
    cnt = got[2]
    assert cnt[0] == length                           # nothing to exclude: every key stays, those beyond nrows too
    if length >= 255:
        assert cnt[1] < length and 0 < cnt[2] < length * 0.6 and length * 0.7 < cnt[3] < length      # 1 / ~59 % / ~11 % of the keys go


@pytest.mark.parametrize("over", [0, 2], ids=["empty-list-query", "full-list-query"])
def test_drop_clamps_and_marks_one_query(over):
    """one count above SORT_CAP (a round whose appends were dropped): clamped, flag[0] set, QSTAT_OVERFLOW for that query alone"""
    lists, excl = fixture(SORT_CAP, seed=77 + over)
    counts = [300, 257, 300, 1]
    counts[over] = 9000
    got = run_drop(lists, counts, excl)
    compare(lists, counts, excl, got, marked=(over,))
    assert got[2][over] <= SORT_CAP and (over != 0 or got[2][0] == SORT_CAP)
    # without qstat (the chain's last selection): clamped and flagged, no query marked
    _, _, cnt2, qstat2, flag2, _ = run_drop(lists, counts, excl, use_qstat=False)
    assert np.array_equal(cnt2, got[2]) and (qstat2 == 0).all() and flag2[0] == 1


def test_every_key_excluded():
    rng = np.random.default_rng(3)
    rows = [rng.permutation(NROWS)[:n].astype(np.uint32) for n in (600, 256, 1)]
    lists = [(rng.standard_normal(len(r)).astype(np.float32), r) for r in rows]
    excl = [np.sort(r.astype(np.int64)) for r in rows]
    got = run_drop(lists, [len(r) for r in rows], excl)
    assert got[2].tolist() == [0, 0, 0]
    compare(lists, [len(r) for r in rows], excl, got)


def test_ids_at_and_beyond_n_match_nothing():
    """a list of ids >= nrows only, the largest an int32 holds among them: every key of [0, nrows) stays"""
    rng = np.random.default_rng(4)
    rows = rng.permutation(NROWS)[:700].astype(np.uint32)
    rows[[0, 350, 699]] = [NROWS - 1, 0, NROWS - 1]
    lists = [(rng.standard_normal(700).astype(np.float32), rows)] * 2
    excl = [[NROWS, NROWS + 1, NROWS + 77, 2 ** 31 - 1], [NROWS - 1, NROWS, 2 ** 31 - 2, 2 ** 31 - 1]]
    got = run_drop(lists, [700, 700], excl)
    compare(lists, [700, 700], excl, got)
    assert got[2][0] == 700 and got[2][1] == 700 - int((rows == NROWS - 1).sum())


@pytest.mark.parametrize("where", ["head", "tail", "steps", "all-three"])
def test_excluded_keys_at_the_head_the_tail_and_every_step_boundary(where):
    """1030 keys are five steps of 256: the excluded keys sit at slot 0, at the last slot, and on both sides of every 256-key step"""
    n = 1030
    rng = np.random.default_rng(6)
    rows = rng.permutation(NROWS)[:n].astype(np.uint32)
    slots = {"head": list(range(0, 9)), "tail": list(range(n - 9, n)), "steps": [s + o for s in (256, 512, 768, 1024) for o in (-1, 0)]}
    slots["all-three"] = sorted(set(slots["head"] + slots["tail"] + slots["steps"]))      # (the last step's boundary lies in the tail)
    lists = [(rng.standard_normal(n).astype(np.float32), rows)]
    excl = [np.sort(rows[slots[where]].astype(np.int64))]
    got = run_drop(lists, [n], excl)
    compare(lists, [n], excl, got)
    assert got[2][0] == n - len(slots[where])
    kept = np.delete(rows, slots[where])
    assert np.array_equal(got[1][0, :len(kept)], kept)                    # the kept keys, in their original order
