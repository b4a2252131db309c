"""The list kernels of the exact search (csrc/search.hip) -- everything between the scan's raw appends and the (D, I) the caller gets --
each against an exact sort in numpy, through om_debug_select_lists / om_debug_query_prep, which launch them as the search does:

    select_radix_kernel   the per-round selection: staged and unstaged (n > cap) branch, the n <= k return, ties beyond the LDS copy
    select_kernel         the final bitonic sort with the certified cut
    drop_disallowed_kernel, append_dense_kernel + check_overflow_kernel, emit_kernel
    merge_kernel          through om_topk_merge
    query_prep_kernel     the float16 query panel and the certified margin

The kernels work on keys, not on arithmetic: key = orderable(score) << 32 | ~row, ordered by score descending, then row ascending.  Every
assertion on a list is bit-exact.  The one bound is the margin's: with E = |q| Ep + |q - fl16(q)| Pn and S = depth 2^-24 max(|q|, |fl16(q)|)
(Pn + Ep) in float64, E + S <= margin <= (1.01 E + S)(1 + 1e-5).  The lower bound is what certifies; the 1e-5 is derived: every float32
sum of the kernel is a chain of at most d / 64 fused multiply-adds plus 6 butterfly additions of non-negative terms, ~40 roundings of 2^-24
at d = 2048 = 2.4e-6 relative, halved by the square roots, plus a handful of roundings in the final expression.

Every list launch runs 5 to 16 queries with different lengths and contents, so q * SORT_CAP, cnt[q] and margin[q] are tested as well.
A list is followed by stale keys with score +inf up to slot 8191 (the tests' own up to m, the hook's behind m): a kernel that reads beyond
its count selects one of them and fails the comparison.

One end-to-end case, for what the kernel tests found: a margin that is not finite has to raise flag[2], the only word om_sim_topk's path
reads -- a query with an element beyond float16 came back empty from it (test_search_with_a_query_beyond_float16_is_still_exact).

Host only (no GPU): the argument refusals of both hooks, and the numpy reference against a plain np.sort of the keys."""
import numpy as np
import pytest
import torch

from openmatch_amd import native as N

DEV = "cuda:0"
SORT_CAP, LIST_MAX, K_MAX = 8192, 4096, 2048
QSTAT_OVERFLOW, QSTAT_WIDE, QSTAT_COVER = 1, 2, 4
STALE_ROW = 0xf0000000          # the hook's stale slots m .. 8191: (+inf, STALE_ROW + slot)
PAD_ROW = 0xe0000000            # this file's stale slots behind a list shorter than m: (+inf, PAD_ROW + slot)
FLT_MIN = np.float32(-3.4028235e38)
THR_UNWRITTEN = 0x7fc00000      # the hook's thr before the kernel
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- the numpy reference
def orderable(s):
    """csrc/common.h f32_orderable: unsigned codes in the order of the floats (-0.0 just below +0.0)"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def code(x):
    return orderable(np.array([x], np.float32))[0]


def keys_of(s, r):
    """csrc/search_keys.h pack_key"""
    return (orderable(s).astype(np.uint64) << np.uint64(32)) | (~np.asarray(r, dtype=np.uint32)).astype(np.uint64)


def cut_of(kth, margin):
    """the certified cut in float32, as the kernels take it"""
    if margin is None:
        return f32(kth)
    with np.errstate(all="ignore"):
        return f32(f32(kth) - f32(2.0) * f32(margin))


def ref_radix(s, r, count, k, margin, cap):
    """What select_radix_kernel must leave of the list (s, r)[0:count].  keys: the kept keys, sorted (None: the list stays as it is);
    subset: more keys pass than the LDS copy of the unstaged branch holds -- any `cap` of them are kept and the round is an overflow"""
    n = min(int(count), SORT_CAP)
    s, r = s[:n], r[:n]
    w = dict(n=n, overflow=count > SORT_CAP, early=n <= k, subset=False, keys=None, keep=int(count), kth=None,
             nonfinite=margin is not None and not np.isfinite(margin))
    if n <= k:
        w["thr"] = cut_of(s.min(), margin) if n == k else f32(-np.inf)
        w["wide"] = w["nonfinite"]
        return w
    keys = keys_of(s, r)
    order = np.argsort(keys, kind="stable")[::-1]
    w["kth"] = s[order[k - 1]]                               # the score of the k-th largest key, by bits
    w["thr"] = cut_of(w["kth"], margin)
    kept = s >= w["thr"]                                     # a FLOAT comparison: -0.0 passes a cut of +0.0
    w["keys"] = np.sort(keys[kept])
    w["keep"] = int(kept.sum())
    if n > cap and w["keep"] > cap:
        w["subset"], w["overflow"], w["keep"] = True, True, cap
    w["wide"] = w["nonfinite"] or (margin is not None and w["keep"] > LIST_MAX)
    return w


def ref_sort(s, r, count, k, margin):
    """What select_kernel must leave: keys = list[0:keep] in key order"""
    n = min(int(count), SORT_CAP)
    s, r = s[:n], r[:n]
    srt = np.sort(keys_of(s, r))[::-1]
    w = dict(n=n, overflow=count > SORT_CAP, nonfinite=margin is not None and not np.isfinite(margin))
    kth = orderable_inv(srt[k - 1] >> np.uint64(32)) if n >= k else None
    if margin is None:
        w["keep"], w["thr"] = min(n, k), f32(-np.inf) if kth is None else kth
    elif kth is None:
        w["keep"], w["thr"] = n, f32(-np.inf)
    else:
        w["thr"] = cut_of(kth, margin)
        w["keep"] = int((s >= w["thr"]).sum())
    w["keys"] = srt[:w["keep"]]
    w["wide"] = margin is not None and (w["keep"] > LIST_MAX or w["nonfinite"])
    return w


def orderable_inv(u):
    """csrc/common.h orderable_f32"""
    u = np.asarray(u).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def same_float(a, b):
    """bit for bit, except that a zero of either sign equals a zero"""
    a, b = f32(a), f32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (a == 0 and b == 0)


PATTERNS = ["gaussian", "negative", "straddle", "lastbyte", "topbyte", "subnormal", "inf", "const", "twoties", "cutmin", "cutmax", "pm0"]


def pattern(name, n, k, rng):
    """n float32 scores.  The structured patterns are built at the length their structure needs, shuffled and cut to n"""
    u32 = np.uint32
    if name == "gaussian":
        s = rng.standard_normal(n)
    elif name == "negative":
        s = -np.abs(rng.standard_normal(n)) - 0.125
    elif name == "straddle":
        s = rng.standard_normal(n) * 1e-3
        s[rng.random(n) < 0.1] = 0.0
        s[rng.random(n) < 0.1] = -0.0
    elif name == "lastbyte":                                 # the top 24 bits shared: decided in the last radix pass only
        s = (u32(0x3f9d7a00) | rng.integers(0, 256, n).astype(u32)).view(np.float32) * f32(rng.choice([1.0, -1.0]))
    elif name == "topbyte":                                  # the low 24 bits shared (bit 23 clear: no infinity, no NaN)
        s = ((rng.integers(0, 256, n).astype(u32) << u32(24)) | u32(0x123456)).view(np.float32)
    elif name == "subnormal":
        s = (rng.integers(1, 0x800000, n).astype(u32) | (rng.integers(0, 2, n).astype(u32) << u32(31))).view(np.float32)
    elif name == "inf":
        s = rng.standard_normal(n)
        s[rng.random(n) < 0.05] = np.inf
        s[rng.random(n) < 0.05] = -np.inf
    elif name == "const":
        s = np.full(n, 0.75)
    else:
        big = max(n, 2 * k + 16)
        if name == "twoties":                                # the k-th falls inside the second tied group
            g1 = k // 2
            s = np.concatenate([np.full(g1, 2.0), np.full(k, 1.0), 0.5 - np.abs(rng.standard_normal(big - g1 - k))])
        elif name == "cutmin":                               # the k-th is the minimum of the list: everything is kept
            s = np.concatenate([1.0 + np.arange(k - 1), np.full(big - (k - 1), -2.5)])
        elif name == "cutmax":                               # the k-th is the maximum
            s = np.concatenate([np.full(k + 3, 9.0), 8.0 - np.abs(rng.standard_normal(big - k - 3))])
        else:                                                # pm0: the k-th key is +0.0, -0.0 entries below it
            s = np.concatenate([0.1 + np.abs(rng.standard_normal(k - 1)), np.full(2, 0.0), np.full(3, -0.0),
                                -0.1 - np.abs(rng.standard_normal(big - k - 4))])
        s = rng.permutation(s)[:n]
    return np.ascontiguousarray(s, dtype=np.float32)


def rows_for(n, rng):
    """n distinct row numbers below PAD_ROW, some beyond 2^31, in no order"""
    return (rng.permutation(SORT_CAP)[:n].astype(np.uint64) * 400009 + 7).astype(np.uint32)


def pick_margin(s, k, rng):
    """a finite margin that puts the certified cut on the score of a random member of the list"""
    n = len(s)
    if n < k:
        return f32(0.25)
    kth, v = float(np.sort(s)[n - k]), float(s[rng.integers(n)])
    m = (kth - v) / 2 if np.isfinite(kth) and np.isfinite(v) and v <= kth else 1.0
    return f32(m) if m < 1e38 else f32(1e37)                # (2 m must not overflow: a fused kth - 2 m would not see it)


def lengths(k, caps):
    out = {0, 1, k - 1, k, k + 1, 255, 256, 257, 8191, 8192}
    for cap in caps:
        out |= {cap - 1, cap, cap + 1}
    return sorted(out) + [SORT_CAP + 5]                      # the last one: 8192 keys under a count of 8197


def make_lists(lens, k, first, rng, certified):
    """one launch: query j gets lens[j] keys of pattern first + j; a length beyond SORT_CAP is a full list under that count"""
    lists, counts, margins = [], [], []
    for j, n in enumerate(lens):
        s = pattern(PATTERNS[(first + j) % len(PATTERNS)], min(n, SORT_CAP), k, rng)
        lists.append((s, rows_for(len(s), rng)))
        counts.append(n)
        margins.append(pick_margin(s, k, rng) if certified else None)
    return lists, counts, margins


# ------------------------------------------------------------------------------------------------------------- host only
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("k", [1, 10, 1000])
def test_reference_agrees_with_a_plain_sort_of_the_keys(name, k):
    """the reference's k-th score and kept set (float comparison) against np.sort of the 64-bit keys alone"""
    rng = np.random.default_rng(k)
    for n in (k + 1, 2 * k + 40, 5000):
        s, r = pattern(name, n, k, rng), rows_for(n, rng)
        keys = keys_of(s, r)
        assert len(np.unique(keys)) == n
        srt = np.sort(keys)[::-1]
        for margin in (None, pick_margin(s, k, rng)):
            w = ref_radix(s, r, n, k, margin, SORT_CAP)
            kth_code = srt[k - 1] >> np.uint64(32)
            assert code(w["kth"]) == kth_code
            cut = w["thr"]
            # in key order the kept set is a prefix: every key at or above the lowest code of the cut's value (that of -0.0 for a zero)
            low = np.uint64(code(-0.0) if cut == 0 else code(cut)) << np.uint64(32)
            assert np.array_equal(w["keys"], np.sort(srt[srt >= low]))
            assert w["keep"] >= k and np.isin(srt[:k], w["keys"]).all()
            if margin is None:                                # exact mode: what is kept beyond the k best ties with the k-th BY VALUE
                extra = orderable_inv(np.setdiff1d(w["keys"], srt[:k]) >> np.uint64(32))
                assert (extra == w["kth"]).all()
            v = ref_sort(s, r, n, k, margin)
            assert same_float(v["thr"], cut) and v["keep"] == (w["keep"] if margin is not None else k)
            assert np.array_equal(v["keys"], srt[:v["keep"]])


def test_reference_on_signed_zeros_and_tie_groups():
    r = np.arange(9, dtype=np.uint32)
    s = np.array([3, 0.0, -0.0, 0.0, -0.0, -1, 2, -0.0, -5], np.float32)
    w = ref_radix(s, r, 9, 3, None, SORT_CAP)                 # keys: 3, 2, then +0.0 of row 1: the k-th
    assert w["kth"].view(np.uint32) == 0 and w["keep"] == 7   # ... and the other +0.0 and the three -0.0 pass the float comparison
    assert ref_sort(s, r, 9, 3, None)["keys"].tolist() == keys_of(s[[0, 6, 1]], r[[0, 6, 1]]).tolist()
    w = ref_radix(s, r, 9, 5, None, SORT_CAP)                 # the k-th is a -0.0 (row 2): the cut is -0.0, kept the same seven
    assert w["kth"].view(np.uint32) == 0x80000000 and w["keep"] == 7 and same_float(w["thr"], 0.0)
    s = np.array([2, 2, 1, 1, 1, 1, 0.5], np.float32)         # two tied groups, the k-th inside the second
    w = ref_radix(s, r[:7], 7, 3, None, SORT_CAP)
    assert w["kth"] == 1 and w["keep"] == 6
    assert ref_sort(s, r[:7], 7, 3, None)["keys"].tolist() == keys_of(s[:3], r[:3]).tolist()      # ties by ascending row
    assert ref_radix(s, r[:7], 7, 3, f32(0.25), SORT_CAP)["keep"] == 7


FAKE = 0x1000


def _lists_refused(op=0, nq=3, m=16, scores=FAKE, rows=FAKE, counts=FAKE, k=10, cap=8192, allow=FAKE, nrows=100, S=FAKE, ldS=32, n=16,
                   emit_scores=FAKE, emit_ids=FAKE, ws=FAKE * 16, ws_bytes=1 << 40):
    """one om_debug_select_lists call with pointers that are never followed: every refusal comes before the first launch"""
    p = N.c_void_p
    return N.lib().om_debug_select_lists(op, nq, m, p(scores), p(rows), p(counts), k, p(0), 1, cap, p(allow), nrows, p(S), ldS, n, 0, 0, 0,
                                         p(emit_scores), p(emit_ids), p(FAKE), p(FAKE), p(FAKE), p(ws), ws_bytes, p(0))


def test_the_hooks_exist():
    lib = N.lib()
    for name in ("om_debug_select_lists", "om_debug_query_prep"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None


def test_select_lists_refusals():
    err = N.lib().om_last_error
    for bad in (dict(scores=0), dict(rows=0), dict(counts=0), dict(op=2, allow=0), dict(op=3, S=0), dict(op=4, emit_scores=0),
                dict(op=4, emit_ids=0)):
        assert _lists_refused(**bad) == 1, bad
        assert b"om_debug_select_lists" in err() and b"null argument" in err(), bad
    for k in (0, -1, K_MAX + 1):
        assert _lists_refused(k=k) == 1 and b"[1, 2048]" in err()
    for m in (0, SORT_CAP + 1):
        assert _lists_refused(m=m) == 1 and b"[1, 8192]" in err()
    for cap in (0, 2048, 4095, 8191, 16384):
        assert _lists_refused(cap=cap) == 1 and b"4096 or 8192" in err()
    for op in (-1, 5):
        assert _lists_refused(op=op) == 1 and b"op must be" in err()
    for nq in (0, 65536):
        assert _lists_refused(nq=nq) == 1 and b"65535" in err()
    assert _lists_refused(op=2, nrows=0) == 1 and b"nrows" in err()
    for bad in (dict(n=0), dict(n=4097, ldS=5000), dict(n=16, ldS=15)):
        assert _lists_refused(op=3, **bad) == 1 and b"ldS" in err()
    assert _lists_refused(ws=0) == 1 and b"256-byte aligned" in err()
    assert _lists_refused(ws=FAKE * 16 + 64) == 1 and b"256-byte aligned" in err()
    need = N.lib().om_sim_topk_async_workspace_bytes(3, 64, 1)
    assert _lists_refused(ws_bytes=need - 1) == 1 and b"workspace too small" in err()


def test_query_prep_refusals():
    lib, p = N.lib(), N.c_void_p
    for hole in range(4):
        a = [p(0) if i == hole else p(FAKE) for i in range(4)]
        assert lib.om_debug_query_prep(a[0], 3, 64, a[1], a[2], a[3], p(0)) == 1
        assert b"om_debug_query_prep" in lib.om_last_error() and b"null argument" in lib.om_last_error()
    for nq, d in ((0, 64), (65536, 64), (3, 0), (3, 16385)):
        assert lib.om_debug_query_prep(p(FAKE), nq, d, p(FAKE), p(FAKE), p(FAKE), p(0)) == 1


# ------------------------------------------------------------------------------------------------------------- GPU: the hook
class Out:
    pass


def run_lists(op, lists, counts, k=1, margins=None, use_qstat=True, cap=SORT_CAP, allow=None, nrows=0, S=None, n=0, row_base=0, cover=0,
              id_offset=0):
    """om_debug_select_lists over lists [(scores, rows)], one per query; margins: one per query, or None for exact mode"""
    lib = N.lib()
    nq = len(lists)
    m = max(1, max(len(s) for s, _ in lists))
    sc = np.full((nq, m), np.inf, np.float32)
    ro = np.tile(PAD_ROW + np.arange(m, dtype=np.uint32), (nq, 1))
    for q, (s, r) in enumerate(lists):
        sc[q, :len(s)], ro[q, :len(s)] = s, r
    o = Out()
    o.keys_in = np.empty((nq, SORT_CAP), np.uint64)
    o.keys_in[:, :m] = keys_of(sc.ravel(), ro.ravel()).reshape(nq, m)
    o.keys_in[:, m:] = keys_of(np.full(SORT_CAP - m, np.inf, np.float32), STALE_ROW + np.arange(m, SORT_CAP, dtype=np.uint32))
    dev = torch.device(DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_sc, d_ro, d_cnt = t(sc), t(ro.view(np.int32)), t(np.asarray(counts, np.uint32).view(np.int32))
    d_margin = t(np.asarray(margins, np.float32)) if margins is not None else None
    d_allow = t(np.asarray(allow, np.uint32).view(np.int32)) if allow is not None else None
    d_S = t(np.asarray(S, np.float32)) if S is not None else None
    o_sc = torch.empty((nq, SORT_CAP), dtype=torch.float32, device=dev)
    o_ro = torch.empty((nq, SORT_CAP), dtype=torch.int32, device=dev)
    o_st = torch.full((nq * 4 + 4,), -1, dtype=torch.int32, device=dev)
    e_sc = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    e_id = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    nbytes = lib.om_sim_topk_async_workspace_bytes(nq, 64, 1)
    _buf, ws = N.Workspace.get(dev, nbytes, "test-select-lists")
    N.check(lib.om_debug_select_lists(N.DEBUG_LISTS[op], nq, m, N.ptr(d_sc), N.ptr(d_ro), N.ptr(d_cnt), k, N.ptr(d_margin), int(use_qstat), cap,
                                      N.ptr(d_allow), nrows, N.ptr(d_S), 0 if S is None else np.asarray(S).shape[1], n, row_base, cover,
                                      id_offset, N.ptr(e_sc), N.ptr(e_id), N.ptr(o_sc), N.ptr(o_ro), N.ptr(o_st), N.c_void_p(ws), nbytes,
                                      N.stream_ptr(dev)))
    torch.cuda.synchronize()
    o.scores, o.rows = o_sc.cpu().numpy(), o_ro.cpu().numpy().view(np.uint32)
    o.keys = keys_of(o.scores.ravel(), o.rows.ravel()).reshape(nq, SORT_CAP)
    st = o_st.cpu().numpy().view(np.uint32)
    per = st[:nq * 4].reshape(nq, 4)
    o.cnt, o.cnt_prev, o.thr_bits, o.qstat, o.flag = per[:, 0], per[:, 1], per[:, 2], per[:, 3], st[nq * 4:]
    o.thr = o.thr_bits.copy().view(np.float32)
    o.D, o.I = e_sc.cpu().numpy(), e_id.cpu().numpy()
    return o


def check_radix(o, q, lst, count, k, margin, cap, ctx, use_qstat=True):
    """query q of a select_radix_kernel launch against the reference; returns the reference"""
    s, r = lst
    w = ref_radix(s, r, count, k, margin, cap)
    ctx = f"{ctx} q={q} n={count} k={k} cap={cap} margin={margin}"
    want_stat = ((QSTAT_OVERFLOW if w["overflow"] else 0) | (QSTAT_WIDE if w["wide"] else 0)) if use_qstat else 0
    assert o.qstat[q] == want_stat, (ctx, o.qstat[q], want_stat)
    assert o.cnt_prev[q] == 0xffffffff, ctx
    assert o.flag[1] >= min(o.cnt[q], SORT_CAP), ctx
    if w["nonfinite"]:                                       # the kept set of such a query is not part of the contract
        return w
    assert same_float(o.thr[q], w["thr"]), (ctx, o.thr[q], w["thr"])
    assert o.cnt[q] == w["keep"], (ctx, o.cnt[q], w["keep"])
    if w["early"]:
        assert np.array_equal(o.keys[q], o.keys_in[q]), ctx                      # the list is untouched
        return w
    got = np.sort(o.keys[q, :o.cnt[q]])
    if w["subset"]:
        assert len(np.unique(got)) == cap and np.isin(got, w["keys"]).all(), ctx
    else:
        assert np.array_equal(got, w["keys"]), (ctx, len(got), len(w["keys"]))
    assert np.array_equal(o.keys[q, w["n"]:], o.keys_in[q, w["n"]:]), ctx        # nothing written behind the list
    return w


def check_radix_launch(o, lists, counts, k, margins, cap, ctx, use_qstat=True):
    ws = [check_radix(o, q, lists[q], counts[q], k, None if margins is None else margins[q], cap, ctx, use_qstat) for q in range(len(lists))]
    assert o.flag[0] == int(any(w["overflow"] for w in ws)), ctx
    assert o.flag[1] <= SORT_CAP and o.flag[3] == 0, ctx
    assert o.flag[2] == int(any(w["wide"] for w in ws)), ctx     # with or without qstat: om_sim_topk's path reads nothing else
    return ws


# ------------------------------------------------------------------------------------------------------------- select_radix_kernel
@pytest.mark.gpu
@pytest.mark.parametrize("certified", [False, True], ids=["exact", "certified"])
@pytest.mark.parametrize("k", [1, 10, 1000, 2048])
@pytest.mark.parametrize("cap", [4096, 8192])
def test_select_radix_against_the_sorted_reference(cap, k, certified):
    """every length against every score pattern: launch i gives query j the pattern i + j"""
    rng = np.random.default_rng(cap + k + certified)
    lens = lengths(k, [cap])
    seen = dict(unstaged=0, subset=0, early=0, wide=0)
    for first in range(len(PATTERNS)):
        lists, counts, margins = make_lists(lens, k, first, rng, certified)
        o = run_lists("radix", lists, counts, k=k, margins=margins if certified else None, cap=cap)
        for w in check_radix_launch(o, lists, counts, k, margins if certified else None, cap, f"first={first}"):
            seen["unstaged"] += w["n"] > cap and not w["early"]
            seen["subset"] += w["subset"]
            seen["early"] += w["early"]
            seen["wide"] += w["wide"]
    print(f"cap={cap} k={k} certified={certified}: {seen}")
    assert seen["early"] and (cap == SORT_CAP or (seen["unstaged"] and seen["subset"]))
    assert seen["wide"] or not (certified and cap == SORT_CAP)          # (beyond cap = 4096 = LIST_MAX keys the unstaged branch overflows instead)


@pytest.mark.gpu
@pytest.mark.parametrize("certified", [False, True], ids=["exact", "certified"])
def test_select_radix_unstaged_branch(certified):
    """n > cap = 4096: every pass reads the list from global memory and only the survivors are staged"""
    rng = np.random.default_rng(11)
    k, lens = 100, [4097, 5000, 6000, 7777, 8191, 8192]
    lists = [(pattern("gaussian", n, k, rng), rows_for(n, rng)) for n in lens]
    # certified: cuts that keep 101 .. ~4000 keys (the LDS copy holds them) and, query 5, ~6000 (it does not: an overflow)
    margins = [f32(0.01), f32(0.3), f32(0.5), f32(0.8), f32(1.0), f32(1.6)] if certified else None
    o = run_lists("radix", lists, lens, k=k, margins=margins, cap=4096)
    ws = check_radix_launch(o, lists, lens, k, margins, 4096, "unstaged")
    assert all(w["n"] > 4096 and not w["early"] for w in ws)
    assert [w["subset"] for w in ws] == [False] * 5 + [certified]
    if not certified:
        assert (o.cnt == k).all()


@pytest.mark.gpu
def test_select_radix_ties_beyond_the_lds_copy():
    """6000 equal scores, cap 4096: more keys pass the cut than the LDS copy holds -- an overflow, 4096 distinct members kept"""
    rng = np.random.default_rng(12)
    k = 10
    lists = [(np.full(6000, v, np.float32), rows_for(6000, rng)) for v in (0.75, -3.0, 0.0, np.inf, 1e-40)]
    lists.append((pattern("gaussian", 6000, k, rng), rows_for(6000, rng)))      # the neighbour in the launch is not touched by it
    counts = [6000] * 6
    o = run_lists("radix", lists, counts, k=k, cap=4096)
    ws = check_radix_launch(o, lists, counts, k, None, 4096, "ties")
    assert [w["subset"] for w in ws] == [True] * 5 + [False]
    for q in range(5):
        assert o.cnt[q] == 4096 and o.qstat[q] == QSTAT_OVERFLOW
        got = o.keys[q, :4096]
        assert len(np.unique(got)) == 4096 and np.isin(got, o.keys_in[q, :6000]).all()
    assert o.flag[0] == 1 and o.cnt[5] == k and o.qstat[5] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("certified", [False, True], ids=["exact", "certified"])
@pytest.mark.parametrize("cap", [4096, 8192])
def test_select_radix_n_le_k_returns_early(cap, certified):
    """n < k: no threshold yet (-inf);  n == k: the minimum (minus twice the margin);  the list and its count stay as they are"""
    rng = np.random.default_rng(13)
    k, lens = 300, [0, 1, 2, 64, 255, 256, 299, 300, 300, 300]
    names = ["gaussian", "negative", "inf", "subnormal", "pm0", "const", "lastbyte", "gaussian", "negative", "const"]
    lists = [(pattern(nm, n, k, rng), rows_for(n, rng)) for nm, n in zip(names, lens)]
    margins = [f32(0.125 * (q + 1)) for q in range(len(lens))] if certified else None
    o = run_lists("radix", lists, lens, k=k, margins=margins, cap=cap)
    ws = check_radix_launch(o, lists, lens, k, margins, cap, "early")
    assert all(w["early"] for w in ws)
    for q, n in enumerate(lens):
        assert o.cnt[q] == n and np.array_equal(o.keys[q], o.keys_in[q])
        if n < k:
            assert o.thr[q] == -np.inf
        else:
            assert o.thr[q] == cut_of(lists[q][0].min(), margins[q] if certified else None)
    assert (o.qstat == 0).all() and o.flag[0] == 0 and o.flag[1] == 300 and o.flag[2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4096, 8192])
def test_select_radix_overflowed_count_clamps_and_marks(cap):
    """counts of 8193 .. 16000: the round lost appends -- flag[0], QSTAT_OVERFLOW, and the selection over the first 8192 keys is right"""
    rng = np.random.default_rng(14)
    k = 10
    counts = [SORT_CAP + 1, SORT_CAP + 5, 8000, 16000, SORT_CAP, 20000]
    lists = [(pattern(nm, min(n, SORT_CAP), k, rng), rows_for(min(n, SORT_CAP), rng))
             for nm, n in zip(["gaussian", "negative", "gaussian", "lastbyte", "gaussian", "inf"], counts)]
    o = run_lists("radix", lists, counts, k=k, cap=cap)
    check_radix_launch(o, lists, counts, k, None, cap, "overflowed count")
    assert o.flag[0] == 1
    assert [bool(x & QSTAT_OVERFLOW) for x in o.qstat] == [True, True, False, True, False, True]
    assert (o.cnt[[0, 1, 2, 4]] == k).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4096, 8192])
def test_select_radix_cut_at_signed_zero(cap):
    """the k-th key at +0.0 with -0.0 entries below it: the float comparison keeps them; and the k-th at -0.0"""
    rng = np.random.default_rng(15)
    lists, ks = [], 7
    for n, n_pos, n_pz, n_nz in ((20, 6, 1, 3), (300, 5, 3, 4), (5000, 6, 2, 200), (8192, 4, 3, 9), (4097, 0, 7, 7), (600, 6, 0, 5)):
        s = np.concatenate([0.1 + np.abs(rng.standard_normal(n_pos)), np.full(n_pz, 0.0), np.full(n_nz, -0.0),
                            -0.1 - np.abs(rng.standard_normal(n - n_pos - n_pz - n_nz))]).astype(np.float32)
        p = rng.permutation(n)
        lists.append((s[p], rows_for(n, rng)))
    lens = [len(s) for s, _ in lists]
    o = run_lists("radix", lists, lens, k=ks, cap=cap)
    ws = check_radix_launch(o, lists, lens, ks, None, cap, "zero")
    assert [int(o.cnt[q]) for q in range(6)] == [6 + 1 + 3, 5 + 3 + 4, 6 + 2 + 200, 4 + 3 + 9, 14, 6 + 5]
    assert [w["kth"].view(np.uint32) == 0 for w in ws] == [True] * 5 + [False] and ws[5]["kth"].view(np.uint32) == 0x80000000
    assert (o.thr == 0).all()
    margins = [f32(0.0)] * 6                                  # certified with a zero margin: kth - 0 is the same cut
    o = run_lists("radix", lists, lens, k=ks, margins=margins, cap=cap)
    check_radix_launch(o, lists, lens, ks, margins, cap, "zero, certified")


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["radix", "sort"])
def test_non_finite_margin_marks_the_query(op):
    """margin = +inf (a value beyond float16 somewhere): QSTAT_WIDE for that query whatever its list, and flag[2] with or without
    qstat; the others are selected as ever"""
    rng = np.random.default_rng(16)
    k, lens = 10, [5000, 5000, 9, 10, 300, 5000]
    lists = [(pattern("gaussian", n, k, rng), rows_for(n, rng)) for n in lens]
    margins = [f32(0.01), f32(np.inf), f32(np.inf), f32(np.inf), f32(np.inf), f32(0.02)]
    o = run_lists(op, lists, lens, k=k, margins=margins, cap=8192)
    if op == "radix":
        check_radix_launch(o, lists, lens, k, margins, 8192, "inf margin")
    else:
        check_sort_launch(o, lists, lens, k, margins, "inf margin")
    assert [bool(x & QSTAT_WIDE) for x in o.qstat] == [False, True, True, True, True, False]
    assert o.flag[2] == 1
    for sub in ([0, 2], [0, 3], [0, 1], [0, 5]):              # one such query short of k, at k, beyond k; none
        o = run_lists(op, [lists[i] for i in sub], [lens[i] for i in sub], k=k, margins=[margins[i] for i in sub], use_qstat=False)
        assert (o.qstat == 0).all() and o.flag[2] == int(sub[1] != 5), sub


@pytest.mark.gpu
def test_select_radix_without_qstat():
    """om_sim_topk's path hands the kernels a null qstat: the same lists, only the global flags tell"""
    rng = np.random.default_rng(17)
    k, lens = 10, [0, 10, 300, 4097, 8192, SORT_CAP + 5, 6000]
    lists, counts, margins = make_lists(lens, k, 0, rng, True)
    lists[6] = (np.full(6000, 1.5, np.float32), lists[6][1])
    margins[6] = f32(0.5)
    for cap in (4096, 8192):
        o = run_lists("radix", lists, counts, k=k, margins=margins, cap=cap, use_qstat=False)
        check_radix_launch(o, lists, counts, k, margins, cap, "no qstat", use_qstat=False)
        assert (o.qstat == 0).all() and o.flag[0] == 1


# ------------------------------------------------------------------------------------------------------------- select_kernel
def check_sort_launch(o, lists, counts, k, margins, ctx, use_qstat=True):
    ws = []
    for q, (s, r) in enumerate(lists):
        margin = None if margins is None else margins[q]
        w = ref_sort(s, r, counts[q], k, margin)
        c = f"{ctx} q={q} n={counts[q]} k={k} margin={margin}"
        want_stat = ((QSTAT_OVERFLOW if w["overflow"] else 0) | (QSTAT_WIDE if w["wide"] else 0)) if use_qstat else 0
        assert o.qstat[q] == want_stat, (c, o.qstat[q], want_stat)
        ws.append(w)
        if w["nonfinite"]:
            continue
        assert same_float(o.thr[q], w["thr"]), (c, o.thr[q], w["thr"])
        assert o.cnt[q] == w["keep"] and o.cnt_prev[q] == w["keep"], (c, o.cnt[q], o.cnt_prev[q], w["keep"])
        assert np.array_equal(o.keys[q, :w["keep"]], w["keys"]), c                # in key order: score descending, ties by ascending row
        assert (o.keys[q, :w["keep"]] != 0).all(), c                             # the padding key of the power-of-two sort
        assert np.array_equal(o.keys[q, w["n"]:], o.keys_in[q, w["n"]:]), c
    if not any(w["nonfinite"] for w in ws):
        assert o.flag[1] == max(w["keep"] for w in ws), ctx
    assert o.flag[2] == int(any(w["wide"] for w in ws)), ctx
    assert o.flag[0] == 0 and o.flag[3] == 0, ctx             # (the overflow flag of the sorted path is check_overflow_kernel's)
    return ws


@pytest.mark.gpu
@pytest.mark.parametrize("certified", [False, True], ids=["exact", "certified"])
@pytest.mark.parametrize("k", [1, 10, 2048])
def test_select_kernel_against_the_sorted_reference(k, certified):
    rng = np.random.default_rng(100 + k + certified)
    lens = lengths(k, [4096])
    wide = 0
    for first in range(len(PATTERNS)):
        lists, counts, margins = make_lists(lens, k, first, rng, certified)
        o = run_lists("sort", lists, counts, k=k, margins=margins if certified else None)
        ws = check_sort_launch(o, lists, counts, k, margins if certified else None, f"first={first}")
        wide += sum(w["wide"] for w in ws)
        assert bool(o.qstat[-1] & QSTAT_OVERFLOW) and not (o.qstat[:-1] & QSTAT_OVERFLOW).any()      # the count of 8197 clamps and marks
    assert not certified or wide


@pytest.mark.gpu
def test_select_kernel_keep_around_list_max():
    """certified lists of 4095, 4096 and 4097 keys: flag[2] and QSTAT_WIDE beyond LIST_MAX only"""
    rng = np.random.default_rng(18)
    k, n = 10, 6000
    keeps = [4095, 4096, 4097, 11, 6000]
    lists = [(rng.permutation(n).astype(np.float32), rows_for(n, rng)) for _ in keeps]      # scores 0 .. n - 1: the k-th is n - k
    margins = [f32((keep - k) / 2) for keep in keeps]                                        # cut = n - keep, exactly
    for sub in ([0, 1, 3], [0, 1, 2, 3, 4]):
        ls, ms = [lists[i] for i in sub], [margins[i] for i in sub]
        o = run_lists("sort", ls, [n] * len(sub), k=k, margins=ms)
        check_sort_launch(o, ls, [n] * len(sub), k, ms, "list max")
        assert o.cnt.tolist() == [keeps[i] for i in sub]
        assert [bool(x & QSTAT_WIDE) for x in o.qstat] == [keeps[i] > LIST_MAX for i in sub]
        assert o.flag[2] == int(len(sub) == 5)


@pytest.mark.gpu
@pytest.mark.parametrize("certified", [False, True], ids=["exact", "certified"])
def test_select_kernel_lengths_0_and_1(certified):
    """P = 2 pads the sort with key 0, which must never come out below keep"""
    rng = np.random.default_rng(19)
    lens = [0, 1, 1, 2, 3, 0]
    lists = [(pattern("negative", n, 1, rng), rows_for(n, rng)) for n in lens]
    lists[2] = (np.array([-np.inf], np.float32), np.array([0xefffffff], np.uint32))          # the lowest key a list can hold
    for k in (1, 2, 5):
        margins = [f32(0.5)] * len(lens) if certified else None
        o = run_lists("sort", lists, lens, k=k, margins=margins)
        check_sort_launch(o, lists, lens, k, margins, "short")
        if not certified:
            assert o.cnt.tolist() == [min(n, k) for n in lens]


# ------------------------------------------------------------------------------------------------------------- drop_disallowed_kernel
NROWS_DROP = 5003          # not a multiple of 32: the last word of the bitmap has 11 valid bits


def bitmaps(rng):
    words = (NROWS_DROP + 31) // 32
    u32 = np.uint32
    rand = lambda p: np.packbits(rng.random(words * 32) < p, bitorder="little").view(u32)
    last = np.zeros(words, u32)
    last[(NROWS_DROP - 1) >> 5] = u32(1) << u32((NROWS_DROP - 1) & 31)
    return {"ones": np.full(words, 0xffffffff, u32),           # (the bits at and beyond nrows as well: they name no row)
            "zeros": np.zeros(words, u32), "alternating": np.full(words, 0x55555555, u32), "bit31": np.full(words, 0x80000000, u32),
            "last_row": last, "p0.9": rand(0.9), "p0.5": rand(0.5), "p0.01": rand(0.01)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ones", "zeros", "alternating", "bit31", "last_row", "p0.9", "p0.5", "p0.01"])
@pytest.mark.parametrize("overflowed", [False, True], ids=["", "overflowed-count"])
def test_drop_disallowed_keeps_the_allowed_keys_in_order(name, overflowed):
    rng = np.random.default_rng(20)
    allow = bitmaps(rng)[name]
    lens = [0, 1, 255, 256, 257, 511, 512, 513, 8192] + ([8200] if overflowed else [])
    lists = []
    for n in lens:
        n = min(n, SORT_CAP)
        r = rng.integers(0, NROWS_DROP + 300, n).astype(np.uint32)               # some rows at and beyond nrows: dropped, the bitmap not read
        r[::7] = NROWS_DROP - 1
        r[3::11] = rng.integers(0, NROWS_DROP // 32, len(r[3::11])) * 32 + 31
        r[5::13] = NROWS_DROP + rng.integers(0, 21, len(r[5::13]))               # ... among them the invalid bits of the last word
        r[6::17] = 0xefffffff
        lists.append((pattern("gaussian", n, 1, rng), r))
    o = run_lists("drop", lists, lens, allow=allow, nrows=NROWS_DROP)
    for q, (s, r) in enumerate(lists):
        ok = (r < NROWS_DROP)
        ok[ok] = (allow[r[ok] >> 5] >> (r[ok] & 31)) & 1 == 1
        want = keys_of(s[ok], r[ok])
        assert o.cnt[q] == len(want), (name, q, o.cnt[q], len(want))
        assert np.array_equal(o.keys[q, :len(want)], want), (name, q)            # in their original order
        assert np.array_equal(o.keys[q, len(s):], o.keys_in[q, len(s):]), (name, q)
        assert o.qstat[q] == (QSTAT_OVERFLOW if lens[q] > SORT_CAP else 0)
    assert o.flag.tolist() == [int(overflowed), 0, 0, 0]
    assert (o.cnt_prev == 0xffffffff).all() and (o.thr_bits == THR_UNWRITTEN).all()
    if name == "ones":
        assert o.cnt[8] > 6000
    if overflowed:
        o = run_lists("drop", lists, lens, allow=allow, nrows=NROWS_DROP, use_qstat=False)
        assert (o.qstat == 0).all() and o.flag[0] == 1


# ------------------------------------------------------------------------------------------------------------- append + overflow check
@pytest.mark.gpu
@pytest.mark.parametrize("n,ld", [(4096, 4100), (1000, 1003), (1, 1)])
@pytest.mark.parametrize("use_qstat", [True, False])
def test_append_dense_and_check_overflow(n, ld, use_qstat):
    """bases 0 and 4000: appended in order;  base 5000 + 4096 keys: nothing written past slot 8191, the count tells, the marks are set"""
    rng = np.random.default_rng(21)
    bases = [0, 4000, 5000, 4096, 8191, 8192, 7193]
    lists = [(pattern("gaussian", b, 1, rng), rows_for(b, rng)) for b in bases]
    S = rng.standard_normal((len(bases), ld)).astype(np.float32)
    S[:, 0] = [np.inf, -np.inf, 0.0, -0.0, 1e-40, 3.0, -3.0]
    row_base, cover = 2 ** 31 + 4090, 8000
    o = run_lists("append", lists, bases, S=S, n=n, row_base=row_base, cover=cover, use_qstat=use_qstat)
    for q, b in enumerate(bases):
        total = b + n
        assert o.cnt[q] == total
        fit = min(total, SORT_CAP) - b
        want = keys_of(S[q, :fit], (row_base + np.arange(fit)).astype(np.uint32))
        assert np.array_equal(o.keys[q, b:b + fit], want), q
        assert np.array_equal(o.keys[q, :b], o.keys_in[q, :b]) and np.array_equal(o.keys[q, b + fit:], o.keys_in[q, b + fit:]), q
        want_stat = (QSTAT_OVERFLOW if total > SORT_CAP else 0) | (QSTAT_COVER if total > cover else 0)
        assert o.qstat[q] == (want_stat if use_qstat else 0), (q, o.qstat[q], want_stat)
    assert o.flag.tolist() == [int(any(b + n > SORT_CAP for b in bases)), 0, 0, 0]
    assert (o.cnt_prev == 0xffffffff).all() and (o.thr_bits == THR_UNWRITTEN).all()


# ------------------------------------------------------------------------------------------------------------- emit_kernel
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 257, 2048])
def test_emit_scores_ids_and_padding(k):
    rng = np.random.default_rng(22)
    id_offset = 5 * 2 ** 32 + 7
    lens = sorted({0, 1, k - 1, k, k + 1, 3000, SORT_CAP}) + [SORT_CAP + 9]
    lists = [(pattern("inf", min(n, SORT_CAP), k, rng), rows_for(min(n, SORT_CAP), rng)) for n in lens]
    o = run_lists("emit", lists, lens, k=k, id_offset=id_offset)
    assert o.D.shape == (len(lens), k)
    for q, (s, r) in enumerate(lists):
        n = min(len(s), k)
        assert np.array_equal(o.D[q, :n].view(np.uint32), s[:n].view(np.uint32)), q
        assert np.array_equal(o.I[q, :n], id_offset + r[:n].astype(np.int64)), q
        assert (o.D[q, n:] == FLT_MIN).all() and (o.I[q, n:] == -1).all(), q
        assert np.array_equal(o.keys[q], o.keys_in[q]) and o.cnt[q] == lens[q]
    assert (o.I[1:, 0] > 2 ** 32).all()


# ------------------------------------------------------------------------------------------------------------- merge_kernel
def ref_merge(ps, pi, k_out):
    """stable sort (score descending) of the valid entries of the concatenated parts: ties by part, then position"""
    W, nq, k_in = ps.shape
    D = np.full((nq, k_out), FLT_MIN, np.float32)
    I = np.full((nq, k_out), -1, np.int64)
    for q in range(nq):
        s, i = ps[:, q].reshape(-1), pi[:, q].reshape(-1)
        s, i = s[i >= 0], i[i >= 0]
        order = np.argsort(-s.astype(np.float64), kind="stable")[:k_out]
        D[q, :len(order)], I[q, :len(order)] = s[order], i[order]
    return D, I


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("W,k_in,k_out", [(1, 1, 5), (2, 3, 3), (3, 7, 10), (8, 1000, 1000), (4, 2048, 2048), (5, 100, 1000)])
def test_merge_kernel_equals_a_stable_sort(W, k_in, k_out, nq):
    rng = np.random.default_rng(W * 10000 + k_in + nq)
    ps = np.full((W, nq, k_in), FLT_MIN, np.float32)
    pi = np.full((W, nq, k_in), -1, np.int64)
    for w in range(W):
        for q in range(nq):
            valid = int(rng.integers(0, k_in + 1)) if (w + q) % 2 else k_in      # -1 padding tails of different lengths per part
            if k_out > W * k_in and w == 0:
                valid = k_in
            # multiples of 1/8 around 1: ties inside a part and across parts (a zero is +0.0: the two zeros never meet)
            s = np.sort(1.0 + np.round(rng.standard_normal(valid) * 8) / 8)[::-1]
            ps[w, q, :valid] = s
            pi[w, q, :valid] = rng.integers(0, 2 ** 40, valid)                    # ids beyond 2^32
    pi[0, :, 0] = 2 ** 33 + 5
    D, I = ref_merge(ps, pi, k_out)
    dev = torch.device(DEV)
    dD = torch.full((nq, k_out), float("nan"), dtype=torch.float32, device=dev)
    dI = torch.full((nq, k_out), -7, dtype=torch.int64, device=dev)
    dps, dpi = torch.from_numpy(ps).to(dev), torch.from_numpy(pi).to(dev)
    N.check(N.lib().om_topk_merge(N.ptr(dps), N.ptr(dpi), W, nq, k_in, k_out, N.ptr(dD), N.ptr(dI), N.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert np.array_equal(dD.cpu().numpy().view(np.uint32), D.view(np.uint32))
    assert np.array_equal(dI.cpu().numpy(), I)
    if (W, k_in, k_out) == (1, 1, 5):
        assert (I[:, 1:] == -1).all() and (D[:, 1:] == FLT_MIN).all() and (I[:, 0] == 2 ** 33 + 5).all()


# ------------------------------------------------------------------------------------------------------------- query_prep_kernel
def run_query_prep(Q, stats):
    nq, d = Q.shape
    dev = torch.device(DEV)
    npad = (nq + 255) // 256 * 256
    q16 = torch.full((npad, d), float("nan"), dtype=torch.float16, device=dev)
    margin = torch.full((nq,), float("nan"), dtype=torch.float32, device=dev)
    dQ, dst = torch.from_numpy(Q).to(dev), torch.from_numpy(np.asarray(stats, np.float32)).to(dev)
    N.check(N.lib().om_debug_query_prep(N.ptr(dQ), nq, d, N.ptr(dst), N.ptr(q16), N.ptr(margin), N.stream_ptr(dev)))
    torch.cuda.synchronize()
    return q16.cpu().numpy(), margin.cpu().numpy()


def to_f16(Q):
    with np.errstate(over="ignore"):                       # a value beyond float16 becomes an infinity, as on the device
        return Q.astype(np.float16)


def margin_terms(Q, stats, d):
    """E and S of the certified margin in float64; depth as query_prep_kernel's comment counts it"""
    Ep, Pn = float(f32(stats[0])), float(f32(stats[1]))
    q = Q.astype(np.float64)
    fl = to_f16(Q).astype(np.float64)
    qn, qe, qbn = np.linalg.norm(q, axis=1), np.linalg.norm(q - fl, axis=1), np.linalg.norm(fl, axis=1)
    depth = 2.0 * (32.0 + d / 16.0) + (d / 64.0 + 8.0)
    return qn * Ep + qe * Pn, depth * 2.0 ** -24 * np.maximum(qn, qbn) * (Pn + Ep)


SPECIALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -25, 3.1e-8, 6e-8, 3e-6, -4.5e-6, 6.1e-5, 65503.9, 65519.0,
                     -65519.99, 0.0, -0.0, 2.0 ** -14 - 2.0 ** -26], np.float32)      # ties to even, subnormal results, just under 65504 / 65520


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3, 255, 256, 257])
@pytest.mark.parametrize("d", [64, 256, 768, 2048])
def test_query_prep_panel_and_margin(d, nq):
    rng = np.random.default_rng(d + nq)
    Q = (rng.standard_normal((nq, d)) * rng.choice([0.05, 1.0, 30.0], size=(nq, 1))).astype(np.float32)
    Q[0, :len(SPECIALS)] = SPECIALS
    if nq > 2:
        Q[nq - 1, -len(SPECIALS):] = SPECIALS[::-1]
    # twice: as drawn, and rounded to float16 first -- queries float16 holds exactly have no rounding term, E = |q| Ep, and with the second
    # pair of statistics (a small Ep, a large Pn) the depth term S outweighs the 1 % slack on E: a wrong depth fails a bound
    worst = 0.0
    for Qv in (Q, to_f16(Q).astype(np.float32)):
        for stats in (np.array([0.0123, 1.7], np.float32), np.array([3e-4, 41.0], np.float32)):
            q16, margin = run_query_prep(Qv, stats)
            assert np.array_equal(q16[:nq].view(np.uint16), to_f16(Qv).view(np.uint16))
            assert (q16[nq:].view(np.uint16) == 0).all() and q16.shape[0] % 256 == 0
            E, S = margin_terms(Qv, stats, d)
            m = margin.astype(np.float64)
            ratio = m / (1.01 * E + S)
            worst = max(worst, ratio.max())
            assert np.isfinite(margin).all()
            assert (m >= E + S).all(), (m / (E + S)).min()            # the certification property
            assert (m <= (1.01 * E + S) * (1 + 1e-5)).all(), ratio.max()
    print(f"d={d} nq={nq}: largest margin / (1.01 E + S) = {worst:.8f}")


@pytest.mark.gpu
def test_query_prep_out_of_range_query_has_no_finite_margin():
    rng = np.random.default_rng(23)
    Q = rng.standard_normal((5, 128)).astype(np.float32)
    Q[1, 77], Q[3, 0] = 7e4, -7e4                             # beyond float16
    q16, margin = run_query_prep(Q, np.array([0.0123, 1.7], np.float32))
    assert (~np.isfinite(margin)).tolist() == [False, True, False, True, False]
    assert np.array_equal(q16[:5].view(np.uint16), to_f16(Q).view(np.uint16))
    E, S = margin_terms(Q[[0, 2, 4]], [0.0123, 1.7], 128)
    m = margin[[0, 2, 4]].astype(np.float64)
    assert (m >= E + S).all() and (m <= (1.01 * E + S) * (1 + 1e-5)).all()


# ------------------------------------------------------------------------------------------------------------- what flag[2] is for
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10])
def test_search_with_a_query_beyond_float16_is_still_exact(k):
    """A query with one element beyond float16: its float16 copy holds an infinity, every 16-bit score is +-inf, the k-th is +inf and
    the certified cut inf - inf keeps no key.  om_sim_topk learns of it from flag[2] alone (it has no qstat) and must fall back to the
    float32 scan; the asynchronous entry redoes the query.  Judged as tests/test_index_f16.py judges a search."""
    from openmatch_amd.index import FlatIPIndex
    from tests.test_index_f16 import judge
    n, nq, d = 5000, 3, 256
    rng = np.random.default_rng(24)
    P = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[1, 7] = 7e4
    idx = FlatIPIndex(d, device=DEV, precision="f16_rescore")
    idx.add(P)
    q = torch.from_numpy(Q).to(DEV)
    D, I = idx.search_device(q, k)
    info = dict(idx.last_search_info)
    print(f"k={k}: sync {info}")
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert (I >= 0).all(), I
    judge(D, I, P, Q, k)
    assert info["margin_too_wide"] and info["scan"] == "f32", info
    h = idx.search_device_async(q, k)
    got = h.info()
    print(f"k={k}: async {got}")
    judge(h.D.cpu().numpy(), h.I.cpu().numpy(), P, Q, k)
    assert got["redone"] >= 1 and got["margin_too_wide_queries"] >= 1, got
