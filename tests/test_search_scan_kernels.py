"""The four table kernels of the filtered scan (csrc/search_scan.hip: sim_filter_kernel, sim_filter_kernel6, sim_filter_kernel7,
sim_filter_kernel7c), each launched alone through om_debug_scan_kernel and held to its own contract: after a launch the
list of every query is EXACTLY the set of rows with score >= thr[q] -- behind the keys the list already held, no id twice, the right
score bits, cnt the true count -- and nothing else in keys or cnt has changed.

Data, as tests/test_search_widths.py makes it: rows and queries are integers in [-4, 4] stored as float16 or float32, so every product
and every partial sum is an integer of magnitude <= 16 d <= 16 * 448 = 7 168 < 2^24 that float32 holds, in ANY accumulation order.  The
reference is an int64 contraction and the tolerance is zero -- derived, not measured.  Thresholds are integers or half-integers, exact
in float32.

Thresholds of one launch (thresholds()): query 0 at -inf (every row passes: more than 64 records per wave and tile, the synchronous
flush of generation 7); query nq // 2 at +inf (an empty list); for nq >= 192 the 32 queries [160, 192) at -inf (one mi block of one wave
stages 32 x 128 = 4 096 records per tile: the capacity flush in the middle of a tile, and in 7c the staging positions beyond 1 024);
every fourth of the rest at the integer score of its 27th best row (ties at the threshold belong to the list: >=); the others at a
half-integer about 3 % of the rows reach (the sparse path: the split append carried across a tile boundary, the retire at the end).

Widths against the pipelines (K steps nk of the main loops): gemm_mainloop2 takes 128-byte steps and starts two of a three-slot ring;
float16 d = 64 / 192 / 448 are nk = 1 / 3 / 7 and float32 d = 64 / 192 / 448 are nk = 2 / 6 / 14, so nk = 2 -- exactly the prologue -- was
missing on the float16 plane: d = 128 is ADDED there.  gemm_mainloop6 takes 64-byte steps and starts min(nk, 3) of a four-slot ring;
float16 d = 64 / 192 / 448 are nk = 2 / 6 / 14 (below, above), float32 d = 64 is nk = 4; nk = 3 does not exist (d % 64 == 0), the nearest
above the prologue is nk = 4, on the float16 plane d = 128: ADDED too.  Generation 7 takes 128-byte steps: d = 64, 128 are nk = 1, 2
(sim_filter_kernel7), d = 192, 256, 448 are nk = 3, 4, 7 (sim_filter_kernel7c).

The cap test of sim_filter_kernel7c runs at d = 192, not 64: the continuous ring exists from three K steps on and the hook refuses less.

check_lists() is tested WITHOUT a GPU (test_checker_*): it accepts lists built from the reference and rejects each single corruption, so
the GPU tests cannot pass on a kernel that is wrong in one of those ways."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N

DEV = "cuda:0"
SORT_CAP = 8192
ROW_BASE = 2 ** 31 + 5
KEY_GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)      # low word has bit 31 set: ~id of no row here (ids are >= 2^31, so ~id < 2^31)
CNT_GUARD = np.uint32(0xDEADBEEF)
TILE2, TILE6, WIDE7, WIDE7C, STREAM = (N.SCAN_KERNEL[k] for k in ("tile2", "tile6", "wide7", "wide7c", "stream"))
NAME = {TILE2: "tile2", TILE6: "tile6", WIDE7: "wide7", WIDE7C: "wide7c"}
NQ_MAX, ROWS_MAX, ROWS_CAP = 600, 2093, 8448


def round_up(x, m):
    return (x + m - 1) // m * m


def f32_orderable(f):
    """csrc/common.h f32_orderable: the order-preserving 32-bit code of a float32"""
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def pack_keys(scores, ids):
    """csrc/search_keys.h pack_key: (orderable score) << 32 | ~id"""
    return (f32_orderable(scores).astype(np.uint64) << np.uint64(32)) | (~np.asarray(ids, np.uint32)).astype(np.uint64)


def prefix_keys(nq, n):
    """n keys a list already holds: no row's id (bit 31 of the low word set), each distinct"""
    q = np.arange(nq, dtype=np.uint64)[:, None]
    j = np.arange(n, dtype=np.uint64)[None, :]
    return np.uint64(0x123456789ABCDEF0) ^ (q << np.uint64(40)) ^ (j << np.uint64(8)) | np.uint64(0x80000000)


# ---------------------------------------------------------------------------------------------------------------------- the checker
def check_lists(keys, cnt, S, thr, row_base, prefix, prefix_key=None):
    """keys [nq + 1][SORT_CAP] uint64 (the last row a guard), cnt [>= nq] uint32 (guards from nq on) as a launch left them; S [nq][nrows]
    the exact integer scores, thr [nq]; prefix: keys every list held before (an int, or one per query), prefix_key [nq][>= prefix] those
    keys.  Raises AssertionError on the first difference from the contract."""
    nq, nrows = S.shape
    assert keys.shape == (nq + 1, SORT_CAP) and keys.dtype == np.uint64 and cnt.dtype == np.uint32 and len(cnt) >= nq
    prefix = np.broadcast_to(np.asarray(prefix, np.int64), (nq,))
    assert (keys[nq] == KEY_GUARD).all(), "the guard row behind the last list was written"
    assert (cnt[nq:] == CNT_GUARD).all(), f"a count beyond nq was written: {np.nonzero(cnt[nq:] != CNT_GUARD)[0][:8] + nq}"
    for q in range(nq):
        p = int(prefix[q])
        want = np.nonzero(S[q] >= thr[q])[0]
        assert int(cnt[q]) - p == len(want), (q, "count", int(cnt[q]) - p, "survivors", len(want))
        if p:
            assert np.array_equal(keys[q, :p], prefix_key[q, :p]), (q, "a key the list already held was changed")
        stored = min(len(want), SORT_CAP - p)                   # a list over the cap keeps the keys whose position is below it
        got = keys[q, p:p + stored]
        assert (keys[q, p + stored:] == KEY_GUARD).all(), (q, "a key was written behind the list's end")
        ids = (~got).astype(np.uint32).astype(np.int64)         # low word = ~id
        rows = ids - row_base
        assert len(np.unique(ids)) == len(ids), (q, "an id appears twice")
        ok = (rows >= 0) & (rows < nrows)
        assert ok.all(), (q, "an id outside the launch's rows", ids[~ok][:8])
        assert (S[q, rows] >= thr[q]).all(), (q, "a key below the threshold", rows[S[q, rows] < thr[q]][:8])
        if stored == len(want):
            assert np.array_equal(np.sort(rows), want), (q, "a survivor is missing", np.setdiff1d(want, rows)[:8])
        bits = (got >> np.uint64(32)).astype(np.uint32)
        exact = f32_orderable(S[q, rows].astype(np.float32))
        assert np.array_equal(bits, exact), (q, "score bits", rows[bits != exact][:8])


def reference_lists(S, thr, row_base, prefix, rng, ncnt=None):
    """What a correct kernel leaves: survivors in a random order behind `prefix` keys, cut at the cap; guards everywhere else"""
    nq, nrows = S.shape
    prefix = np.broadcast_to(np.asarray(prefix, np.int64), (nq,))
    pk = prefix_keys(nq, int(prefix.max())) if prefix.max() else None
    keys = np.full((nq + 1, SORT_CAP), KEY_GUARD, np.uint64)
    cnt = np.full(ncnt or round_up(nq, 256) + 256, CNT_GUARD, np.uint32)
    for q in range(nq):
        p = int(prefix[q])
        want = rng.permutation(np.nonzero(S[q] >= thr[q])[0])
        if p:
            keys[q, :p] = pk[q, :p]
        stored = min(len(want), SORT_CAP - p)
        keys[q, p:p + stored] = pack_keys(S[q, want[:stored]].astype(np.float32), row_base + want[:stored])
        cnt[q] = p + len(want)
    return keys, cnt, pk


def _checker_case():
    rng = np.random.default_rng(7)
    S = rng.integers(-40, 41, size=(6, 400)).astype(np.int64)
    thr = np.array([-np.inf, 30.5, 25.0, np.inf, 12.5, 33.0])
    return S, thr, rng


def test_checker_accepts_the_reference_lists():
    S, thr, rng = _checker_case()
    for prefix in (0, 5):
        keys, cnt, pk = reference_lists(S, thr, ROW_BASE, prefix, rng)
        check_lists(keys, cnt, S, thr, ROW_BASE, prefix, pk)
    assert (S[2] == 25).any(), "the case holds a tie at an integer threshold"


def _corrupt_remove(keys, cnt, pk):           # one survivor removed (the list closed up, the count follows)
    n = int(cnt[1]) - 5
    keys[1, 5:5 + n - 1] = keys[1, 6:5 + n].copy(); keys[1, 5 + n - 1] = KEY_GUARD; cnt[1] -= 1


def _corrupt_remove_keep_count(keys, cnt, pk):      # one survivor's store lost: the count is right, its slot was never written
    keys[1, 6] = KEY_GUARD


def _corrupt_duplicate(keys, cnt, pk):        # one id twice, in place of another survivor
    keys[4, 7] = keys[4, 6]


def _corrupt_duplicate_extra(keys, cnt, pk):  # one id twice, appended
    keys[4, cnt[4]] = keys[4, 6]; cnt[4] += 1


def _corrupt_ulp(keys, cnt, pk):              # one score one ulp off
    keys[0, 17] += np.uint64(1 << 32)


def _corrupt_extra_below(keys, cnt, pk):      # one extra key below the threshold, with its exact score
    S, thr, _ = _checker_case()
    row = int(np.nonzero(S[2] == 24)[0][0])
    keys[2, cnt[2]] = pack_keys(np.float32(24), ROW_BASE + row); cnt[2] += 1


def _corrupt_count(keys, cnt, pk):            # a count off by one
    cnt[5] += 1


def _corrupt_count_empty(keys, cnt, pk):      # ... on the empty list
    cnt[3] += 1


def _corrupt_prefix(keys, cnt, pk):           # a key the list held before
    keys[4, 2] ^= np.uint64(1)


def _corrupt_key_guard(keys, cnt, pk):        # a word of the guard row
    keys[6, 0] = np.uint64(0)


def _corrupt_cnt_guard(keys, cnt, pk):        # a count beyond nq (generation 7 computes on the padded queries)
    cnt[6] = 0


def _corrupt_behind_end(keys, cnt, pk):       # a store behind a list's end
    keys[1, 4000] = keys[1, 6]


def _corrupt_row_base(keys, cnt, pk):         # an id that lost bit 31 of row_base
    keys[1, 6] ^= np.uint64(0x80000000)


@pytest.mark.parametrize("corrupt", [_corrupt_remove, _corrupt_remove_keep_count, _corrupt_duplicate, _corrupt_duplicate_extra, _corrupt_ulp,
                                     _corrupt_extra_below, _corrupt_count, _corrupt_count_empty, _corrupt_prefix, _corrupt_key_guard,
                                     _corrupt_cnt_guard, _corrupt_behind_end, _corrupt_row_base], ids=lambda f: f.__name__[9:])
def test_checker_rejects_each_corruption(corrupt):
    S, thr, rng = _checker_case()
    keys, cnt, pk = reference_lists(S, thr, ROW_BASE, 5, rng)
    check_lists(keys, cnt, S, thr, ROW_BASE, 5, pk)
    corrupt(keys, cnt, pk)
    with pytest.raises(AssertionError):
        check_lists(keys, cnt, S, thr, ROW_BASE, 5, pk)


def test_checker_holds_a_list_over_the_cap_to_true_survivors():
    rng = np.random.default_rng(8)
    S = rng.integers(-40, 41, size=(3, 8448)).astype(np.int64)
    thr = np.array([-np.inf, 30.5, 20.5])
    prefix = np.array([0, 0, 8190])
    keys, cnt, pk = reference_lists(S, thr, ROW_BASE, prefix, rng)
    assert int(cnt[0]) == 8448 and int(cnt[2]) - 8190 > 2
    check_lists(keys, cnt, S, thr, ROW_BASE, prefix, pk)
    below = int(np.nonzero(S[2] < 20.5)[0][0])
    for q, slot, key in ((2, 8191, pack_keys(np.float32(S[2, below]), ROW_BASE + below)),     # one stored key that is no survivor
                         (0, 8191, keys[0, 3]),                                               # one stored key twice
                         (0, 100, keys[0, 100] + np.uint64(1 << 32)),                         # one stored score one ulp off
                         (2, 8190, KEY_GUARD)):                                               # one position below the cap never written
        k2 = keys.copy()
        k2[q, slot] = key
        with pytest.raises(AssertionError):
            check_lists(k2, cnt, S, thr, ROW_BASE, prefix, pk)
    for q, value in ((0, SORT_CAP), (2, int(cnt[2]) - 1)):                                    # cnt clamped at the cap, cnt one short
        c2 = cnt.copy()
        c2[q] = value
        with pytest.raises(AssertionError):
            check_lists(keys, c2, S, thr, ROW_BASE, prefix, pk)


# ------------------------------------------------------------------------------------------------------------ data and thresholds
_CASE = {}


def scan_case(d):
    """Rows, 600 queries and their exact scores at width d, made once: a case takes the first nq queries and the first nrows rows
    (d = 64 and 192 carry the 8 448 rows of the cap test; S covers the 2 093 rows of the exact cases)"""
    if d not in _CASE:
        rng = np.random.default_rng(1000 + d)
        R = rng.integers(-4, 5, size=(ROWS_CAP if d in (64, 192) else ROWS_MAX, d))
        Q = rng.integers(-4, 5, size=(NQ_MAX, d))
        S = Q @ R[:ROWS_MAX].T                                 # int64: exact
        assert np.abs(S).max() <= 16 * d < 2 ** 24
        _CASE[d] = (R, Q, S)
    return _CASE[d]


def thresholds(S):
    """The regimes of one launch (module docstring), float32-exact"""
    nq, nrows = S.shape
    srt = np.sort(S, axis=1)
    thr = srt[:, nrows - max(1, round(0.03 * nrows))] - 0.5            # a half-integer about 3 % of the rows reach
    integer = np.arange(nq) % 4 == 1
    thr[integer] = srt[integer, nrows - min(27, nrows)]                # the 27th best score itself: its ties belong to the list
    thr[0] = -np.inf
    if nq > 1:
        thr[nq // 2] = np.inf
    if nq >= 192:
        thr[160:192] = -np.inf
    assert np.array_equal(thr.astype(np.float32).astype(np.float64), thr)
    return thr


def test_thresholds_cover_the_regimes_and_fit_the_cap():
    rng = np.random.default_rng(3)
    S = rng.integers(-60, 61, size=(600, 1792)).astype(np.int64)
    thr = thresholds(S)
    n = (S >= thr[:, None]).sum(1)
    assert n[0] == 1792 and n[300] == 0 and (n[160:192] == 1792).all() and n.max() <= SORT_CAP
    assert (thr[1::4][np.isfinite(thr[1::4])] % 1 == 0).all() and (n[1] >= 27)
    sparse = n[(np.arange(600) % 4 != 1) & np.isfinite(thr)]
    assert 0.02 * 1792 <= sparse.min() and sparse.max() <= 0.06 * 1792


# -------------------------------------------------------------------------------------------------------------------- the launches
class Lists:
    """keys [nq + 1][SORT_CAP] and cnt [round_up(nq, 256) + 256] on the device: guards everywhere, `prefix` keys and counts in front"""

    def __init__(self, nq, prefix=0):
        self.nq = nq
        self.prefix = np.broadcast_to(np.asarray(prefix, np.int64), (nq,))
        self.pk = prefix_keys(nq, int(self.prefix.max())) if self.prefix.max() else None
        keys = np.full((nq + 1, SORT_CAP), KEY_GUARD, np.uint64)
        cnt = np.full(round_up(nq, 256) + 256, CNT_GUARD, np.uint32)
        cnt[:nq] = self.prefix
        for q in np.nonzero(self.prefix)[0]:
            keys[q, :self.prefix[q]] = self.pk[q, :self.prefix[q]]
        self.keys0, self.cnt0 = keys, cnt
        self.keys = torch.from_numpy(keys.view(np.int64)).to(DEV)
        self.cnt = torch.from_numpy(cnt.view(np.int32)).to(DEV)

    def read(self):
        torch.cuda.synchronize()
        return self.keys.cpu().numpy().view(np.uint64), self.cnt.cpu().numpy().view(np.uint32)


def device_operands(half, R, Q, nq, thr):
    """rows, the query panel (round_up(nq, 256) rows, zero beyond nq) and thr (round_up(nq, 256) + 256 entries, +inf beyond nq)"""
    dt = np.float16 if half else np.float32
    rows = torch.from_numpy(R.astype(dt)).to(DEV)
    qpad = np.zeros((round_up(nq, 256), Q.shape[1]), dt)
    qpad[:nq] = Q[:nq]
    t = np.full(round_up(nq, 256) + 256, np.inf, np.float32)
    t[:nq] = thr
    return rows, torch.from_numpy(qpad).to(DEV), torch.from_numpy(t).to(DEV)


def launch(kernel, half, rows, nrows, row_base, queries, nq, d, thr, lists, grid, group):
    return N.lib().om_debug_scan_kernel(kernel, int(half), N.ptr(rows), nrows, row_base, N.ptr(queries), nq, d, N.ptr(thr), N.ptr(lists.keys),
                                        N.ptr(lists.cnt), grid, group, N.stream_ptr(DEV))


def tile_grid(kernel, nq, nrows):
    return round_up(nrows, 256) // 256 * (round_up(nq, 128) // 128 if kernel == TILE2 else round_up(nq, 256) // 256)


def run_exact(kernel, half, d, nq, nrows, grid=None, qgroup=None, prefix=0):
    assert nrows <= SORT_CAP, "a list at -inf must fit the cap in an exact case"
    R, Q, S = scan_case(d)
    R, S = R[:nrows], S[:nq, :nrows]
    thr = thresholds(S)
    rows, queries, t = device_operands(half, R, Q, nq, thr)
    lists = Lists(nq, prefix)
    if grid is None:
        grid = tile_grid(kernel, nq, nrows)
    rc = launch(kernel, half, rows, nrows, ROW_BASE, queries, nq, d, t, lists, grid, 8 | ((qgroup or 0) << 8))
    assert rc == 0, N.lib().om_last_error()
    keys, cnt = lists.read()
    check_lists(keys, cnt, S, thr, ROW_BASE, prefix, lists.pk)
    assert int(cnt[0]) - int(lists.prefix[0]) == nrows
    if nq > 1:
        assert int(cnt[nq // 2]) == int(lists.prefix[nq // 2])
    if nq >= 192:
        assert (cnt[160:192] - lists.prefix[160:192] == nrows).all()


# generations 2 and 6: (half, d, nq, nrows); every d of a format, every nq and every nrows at least once per format
TILE2_CASES = [(1, 64, 1, 45), (1, 128, 33, 256), (1, 192, 128, 301), (1, 448, 33, 301), (1, 64, 128, 256), (1, 448, 1, 45),
               (0, 64, 33, 301), (0, 192, 1, 256), (0, 448, 128, 45), (0, 192, 128, 301)]
TILE6_CASES = [(1, 64, 129, 45), (1, 128, 256, 256), (1, 192, 257, 301), (1, 448, 600, 2093), (1, 64, 600, 2093), (1, 128, 257, 2093),
               (0, 64, 600, 2093), (0, 192, 129, 256), (0, 448, 257, 301), (0, 192, 256, 45), (0, 448, 600, 2093)]


@pytest.mark.gpu
@pytest.mark.parametrize("half,d,nq,nrows", TILE2_CASES)
def test_tile2_lists_are_exactly_the_survivors(half, d, nq, nrows):
    run_exact(TILE2, half, d, nq, nrows)


@pytest.mark.gpu
@pytest.mark.parametrize("half,d,nq,nrows", TILE6_CASES)
def test_tile6_lists_are_exactly_the_survivors(half, d, nq, nrows):
    run_exact(TILE6, half, d, nq, nrows)


# Generation 7: (d, nq, nrows, grid, qgroup) with group_m = 8.  1 792 rows = 7 row tiles, 600 queries = 3 query tiles: 21 pairs.
#   (1, 8)           one workgroup walks every pair (g7_tile)             (3, 8), (21, 8)   grids that are no multiple of 8 (g7_tile)
#   (8, 8), (16, 8)  the owned walk, one query group                      (16, 2)           3 query tiles: two groups
#   (16, 1)          3 query tiles: four groups, one of them with no query tile -- its workgroups leave at once
#   (64, 8)          256 rows: far more workgroups than pairs
WIDE7_CASES = [(64, 600, 1792, 1, 8), (128, 257, 1792, 3, 8), (64, 129, 1792, 21, 8), (128, 600, 1792, 8, 8), (64, 257, 1792, 16, 8),
               (128, 600, 1792, 16, 2), (64, 600, 1792, 16, 1), (128, 129, 256, 64, 8), (64, 600, 256, 8, 8), (64, 600, 1792, 16, 2),
               (128, 600, 1792, 16, 1), (128, 600, 1792, 1, 8)]
WIDE7C_CASES = [(192, 600, 1792, 1, 8), (256, 257, 1792, 3, 8), (448, 129, 1792, 21, 8), (256, 600, 1792, 8, 8), (192, 257, 1792, 16, 8),
                (448, 600, 1792, 16, 2), (256, 600, 1792, 16, 1), (192, 129, 256, 64, 8), (448, 600, 256, 8, 8), (192, 600, 1792, 16, 2),
                (448, 600, 1792, 16, 1), (448, 600, 1792, 21, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,nq,nrows,grid,qgroup", WIDE7_CASES)
def test_wide7_lists_are_exactly_the_survivors(d, nq, nrows, grid, qgroup):
    run_exact(WIDE7, 1, d, nq, nrows, grid, qgroup)


@pytest.mark.gpu
@pytest.mark.parametrize("d,nq,nrows,grid,qgroup", WIDE7C_CASES)
def test_wide7c_lists_are_exactly_the_survivors(d, nq, nrows, grid, qgroup):
    run_exact(WIDE7C, 1, d, nq, nrows, grid, qgroup)


# once per kernel and format: (kernel, half, d, nq, nrows, grid, qgroup)
APPEND_CASES = [(TILE2, 0, 192, 33, 301, None, None), (TILE2, 1, 192, 33, 301, None, None), (TILE6, 0, 192, 257, 301, None, None),
                (TILE6, 1, 192, 257, 301, None, None), (WIDE7, 1, 128, 257, 1792, 16, 8), (WIDE7C, 1, 192, 257, 1792, 16, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,half,d,nq,nrows,grid,qgroup", APPEND_CASES, ids=[f"{NAME[c[0]]}-{'f16' if c[1] else 'f32'}" for c in APPEND_CASES])
def test_survivors_are_appended_behind_the_keys_a_list_holds(kernel, half, d, nq, nrows, grid, qgroup):
    run_exact(kernel, half, d, nq, nrows, grid, qgroup, prefix=5)


# once per kernel and format: (kernel, half, d, nq, grid, qgroup) over 8 448 rows = 33 row tiles
CAP_CASES = [(TILE2, 0, 64, 3, None, None), (TILE2, 1, 64, 3, None, None), (TILE6, 0, 64, 129, None, None), (TILE6, 1, 64, 129, None, None),
             (WIDE7, 1, 64, 129, 8, 8), (WIDE7C, 1, 192, 129, 8, 8)]
_CAP_S = {}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,half,d,nq,grid,qgroup", CAP_CASES, ids=[f"{NAME[c[0]]}-{'f16' if c[1] else 'f32'}" for c in CAP_CASES])
def test_a_full_list_keeps_the_true_count_and_leaves_its_neighbours_alone(kernel, half, d, nq, grid, qgroup):
    """Queries 0 and 1 at -inf over 8 448 rows, the last query behind 8 190 keys at a 3 % threshold: cnt is the full count, the keys
    below the cap are distinct true survivors with their exact scores, every other list is exact, the guard row behind the last --
    over-full -- list is untouched."""
    R, Q, _ = scan_case(d)
    if d not in _CAP_S:
        _CAP_S[d] = Q[:129] @ R.T
    nrows = ROWS_CAP
    S = _CAP_S[d][:nq]
    thr = thresholds(S)
    thr[1] = -np.inf
    srt = np.sort(S[nq - 1])
    thr[nq - 1] = srt[nrows - round(0.03 * nrows)] - 0.5
    prefix = np.zeros(nq, np.int64)
    prefix[nq - 1] = SORT_CAP - 2
    rows, queries, t = device_operands(half, R, Q, nq, thr)
    lists = Lists(nq, prefix)
    rc = launch(kernel, half, rows, nrows, ROW_BASE, queries, nq, d, t, lists, grid or tile_grid(kernel, nq, nrows), 8 | ((qgroup or 0) << 8))
    assert rc == 0, N.lib().om_last_error()
    keys, cnt = lists.read()
    check_lists(keys, cnt, S, thr, ROW_BASE, prefix, lists.pk)
    assert int(cnt[0]) == int(cnt[1]) == nrows > SORT_CAP
    assert int(cnt[nq - 1]) == SORT_CAP - 2 + int((S[nq - 1] >= thr[nq - 1]).sum()) > SORT_CAP


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    if value is not None:
        N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


@pytest.mark.gpu
@pytest.mark.parametrize("gen7,half,nq,d", [(None, 1, 300, 64), (None, 1, 300, 192), (None, 0, 300, 192), (None, 0, 64, 192),
                                            (0, 1, 300, 192), (0, 1, 64, 192)])
def test_the_planned_round_fills_the_lists_exactly(gen7, half, nq, d):
    """What om_debug_scan_round plans for 1 837 = 7 x 256 + 45 rows on THIS device's compute units, launched as planned -- main and tail
    into the same lists -- leaves exactly the survivors of all the rows: the planner's kernel, rows, grid and group are numbers the
    kernels honour."""
    nrows = 1837
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = (C.c_int64 * 8)()
    with switched(N.OPT_SCAN_GEN7, gen7):
        N.check(N.lib().om_debug_scan_round(half, nq, d, nrows, cus, out))
    main, tail = tuple(out[:4]), tuple(out[4:])
    print(f"gen7={gen7} half={half} nq={nq} d={d} cus={cus}: main {main} tail {tail}")
    assert main[1] + tail[1] == nrows
    R, Q, S = scan_case(d)
    R, S = R[:nrows], S[:nq, :nrows]
    thr = thresholds(S)
    rows, queries, t = device_operands(half, R, Q, nq, thr)
    lists = Lists(nq)
    row0 = 0
    for kernel, n, grid, group in (main, tail):
        if n:
            assert kernel in NAME, kernel
            rc = launch(kernel, half, rows[row0:], n, ROW_BASE + row0, queries, nq, d, t, lists, grid, group)
            assert rc == 0, N.lib().om_last_error()
        row0 += n
    keys, cnt = lists.read()
    check_lists(keys, cnt, S, thr, ROW_BASE, 0)


# ------------------------------------------------------------------------------------------------------------------- the refusals
# (what changes against a launch the hook accepts, a piece of its message); the accepted launch: kernel TILE6, half 1, 256 rows, 129 queries,
# d = 64, grid 1, group 8
REFUSALS = [
    (dict(rows=None), b"null"), (dict(queries=None), b"null"), (dict(thr=None), b"null"), (dict(keys=None), b"null"), (dict(cnt=None), b"null"),
    (dict(kernel=0), b"kernel must be"), (dict(kernel=STREAM), b"kernel must be"), (dict(kernel=-1), b"kernel must be"),
    (dict(kernel=WIDE7, half=0, grid=8), b"16-bit"), (dict(kernel=WIDE7C, half=0, d=192, grid=8), b"16-bit"),
    (dict(d=0), b"multiple of 64"), (dict(d=-64), b"multiple of 64"), (dict(d=96), b"multiple of 64"),
    (dict(nrows=0), b"nrows >= 1"), (dict(nq=0), b"nq >= 1"),
    (dict(kernel=WIDE7, grid=0), b"grid"), (dict(kernel=WIDE7, grid=2 ** 31), b"grid"), (dict(grid=0), b"grid"),
    (dict(group=8 << 8), b"group_m"),
    (dict(kernel=WIDE7, nrows=255, grid=8), b"whole 256-row tiles"), (dict(kernel=WIDE7C, d=192, nrows=257, grid=8), b"whole 256-row tiles"),
    (dict(kernel=WIDE7C, d=128, grid=8), b"three"),
    (dict(grid=2), b"one workgroup per"), (dict(kernel=TILE2, grid=1), b"one workgroup per"),
]


def _refused(bufs, change):
    a = dict(kernel=TILE6, half=1, nrows=256, nq=129, d=64, grid=1, group=8, **bufs)
    a.update(change)
    return N.lib().om_debug_scan_kernel(a["kernel"], a["half"], a["rows"], a["nrows"], ROW_BASE, a["queries"], a["nq"], a["d"], a["thr"],
                                        a["keys"], a["cnt"], a["grid"], a["group"], None)


@pytest.mark.parametrize("change,message", REFUSALS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_hook_refuses_before_any_device_call(change, message):
    """Without a GPU: every refusal is decided on the host, before the first HIP call (the pointers are never followed)"""
    host = np.zeros(64, np.uint64)
    p = C.c_void_p(host.ctypes.data)
    assert _refused(dict(rows=p, queries=p, thr=p, keys=p, cnt=p), change) == 1
    assert message in N.lib().om_last_error(), N.lib().om_last_error()


@pytest.mark.gpu
def test_hook_refusals_launch_nothing():
    R, Q, S = scan_case(64)
    thr = np.full(129, -np.inf)                       # a launch would fill every list
    rows, queries, t = device_operands(1, R[:512], Q, 129, thr)
    lists = Lists(129)
    bufs = dict(rows=N.ptr(rows), queries=N.ptr(queries), thr=N.ptr(t), keys=N.ptr(lists.keys), cnt=N.ptr(lists.cnt))
    for change, message in REFUSALS:
        assert _refused(bufs, change) == 1, change
        assert message in N.lib().om_last_error(), (change, N.lib().om_last_error())
    keys, cnt = lists.read()
    assert np.array_equal(keys, lists.keys0) and np.array_equal(cnt, lists.cnt0)
