"""Filtered exact search, the parts that need no GPU (DESIGN.md 4f "Filtered search"): the symbols of om_sim_topk_filtered, its refusals
(each before any launch: the pointers are fake and never followed), the filtered schedule (csrc/search_plan.h search_schedule_filtered
through om_debug_search_schedule_filtered) by its properties, the route table (openmatch_amd.index.filter_route) and RowFilter.pack."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from openmatch_amd.index import LIST_MAX, RowFilter, filter_route

DENSE_CHUNK = 4096


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


def test_the_three_symbols_exist_and_are_bound():
    lib = N.lib()
    for name in ("om_sim_topk_filtered_workspace_bytes", "om_sim_topk_filtered", "om_debug_search_schedule_filtered"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None
    assert lib.om_abi_version() == 6
    for n, d, k in [(1, 64, 1), (300, 768, 100), (32768, 64, 2048)]:
        assert lib.om_sim_topk_filtered_workspace_bytes(n, d, k) >= lib.om_sim_topk_async_workspace_bytes(n, d, k) > 0
    assert lib.om_sim_topk_filtered_workspace_bytes(0, 64, 10) == 0


def _refused(k=10, d=64, n=5000, bits=0x3000, n_allowed=100, status=0x2000, mode=N.SEARCH_F16_RESCORE):
    fake = N.c_void_p(0x1000)
    return N.lib().om_sim_topk_filtered(mode, fake, 3, fake, fake, fake, n, d, k, 0, N.c_void_p(bits), n_allowed, fake, fake,
                                        N.c_void_p(status), fake, 1 << 40, N.c_void_p(0))


@pytest.mark.parametrize("mode", [N.SEARCH_F32, N.SEARCH_F16_RESCORE, N.SEARCH_F16_ONLY])
def test_refusals_of_the_async_entry(mode):
    err = N.lib().om_last_error
    assert _refused(k=2049, mode=mode) == 1 and b"2048" in err()
    assert _refused(d=16384 + 64, mode=mode) == 1 and b"16384" in err()
    with switched(N.OPT_SCAN_GEN7, 0):
        assert _refused(mode=mode) == 1 and b"OM_OPT_SCAN_GEN7" in err()


def test_a_null_bitmap_is_refused():
    assert _refused(bits=0) == 1 and b"allow_bits" in N.lib().om_last_error()


@pytest.mark.parametrize("n_allowed", [-1, 5001, 1 << 40])
def test_n_allowed_outside_the_shard_is_refused(n_allowed):
    assert _refused(n_allowed=n_allowed) == 1 and b"n_allowed" in N.lib().om_last_error()


def test_too_small_a_workspace_is_refused():
    fake = N.c_void_p(0x1000)
    rc = N.lib().om_sim_topk_filtered(N.SEARCH_F32, fake, 3, fake, fake, fake, 5000, 64, 10, 0, fake, 100, fake, fake, N.c_void_p(0), fake, 4096,
                                      N.c_void_p(0))
    assert rc == 1 and b"workspace" in N.lib().om_last_error()


# ---------------------------------------------------------------------------------------------------------- the schedule
def schedule_filtered(mode, nq, n, k, n_allowed):
    cap = 1024
    chunks, cnt, boot = (C.c_int64 * cap)(), C.c_int(-1), C.c_int64(-1)
    N.check(N.lib().om_debug_search_schedule_filtered(mode, nq, n, k, n_allowed, chunks, cap, C.byref(cnt), C.byref(boot)))
    assert 0 <= cnt.value <= cap
    return boot.value, list(chunks[:cnt.value])


def schedule(mode, nq, n, k):
    cap = 1024
    chunks, cnt = (C.c_int64 * cap)(), C.c_int(-1)
    N.check(N.lib().om_debug_search_schedule(mode, nq, n, k, chunks, cap, C.byref(cnt)))
    return list(chunks[:cnt.value])


MODES = pytest.mark.parametrize("mode", [N.SEARCH_F32, N.SEARCH_F16_RESCORE, N.SEARCH_F16_ONLY], ids=["f32", "f16_rescore", "f16"])


@MODES
@pytest.mark.parametrize("k", [10, 100, 1000, 2048])
@pytest.mark.parametrize("nq", [1, 64, 300, 6980])
@pytest.mark.parametrize("n", [0, 300, 4096, 4097, 50000, 8841823])
def test_all_rows_allowed_is_the_unfiltered_schedule(mode, k, nq, n):
    boot, chunks = schedule_filtered(mode, nq, n, k, n)
    assert boot == 1 and chunks == schedule(mode, nq, n, k)


@MODES
@pytest.mark.parametrize("k", [10, 1000])
@pytest.mark.parametrize("nq", [1, 64, 300, 6980])
@pytest.mark.parametrize("n", [4097, 50000, 8841823])
@pytest.mark.parametrize("p", [0.9, 0.5, 0.1, 0.01, 0.0001])
def test_filtered_schedule_properties(mode, k, nq, n, p):
    n_allowed = max(1, int(n * p))
    boot, chunks = schedule_filtered(mode, nq, n, k, n_allowed)
    all_chunks = -(-n // DENSE_CHUNK)
    want = -(-2 * k * n // (DENSE_CHUNK * n_allowed))                   # smallest B with B * 4096 * n_allowed / n >= 2 k
    assert boot == min(max(want, 1), all_chunks)
    assert (boot - 1) * DENSE_CHUNK * n_allowed < 2 * k * n             # ... and no smaller one (or every row is scored densely)
    assert boot * DENSE_CHUNK * n_allowed >= 2 * k * n or boot == all_chunks
    if boot * DENSE_CHUNK >= n:
        assert chunks == []
        return
    assert chunks and all(c > 0 for c in chunks)
    starts = np.concatenate([[boot * DENSE_CHUNK], boot * DENSE_CHUNK + np.cumsum(chunks)])
    assert starts[0] == boot * DENSE_CHUNK and starts[-1] == n           # starts behind the bootstrap, contiguous to N
    assert all(c % 256 == 0 for c in chunks[:-1])                        # whole tiles
    assert all(4 * b >= a for a, b in zip(chunks, chunks[1:])), chunks   # no sliver
    assert all(c >= DENSE_CHUNK for c in chunks[:-1])


@MODES
def test_the_bootstrap_grows_as_the_filter_thins(mode):
    n, k = 8841823, 100
    boots = [schedule_filtered(mode, 64, n, k, max(1, int(n * p)))[0] for p in (1.0, 0.5, 0.1, 0.01, 0.001)]
    assert boots[0] == 1 and boots == sorted(boots) and boots[-1] > boots[1] >= 1, boots
    assert boots[2:] == [1, 5, 49], boots                                # ceil(200 / (4096 p))
    # k_eff: the rounds are never longer than those of the unfiltered schedule for the same k
    full = schedule(mode, 64, n, k)
    for p in (0.5, 0.1):
        _, chunks = schedule_filtered(mode, 64, n, k, int(n * p))
        assert len(chunks) >= len(full) and chunks[0] <= full[0]


def test_no_row_allowed_counts_as_one():
    assert schedule_filtered(N.SEARCH_F32, 4, 20000, 10, 0) == schedule_filtered(N.SEARCH_F32, 4, 20000, 10, 1) == (5, [])


# ---------------------------------------------------------------------------------------------------------- the route table
def list_estimate(precision, k_eff):
    return k_eff * 13 // 10 + 64 if precision != "f32" else k_eff + 16


def test_route_empty_and_contiguous():
    for precision in ("f16_rescore", "f32", "f16"):
        assert filter_route(precision, 10, 0, -1, 0) == "empty"
        assert filter_route(precision, 10, 0, -1, 0, route="scan") == "empty"
        assert filter_route(precision, 10, 5000, 16999, 12000) == "range"
        assert filter_route(precision, 10, 0, 19999, 20000) == "range"
        assert filter_route(precision, 10, 7, 7, 1) == "range"
        assert filter_route(precision, 10, 5000, 16999, 11999) != "range"


@pytest.mark.parametrize("precision", ["f16_rescore", "f32", "f16"])
@pytest.mark.parametrize("k", [10, 100, 1000])
def test_route_boundary_is_list_max(precision, k):
    rows = 1 << 20                                                       # first = 0: the scan would read [0, rows)
    # the sparsest filter that still scans: the largest k_eff whose list estimate is at most LIST_MAX
    k_max = max(ke for ke in range(k, 5000) if list_estimate(precision, ke) <= LIST_MAX)
    assert list_estimate(precision, k_max) <= LIST_MAX < list_estimate(precision, k_max + 1)
    # the smallest n_allowed with ceil(k * rows / n_allowed) <= k_max scans, one allowed row fewer gathers
    n_scan = -(-k * rows // k_max)
    n_gather = n_scan - 1
    assert -(-k * rows // n_scan) <= k_max < -(-k * rows // n_gather)
    assert filter_route(precision, k, 0, rows - 1, n_scan) == "scan"
    assert filter_route(precision, k, 0, rows - 1, n_gather) == "gather"
    assert filter_route(precision, k, 0, rows - 1, n_gather, route="scan") == "scan"
    assert filter_route(precision, k, 0, rows - 1, n_scan, route="gather") == "gather"
    assert filter_route(precision, k, 0, rows - 1, rows, route="scan") == "scan"       # a forced route comes before 'range'
    with pytest.raises(ValueError):
        filter_route(precision, k, 0, rows - 1, n_scan, route="range")


MODE_OF = {"f16_rescore": N.SEARCH_F16_RESCORE, "f32": N.SEARCH_F32, "f16": N.SEARCH_F16_ONLY}


@pytest.mark.parametrize("precision", ["f16_rescore", "f32", "f16"])
def test_route_rule_is_the_native_estimate(precision):
    """filter_route repeats in Python what csrc/search_plan.h computes (k_eff, the mode's list estimate) and search.hip's LIST_MAX: it
    scans exactly where the estimate the device schedule sizes its rounds from is at most the native LIST_MAX"""
    lib = N.lib()
    assert "om_debug_search_filter_estimate" in N.exported_symbols()
    est, cap = C.c_int64(), C.c_int64()
    rng = np.random.default_rng(7)
    seen = set()
    for k in (1, 10, 100, 1000, 2048):
        for rows in (4097, 20000, 1 << 20, 8_800_000):
            dense = [rows - 1, rows // 2, max(1, rows // 10)]
            # around the boundary: n_allowed where ceil(k rows / n_allowed) sits near the k_eff that fills LIST_MAX
            near = [max(1, min(rows - 1, k * rows // ke + o)) for ke in (3100, 3101, 4079, 4080, 4081) for o in (-1, 0, 1)]
            for n_allowed in dense + near + [int(x) for x in rng.integers(1, rows, 8)]:
                N.check(lib.om_debug_search_filter_estimate(MODE_OF[precision], rows, k, n_allowed, C.byref(est), C.byref(cap)))
                assert cap.value == LIST_MAX
                assert est.value == list_estimate(precision, -(-k * rows // n_allowed))
                want = "scan" if est.value <= cap.value else "gather"
                assert filter_route(precision, k, 0, rows - 1, n_allowed) == want
                seen.add(want)
    assert seen == {"scan", "gather"}
    assert lib.om_debug_search_filter_estimate(MODE_OF[precision], 100, 10, 0, C.byref(est), C.byref(cap)) == 1
    assert lib.om_debug_search_filter_estimate(MODE_OF[precision], 100, 10, 101, C.byref(est), C.byref(cap)) == 1


def test_route_counts_the_rows_the_scan_reads():
    # 2000 allowed rows spread over [1000000, 1100000): k_eff is taken over the 100 000-odd rows from 999 936 on, not over the index
    assert filter_route("f16_rescore", 10, 1000000, 1099999, 2000) == "scan"          # k_eff 501
    assert filter_route("f16_rescore", 100, 1000000, 1099999, 2000) == "gather"       # k_eff 5004


# ---------------------------------------------------------------------------------------------------------- RowFilter
class _Host:
    """what RowFilter reads of an index"""
    def __init__(self, ntotal):
        self.ntotal, self.device = ntotal, torch.device("cpu")


def bits_of(words, n):
    w = words.numpy().view(np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000, 4097, 100003])
def test_pack_against_numpy(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.4
    words = RowFilter.pack(torch.from_numpy(mask))
    assert words.dtype == torch.int32 and words.shape == ((n + 31) // 32,)
    assert np.array_equal(bits_of(words, n), mask)
    w = words.numpy().view(np.uint32)
    assert int(np.unpackbits(w.view(np.uint8)).sum()) == int(mask.sum())   # the bits of the last word beyond n are clear
    assert np.array_equal(w, np.packbits(np.concatenate([mask, np.zeros(-n % 32, bool)]), bitorder="little").view(np.uint32))


def test_pack_all_ones_sets_bit_31():
    words = RowFilter.pack(torch.ones(70, dtype=torch.bool))
    assert words.tolist() == [-1, -1, 63]


@pytest.mark.parametrize("n", [37, 4097])
def test_ids_mask_and_invert_agree(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.3
    ids = np.nonzero(mask)[0]
    host = _Host(n)
    by_mask = RowFilter(host, torch.from_numpy(mask))
    by_ids = RowFilter(host, ids[rng.permutation(len(ids))])             # any order; numpy ids
    by_list = RowFilter(host, [int(i) for i in ids] + [int(ids[0])])     # a plain sequence, with a repeat
    excluded = RowFilter(host, torch.from_numpy(np.nonzero(~mask)[0]), invert=True)
    not_mask = RowFilter(host, torch.from_numpy(~mask), invert=True)
    for f in (by_mask, by_ids, by_list, excluded, not_mask):
        assert torch.equal(f.words, by_mask.words)
        assert (f.n_allowed, f.first, f.last) == (int(mask.sum()), int(ids[0]), int(ids[-1]))
        assert f.ntotal == n and np.array_equal(f.ids().numpy(), ids)
    nothing = RowFilter(host, torch.zeros(0, dtype=torch.int64))
    assert nothing.n_allowed == 0 and not nothing.words.any()
    everything = RowFilter(host, torch.zeros(0, dtype=torch.int64), invert=True)
    assert (everything.n_allowed, everything.first, everything.last) == (n, 0, n - 1)


def test_filter_argument_errors():
    host = _Host(100)
    with pytest.raises(ValueError):
        RowFilter(host, torch.ones(99, dtype=torch.bool))
    with pytest.raises(ValueError):
        RowFilter(host, [3, 100])
    with pytest.raises(ValueError):
        RowFilter(host, [-1])
