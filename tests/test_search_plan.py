"""Which kernel a filtered-scan round of om_sim_topk runs (csrc/search_plan.h), walked on the CPU through
om_debug_scan_plan.  Every expected value is written out by hand from the rules; the rows for 256 <= d <= 768, for d < 256, for more
than 128 queries, for the float32 index and for OM_OPT_SCAN_GEN7 = 0 are what Scan::filter_step's own `if` chain chose before the plan
existed."""
import contextlib
import ctypes as C

import pytest

from openmatch_amd import native as N

GENERIC, WIDE, STREAM32, STREAM16 = (N.SCAN_FAMILY[k] for k in ("generic", "wide", "stream32", "stream16"))
OPT_SCAN_GEN7 = 3          # include/openmatch_hip.h


def plan(half, nq, d):
    out = (C.c_int * 4)()
    N.check(N.lib().om_debug_scan_plan(int(half), nq, d, out))
    return tuple(out)


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


NQ32 = [(1, 1), (32, 1), (33, 2), (64, 2), (65, 4), (128, 4)]          # (queries, resident 32-query blocks)
NQ16 = [(1, 1), (16, 1), (17, 2), (32, 2), (33, 4), (64, 4)]           # (queries, resident 16-query blocks)


@pytest.mark.parametrize("d", [256, 320, 768])
def test_narrow_rows_run_the_32_query_stream_kernel_with_12_k_steps(d):
    for nq, nb in NQ32:
        assert plan(1, nq, d) == (STREAM32, 32, nb, 12), (nq, d)


@pytest.mark.parametrize("d", [832, 896, 1024])
def test_rows_up_to_1024_run_the_32_query_stream_kernel_with_16_k_steps(d):
    for nq, nb in NQ32:
        assert plan(1, nq, d) == (STREAM32, 32, nb, 16), (nq, d)


@pytest.mark.parametrize("d", [1088, 1536, 2048])
def test_rows_up_to_2048_run_the_16_query_stream_kernel(d):
    for nq, nb in NQ16:
        assert plan(1, nq, d) == (STREAM16, 16, nb, 32), (nq, d)
    for nq in (65, 128):
        assert plan(1, nq, d) == (GENERIC, 0, 0, 0), (nq, d)


@pytest.mark.parametrize("d", [64, 192, 2112])
def test_rows_outside_the_stream_kernels_stay_on_the_generic_tile(d):
    for nq in (1, 16, 32, 64, 128):
        assert plan(1, nq, d) == (GENERIC, 0, 0, 0), (nq, d)


@pytest.mark.parametrize("d", [64, 768, 1024, 2048, 2112])
def test_more_than_128_queries_are_wide_in_both_formats(d):
    for half in (0, 1):
        assert plan(half, 129, d) == (WIDE, 0, 0, 0)
        assert plan(half, 4096, d) == (WIDE, 0, 0, 0)


@pytest.mark.parametrize("d", [256, 768, 1024, 2048])
def test_the_float32_index_stays_on_the_generic_tile(d):
    for nq in (1, 16, 64, 128):
        assert plan(0, nq, d) == (GENERIC, 0, 0, 0), (nq, d)


@pytest.mark.parametrize("d", [256, 768, 1024, 2048])
def test_switch_off_sends_small_batches_to_the_generic_tile(d):
    with switched(OPT_SCAN_GEN7, 0):
        for nq in (1, 16, 64, 128):
            assert plan(1, nq, d) == (GENERIC, 0, 0, 0), (nq, d)
        assert plan(1, 129, d) == (WIDE, 0, 0, 0)
    assert plan(1, 1, d)[0] in (STREAM32, STREAM16)            # restored


def test_null_output_is_refused():
    assert N.lib().om_debug_scan_plan(1, 1, 768, None) == 1
    assert b"null argument" in N.lib().om_last_error()


# ---- the launches of a round (scan_round through om_debug_scan_round), on a device of 256 compute units -------------------------------
TILE2, TILE6, WIDE7, WIDE7C, STREAM = (N.SCAN_KERNEL[k] for k in ("tile2", "tile6", "wide7", "wide7c", "stream"))
OPT_SCAN_QGROUP, OPT_SEARCH_DEBUG, OPT_GEMM_CONT = 7, 13, 16          # include/openmatch_hip.h
NONE = (0, 0, 0, 0)
QGROUP8 = 8 | 8 << 8                                                   # group_m 8, OM_OPT_SCAN_QGROUP's default 8


def scan_round(half, nq, d, rows, cus=256):
    """((kernel, rows, grid, group) of the main launch, the same of the tail)"""
    out = (C.c_int64 * 8)()
    N.check(N.lib().om_debug_scan_round(int(half), nq, d, rows, cus, out))
    return tuple(out[:4]), tuple(out[4:])


def test_a_wide_round_splits_into_whole_tiles_on_the_ring_and_a_ragged_tail():
    # 3629 = 14 * 256 + 45 rows, 300 queries = 2 query tiles: 28 (row tile, query tile) pairs, fewer than the CUs
    assert scan_round(1, 300, 768, 3629) == ((WIDE7C, 3584, 28, QGROUP8), (TILE6, 45, 2, 8))
    assert scan_round(1, 300, 768, 255) == (NONE, (TILE6, 255, 2, 8))
    assert scan_round(1, 300, 768, 4096) == ((WIDE7C, 4096, 32, QGROUP8), NONE)
    assert scan_round(1, 300, 768, 256) == ((WIDE7C, 256, 2, QGROUP8), NONE)


def test_the_continuous_ring_needs_three_k_steps():
    for d, kernel in ((64, WIDE7), (128, WIDE7), (192, WIDE7C), (256, WIDE7C)):
        assert scan_round(1, 300, d, 3629) == ((kernel, 3584, 28, QGROUP8), (TILE6, 45, 2, 8)), d


@pytest.mark.parametrize("cont", [495, 495 & ~4, 495 | 1024, (495 & ~4) | 1024, 0])
def test_bits_2_and_10_of_the_gemm_switch_change_nothing(cont):
    with switched(OPT_GEMM_CONT, cont):
        assert scan_round(1, 300, 768, 3629) == ((WIDE7C, 3584, 28, QGROUP8), (TILE6, 45, 2, 8))
        assert scan_round(1, 300, 128, 3629) == ((WIDE7, 3584, 28, QGROUP8), (TILE6, 45, 2, 8))
        assert scan_round(1, 64, 768, 3629) == ((STREAM, 3584, 28, 1), (TILE2, 45, 1, 8))


def test_switch_off_is_one_launch_of_a_tile_kernel():
    with switched(OPT_SCAN_GEN7, 0):
        assert scan_round(1, 300, 768, 3629) == ((TILE6, 3629, 15 * 2, 8), NONE)      # 15 row tiles x 2 query tiles
        assert scan_round(1, 64, 768, 3629) == ((TILE2, 3629, 15 * 1, 8), NONE)       # 15 row tiles x 1 query tile of 128
        assert scan_round(1, 300, 768, 4096) == ((TILE6, 4096, 32, 8), NONE)


def test_the_float32_index_is_one_launch_of_a_tile_kernel():
    assert scan_round(0, 300, 768, 3629) == ((TILE6, 3629, 30, 8), NONE)
    assert scan_round(0, 64, 768, 3629) == ((TILE2, 3629, 15, 8), NONE)
    assert scan_round(0, 128, 768, 256) == ((TILE2, 256, 1, 8), NONE)
    assert scan_round(0, 257, 64, 257) == ((TILE6, 257, 4, 8), NONE)                  # 2 row tiles x 2 query tiles


def test_a_stream_round_splits_into_128_row_tiles_and_a_generic_tail():
    # 3629 = 28 * 128 + 45
    for nq, d in ((1, 768), (64, 768), (128, 1024), (64, 2048)):
        assert scan_round(1, nq, d, 3629) == ((STREAM, 3584, 28, 1), (TILE2, 45, 1, 8)), (nq, d)
    assert scan_round(1, 64, 768, 127) == (NONE, (TILE2, 127, 1, 8))
    assert scan_round(1, 64, 768, 3584) == ((STREAM, 3584, 28, 1), NONE)
    assert scan_round(1, 64, 192, 3629) == ((TILE2, 3629, 15, 8), NONE)               # no stream kernel below four K steps


def test_persistent_grids_never_exceed_the_compute_units():
    rows = 1 << 20
    assert scan_round(1, 300, 768, rows) == ((WIDE7C, rows, 256, QGROUP8), NONE)       # 4096 x 2 pairs
    assert scan_round(1, 300, 128, rows + 45) == ((WIDE7, rows, 256, QGROUP8), (TILE6, 45, 2, 8))
    assert scan_round(1, 64, 768, rows) == ((STREAM, rows, 256, 1), NONE)               # 8192 tiles
    assert scan_round(1, 300, 768, rows, cus=7)[0] == (WIDE7C, rows, 7, QGROUP8)
    assert scan_round(1, 64, 768, rows, cus=7)[0] == (STREAM, rows, 7, 1)
    for cus in (1, 13, 256, 304):
        for nq, d in ((300, 768), (4096, 128), (1, 768), (64, 2048)):
            for r in (128, 256, 3629, rows):
                main, _tail = scan_round(1, nq, d, r, cus=cus)
                assert main == NONE or 1 <= main[2] <= cus, (cus, nq, d, r, main)


def test_the_query_group_switch_appears_in_the_group_argument():
    with switched(OPT_SCAN_QGROUP, 3):
        assert scan_round(1, 300, 768, 3629) == ((WIDE7C, 3584, 28, 8 | 3 << 8), (TILE6, 45, 2, 8))
    with switched(OPT_SCAN_QGROUP, 0):                                                  # at least one tile
        assert scan_round(1, 300, 768, 3629)[0] == (WIDE7C, 3584, 28, 8 | 1 << 8)
    assert scan_round(1, 300, 768, 3629)[0] == (WIDE7C, 3584, 28, QGROUP8)              # restored


def test_the_cache_policy_switch_appears_in_the_stream_kernels_last_argument():
    with switched(OPT_SEARCH_DEBUG, 4):
        assert scan_round(1, 64, 768, 3629) == ((STREAM, 3584, 28, 0), (TILE2, 45, 1, 8))
    assert scan_round(1, 64, 768, 3629)[0] == (STREAM, 3584, 28, 1)


def test_a_grid_above_31_bits_is_refused_where_it_is_one_workgroup_per_tile():
    rows = (1 << 32) - 1                                                                # 2^24 row tiles x 128 query tiles = 2^31
    assert N.lib().om_debug_scan_round(0, 32768, 768, rows, 256, (C.c_int64 * 8)()) == 1
    assert b"scan grid too large" in N.lib().om_last_error()
    assert scan_round(1, 32768, 768, rows)[0] == (WIDE7C, rows & ~255, 256, QGROUP8)    # persistent: the grid is the CUs


def test_null_round_output_is_refused():
    assert N.lib().om_debug_scan_round(1, 1, 768, 4096, 256, None) == 1
    assert b"null argument" in N.lib().om_last_error()
