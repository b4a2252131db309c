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
