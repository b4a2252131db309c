"""The accumulation term of the certified margin (csrc/search.hip query_prep_kernel) against the scan's own scores.

The margin bounds |s_f16 - s_f32| by the rounding of the operands plus the float32 accumulation error of the 16-bit scan and of the
re-score.  The accumulation part is bounded by depth: a product (exact in float32: two 11-bit significands) takes part in at most the
32 additions inside one MFMA and one addition per later MFMA of its chain, d / 16 at most, each taken at 2^-23.  This file measures
that error where it is largest relative to its bound -- operands of one sign, so that sum |q_i p_i| = <q, p> -- on both matrix-core
shapes the stream kernels use, through om_debug_sim_stream with every threshold at -inf, and asserts the bound for every (query, row):
    |score - <q, p> in float64|  <=  2 (32 + d / 16) 2^-24 |q| |p|
The operands are float16 values already, so nothing but accumulation separates the two sides."""
import numpy as np
import pytest

from tests.test_search_widths import NROWS, ROW_BASE, orderable_f32, run_stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,nq", [(768, 33), (1024, 128), (2048, 64)])       # 32 x 32 x 16 with 12 and 16 K steps; 16 x 16 x 32
def test_scan_accumulation_error_is_inside_the_margins_depth_bound(d, nq):
    rng = np.random.default_rng(d + nq)
    R = rng.random((NROWS, d)).astype(np.float16)
    Q = rng.random((nq, d)).astype(np.float16)
    rc, keys, cnt = run_stream(R, Q, np.full(nq, -np.inf, np.float32), nq, d)
    assert rc == 0
    assert (cnt == NROWS).all()
    exact = Q.astype(np.float64) @ R.astype(np.float64).T
    bound = 2.0 * (32 + d / 16) * 2.0 ** -24 * np.outer(np.linalg.norm(Q.astype(np.float64), axis=1), np.linalg.norm(R.astype(np.float64), axis=1))
    worst = 0.0
    for q in range(nq):
        ids = (~keys[q, :NROWS]).astype(np.uint32).astype(np.int64) - ROW_BASE
        assert sorted(ids.tolist()) == list(range(NROWS))
        got = orderable_f32(keys[q, :NROWS] >> np.uint64(32)).astype(np.float64)
        err = np.abs(got - exact[q, ids])
        worst = max(worst, float((err / bound[q, ids]).max()))
    print(f"d={d} nq={nq}: largest accumulation error / bound = {worst:.3f}")
    assert worst <= 1.0
