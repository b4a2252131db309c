"""Every launch branch of a filtered round (csrc/search_plan.h scan_round, launched from the kernel table of csrc/search_scan.hip by
Scan::filter_step), once each, end to end at the smallest shape that reaches it: 20 013 rows, k = 100 -- the schedule is
the dense bootstrap, three whole rounds of 4 096 rows and a last round of 3 629 = 14 x 256 + 45 = 28 x 128 + 45 rows, so the persistent
kernel of a case and its ragged tail both run.  d = 64 is the one-K-step path of generation 7, d = 128 its two-K-step path, d = 192 the
shortest continuous ring.

Adjudicated as tests/test_search_widths.py adjudicates its end-to-end cases, against oracle/flatip.py: id sets equal up to float64 ties
at the k-th score (rel_tol 2e-6), scores the exact float32 inner products of the returned ids within 1e-4 * max(1, |exact|), descending.
Rows and queries are 0.3 * standard_normal, unclustered: the certified lists stay far below LIST_MAX = 4 096 (at most 120 keys at the
end, at most 270 behind the bootstrap, from query_prep_kernel's margin restated in numpy), so the 16-bit scan holds and no case ends on
the float32 retry."""
import contextlib

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from oracle import flatip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, K = 20013, 100

_DATA = {}


def data(d):
    """Rows, 300 queries and the oracle's top-k at width d, made once: a case takes the first nq queries"""
    if d not in _DATA:
        rng = np.random.default_rng(ROWS + K + d)
        P = (0.3 * rng.standard_normal((ROWS, d))).astype(np.float32)
        Q = (0.3 * rng.standard_normal((300, d))).astype(np.float32)
        ref = flatip.IndexFlatIP(d); ref.add(P)
        _Dr, Ir = ref.search(Q, K)
        _DATA[d] = (P, Q, Ir)
    return _DATA[d]


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


def _adjudicate(I_gpu, I_ref, P, Q):
    def full(q, disputed):
        sc = torch.from_numpy(P).double() @ torch.from_numpy(Q[q]).double()
        kth = torch.topk(sc, K).values[-1].item()
        return sc[torch.tensor(disputed)].numpy(), kth
    return flatip.topk_sets_equal(I_gpu, I_ref, full, rel_tol=2e-6)


@pytest.mark.parametrize("precision,d,nq,gen7,launch", [
    ("f16_rescore", 64, 300, None, "wide7"),
    ("f16_rescore", 128, 300, None, "wide7"),
    ("f16_rescore", 192, 129, None, "wide7c"),
    ("f16_rescore", 768, 300, None, "wide7c"),
    ("f16_rescore", 768, 300, 0, "tile6"),
    ("f16_rescore", 768, 64, 0, "tile2"),
    ("f32", 768, 300, None, "tile6"),
    ("f32", 768, 64, None, "tile2"),
    ("f16_rescore", 768, 64, None, "stream"),
])
def test_every_launch_branch_of_a_round_matches_the_oracle(precision, d, nq, gen7, launch):
    from openmatch_amd.index import FlatIPIndex
    P, Q, Ir = data(d)
    Q, Ir = Q[:nq], Ir[:nq]
    idx = FlatIPIndex(d, device=DEV, precision=precision)
    idx.add(P[: ROWS // 2]); idx.add(P[ROWS // 2:])
    with switched(N.OPT_SCAN_GEN7, gen7):
        D, I = idx.search(Q, K)
    info = idx.last_search_info
    assert (np.diff(D, axis=1) <= 0).all()
    n_exact, n_tie, n_bad, detail = _adjudicate(I, Ir, P, Q)
    print(f"[{precision}] d={d} nq={nq} OM_OPT_SCAN_GEN7={gen7}: id sets identical for {n_exact}/{nq}, near-tie only {n_tie}, "
          f"wrong {n_bad}; {info}")
    assert n_bad == 0, detail
    # returned scores are the exact f32 inner products of the returned ids
    exact = np.stack([P[I[q]].astype(np.float64) @ Q[q].astype(np.float64) for q in range(nq)])
    assert np.abs(D - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())
    if precision == "f16_rescore":
        assert info["scan"] == "f16+rescore", info                       # no silent f32 retry
    assert info["launch"] == launch, info
