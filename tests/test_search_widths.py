"""The register-resident stream scan beyond d = 768 (csrc/search_scan.hip sim_stream_reg_kernel<.., 16> for 832 <= d <= 1024,
sim_stream_reg_kernel<.., 32, 16> for 1088 <= d <= 2048).

Kernel level, through om_debug_sim_stream: index rows and queries are integers in [-4, 4] stored as float16, so every product is an
integer, |score| <= 16 * 2048 = 32 768 < 2^24, and the float32 accumulation of the matrix core is exact in ANY order: the expected
survivor lists are those of an int64 contraction and the tolerance is zero -- derived, not measured.  896 rows = 7 tiles on 2 workgroups
(4 and 3 tiles each): the ten-slot ring wraps inside and across tiles, a pending append crosses a tile boundary, the last one retires at
the end of the launch.

End to end: FlatIPIndex(precision="f16_rescore") against oracle/flatip.py exactly as test_gpu_parity.py::test_flat_ip_search_matches_oracle
adjudicates it, at widths whose filtered rounds run the new instantiations (4 096 rows dense-scored, 124 whole tiles, a 45-row tail)."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from oracle import flatip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SORT_CAP = 8192
NROWS, GRID, ROW_BASE = 896, 2, 2 ** 31 + 5


def plan(nq, d):
    out = (C.c_int * 4)()
    N.check(N.lib().om_debug_scan_plan(1, nq, d, out))
    return tuple(out)


def orderable_f32(u):
    """csrc/common.h orderable_f32: the float32 whose order-preserving 32-bit code is u"""
    u = u.astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


_CASE = {}


def stream_case(d):
    """Rows, 128 queries and their exact scores at width d, made once: every batch size takes the first nq queries"""
    if d not in _CASE:
        rng = np.random.default_rng(d)
        R = rng.integers(-4, 5, size=(NROWS, d))
        Q = rng.integers(-4, 5, size=(128, d))
        S = Q @ R.T                                         # int64: exact
        assert np.abs(S).max() < 2 ** 24
        _CASE[d] = (R, Q, S)
    return _CASE[d]


def run_stream(R, Q, thr, nq, d):
    rows = torch.from_numpy(R.astype(np.float16)).to(DEV)
    qpad = np.zeros(((nq + 255) // 256 * 256, d), np.float16)          # query_prep_kernel: whole 256-query tiles, zero rows beyond nq
    qpad[:nq] = Q[:nq]
    queries = torch.from_numpy(qpad).to(DEV)
    t = np.full(128, np.inf, np.float32)
    t[:nq] = thr
    t = torch.from_numpy(t).to(DEV)
    keys = torch.zeros(nq, SORT_CAP, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(nq, dtype=torch.int32, device=DEV)
    rc = N.lib().om_debug_sim_stream(N.ptr(rows), NROWS, ROW_BASE, N.ptr(queries), nq, d, N.ptr(t), N.ptr(keys), N.ptr(cnt), GRID,
                                     N.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, keys.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32)


CASES = [(d, nq) for d in (768, 832, 1024) for nq in (1, 32, 33, 64, 65, 128)] + \
        [(d, nq) for d in (1088, 2048) for nq in (1, 16, 17, 32, 33, 64)]


@pytest.mark.parametrize("d,nq", CASES)
def test_stream_kernel_lists_are_exactly_the_float64_survivors(d, nq):
    R, Q, S = stream_case(d)
    S = S[:nq].astype(np.float64)
    # a half-integer per query that about 3 % of the rows reach; query 0 keeps every row (896 < SORT_CAP), one query keeps none
    srt = np.sort(S, axis=1)
    thr = srt[:, NROWS - 27] - 0.5
    thr[0] = -np.inf
    if nq > 1:
        thr[nq // 2] = np.inf
    family, qblock, nb, nkmax = plan(nq, d)
    assert family == (N.SCAN_FAMILY["stream16"] if d > 1024 else N.SCAN_FAMILY["stream32"])
    rc, keys, cnt = run_stream(R, Q, thr.astype(np.float32), nq, d)
    assert rc == 0, N.lib().om_last_error()
    for q in range(nq):
        want_rows = np.nonzero(S[q] >= thr[q])[0]
        assert int(cnt[q]) == len(want_rows), (q, int(cnt[q]), len(want_rows))
        got = keys[q, :cnt[q]]
        ids = (~got).astype(np.uint32).astype(np.int64)                # low word = ~id
        assert len(set(ids.tolist())) == len(ids), (q, "an id appears twice")
        assert set(ids.tolist()) == set((ROW_BASE + want_rows).tolist()), q            # row_base = 2^31 + 5 survives the packing
        score = orderable_f32(got >> np.uint64(32))
        assert np.array_equal(score.view(np.uint32), S[q, ids - ROW_BASE].astype(np.float32).view(np.uint32)), q
    assert int(cnt[0]) == NROWS
    if nq > 1:
        assert int(cnt[nq // 2]) == 0


@pytest.mark.parametrize("d,nq,why", [(2048, 65, "more than 64 queries at a 16-query width"), (192, 1, "fewer than four K steps")])
def test_stream_hook_refuses_what_the_plan_sends_elsewhere(d, nq, why):
    assert plan(nq, d)[0] == N.SCAN_FAMILY["generic"]
    rng = np.random.default_rng(1)
    R = rng.integers(-4, 5, size=(NROWS, d))
    Q = rng.integers(-4, 5, size=(nq, d))
    rc, keys, cnt = run_stream(R, Q, np.zeros(nq, np.float32), nq, d)
    assert rc == 1
    assert b"no stream kernel" in N.lib().om_last_error()
    assert not cnt.any() and not keys.any()                              # nothing was launched


# ------------------------------------------------------------------------------- end to end
def _adjudicate(I_gpu, I_ref, P, Q, k):
    def full(q, disputed):
        sc = torch.from_numpy(P).double() @ torch.from_numpy(Q[q]).double()
        kth = torch.topk(sc, min(k, sc.numel())).values[-1].item()
        return sc[torch.tensor(disputed)].numpy(), kth
    return flatip.topk_sets_equal(I_gpu, I_ref, full, rel_tol=2e-6)


@pytest.mark.parametrize("d,nq,k", [(1024, 1, 10), (1024, 128, 1000), (896, 33, 100), (2048, 16, 100), (2048, 64, 1000), (1536, 17, 10)])
def test_flat_ip_search_matches_oracle_at_wide_rows(d, nq, k):
    """Lists of these cases (longest per case, `max_list`): 35 ... 2 473 keys, all under LIST_MAX = 4 096, so every one stays on the
    16-bit scan.  (2048, 64, 1000) is the tight one: with the margin's accumulation term at 3 d 2^-24 its list held 4 225 keys and the
    search ended on the float32 scan; bounded by depth (query_prep_kernel, tests/test_search_margin.py) it holds 2 473."""
    from openmatch_amd.index import FlatIPIndex
    n = 20013
    rng = np.random.default_rng(n + k)
    mean = rng.standard_normal(d).astype(np.float32)
    P = (mean + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    Q = (mean + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    idx = FlatIPIndex(d, device=DEV, precision="f16_rescore")
    idx.add(P[: n // 2]); idx.add(P[n // 2:])
    D, I = idx.search(Q, k)
    info = idx.last_search_info
    ref = flatip.IndexFlatIP(d); ref.add(P)
    Dr, Ir = ref.search(Q, k)
    assert (np.diff(D, axis=1) <= 0).all()
    n_exact, n_tie, n_bad, detail = _adjudicate(I, Ir, P, Q, k)
    print(f"d={d} nq={nq} k={k}: id sets identical for {n_exact}/{nq}, near-tie only {n_tie}, wrong {n_bad}; {info}")
    assert n_bad == 0, detail
    # returned scores are the exact f32 inner products of the returned ids
    exact = np.stack([P[I[q]].astype(np.float64) @ Q[q].astype(np.float64) for q in range(nq)])
    assert np.abs(D - exact).max() < 1e-4 * max(1.0, np.abs(exact).max())
    assert info["scan"] == "f16+rescore", info                           # no silent f32 retry
    assert info["kernel"] == N.SCAN_FAMILY_NAME[plan(nq, d)[0]] == ("stream16" if d > 1024 else "stream32"), info


def test_flat_ip_search_with_heavily_duplicated_rows_at_d1024():
    """test_gpu_parity.py::test_flat_ip_search_with_heavily_duplicated_rows at d = 1024, scaled to 40 vectors x 500 copies: every score
    level is a 500-way exact tie, and the result must stay exact with the sixteen-K-step instantiation under it.  (At this scale the lists
    stay short -- 1 133 keys -- and the fast schedule finishes.)"""
    from openmatch_amd.index import FlatIPIndex
    nq = 4
    rng = np.random.default_rng(11 + nq)
    d, groups, copies, k = 1024, 40, 500, 1000
    base = rng.standard_normal((groups, d)).astype(np.float32)
    P = np.repeat(base, copies, axis=0)[rng.permutation(groups * copies)]
    Q = (base[rng.integers(0, groups, nq)] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    idx = FlatIPIndex(d, device=DEV, precision="f16_rescore")
    idx.add(P)
    D, I = idx.search(Q, k)
    info = idx.last_search_info                                          # (a margin too wide for the ties ends on the float32 scan's tile)
    assert info["kernel"] == ("stream32" if info["scan"] == "f16+rescore" else "generic"), info
    ref = flatip.IndexFlatIP(d); ref.add(P)
    Dr, Ir = ref.search(Q, k)
    assert (np.diff(D, axis=1) <= 0).all()
    assert np.abs(D - Dr).max() <= 1e-4 * np.abs(Dr).max(), np.abs(D - Dr).max()
    n_exact, n_tie, n_bad, detail = _adjudicate(I, Ir, P, Q, k)
    print(f"[duplicated rows, d={d}] id sets identical for {n_exact}/{nq}, tie-only {n_tie}, wrong {n_bad}; {idx.last_search_info}")
    assert n_bad == 0, detail
    assert all(len(set(row.tolist())) == k for row in I)                 # no id returned twice
