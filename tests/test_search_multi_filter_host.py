"""A filter per query and candidate lists, the parts that need no GPU (DESIGN.md 4f "A filter per query"): the symbols of
om_sim_topk_filtered_multi / om_sim_topk_candidates / om_debug_drop_lists_multi, their refusals (each before any launch: the pointers
are fake and never followed), the part table (openmatch_amd.index.multi_filter_route), the candidate tensor's preparation and the
Retriever's doc_filters plumbing over a stub index."""
import contextlib

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from openmatch_amd.index import CANDIDATES_MAX_QUERIES, CANDIDATES_MAX_ROWS, filter_route, multi_filter_route, prepare_candidates

MODES = pytest.mark.parametrize("mode", [N.SEARCH_F32, N.SEARCH_F16_RESCORE, N.SEARCH_F16_ONLY], ids=["f32", "f16_rescore", "f16"])


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


def test_the_new_symbols_exist_and_are_bound():
    lib = N.lib()
    for name in ("om_sim_topk_filtered_multi_workspace_bytes", "om_sim_topk_filtered_multi", "om_sim_topk_candidates_workspace_bytes",
                 "om_sim_topk_candidates", "om_debug_drop_lists_multi"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None
    assert lib.om_abi_version() == 6
    for n, d, k in [(1, 64, 1), (300, 768, 100), (32768, 64, 2048)]:
        for f in (1, 7, n):
            assert lib.om_sim_topk_filtered_multi_workspace_bytes(n, d, k, f) >= lib.om_sim_topk_filtered_workspace_bytes(n, d, k) + 4 * f
        assert 0 < lib.om_sim_topk_candidates_workspace_bytes(n, d, k) <= lib.om_sim_topk_workspace_bytes(n, d, k)
    assert lib.om_sim_topk_filtered_multi_workspace_bytes(0, 64, 10, 1) == 0 and lib.om_sim_topk_filtered_multi_workspace_bytes(3, 64, 10, 0) == 0
    assert lib.om_sim_topk_candidates_workspace_bytes(0, 64, 10) == 0


# ---------------------------------------------------------------------------------------------------------- refusals: the multi entry
def _multi(k=10, d=64, n=5000, nq=3, bits=0x3000, pitch=157, n_filters=2, filter_of=0x4000, n_allowed_min=100, status=0x2000,
           mode=N.SEARCH_F16_RESCORE, ws_bytes=1 << 40):
    fake = N.c_void_p(0x1000)
    return N.lib().om_sim_topk_filtered_multi(mode, fake, nq, fake, fake, fake, n, d, k, 0, N.c_void_p(bits), pitch, n_filters,
                                              N.c_void_p(filter_of), n_allowed_min, fake, fake, N.c_void_p(status), fake, ws_bytes,
                                              N.c_void_p(0))


@MODES
def test_multi_refuses_what_the_single_entry_refuses(mode):
    err = N.lib().om_last_error
    assert _multi(k=2049, mode=mode) == 1 and b"2048" in err()
    assert _multi(d=16384 + 64, mode=mode) == 1 and b"16384" in err()
    assert _multi(d=100, mode=mode) == 1 and b"d must be" in err()
    with switched(N.OPT_SCAN_GEN7, 0):
        assert _multi(mode=mode) == 1 and b"OM_OPT_SCAN_GEN7" in err()
    assert _multi(bits=0, mode=mode) == 1 and b"allow_bits" in err()
    assert _multi(ws_bytes=4096, mode=mode) == 1 and b"workspace" in err()
    for name in (b"om_sim_topk_filtered_multi",):
        assert name in err()


@pytest.mark.parametrize("n_filters", [0, -1])
def test_multi_refuses_no_filters(n_filters):
    assert _multi(n_filters=n_filters) == 1 and b"n_filters" in N.lib().om_last_error()


def test_multi_refuses_a_pitch_below_the_word_count():
    assert _multi(n=5000, pitch=156) == 1 and b"words_pitch" in N.lib().om_last_error()      # (5000 + 31) // 32 = 157
    assert _multi(n=5000, pitch=0) == 1 and b"words_pitch" in N.lib().om_last_error()


def test_multi_refuses_a_null_filter_of_unless_one_bitmap_per_query():
    assert _multi(filter_of=0, nq=3, n_filters=2) == 1 and b"filter_of" in N.lib().om_last_error()
    assert _multi(filter_of=0, nq=3, n_filters=4) == 1 and b"filter_of" in N.lib().om_last_error()


@pytest.mark.parametrize("n_allowed_min", [-1, 5001, 1 << 40])
def test_multi_refuses_a_count_outside_the_shard(n_allowed_min):
    assert _multi(n_allowed_min=n_allowed_min) == 1 and b"n_allowed_min" in N.lib().om_last_error()


def test_workspace_holds_one_count_per_bitmap():
    lib = N.lib()
    enough = lib.om_sim_topk_filtered_multi_workspace_bytes(3, 64, 10, 1000)
    assert _multi(n_filters=1000, ws_bytes=enough - 1) == 1 and b"workspace" in lib.om_last_error()


# ---------------------------------------------------------------------------------------------------------- refusals: candidate lists
def _cands(k=10, d=64, n=5000, nq=3, cand=0x3000, pitch=100, f32=0x1000, f16=0x1000, ws=0x1000, mode=N.SEARCH_F16_RESCORE, ws_bytes=1 << 40):
    fake = N.c_void_p(0x1000)
    return N.lib().om_sim_topk_candidates(mode, fake, nq, N.c_void_p(f32), N.c_void_p(f16), n, d, k, 0, N.c_void_p(cand), pitch, fake, fake,
                                          N.c_void_p(ws), ws_bytes, N.c_void_p(0))


@MODES
def test_candidates_refusals(mode):
    err = N.lib().om_last_error
    assert _cands(k=2049, mode=mode) == 1 and b"2048" in err()
    assert _cands(k=0, mode=mode) == 1 and b"2048" in err()
    assert _cands(d=100, mode=mode) == 1 and b"d must be" in err()
    assert _cands(ws=0x1010, mode=mode) == 1 and b"aligned" in err()
    assert _cands(pitch=0, mode=mode) == 1 and b"cand_pitch" in err()
    assert _cands(cand=0, mode=mode) == 1 and b"cand is null" in err()
    assert _cands(ws_bytes=4096, mode=mode) == 1 and b"workspace" in err()
    assert b"om_sim_topk_candidates" in err()


def test_candidates_refuse_a_null_plane_of_the_kind_the_mode_reads():
    err = N.lib().om_last_error
    assert _cands(mode=N.SEARCH_F16_ONLY, f16=0) == 1 and b"index_f16" in err()
    assert _cands(mode=N.SEARCH_F16_RESCORE, f32=0) == 1 and b"index_f32" in err()
    assert _cands(mode=N.SEARCH_F32, f32=0) == 1 and b"index_f32" in err()
    assert _cands(mode=7) == 1 and b"mode" in err()


def test_drop_hook_refusals():
    fake = N.c_void_p(0x1000)
    lib = N.lib()

    def drop(nq=3, m=16, allow=0x3000, nrows=100, pitch=4, n_filters=2, filter_of=0x4000):
        return lib.om_debug_drop_lists_multi(nq, m, fake, fake, fake, 1, N.c_void_p(allow), nrows, pitch, n_filters, N.c_void_p(filter_of),
                                             fake, fake, fake, fake, 4096, N.c_void_p(0))
    assert drop(allow=0) == 1 and b"allow" in lib.om_last_error()
    assert drop(pitch=3) == 1 and b"words_pitch" in lib.om_last_error()
    assert drop(n_filters=0) == 1 and b"n_filters" in lib.om_last_error()
    assert drop(filter_of=0) == 1 and b"filter_of" in lib.om_last_error()
    assert drop(m=8193) == 1 and b"8192" in lib.om_last_error()
    assert drop() == 1 and b"workspace" in lib.om_last_error()              # every argument fine, 4096 bytes are too few


# ---------------------------------------------------------------------------------------------------------- the part table
N_ROWS = 1 << 20
DENSE = (N_ROWS // 2, 0, N_ROWS - 1)              # (n_allowed, first, last): half the rows, scans at any k below
SPARSE = (1000, 5, N_ROWS - 7)                    # k_eff above a million: gathers
RUN = (5000, 70000, 74999)                        # contiguous: a range
EMPTY = (0, 0, -1)


def test_the_fixture_filters_route_as_named():
    for k in (10, 100):
        assert filter_route("f16_rescore", k, DENSE[1], DENSE[2], DENSE[0]) == "scan"
        assert filter_route("f16_rescore", k, SPARSE[1], SPARSE[2], SPARSE[0]) == "gather"
        assert filter_route("f16_rescore", k, RUN[1], RUN[2], RUN[0]) == "range"
        assert filter_route("f16_rescore", k, EMPTY[1], EMPTY[2], EMPTY[0]) == "empty"


@pytest.mark.parametrize("precision", ["f16_rescore", "f32", "f16"])
@pytest.mark.parametrize("group", [DENSE, SPARSE, RUN, EMPTY], ids=["dense", "sparse", "run", "empty"])
def test_one_filter_for_all_queries_delegates_to_the_single_form(precision, group):
    parts = multi_filter_route(precision, 10, [(64,) + group])
    assert [p["route"] for p in parts] == ["single"] and parts[0]["groups"] == [0]
    # ... but not when a query of the call is unfiltered
    parts = multi_filter_route(precision, 10, [(64,) + DENSE], unfiltered=1, ntotal=N_ROWS)
    assert [p["route"] for p in parts] == ["scan"]


def test_dense_groups_and_unfiltered_queries_form_one_scan_part():
    third = (N_ROWS // 3, 300, N_ROWS - 300)
    parts = multi_filter_route("f16_rescore", 10, [(8,) + DENSE, (8,) + third, (2,) + RUN], unfiltered=5, ntotal=N_ROWS)
    assert len(parts) == 1
    (p,) = parts
    assert p["route"] == "scan" and p["groups"] == [0, 1, 2] and p["unfiltered"] is True
    assert p["n_allowed_min"] == RUN[0]                                   # the sparsest of them sizes the schedule
    assert p["rows"] == (0, N_ROWS)                                       # an unfiltered query: every row
    # only unfiltered queries: the scan part plans for all rows
    (p,) = multi_filter_route("f16_rescore", 10, [], unfiltered=3, ntotal=N_ROWS)
    assert p["route"] == "scan" and p["groups"] == [] and p["n_allowed_min"] == N_ROWS and p["rows"] == (0, N_ROWS)
    with pytest.raises(ValueError, match="ntotal"):
        multi_filter_route("f16_rescore", 10, [(8,) + DENSE], unfiltered=3)


def test_the_row_span_of_a_scan_part():
    a, b = (40000, 70100, 190000), (30000, 100000, 250007)
    (p,) = multi_filter_route("f16_rescore", 10, [(4,) + a, (4,) + b])
    assert p["route"] == "scan" and p["rows"] == (70100 // 256 * 256, 250008) and p["n_allowed_min"] == 30000
    (p,) = multi_filter_route("f16_rescore", 10, [(4,) + a, (4,) + b], unfiltered=1, ntotal=N_ROWS)
    assert p["rows"] == (0, N_ROWS) and p["n_allowed_min"] == 30000


def test_sparse_groups_split_at_the_measured_crossover():
    """lists for at most 8 queries over at most 4096 allowed rows (the issue's byte count said 3 queries; measured at 1 000 rows the
    crossover against cached planes is 8, and at 19 944 rows gathering wins at every count: DESIGN.md 4f)"""
    assert (CANDIDATES_MAX_QUERIES, CANDIDATES_MAX_ROWS) == (8, 4096)
    for nq, want in [(1, "candidates"), (3, "candidates"), (4, "candidates"), (8, "candidates"), (9, "gather"), (64, "gather")]:
        parts = multi_filter_route("f16_rescore", 100, [(8,) + DENSE, (nq,) + SPARSE])
        assert [p["route"] for p in parts] == ["scan", want], (nq, parts)
        assert parts[1]["groups"] == [1]
    for rows, want in [(4096, "candidates"), (4097, "gather"), (20000, "gather")]:
        group = (1, rows, 5, N_ROWS - 7)
        assert filter_route("f16_rescore", 100, group[2], group[3], group[1]) == "gather"
        parts = multi_filter_route("f16_rescore", 100, [(8,) + DENSE, group])
        assert [p["route"] for p in parts] == ["scan", want], (rows, parts)
    # several small sparse groups share ONE candidates part; every larger one gathers on its own; the scan part comes first
    other = (900, 17, N_ROWS - 100)
    parts = multi_filter_route("f16_rescore", 100, [(2,) + SPARSE, (12,) + other, (8,) + DENSE, (8,) + other, (9,) + SPARSE])
    assert [(p["route"], p["groups"]) for p in parts] == [("scan", [2]), ("gather", [1]), ("gather", [4]), ("candidates", [0, 3])]


def test_empty_groups_go_to_candidates():
    for nq in (1, 3, 4, 100):
        parts = multi_filter_route("f32", 10, [(8,) + DENSE, (nq,) + EMPTY])
        assert [(p["route"], p["groups"]) for p in parts] == [("scan", [0]), ("candidates", [1])]


def test_forced_routes_make_one_part():
    groups = [(8,) + DENSE, (2,) + SPARSE, (9,) + SPARSE, (1,) + EMPTY]
    (p,) = multi_filter_route("f16_rescore", 100, groups, route="scan")
    assert p["route"] == "scan" and p["groups"] == [0, 1, 2, 3] and p["n_allowed_min"] == 0
    assert p["rows"] == (0, N_ROWS)                                       # first 0 .. last N_ROWS - 1 of the live groups
    (p,) = multi_filter_route("f16_rescore", 100, groups, route="candidates")
    assert p["route"] == "candidates" and p["groups"] == [0, 1, 2, 3]
    (p,) = multi_filter_route("f16_rescore", 100, [(8,) + SPARSE], route="scan")      # a forced route comes before the delegation
    assert p["route"] == "scan" and p["n_allowed_min"] == SPARSE[0]
    with pytest.raises(ValueError, match="candidate"):
        multi_filter_route("f16_rescore", 100, groups, unfiltered=1, ntotal=N_ROWS, route="candidates")
    with pytest.raises(ValueError, match="route"):
        multi_filter_route("f16_rescore", 100, groups, route="gather")
    assert multi_filter_route("f16_rescore", 100, []) == []


# ---------------------------------------------------------------------------------------------------------- the candidate tensor
def test_candidates_are_sorted_and_repeats_become_holes():
    cand = torch.tensor([[5, 3, 5, -1, 0, 0], [7, 7, 7, 7, 7, 7], [-1, -1, -1, -1, -1, -1], [4, 3, 2, 1, 0, 6]])
    out, bad = prepare_candidates(cand, 8)
    assert out.dtype == torch.int32 and out.shape == cand.shape and int(bad) == 0
    for row, want in zip(out.tolist(), [[0, 3, 5], [7], [], [0, 1, 2, 3, 4, 6]]):
        kept = [v for v in row if v >= 0]
        assert sorted(kept) == want and len(set(kept)) == len(kept)
        assert all(v == -1 for v in row if v < 0) and len(row) == 6
    out1, _ = prepare_candidates(torch.tensor([[3], [-1]], dtype=torch.int32), 8)      # one column: nothing to compare
    assert out1.tolist() == [[3], [-1]]


def test_candidates_against_numpy():
    rng = np.random.default_rng(5)
    cand = rng.integers(-1, 50, size=(40, 64))
    out, bad = prepare_candidates(torch.from_numpy(cand), 50)
    assert int(bad) == 0
    for row, got in zip(cand, out.numpy()):
        assert np.array_equal(np.sort(got[got >= 0]), np.unique(row[row >= 0])) and (got[got < 0] == -1).all()


def test_ids_outside_the_index_are_counted_and_never_kept():
    out, bad = prepare_candidates(torch.tensor([[8, 2, -2, 100000, 2 ** 40, -1]]), 8)
    assert int(bad) == 4
    assert sorted(out[0].tolist()) == [-1, -1, -1, -1, -1, 2]              # 2 ** 40 does not wrap into a row number
    with pytest.raises(ValueError):
        prepare_candidates(torch.tensor([1, 2, 3]), 8)


# ---------------------------------------------------------------------------------------------------------- Retriever plumbing
class _StubIndex:
    """records what Retriever.search hands the index; scores are the negated column position, ids the candidates in their order"""

    def __init__(self):
        self.calls = []

    def search_candidates(self, x, k, cand):
        self.calls.append(("candidates", np.array(x), k, np.array(cand)))
        c = np.asarray(cand)
        I = np.full((len(x), k), -1, dtype=np.int64)
        D = np.full((len(x), k), np.finfo(np.float32).min, dtype=np.float32)
        for q in range(len(x)):
            rows = c[q][c[q] >= 0][:k]
            I[q, :len(rows)] = rows
            D[q, :len(rows)] = -np.arange(len(rows))
        return D, I

    def search(self, x, k):
        self.calls.append(("search", np.array(x), k))
        return np.zeros((len(x), k), dtype=np.float32), np.tile(np.arange(k), (len(x), 1))

    def search_filtered(self, x, k, rf):
        raise AssertionError("doc_filters builds no bitmap")


def stub_retriever(tmp_path, nq=4, ndocs=10, world_size=1):
    import os
    import pickle
    from types import SimpleNamespace as NS
    from openmatch_amd.retriever import Retriever
    r = Retriever.__new__(Retriever)
    r.args = NS(output_dir=str(tmp_path), world_size=world_size, process_index=0, local_process_index=0)
    r.index = _StubIndex()
    r._sharded = False
    r.doc_lookup = [f"d{i}" for i in range(ndocs)]
    r.query_lookup = []
    for rank in range(world_size):
        with open(os.path.join(tmp_path, f"embeddings.query.rank.{rank}"), "wb") as f:
            pickle.dump((np.arange(nq * 4, dtype=np.float32).reshape(nq, 4) + rank, [f"q{i}" for i in range(nq)]), f, protocol=4)
    return r


def test_doc_candidates_maps_doc_ids_to_rows(tmp_path):
    r = stub_retriever(tmp_path)
    run = {"q0": {"d3": 1.5, "d1": 0.2, "not-a-doc": 9.0}, "q1": [], "q3": ("d9", "d9", "d0")}
    assert r._doc_candidates(run, ["q0", "q1", "q2", "q3"]) == [[1, 3], [], None, [0, 9]]
    assert r._doc_candidates({7: [3]}, [7]) == [[]]                       # ids are compared as strings: 3 is no document here
    r.doc_lookup = [3, 4]
    assert r._doc_candidates({7: [4, "3"]}, ["7"]) == [[0, 1]]


def test_retriever_doc_filters_plumbing(tmp_path):
    r = stub_retriever(tmp_path)
    run = {"q0": {"d3": 1.5, "d1": 0.2, "not-a-doc": 9.0}, "q1": [], "q3": ("d9", "d9", "d0")}
    got = r.search(3, doc_filters=run)
    kinds = [c[0] for c in r.index.calls]
    assert sorted(kinds) == ["candidates", "search"]
    cand_call = r.index.calls[kinds.index("candidates")]
    plain_call = r.index.calls[kinds.index("search")]
    assert cand_call[3].tolist() == [[1, 3], [-1, -1], [0, 9]] and cand_call[2] == 3       # padded with -1, unknown doc ignored
    assert cand_call[1][:, 0].tolist() == [0.0, 4.0, 12.0] and plain_call[1][:, 0].tolist() == [8.0]      # q0, q1, q3 | q2
    assert got["q0"] == {"d1": 0.0, "d3": -1.0}                           # padding dropped
    assert got["q1"] == {}                                                # an empty collection: no hits
    assert got["q3"] == {"d0": 0.0, "d9": -1.0}
    assert list(got["q2"]) == ["d0", "d1", "d2"]                          # absent from the mapping: searched unfiltered


def test_retriever_refuses_both_arguments_and_sharded_indexes(tmp_path):
    r = stub_retriever(tmp_path)
    with pytest.raises(ValueError, match="doc_filter"):
        r.search(3, doc_filter=["d1"], doc_filters={"q0": ["d1"]})
    r._sharded = True
    with pytest.raises(NotImplementedError, match="shard"):
        r.search(3, doc_filters={"q0": ["d1"]})
    r._sharded = False
    r.args.world_size = 2
    with pytest.raises(NotImplementedError, match="shard"):
        r.search(3, doc_filters={"q0": ["d1"]})
    assert r.index.calls == []
