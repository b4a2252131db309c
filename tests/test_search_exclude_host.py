"""Exact search with a per-query exclusion list, the parts that need no GPU (DESIGN.md 4f "Exclusion lists"): the exclusion table's
preparation (openmatch_amd.index.prepare_exclusions), the schedule (csrc/search_plan.h search_schedule_excluding through
om_debug_search_exclude_schedule) against the filtered schedule's hook, the refusals of om_sim_topk_excluding and of the drop hook
(each before any launch: the pointers are fake and never followed), the Retriever's `exclude` plumbing over a stub index, and
openmatch.utils.sample_hard_negatives on a hand-written run."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from openmatch_amd.index import EXCLUDE_MAX, prepare_exclusions
from openmatch.utils import sample_hard_negatives

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
    for name in ("om_sim_topk_excluding_workspace_bytes", "om_sim_topk_excluding", "om_debug_search_exclude_schedule",
                 "om_debug_drop_lists_excluding"):
        assert name in N.exported_symbols() and getattr(lib, name) is not None
    assert lib.om_abi_version() == 6
    assert EXCLUDE_MAX == 4096
    for n, d, k in [(1, 64, 1), (300, 768, 100), (32768, 64, 2048)]:
        for pitch in (0, 3, 4096):          # one count per query behind the asynchronous workspace, whatever the pitch
            assert lib.om_sim_topk_excluding_workspace_bytes(n, d, k, pitch) >= lib.om_sim_topk_async_workspace_bytes(n, d, k) + 4 * n
    assert lib.om_sim_topk_excluding_workspace_bytes(0, 64, 10, 4) == 0


# ---------------------------------------------------------------------------------------------------------- the exclusion table
def test_rows_are_sorted_deduplicated_and_padded_at_the_end():
    excl = torch.tensor([[5, 3, 5, -1, 0, 0], [7, 7, 7, 7, 7, 7], [-1, -1, -1, -1, -1, -1], [4, 3, 2, 1, 0, 6], [-7, 2, -1, 9, 2, -3]])
    out = prepare_exclusions(excl, 8)
    assert out.dtype == torch.int32 and out.device == excl.device
    assert out.tolist() == [[0, 3, 5, -1, -1, -1], [7, -1, -1, -1, -1, -1], [-1] * 6, [0, 1, 2, 3, 4, 6], [2, 9, -1, -1, -1, -1]]
    # the pitch is the longest CLEANED list
    assert prepare_exclusions(torch.tensor([[4, 4, 4, -1], [1, 0, 1, 0]]), 8).tolist() == [[4, -1], [0, 1]]
    assert prepare_exclusions(torch.tensor([[3], [-1]], dtype=torch.int32), 8).tolist() == [[3], [-1]]


def test_ids_beyond_the_index_stay_and_ids_no_int32_names_go():
    out = prepare_exclusions(torch.tensor([[100000, 2, 8, 2 ** 40, 2 ** 31, 2 ** 31 - 1]]), 8)
    assert out.tolist() == [[2, 8, 100000, 2 ** 31 - 1]]                  # legal: they match no row; 2 ** 40 does not wrap into one
    with pytest.raises(ValueError, match="int32"):
        prepare_exclusions(torch.tensor([[1]]), 2 ** 31)


def test_against_numpy():
    rng = np.random.default_rng(5)
    excl = rng.integers(-3, 50, size=(40, 64))
    out = prepare_exclusions(excl, 50).numpy()                            # a numpy array is taken as the tensor is
    want = [np.unique(row[row >= 0]) for row in excl]
    assert out.shape == (40, max(len(w) for w in want))
    for got, w in zip(out, want):
        assert np.array_equal(got[:len(w)], w) and (got[len(w):] == -1).all()


def test_ragged_sequences():
    out = prepare_exclusions([[9, 1, 1], [], (4,), np.array([7, 3, 5, 3]), torch.tensor([2, -1])], 10)
    assert out.tolist() == [[1, 9, -1], [-1, -1, -1], [4, -1, -1], [3, 5, 7], [2, -1, -1]]
    assert prepare_exclusions([[], []], 10).shape == (2, 0)


def test_an_empty_table():
    for excl in (torch.zeros(3, 0, dtype=torch.int64), torch.full((3, 5), -1), [[], [], []]):
        out = prepare_exclusions(excl, 10)
        assert out.shape == (3, 0) and out.dtype == torch.int32
    assert prepare_exclusions(torch.zeros(0, 4, dtype=torch.int64), 10).shape == (0, 0)
    assert prepare_exclusions([], 10).shape == (0, 0)


def test_more_than_exclude_max_ids_for_one_query_are_refused():
    full = torch.arange(EXCLUDE_MAX + 1).repeat(2, 1)
    with pytest.raises(ValueError, match="EXCLUDE_MAX"):
        prepare_exclusions(full, 10 ** 6)
    assert prepare_exclusions(full[:, :EXCLUDE_MAX], 10 ** 6).shape == (2, EXCLUDE_MAX)
    # repeats do not count: 2 * EXCLUDE_MAX entries that name EXCLUDE_MAX rows
    assert prepare_exclusions(torch.cat([full[:, :EXCLUDE_MAX]] * 2, dim=1), 10 ** 6).shape == (2, EXCLUDE_MAX)


def test_argument_errors():
    with pytest.raises(ValueError, match="excl"):
        prepare_exclusions(torch.tensor([1, 2, 3]), 8)
    with pytest.raises(ValueError, match="excl"):
        prepare_exclusions(torch.tensor([[1.0, 2.0]]), 8)


# ---------------------------------------------------------------------------------------------------------- the schedule
def schedule_excluding(mode, nq, n, k, pitch):
    cap = 1024
    chunks, cnt, boot = (N.c_int64 * cap)(), C.c_int(0), N.c_int64(0)
    N.check(N.lib().om_debug_search_exclude_schedule(mode, nq, n, k, pitch, chunks, cap, C.byref(cnt), C.byref(boot)))
    return int(boot.value), [int(chunks[i]) for i in range(cnt.value)]


def schedule_filtered(mode, nq, n, k, n_allowed):
    cap = 1024
    chunks, cnt, boot = (N.c_int64 * cap)(), C.c_int(0), N.c_int64(0)
    N.check(N.lib().om_debug_search_schedule_filtered(mode, nq, n, k, n_allowed, chunks, cap, C.byref(cnt), C.byref(boot)))
    return int(boot.value), [int(chunks[i]) for i in range(cnt.value)]


def schedule_unfiltered(mode, nq, n, k):
    cap = 1024
    chunks, cnt = (N.c_int64 * cap)(), C.c_int(0)
    N.check(N.lib().om_debug_search_schedule(mode, nq, n, k, chunks, cap, C.byref(cnt)))
    return 1, [int(chunks[i]) for i in range(cnt.value)]


#          (N, k, pitch, nq)
SCHEDULES = [(5000, 10, 5, 3), (70000, 100, 300, 33), (70000, 100, 0, 33), (2000000, 200, 4, 64), (2000000, 1000, 1024, 1024),
             (8800000, 200, 3, 1024), (8800000, 2048, 4096, 1), (20000, 10, 6, 2), (40, 10, 35, 1), (4096, 10, 4096, 4), (3000, 10, 4096, 4),
             (1, 1, 1, 1), (0, 10, 0, 2), (0, 10, 7, 2), (9000, 100, 4096, 200), (4100, 2048, 4096, 64)]


@MODES
@pytest.mark.parametrize("n,k,pitch,nq", SCHEDULES)
def test_the_schedule_is_the_filtered_one_for_n_minus_pitch(mode, n, k, pitch, nq):
    got = schedule_excluding(mode, nq, n, k, pitch)
    assert got == schedule_filtered(mode, nq, n, k, max(n - pitch, 0))
    if pitch == 0:
        assert got == schedule_unfiltered(mode, nq, n, k)
    if n - pitch < 1 and n > 0:                       # everything is scored densely: no rounds
        assert got == ((n + 4095) // 4096, [])


def test_the_schedule_hook_refuses_a_pitch_outside_the_table():
    lib = N.lib()
    chunks, cnt, boot = (N.c_int64 * 4)(), C.c_int(0), N.c_int64(0)
    for pitch in (-1, EXCLUDE_MAX + 1):
        assert lib.om_debug_search_exclude_schedule(N.SEARCH_F32, 4, 70000, 10, pitch, chunks, 4, C.byref(cnt), C.byref(boot)) == 1
        assert b"pitch" in lib.om_last_error()
    assert lib.om_debug_search_exclude_schedule(N.SEARCH_F32, 4, 70000, 2049, 3, chunks, 4, C.byref(cnt), C.byref(boot)) == 1
    assert b"2048" in lib.om_last_error()
    assert lib.om_debug_search_exclude_schedule(N.SEARCH_F32, 4, 70000, 10, 3, chunks, 4, None, C.byref(boot)) == 1


# ---------------------------------------------------------------------------------------------------------- refusals
def _excluding(k=10, d=64, n=5000, nq=3, queries=0x1000, f32=0x1000, f16=0x1000, stats=0x1000, excl=0x3000, pitch=5, out=0x1000, ws=0x1000,
               status=0x2000, mode=N.SEARCH_F16_RESCORE, ws_bytes=1 << 40):
    p = N.c_void_p
    return N.lib().om_sim_topk_excluding(mode, p(queries), nq, p(f32), p(f16), p(stats), n, d, k, 0, p(excl), pitch, p(out), p(out), p(status),
                                         p(ws), ws_bytes, p(0))


@MODES
def test_every_refusal_comes_back_through_the_c_entry(mode):
    """whatever om_sim_topk_filtered refuses, then the entry's own: each by name, before any launch (nothing here could be launched)"""
    err = N.lib().om_last_error
    assert _excluding(k=2049, mode=mode) == 1 and b"2048" in err()
    assert _excluding(k=0, mode=mode) == 1 and b"2048" in err()
    assert _excluding(n=1 << 32, mode=mode) == 1 and b"32 bits" in err()
    assert _excluding(d=100, mode=mode) == 1 and b"d must be" in err()
    assert _excluding(d=16384 + 64, mode=mode) == 1 and b"16384" in err()
    assert _excluding(nq=65536, mode=mode) == 1 and b"65535" in err()
    assert _excluding(queries=0, mode=mode) == 1 and b"null argument" in err()
    assert _excluding(out=0, mode=mode) == 1 and b"null argument" in err()
    assert _excluding(ws=0x1010, mode=mode) == 1 and b"aligned" in err()
    assert _excluding(ws=0, mode=mode) == 1 and b"aligned" in err()
    with switched(N.OPT_SCAN_GEN7, 0):
        assert _excluding(mode=mode) == 1 and b"OM_OPT_SCAN_GEN7" in err()
    assert _excluding(excl=0, mode=mode) == 1 and b"excl is null" in err()
    for pitch in (-1, EXCLUDE_MAX + 1, 1 << 40):
        assert _excluding(pitch=pitch, mode=mode) == 1 and b"pitch" in err() and b"EXCLUDE_MAX" in err()
    assert _excluding(ws_bytes=4096, mode=mode) == 1 and b"om_sim_topk_excluding_workspace_bytes" in err()
    assert _excluding(pitch=0, excl=0, ws_bytes=4096, mode=mode) == 1 and b"workspace" in err()      # pitch 0 needs no table, but a workspace
    enough = N.lib().om_sim_topk_excluding_workspace_bytes(3, 64, 10, 5)
    assert _excluding(ws_bytes=enough - 1, mode=mode) == 1 and b"workspace" in err()
    assert b"om_sim_topk_excluding: " in err()


def test_refuses_a_null_plane_of_the_kind_the_mode_reads():
    err = N.lib().om_last_error
    assert _excluding(mode=N.SEARCH_F32, f32=0) == 1 and b"index_f32" in err()
    assert _excluding(mode=N.SEARCH_F16_RESCORE, f32=0) == 1 and b"index_f32" in err()
    assert _excluding(mode=N.SEARCH_F16_RESCORE, f16=0) == 1 and b"index_f16" in err()
    assert _excluding(mode=N.SEARCH_F16_RESCORE, stats=0) == 1 and b"stats" in err()
    assert _excluding(mode=N.SEARCH_F16_ONLY, f16=0) == 1 and b"index_f16" in err()
    assert _excluding(mode=N.SEARCH_F16_ONLY, stats=0) == 1 and b"stats" in err()


def test_no_queries_is_no_work():
    assert _excluding(nq=0, k=99999, excl=0) == 0


def test_drop_hook_refusals():
    fake = N.c_void_p(0x1000)
    lib = N.lib()

    def drop(nq=3, m=16, excl=0x3000, pitch=4, nrows=100, ws=0x1000):
        return lib.om_debug_drop_lists_excluding(nq, m, fake, fake, fake, 1, N.c_void_p(excl), pitch, nrows, fake, fake, fake, N.c_void_p(ws), 4096,
                                                 N.c_void_p(0))
    assert drop(excl=0) == 1 and b"excl" in lib.om_last_error()
    assert drop(nrows=0) == 1 and b"nrows" in lib.om_last_error()
    assert drop(pitch=0) == 1 and b"pitch" in lib.om_last_error()
    assert drop(pitch=EXCLUDE_MAX + 1) == 1 and b"pitch" in lib.om_last_error()
    assert drop(m=8193) == 1 and b"8192" in lib.om_last_error()
    assert drop(nq=0) == 1 and b"queries" in lib.om_last_error()
    assert drop(ws=0x1010) == 1 and b"aligned" in lib.om_last_error()
    assert drop() == 1 and b"workspace" in lib.om_last_error()              # every argument fine, 4096 bytes are too few


# ---------------------------------------------------------------------------------------------------------- Retriever plumbing
class _StubIndex:
    """records what Retriever.search hands the index; the hits are the rows 0, 1, ... a query does not exclude, scores descending"""

    def __init__(self, nrows):
        self.calls, self.nrows = [], nrows

    def search_excluding(self, x, k, excl):
        self.calls.append(("excluding", np.array(x), k, [list(r) for r in excl]))
        I = np.full((len(x), k), -1, dtype=np.int64)
        D = np.full((len(x), k), np.finfo(np.float32).min, dtype=np.float32)
        for q in range(len(x)):
            rows = [r for r in range(self.nrows) if r not in set(excl[q])][:k]
            I[q, :len(rows)] = rows
            D[q, :len(rows)] = -np.arange(len(rows))
        return D, I

    def search(self, x, k):
        raise AssertionError("an excluded search is one call of search_excluding")

    search_filtered = search_candidates = search


def stub_retriever(tmp_path, nq=4, ndocs=10, world_size=1):
    import os
    import pickle
    from types import SimpleNamespace as NS
    from openmatch_amd.retriever import Retriever
    r = Retriever.__new__(Retriever)
    r.args = NS(output_dir=str(tmp_path), world_size=world_size, process_index=0, local_process_index=0)
    r.index = _StubIndex(ndocs)
    r._sharded = False
    r.doc_lookup = [f"d{i}" for i in range(ndocs)]
    r.query_lookup = []
    for rank in range(world_size):
        with open(os.path.join(tmp_path, f"embeddings.query.rank.{rank}"), "wb") as f:
            pickle.dump((np.arange(nq * 4, dtype=np.float32).reshape(nq, 4) + rank, [f"q{i}" for i in range(nq)]), f, protocol=4)
    return r


def test_doc_exclusions_map_doc_ids_to_rows(tmp_path):
    r = stub_retriever(tmp_path)
    exclude = {"q0": {"d3": 1, "d1": 0, "not-a-doc": 2}, "q1": [], "q3": ("d9", "d9", "d0")}
    assert r._doc_exclusions(exclude, ["q0", "q1", "q2", "q3"]) == [[1, 3], [], [], [0, 9]]      # q2: absent, excludes nothing
    r.doc_lookup = [3, 4]
    assert r._doc_exclusions({7: [4, "3"]}, ["7"]) == [[0, 1]]            # ids are compared as strings


def test_retriever_exclude_plumbing(tmp_path):
    r = stub_retriever(tmp_path, ndocs=5)
    got = r.search(4, exclude={"q0": ["d0", "d2", "not-a-doc"], "q3": ["d0", "d1", "d2", "d3"]})
    (call,) = r.index.calls
    assert call[0] == "excluding" and call[2] == 4 and call[3] == [[0, 2], [], [], [0, 1, 2, 3]]
    assert call[1][:, 0].tolist() == [0.0, 4.0, 8.0, 12.0]                # every query, in order, in ONE call
    assert list(got["q0"]) == ["d1", "d3", "d4"]                          # padding dropped, not mapped to a document
    assert list(got["q1"]) == list(got["q2"]) == ["d0", "d1", "d2", "d3"]
    assert got["q3"] == {"d4": 0.0}


def test_retriever_exclude_goes_with_no_filter_and_no_sharded_index(tmp_path):
    r = stub_retriever(tmp_path)
    with pytest.raises(ValueError, match="exclude"):
        r.search(3, doc_filter=["d1"], exclude={"q0": ["d1"]})
    with pytest.raises(ValueError, match="exclude"):
        r.search(3, doc_filters={"q0": ["d1"]}, exclude={"q0": ["d1"]})
    with pytest.raises(ValueError, match="doc_filter"):                   # the existing refusal, as it was
        r.search(3, doc_filter=["d1"], doc_filters={"q0": ["d1"]}, exclude={"q0": ["d1"]})
    r._sharded = True
    with pytest.raises(NotImplementedError, match="shard"):
        r.search(3, exclude={"q0": ["d1"]})
    r._sharded = False
    r.args.world_size = 2
    with pytest.raises(NotImplementedError, match="shard"):
        r.search(3, exclude={"q0": ["d1"]})
    assert r.index.calls == []


def test_mine_hard_negatives_is_one_excluded_search_and_a_sample(tmp_path):
    r = stub_retriever(tmp_path, ndocs=10)
    qrels = {"q0": {"d0": 1, "d1": 0, "d5": 2}, "q2": {"d9": 1}}
    mined = r.mine_hard_negatives(qrels, depth=6, n_sample=3, seed=11)
    (call,) = r.index.calls
    assert call[0] == "excluding" and call[2] == 6 and call[3] == [[0, 5], [], [9], []]      # grade 0 is no positive
    assert set(mined) == {"q0", "q1", "q2", "q3"}
    assert mined["q0"][0] == ["d0", "d5"] and mined["q1"][0] == [] and mined["q2"][0] == ["d9"]
    pool = {"q0": ["d1", "d2", "d3", "d4", "d6", "d7"], "q1": [f"d{i}" for i in range(6)], "q2": [f"d{i}" for i in range(6)]}
    for qid, docs in pool.items():                    # a FULL depth of negatives to draw from, whatever was excluded
        assert len(mined[qid][1]) == 3 and set(mined[qid][1]) <= set(docs)
    r.index.calls.clear()
    r.query_lookup = []
    assert r.mine_hard_negatives(qrels, depth=6, n_sample=3, seed=11) == mined


# ---------------------------------------------------------------------------------------------------------- the sampling
RUN = {"q1": {"a": 9.0, "b": 8.0, "c": 7.0, "d": 6.0, "e": 5.0, "f": 4.0, "g": 3.0, "h": 2.0},
       "q2": {"c": 1.0, "a": 3.0, "b": 2.0},                             # not in rank order: the scores decide
       "q3": {"x": 1.0}}
QREL = {"q1": {"b": 1, "d": 2, "e": 0, "zz": 1}, "q2": ["a"]}            # e is judged but not relevant: a negative like any other


def test_sampling_drops_positives_then_cuts_then_shuffles():
    out = sample_hard_negatives(RUN, QREL, n_sample=3, depth=4, seed=0)
    assert list(out) == ["q1", "q2", "q3"]
    pos, neg = out["q1"]
    assert pos == ["b", "d", "zz"]
    assert len(neg) == 3 and len(set(neg)) == 3 and not set(neg) & set(pos)
    assert set(neg) <= {"a", "c", "e", "f"}                               # the first `depth` NON-positives, not the first `depth` hits
    assert out["q2"] == (["a"], ["b", "c"]) or out["q2"] == (["a"], ["c", "b"])      # fewer than n_sample candidates: all of them
    assert out["q3"] == ([], ["x"])                                       # no qrel entry: no positives


def test_sampling_is_fixed_by_the_seed_and_varies_without_one():
    a = sample_hard_negatives(RUN, QREL, n_sample=3, depth=6, seed=123)
    assert a == sample_hard_negatives(RUN, QREL, n_sample=3, depth=6, seed=123)
    seen = {tuple(sample_hard_negatives(RUN, QREL, n_sample=3, depth=6, seed=s)["q1"][1]) for s in range(40)}
    assert len(seen) > 1                              # 120 ordered draws of 3 from 6: forty seeds do not all agree
    every = sample_hard_negatives(RUN, QREL, n_sample=30, depth=200, seed=1)
    assert sorted(every["q1"][1]) == ["a", "c", "e", "f", "g", "h"]       # the defaults of the reference's script: everything kept


def test_sampling_matches_the_reference_procedure():
    """positives removed, the first `depth` kept, random.shuffle, the first `n_sample` -- with the generator's state carried from query to query"""
    import random
    rng = random.Random(7)
    want = {}
    for qid, pos in (("q1", {"b", "d", "zz"}), ("q2", {"a"}), ("q3", set())):
        negatives = [doc for doc, _ in sorted(RUN[qid].items(), key=lambda kv: -kv[1]) if doc not in pos][:5]
        rng.shuffle(negatives)
        want[qid] = negatives[:2]
    got = sample_hard_negatives(RUN, QREL, n_sample=2, depth=5, seed=7)
    assert {qid: neg for qid, (_pos, neg) in got.items()} == want
