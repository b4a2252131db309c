"""Exact search with an exclusion list per query on the GPU (om_sim_topk_excluding through FlatIPIndex.search_device_excluding* /
search_excluding, Retriever.search(exclude=...) and Retriever.mine_hard_negatives; DESIGN.md 4f "Exclusion lists").

Two oracles, and the new entry must return the bits of both in D and I, in all three precisions:
  (a) per query, an unfiltered search of a second index that holds only the rows the query keeps, ids mapped back.  The second index is
      searched with the whole query batch and row q is taken, so both searches plan their kernels for the same batch;
  (b) search_device_filtered_multi with one RowFilter(invert=True) per query: the bitmap route.
Gaussian data throughout: no exact score ties, except in the one test that is about them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLT_MIN = np.float32(-3.4028235e38)
PRECISIONS = ["f16_rescore", "f32", "f16"]
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def data(n, nq, d):
    key = ("data", n, nq, d)
    if key not in _CACHE:
        rng = np.random.default_rng(7 * n + nq + d)
        _CACHE[key] = (rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32))
    return _CACHE[key]


def index_of(n, nq, d, precision):
    from openmatch_amd.index import FlatIPIndex
    key = ("index", n, nq, d, precision)
    if key not in _CACHE:
        idx = FlatIPIndex(d, device=DEV, precision=precision)
        idx.add(data(n, nq, d)[0])
        _CACHE[key] = idx
    return _CACHE[key]


def top_hits(n, nq, d, m):
    """the true top-m rows of every query (float64 on the host), best first: computed once per shape"""
    key = ("top", n, nq, d, m)
    if key not in _CACHE:
        P, Q = data(n, nq, d)
        _CACHE[key] = np.argsort(-(Q.astype(np.float64) @ P.astype(np.float64).T), axis=1, kind="stable")[:, :m]
    return _CACHE[key]


def oracle_kept_rows(precision, P, Q, k, excl, id_offset=0):
    """(a): per query the unfiltered search of an index over the rows it keeps"""
    from openmatch_amd.index import FlatIPIndex
    n = len(P)
    D = torch.empty((len(Q), k), dtype=torch.float32, device=DEV)
    I = torch.empty((len(Q), k), dtype=torch.int64, device=DEV)
    for q, gone in enumerate(excl):
        gone = np.asarray([r for r in gone if 0 <= r < n], np.int64)
        kept = np.setdiff1d(np.arange(n), gone)
        ref = FlatIPIndex(P.shape[1], device=DEV, precision=precision)
        ref.add(P[kept])
        h = ref.search_device_async(dev(Q), k)
        assert h.info()["redone"] == 0
        t = dev(kept)
        D[q] = h.D[q]
        I[q] = torch.where(h.I[q] >= 0, t[h.I[q].clamp(min=0)] + id_offset, h.I[q])
    return D, I


def oracle_bitmaps(idx, Q, k, excl, id_offset=0):
    """(b): one inverted RowFilter per query through the multi-filter search"""
    from openmatch_amd.index import RowFilter
    n = idx.ntotal
    filters = [RowFilter(idx, torch.tensor([r for r in gone if 0 <= r < n], dtype=torch.int64), invert=True) for gone in excl]
    h = idx.search_device_filtered_multi_async(dev(Q), k, filters, id_offset=id_offset)
    info = h.info()
    return h.D, h.I, info


def same(what, D, I, Dw, Iw):
    assert torch.equal(I, Iw), f"{what}: ids differ in {(I != Iw).sum().item()} places, first rows {(I != Iw).any(1).nonzero().reshape(-1)[:4].tolist()}"
    assert torch.equal(D, Dw), (f"{what}: scores differ in {(D != Dw).sum().item()} places, "
                                f"largest difference {(D - Dw).abs().max().item():.3e}")


def against_both(precision, idx, P, Q, k, excl, h, id_offset=0):
    n = len(P)
    In = h.I.cpu().numpy()
    Dn = h.D.cpu().numpy()
    for q, gone in enumerate(excl):
        m = min(k, n - len({r for r in gone if 0 <= r < n}))
        rows = In[q, :m] - id_offset
        assert not set(rows.tolist()) & set(gone), f"query {q} got a row it excludes"
        assert (In[q, m:] == -1).all() and (Dn[q, m:] == FLT_MIN).all() and (In[q, :m] >= 0).all()      # padding, and only there
        assert (np.diff(Dn[q, :m]) <= 0).all()
    Db, Ib, info_b = oracle_bitmaps(idx, Q, k, excl, id_offset)
    same(f"[{precision}] against the bitmap route {info_b['parts']}", h.D, h.I, Db, Ib)
    Da, Ia = oracle_kept_rows(precision, P, Q, k, excl, id_offset)
    same(f"[{precision}] against an index of the kept rows", h.D, h.I, Da, Ia)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("precision", PRECISIONS)
def test_each_querys_own_top_hits_excluded_inside_the_bootstrap(precision):
    n, nq, k, d = 5000, 3, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    plain = idx.search_device_async(dev(Q), k)
    excl = [sorted(r) for r in plain.I[:, :5].tolist()]                   # the index's own five best hits of every query
    h = idx.search_device_excluding_async(dev(Q), k, dev(np.array(excl)))
    info = h.info()
    print(f"[{precision}] {info}")
    assert info["route"] == "exclude" and info["pitch"] == 5 and info["redone"] == 0
    assert not torch.equal(h.I, plain.I)              # the drop changes the answer
    assert torch.equal(h.I[:, :5], plain.I[:, 5:10])
    against_both(precision, idx, P, Q, k, excl, h)


# ---------------------------------------------------------------------------------------------------------------- 2
def ragged_lists(n, nq, d):
    """0 .. 300 ids per query: the query's own best hits first, random rows, some ids at and beyond n; query 4 excludes nothing"""
    rng = np.random.default_rng(21)
    top = top_hits(n, nq, d, 150)
    out = []
    for q in range(nq):
        size = int(rng.integers(1, 301)) if q != 4 else 0
        if q == 9:
            size = 300
        own = top[q, :min(size, int(rng.integers(1, 151)))].tolist()
        beyond = [n, n + 1 + q, 2 ** 31 - 1][:max(0, min(3, size - len(own)))] if q % 3 == 0 else []
        rest = rng.choice(n, size, replace=False).tolist()
        ids = list(dict.fromkeys(own + beyond + rest))[:size]
        out.append(ids)
    assert out[4] == [] and max(len(e) for e in out) == 300 and any(r >= n for e in out for r in e)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_lists_past_the_bootstrap_into_the_scan_rounds(precision):
    n, nq, k, d = 70000, 33, 100, 128
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    excl = ragged_lists(n, nq, d)
    h = idx.search_device_excluding_async(dev(Q), k, excl)                # the ragged form, in any order, ids beyond n included
    info = h.info()
    print(f"[{precision}] {info}")
    assert info["route"] == "exclude" and info["pitch"] == 300
    assert info["rounds"] > 1 and info["kernel"] != "dense"               # past the bootstrap
    assert info["redone"] == 0, info
    plain = idx.search_device_async(dev(Q), k)
    assert torch.equal(h.I[4], plain.I[4]) and torch.equal(h.D[4], plain.D[4])      # the empty list
    against_both(precision, idx, P, Q, k, excl, h)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fewer_rows_than_k_remain(precision):
    n, nq, k, d = 40, 2, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    rng = np.random.default_rng(3)
    excl = [sorted(rng.choice(n, 35, replace=False).tolist()) for _ in range(nq)]
    D, I = idx.search_device_excluding(dev(Q), k, excl)
    assert idx.last_search_info["route"] == "exclude" and idx.last_search_info["redone"] == 0
    assert (I[:, 5:] == -1).all() and (D[:, 5:] == float(FLT_MIN)).all() and (I[:, :5] >= 0).all()
    for q in range(nq):
        assert sorted(I[q, :5].tolist()) == sorted(set(range(n)) - set(excl[q]))
    h = idx.search_device_excluding_async(dev(Q), k, excl)
    against_both(precision, idx, P, Q, k, excl, h)
    # everything excluded: padding alone
    D, I = idx.search_device_excluding(dev(Q), k, [list(range(n))] * nq)
    assert (I == -1).all() and (D == float(FLT_MIN)).all()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("precision", PRECISIONS)
def test_identical_rows_are_redone_on_the_device(precision):
    """20 000 copies of one row: every score ties, the candidate lists fill, and the on-device redo selects by (score, ascending row)
    among the rows the list leaves"""
    from openmatch_amd.index import FlatIPIndex
    n, nq, k, d = 20000, 2, 10, 64
    rng = np.random.default_rng(5)
    row = rng.standard_normal(d).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = FlatIPIndex(d, device=DEV, precision=precision)
    idx.add(np.tile(row, (n, 1)))
    h = idx.search_device_excluding_async(dev(Q), k, [[0, 1, 2, 3, 4, 7]] * nq)
    info = h.info()
    print(f"[{precision}] {info}")
    assert info["redone"] >= 1, info
    want = [5, 6] + list(range(8, 16))
    assert h.I.tolist() == [want] * nq
    plain = idx.search_device_async(dev(Q), k)
    assert plain.I.tolist() == [list(range(10))] * nq
    assert torch.equal(h.D, plain.D)                  # the one score there is, in the bits the unfiltered search returns


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("precision", PRECISIONS)
def test_id_offset_and_two_searches_in_flight(precision):
    n, nq, k, d = 5000, 3, 10, 64
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    best = idx.search_device_async(dev(Q), 12).I.tolist()
    excl, other = [sorted(r[:5]) for r in best], [sorted(r[3:]) for r in best]
    table = dev(np.array(excl, np.int32))             # int32 on the device: taken as prepared, nothing is read back
    offset = (1 << 33) + 17
    h1 = idx.search_device_excluding_async(dev(Q), k, table, id_offset=offset)      # both enqueued before either is waited for
    h2 = idx.search_device_excluding_async(dev(Q), k, other)
    again = idx.search_device_excluding_async(dev(Q), k, table, id_offset=offset)
    i1, i2 = h1.info(), h2.info()
    assert i1["redone"] == 0 and i2["redone"] == 0 and (i1["pitch"], i2["pitch"]) == (5, 9)
    base = idx.search_device_excluding_async(dev(Q), k, excl)
    assert torch.equal(h1.D, base.D) and torch.equal(h1.I, torch.where(base.I >= 0, base.I + offset, base.I))
    assert torch.equal(again.D, h1.D) and torch.equal(again.I, h1.I)
    against_both(precision, idx, P, Q, k, excl, h1, id_offset=offset)
    against_both(precision, idx, P, Q, k, other, h2)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,nq,k,d", [(5000, 3, 10, 64), (70000, 33, 100, 128)], ids=["5000", "70000"])
def test_no_exclusions_is_the_unfiltered_search(precision, n, nq, k, d):
    """pitch = 0 is search_device_async bit for bit; so is a table of padding alone"""
    P, Q = data(n, nq, d)
    idx = index_of(n, nq, d, precision)
    want = idx.search_device_async(dev(Q), k, id_offset=3)
    wi = want.info()
    for excl in (torch.zeros((nq, 0), dtype=torch.int32, device=DEV), [[]] * nq, torch.full((nq, 4), -1, dtype=torch.int64, device=DEV)):
        h = idx.search_device_excluding_async(dev(Q), k, excl, id_offset=3)
        info = h.info()
        assert info["pitch"] == 0 and info["route"] == "exclude"
        assert torch.equal(h.D, want.D) and torch.equal(h.I, want.I)
        assert info["redone"] == 0 and info["rounds"] == wi["rounds"] and info["kernel"] == wi["kernel"] and info["scan"] == wi["scan"]
    # a prepared table that holds padding alone runs the exclusion chain (the schedule of N - 4 rows) and drops nothing
    h = idx.search_device_excluding_async(dev(Q), k, torch.full((nq, 4), -1, dtype=torch.int32, device=DEV), id_offset=3)
    assert h.info()["pitch"] == 4 and h.info()["redone"] == 0 and torch.equal(h.I, want.I)
    if precision != "f32":                            # (f32 scores are the scan's own: another schedule may score a row in another kernel)
        assert torch.equal(h.D, want.D)
    Dn, In = idx.search_excluding(Q, k, np.full((nq, 2), -1))             # the numpy form
    assert np.array_equal(In + 3 * (In >= 0), want.I.cpu().numpy()) and np.array_equal(Dn, want.D.cpu().numpy())


def test_argument_errors():
    n, nq, k, d = 5000, 3, 10, 64
    _, Q = data(n, nq, d)
    idx = index_of(n, nq, d, "f16_rescore")
    with pytest.raises(ValueError, match="2 exclusion lists for 3 queries"):
        idx.search_device_excluding(dev(Q), k, [[1], [2]])
    with pytest.raises(ValueError, match="EXCLUDE_MAX"):
        idx.search_device_excluding(dev(Q), k, [list(range(4097)), [], []])
    with pytest.raises(ValueError, match="EXCLUDE_MAX"):
        idx.search_device_excluding(dev(Q), k, torch.zeros((nq, 4097), dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- 7
class _Rows(torch.utils.data.IterableDataset):
    """What InferenceDataset yields: {"text_id", input_ids, attention_mask} per record."""

    def __init__(self, ids, mask, names):
        self.ids, self.mask, self.names = ids, mask, names

    def __iter__(self):
        for i, n in enumerate(self.names):
            yield {"text_id": n, "input_ids": self.ids[i], "attention_mask": self.mask[i]}


def test_retriever_exclude_and_hard_negative_mining(tmp_path):
    """300 documents and 8 queries through a random-init BERT: the excluded search returns no excluded document and otherwise the
    unfiltered ranking of ALL documents with those removed, re-cut; the mined negatives hold no positive"""
    from types import SimpleNamespace as NS
    from transformers import BertConfig, BertModel
    from openmatch.modeling import DRModelForInference
    from openmatch.retriever import Retriever
    ndocs, nq, k = 300, 8, 20
    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=600, max_position_embeddings=64)
    lm = BertModel(cfg).eval()
    torch.nn.init.normal_(lm.embeddings.word_embeddings.weight, std=1.0)      # the tokens decide the embedding: scores spread, no exact ties
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="first", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    rng = np.random.default_rng(0)
    tokens = lambda rows, length: (torch.from_numpy(rng.integers(1, 600, size=(rows, length))), torch.ones(rows, length, dtype=torch.long))
    docs, queries = [f"d{i}" for i in range(ndocs)], [f"q{i}" for i in range(nq)]
    args = NS(device=DEV, output_dir=str(tmp_path), world_size=1, process_index=0, local_process_index=0, fp16=False,
              per_device_eval_batch_size=128, dataloader_num_workers=0, dataloader_pin_memory=False)
    retriever = Retriever.build_all(model, _Rows(*tokens(ndocs, 32), docs), args)
    full = retriever.retrieve(_Rows(*tokens(nq, 16), queries), topk=ndocs)
    assert all(len(full[q]) == ndocs for q in queries)
    for q in queries:
        scores = list(full[q].values())
        assert len(set(scores)) == ndocs, "the toy corpus has an exact score tie"
    # qrels: the best hit, the 3rd and the 25th of every query but q5 (no entry), a judged non-relevant document and one the corpus lacks
    qrels = {q: {list(full[q])[0]: 1, list(full[q])[2]: 2, list(full[q])[24]: 1, list(full[q])[1]: 0, "not-a-doc": 1} for q in queries if q != "q5"}
    exclude = {q: [doc for doc, grade in judged.items() if grade > 0] for q, judged in qrels.items()}
    retriever.query_lookup = []
    got = retriever.search(k, exclude=exclude)
    for q in queries:
        gone = set(exclude.get(q, ()))
        assert not set(got[q]) & gone
        want = [(doc, score) for doc, score in full[q].items() if doc not in gone][:k]
        assert list(got[q].items()) == want, q
    retriever.query_lookup = []
    mined = retriever.mine_hard_negatives(qrels, depth=50, n_sample=10, seed=3)
    assert set(mined) == set(queries)
    for q in queries:
        positives, negatives = mined[q]
        assert set(positives) == set(exclude.get(q, ()))
        assert len(negatives) == 10 and len(set(negatives)) == 10 and not set(negatives) & set(positives)
        pool = [doc for doc in full[q] if doc not in set(positives)][:50]
        assert set(negatives) <= set(pool)            # a full depth of non-positives to draw from
    retriever.query_lookup = []
    assert retriever.mine_hard_negatives(qrels, depth=50, n_sample=10, seed=3) == mined
    assert os.path.exists(os.path.join(tmp_path, "embeddings.query.rank.0"))
