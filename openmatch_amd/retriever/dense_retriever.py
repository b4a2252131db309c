"""Corpus / query encoding loops and exact top-k retrieval with the reference's `Retriever`
surface (src/openmatch/retriever/dense_retriever.py:25-236), re-designed for one process per
MI355X:

* embeddings stay resident on the GPU that produced them (one device->host copy at the end of
  the loop, for the compatibility pickle, instead of one per batch — reference :81);
* the index is `FlatIPIndex` (HIP, no faiss): in a multi-rank job every rank keeps ITS shard,
  queries are all-gathered over RCCL, every shard is searched in parallel and the per-shard
  top-k are merged on the GPU — replacing "rank 0 reads all pickles, faiss shards across GPUs,
  7 ranks wait at a barrier" (:43-58,94-106,166-206);
* file formats are unchanged: `embeddings.{corpus,query}.rank.{r}` = pickle protocol 4 of
  (float32 ndarray [n,dim], list of ids).
"""
import gc
import glob
import logging
import os
import pickle
import re
from contextlib import nullcontext
from typing import Dict

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, IterableDataset
from tqdm import tqdm

from ..arguments import InferenceArguments as EncodingArguments
from ..dataset import DRInferenceCollator
from ..feed import model_batch
from ..index import FlatIPIndex, RowFilter, merge_topk, sharded_topk
from ..modeling import DRModelForInference, DROutput
from ..utils import merge_retrieval_results_by_score, qrel_positives, sample_hard_negatives

logger = logging.getLogger(__name__)


def _rank_of(path):
    m = re.search(r"\.rank\.(\d+)$", path)
    return int(m.group(1)) if m else 1 << 30


def _corpus_partitions(output_dir):
    """Shard files in rank order (the reference takes raw glob order, which is OS dependent)."""
    return sorted(glob.glob(os.path.join(output_dir, "embeddings.corpus.rank.*")), key=lambda p: (_rank_of(p), p))


class Retriever:

    def __init__(self, model: DRModelForInference, corpus_dataset: IterableDataset, args: EncodingArguments):
        logger.info("Initializing retriever")
        self.model = model
        self.corpus_dataset = corpus_dataset
        self.args = args
        self.doc_lookup = []
        self.query_lookup = []
        self.index = None
        self._sharded = False          # True: self.index holds only this rank's rows
        self._shard_offset = 0
        self._resident_docs = None     # (device tensor [n,dim], ids) left by doc_embedding_inference
        self._resident_queries = None

        self.model.to(self.args.device)
        self.model.eval()

    # ------------------------------------------------------------------ encoding
    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.float16) if getattr(self.args, "fp16", False) else nullcontext()

    def _encode_loop(self, dataset, is_query):
        loader = DataLoader(
            dataset,
            batch_size=self.args.per_device_eval_batch_size,
            collate_fn=DRInferenceCollator(),
            num_workers=self.args.dataloader_num_workers,
            pin_memory=self.args.dataloader_pin_memory,
        )
        chunks, ids = [], []
        for batch_ids, batch in tqdm(loader, disable=self.args.local_process_index > 0):
            ids.extend(batch_ids)
            with self._autocast(), torch.no_grad():
                batch = model_batch(batch, self.args.device, self.model)      # 16-bit ids + lengths on the wire (feed.py)
                out: DROutput = self.model(query=batch) if is_query else self.model(passage=batch)
                chunks.append(out.q_reps if is_query else out.p_reps)      # stays in HBM
        if chunks:
            encoded = torch.cat(chunks)
        else:
            encoded = torch.empty(0, 0, device=self.args.device)
        return encoded, ids

    def _dump(self, kind, encoded, ids):
        os.makedirs(self.args.output_dir, exist_ok=True)
        path = os.path.join(self.args.output_dir, "embeddings.{}.rank.{}".format(kind, self.args.process_index))
        with open(path, "wb") as f:
            pickle.dump((encoded.cpu().numpy(), ids), f, protocol=4)

    def doc_embedding_inference(self):
        if self.corpus_dataset is None:
            raise ValueError("No corpus dataset provided")
        encoded, ids = self._encode_loop(self.corpus_dataset, is_query=False)
        self._resident_docs = (encoded, ids)
        self._dump("corpus", encoded, ids)
        if self.args.world_size > 1:
            dist.barrier()

    def query_embedding_inference(self, query_dataset: IterableDataset):
        encoded, ids = self._encode_loop(query_dataset, is_query=True)
        self._resident_queries = (encoded, ids)
        self._dump("query", encoded, ids)
        if self.args.world_size > 1:
            dist.barrier()

    # ------------------------------------------------------------------ index
    def _initialize_faiss_index(self, dim: int):
        """Kept under the reference's name; the index is the HIP FlatIPIndex."""
        self.index = FlatIPIndex(dim, device=self.args.device,
                                 precision=os.environ.get("OPENMATCH_AMD_SEARCH", "f16_rescore"))

    def _move_index_to_gpu(self):
        """No-op: the index is born on the GPU (the reference clones a CPU index into faiss-GPU)."""
        logger.info("Index already resides in HBM")

    def init_index_and_add(self, partition: str = None):
        """Reference semantics (:94-106): load the given partition file, or ALL of them, into one
        complete local index; `doc_lookup[i]` is the id of index row i."""
        logger.info("Initializing the inner-product index from pre-computed document embeddings")
        partitions = [partition] if partition is not None else _corpus_partitions(self.args.output_dir)
        for i, part in enumerate(partitions):
            with open(part, "rb") as f:
                encoded, lookup = pickle.load(f)
            if i == 0:
                self._initialize_faiss_index(encoded.shape[1])
            self.index.add(encoded)
            self.doc_lookup.extend(lookup)
        self._sharded = False

    def _init_sharded_index(self):
        """Multi-rank path: every rank indexes only its own rows (the resident tensor if this process encoded them,
        else a contiguous slice of the partition files in rank order -- counts need not divide evenly, a rank may
        end up with no rows).  Collective."""
        W, r = self.args.world_size, self.args.process_index
        if self._resident_docs is not None:
            encoded, lookup = self._resident_docs
            parts = [(encoded, lookup)] if len(lookup) else []
        else:
            files = _corpus_partitions(self.args.output_dir)
            lo, hi = (len(files) * r) // W, (len(files) * (r + 1)) // W
            parts = []
            for path in files[lo:hi]:
                with open(path, "rb") as f:
                    parts.append(pickle.load(f))
        local_lookup = []
        for encoded, lookup in parts:
            local_lookup.extend(lookup)
        dims = [None] * W
        dist.all_gather_object(dims, (len(local_lookup), int(parts[0][0].shape[1]) if parts else 0))
        dim = max(d for _, d in dims)
        if dim == 0:
            raise ValueError("no document embeddings on any rank")
        self._initialize_faiss_index(dim)              # an empty shard still takes part in the collectives
        for encoded, _ in parts:
            self.index.add(encoded)
        self._shard_offset = int(sum(n for n, _ in dims[:r]))
        gathered = [None] * W if r == 0 else None
        dist.gather_object(local_lookup, gathered, dst=0)
        self.doc_lookup = [x for part in gathered for x in part] if r == 0 else []
        self._sharded = True

    @classmethod
    def build_all(cls, model: DRModelForInference, corpus_dataset: IterableDataset, args: EncodingArguments):
        retriever = cls(model, corpus_dataset, args)
        retriever.doc_embedding_inference()
        if args.world_size > 1:
            retriever._init_sharded_index()
            dist.barrier()
        else:
            retriever.init_index_and_add()
        return retriever

    @classmethod
    def build_embeddings(cls, model: DRModelForInference, corpus_dataset: IterableDataset, args: EncodingArguments):
        retriever = cls(model, corpus_dataset, args)
        retriever.doc_embedding_inference()
        return retriever

    @classmethod
    def from_embeddings(cls, model: DRModelForInference, args: EncodingArguments):
        retriever = cls(model, None, args)
        if args.world_size > 1:
            retriever._init_sharded_index()
            dist.barrier()
        else:
            retriever.init_index_and_add()
        return retriever

    def reset_index(self):
        if self.index:
            self.index.reset()
        self.doc_lookup = []
        self.query_lookup = []

    # ------------------------------------------------------------------ search
    def _load_queries(self):
        """All ranks' query embeddings in rank order + ids (reference :170-177)."""
        encoded, lookup = [], []
        for i in range(self.args.world_size):
            with open(os.path.join(self.args.output_dir, "embeddings.query.rank.{}".format(i)), "rb") as f:
                e, ids = pickle.load(f)
            encoded.append(e)
            lookup.extend(ids)
        return np.concatenate(encoded), lookup

    def _hits_to_dict(self, D, I, topk, drop_padding=False):
        original = np.array(self.doc_lookup)[I]      # I == -1 (fewer than k rows) -> last doc, as in faiss+numpy
        out = {}
        for q in range(D.shape[0]):
            qid = str(self.query_lookup[q])
            # drop_padding (a doc_filter): the padding is no hit -- it would name the last document, kept by the filter or not
            hits = zip(original[q], D[q], I[q])
            drop = drop_padding if isinstance(drop_padding, bool) else bool(drop_padding[q])      # (per query under doc_filters)
            out[qid] = {str(doc): float(score) for doc, score, row in hits if not (drop and row < 0)}
        return out

    def _doc_row_filter(self, doc_filter):
        """`doc_filter` (a collection of doc ids to keep; ids the index does not hold are ignored) -> RowFilter through `doc_lookup`."""
        row_of = {str(doc): row for row, doc in enumerate(self.doc_lookup)}
        rows = sorted({row_of[str(doc)] for doc in doc_filter if str(doc) in row_of})
        return RowFilter(self.index, torch.tensor(rows, dtype=torch.int64))

    def _doc_candidates(self, doc_filters, qids):
        """`doc_filters` ({query id: collection of doc ids}; a {qid: {docid: score}} run works) -> per query of `qids` the ascending rows of
        its documents through `doc_lookup` (doc ids the index does not hold are ignored; an empty collection gives []), or None for a
        query id the mapping does not hold: that query is searched unfiltered."""
        row_of = {str(doc): row for row, doc in enumerate(self.doc_lookup)}
        by_qid = {str(qid): docs for qid, docs in doc_filters.items()}
        return [sorted({row_of[str(doc)] for doc in by_qid[str(qid)] if str(doc) in row_of}) if str(qid) in by_qid else None for qid in qids]

    def _doc_exclusions(self, exclude, qids):
        """`exclude` ({query id: collection of doc ids}; a qrel's {docid: grade} works, every doc of it is excluded) -> per query of `qids`
        the rows of its documents through `doc_lookup` (doc ids the index does not hold are ignored), [] for a query id the mapping does
        not hold: that query excludes nothing."""
        row_of = {str(doc): row for row, doc in enumerate(self.doc_lookup)}
        by_qid = {str(qid): docs for qid, docs in exclude.items()}
        return [sorted({row_of[str(doc)] for doc in by_qid.get(str(qid), ()) if str(doc) in row_of}) for qid in qids]

    def search(self, topk: int = 100, doc_filter=None, doc_filters=None, exclude=None):
        """doc_filter: None, or a collection of doc ids: only those documents are returned (an exact filtered search:
        `FlatIPIndex.search_filtered`).  Where fewer than `topk` of them are in the index a query gets that many hits and no more:
        the search's padding is dropped, not mapped to a document as the unfiltered path's is (`_hits_to_dict`).
        doc_filters: None, or a mapping from query id to a collection of doc ids -- a first-stage run as `load_from_trec` returns it
        works: every query is scored over ITS OWN documents (`FlatIPIndex.search_candidates`: dense re-ranking, no bitmap anywhere).  A
        query id the mapping does not hold is searched unfiltered; one with an empty collection gets no hits; padding is dropped.
        exclude: None, or a mapping from query id to a collection of doc ids that query must NOT return -- its known positives, when
        mining hard negatives: an exact search over every other document (`FlatIPIndex.search_excluding`, at most
        `openmatch_amd.index.EXCLUDE_MAX` documents a query).  Doc ids the index does not hold are ignored, a query id the mapping does not
        hold excludes nothing; padding is dropped."""
        logger.info("Searching")
        if self.index is None:
            raise ValueError("Index is not initialized")
        if doc_filter is not None and doc_filters is not None:
            raise ValueError("give doc_filter (one set of documents for all queries) or doc_filters (one per query), not both")
        if exclude is not None and (doc_filter is not None or doc_filters is not None):
            raise ValueError("give exclude (documents a query must not return) or a doc_filter / doc_filters (documents it may), not both")
        if (doc_filter is not None or doc_filters is not None or exclude is not None) and (self._sharded or self.args.world_size > 1):
            raise NotImplementedError("doc_filter with an index sharded across ranks: the filtered search serves one local index only")
        if self._sharded:
            return self._search_sharded(topk)
        encoded, lookup = self._load_queries()
        self.query_lookup.extend(lookup)
        drop = doc_filter is not None
        if doc_filter is not None:
            D, I = self.index.search_filtered(encoded, topk, self._doc_row_filter(doc_filter))
        elif doc_filters is not None:
            rows = self._doc_candidates(doc_filters, self.query_lookup[:len(encoded)])
            own = np.array([r is not None for r in rows], dtype=bool)
            D = np.full((len(rows), topk), np.finfo(np.float32).min, dtype=np.float32)
            I = np.full((len(rows), topk), -1, dtype=np.int64)
            if own.any():
                lists = [r for r in rows if r is not None]
                cand = np.full((len(lists), max(1, max(len(r) for r in lists))), -1, dtype=np.int64)
                for i, r in enumerate(lists):
                    cand[i, :len(r)] = r
                D[own], I[own] = self.index.search_candidates(encoded[own], topk, cand)
            if not own.all():
                D[~own], I[~own] = self.index.search(encoded[~own], topk)
            drop = own
        elif exclude is not None:
            D, I = self.index.search_excluding(encoded, topk, self._doc_exclusions(exclude, self.query_lookup[:len(encoded)]))
            drop = True
        else:
            D, I = self.index.search(encoded, topk)
        result = self._hits_to_dict(D, I, topk, drop_padding=drop)
        logger.info("End searching with {} queries".format(len(result)))
        return result

    def mine_hard_negatives(self, qrels, depth: int = 200, n_sample: int = 30, seed=None):
        """Hard negatives for the next training round (the reference's "update the negatives" step, scripts/msmarco/build_hn.py): ONE
        search of the encoded queries for `depth` hits that excludes every query's positives (`qrels`: {qid: {docid: grade}}, positive
        above 0, or {qid: collection of positive doc ids}), then `n_sample` of them drawn without replacement by
        `utils.sample_hard_negatives`.  The positives are dropped inside the search, so a query gets a full `depth` of negatives to draw
        from where the reference's run of `depth` hits leaves `depth` minus the positives found.  Returns {qid: (positives, negatives)}."""
        run = self.search(depth, exclude={qid: qrel_positives(judged) for qid, judged in qrels.items()})
        return sample_hard_negatives(run, qrels, n_sample=n_sample, depth=depth, seed=seed)

    def _search_sharded(self, topk):
        """Collective over all ranks: all-gather the queries, search the local shard, then merge BY QUERY RANGE --
        rank r receives every shard's candidates for its own slice of the queries (one all-to-all, (W-1)/W of
        Q x k x 12 bytes per rank over point-to-point xGMI links instead of W-1 full result sets into rank 0),
        merges them with the HIP top-k merge, and only the merged [Q/W, k] blocks travel to rank 0 for the result
        dict.  Returns the dict on rank 0 and {} elsewhere (as `retrieve` does)."""
        W, r, dev = self.args.world_size, self.args.process_index, self.args.device
        if self._resident_queries is not None:
            q_local, ids_local = self._resident_queries
        else:
            with open(os.path.join(self.args.output_dir, "embeddings.query.rank.{}".format(r)), "rb") as f:
                e, ids_local = pickle.load(f)
            q_local = torch.from_numpy(e).to(dev)
        counts = [None] * W
        dist.all_gather_object(counts, (int(q_local.shape[0]), list(ids_local)))
        nmax, dim = max(c[0] for c in counts), self.index.d
        padded = torch.zeros(nmax, dim, dtype=torch.float32, device=dev)
        if q_local.shape[0]:
            padded[:q_local.shape[0]].copy_(q_local)
        gathered = torch.empty(W * nmax, dim, dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(gathered, padded)
        queries = torch.cat([gathered[i * nmax:i * nmax + counts[i][0]] for i in range(W)])
        Q = queries.shape[0]
        Dm, Im, _blk = sharded_topk(self.index, queries, topk, self._shard_offset, merge=merge_topk)
        parts_D = [torch.empty_like(Dm) for _ in range(W)] if r == 0 else None
        parts_I = [torch.empty_like(Im) for _ in range(W)] if r == 0 else None
        dist.gather(Dm.contiguous(), parts_D, dst=0)
        dist.gather(Im.contiguous(), parts_I, dst=0)
        if r != 0:
            return {}
        Dall, Iall = torch.cat(parts_D)[:Q], torch.cat(parts_I)[:Q]
        self.query_lookup.extend(x for c in counts for x in c[1])
        return self._hits_to_dict(Dall.cpu().numpy(), Iall.cpu().numpy(), topk)

    def retrieve(self, query_dataset: IterableDataset, topk: int = 100):
        self.query_embedding_inference(query_dataset)
        del self.model                       # as the reference: the retriever gives the encoder up
        gc.collect()
        torch.cuda.empty_cache()
        results = {}
        if self._sharded:
            results = self.search(topk)      # collective; non-zero ranks get {}
        elif self.args.process_index == 0:
            results = self.search(topk)
        if self.args.world_size > 1:
            dist.barrier()
        return results


class SuccessiveRetriever(Retriever):
    """Out-of-core variant (reference :209-236): one partition resident at a time on rank 0,
    partial results merged by score."""

    @classmethod
    def from_embeddings(cls, model: DRModelForInference, args: EncodingArguments):
        return cls(model, None, args)

    def retrieve(self, query_dataset: IterableDataset, topk: int = 100):
        self.query_embedding_inference(query_dataset)
        del self.model
        gc.collect()
        torch.cuda.empty_cache()
        final_result: Dict[str, Dict[str, float]] = {}
        if self.args.process_index == 0:
            for partition in _corpus_partitions(self.args.output_dir):
                logger.info("Loading partition {}".format(partition))
                self.init_index_and_add(partition)
                cur_result = self.search(topk)
                self.reset_index()
                final_result = merge_retrieval_results_by_score([final_result, cur_result], topk)
        if self.args.world_size > 1:
            dist.barrier()
        return final_result
