"""`FlatIPIndex`: an exact inner-product index resident in HBM, with the `faiss.IndexFlatIP`
methods the reference uses (`add`, `search`, `reset`, `ntotal`;
src/openmatch/retriever/dense_retriever.py:38-41,105,135,180) and no faiss underneath.

Rows stay on the GPU that encoded them (f32, plus an IEEE-f16 shadow copy for the MFMA candidate
scan; with precision="f16" the float16 rows alone, 2 bytes per element instead of 6); `search` runs `om_sim_topk` on the local shard and, when the process group has more than
one rank, all-gathers the queries, searches every shard in parallel and merges the per-shard
top-k with `om_topk_merge` — the reference's "rank 0 loads every pickle and calls faiss" step
(:94-106,166-192) without the filesystem round trip and with all GPUs busy.
"""
import numpy as np
import torch

from . import native as N

_GROW = 1.5


class SearchHandle:
    """A search in flight (`FlatIPIndex.search_device_async`).  `D` [Q,k] f32 and `I` [Q,k] int64 are device tensors, valid in the order
    of the stream the search was enqueued on; the handle keeps the workspace, the status words and the query copy of every chunk of
    at most 32 768 queries alive."""

    def __init__(self, D, I, queries, chunks, device, extra=None):
        self.D, self.I = D, I
        self._queries, self._chunks, self._device = queries, chunks, device
        self._extra = extra                # a filtered search: {"route", "n_allowed"} (and whatever else has to stay alive)

    def info(self):
        """Synchronises the device, then the `last_search_info` keys (of the last chunk; `max_list` / `margin_too_wide` over all chunks)
        plus `redone`: queries the on-device redo recomputed.  `overflow_fallbacks` is always 0: no batch is ever started over.
        A filtered search adds `route` and `n_allowed`."""
        torch.cuda.synchronize(self._device)
        st = [s.cpu().tolist() for _buf, s in self._chunks]
        extra = {k: v for k, v in (self._extra or {}).items() if not k.startswith("_")}
        if not st:
            return {"scan": "f32", "rounds": 0, "overflow_fallbacks": 0, "max_list": 0, "margin_too_wide": False, "kernel": "dense",
                    "redone": 0, **extra}
        if any(s[6] != 1 for s in st):
            raise N.NativeError("the search has not run (a captured search reports after its first replay)")
        last = st[-1]
        return {"scan": "f16+rescore" if last[0] == 1 else "f32", "rounds": int(last[1]), "overflow_fallbacks": 0,
                "max_list": max(int(s[3]) for s in st), "margin_too_wide": any(s[4] != 0 for s in st),
                "kernel": N.SCAN_FAMILY_NAME[int(last[5])], "redone": sum(int(s[2]) for s in st),
                "margin_too_wide_queries": sum(int(s[4]) for s in st), **extra}


LIST_MAX = 4096            # csrc/search.hip: the longest list a selection may leave (SORT_CAP - DENSE_CHUNK).  This and filter_route's
#                            estimate repeat native code; tests/test_search_filter_host.py holds both to om_debug_search_filter_estimate
ROUTES = ("empty", "range", "scan", "gather")


def filter_route(precision: str, k: int, first: int, last: int, n_allowed: int, route=None):
    """Which way a filtered search goes (pure: no tensor, no device).  `first` / `last`: the lowest and the highest allowed row.
    In order:  'empty' nothing is allowed;  a forced `route` ('scan' | 'gather');  'range' the allowed rows are one contiguous run;
    'scan' the list estimate of k_eff = ceil(k * rows / n_allowed) -- in the precision's own formula (csrc/search_plan.h), over the rows
    the scan would read: `first` rounded down to 256 through `last` -- is at most LIST_MAX;  'gather' anything sparser."""
    if route not in (None, "scan", "gather"):
        raise ValueError("route must be None, 'scan' or 'gather'")
    if n_allowed <= 0:
        return "empty"
    if route is not None:
        return route
    if last - first + 1 == n_allowed:
        return "range"
    rows = last + 1 - first // 256 * 256
    k_eff = (k * rows + n_allowed - 1) // n_allowed
    est = k_eff * 13 // 10 + 64 if precision in ("f16_rescore", "f16") else k_eff + 16
    return "scan" if est <= LIST_MAX else "gather"


class MultiSearchHandle(SearchHandle):
    """A filtered search of several parts in flight (`FlatIPIndex.search_device_filtered_multi_async`): `D` / `I` in the caller's query
    order; the handle keeps every part's handle -- workspace, status words, query slice -- alive."""

    def __init__(self, D, I, queries, parts, device, keep=None):
        super().__init__(D, I, queries, [], device, {"route": "multi"})
        self._parts = parts                # [(route, SearchHandle, queries, n_filters)]
        self._keep = keep

    def info(self):
        """Synchronises the device; the keys of `SearchHandle.info()` taken from the 'scan' part where there is one (else the first part),
        `max_list` / `margin_too_wide` over all parts, `redone` summed over them, and `parts`: [{route, queries, n_filters}]."""
        if not self._parts:
            return {**super().info(), "parts": []}
        infos = [h.info() for _way, h, _nq, _nf in self._parts]
        ways = [way for way, _h, _nq, _nf in self._parts]
        out = dict(infos[ways.index("scan")] if "scan" in ways else infos[0])
        out.pop("n_allowed", None)
        out.update(route="multi", redone=sum(i["redone"] for i in infos), max_list=max(i["max_list"] for i in infos),
                   margin_too_wide=any(i["margin_too_wide"] for i in infos),
                   parts=[{"route": way, "queries": nq, "n_filters": nf} for way, _h, nq, nf in self._parts])
        return out


# A sparse group of at most CANDIDATES_MAX_QUERIES queries whose filter allows at most CANDIDATES_MAX_ROWS rows is scored from candidate
# lists, any other sparse group gathers its rows.  Measured (tools/search_multi_filter_bench.py): at 1 000 allowed rows lists
# are faster than the gather route with CACHED planes up to 8 queries (equal at 8) and than a gather that builds its planes up to 16; at
# 19 944 allowed rows gathering wins at every query count.  4 096 is one block of the candidates chain (not measured between the two).
CANDIDATES_MAX_QUERIES = 8
CANDIDATES_MAX_ROWS = 4096
MULTI_ROUTES = ("single", "scan", "candidates", "gather")


def multi_filter_route(precision: str, k: int, groups, unfiltered: int = 0, ntotal=None, route=None):
    """How a search with a filter per query is split into parts (pure: no tensor, no device).
    groups: [(n_queries, n_allowed, first, last)] per DISTINCT filter in use (`first` / `last`: its lowest and highest allowed row);
    unfiltered: queries under no filter (`ntotal`, the rows of the index, is needed when there are any).
    Returns a list of parts {"route", "groups": indices into `groups`, "unfiltered": bool, "rows": (lo, hi) of a 'scan' part,
    "n_allowed_min": the sparsest bitmap of a 'scan' part}.  In order:
      one distinct filter and every query under it, no forced route: one 'single' part -- `search_device_filtered_async` itself;
      a forced `route` ('scan' | 'candidates'): ONE part of that route for everything (unfiltered queries cannot be 'candidates');
      groups whose own `filter_route` is 'scan' or 'range', and the unfiltered queries: together ONE 'scan' part over the rows from the
        smallest `first` rounded down to 256 through the largest `last` -- all rows when an unfiltered query is present;
      'empty' groups, and 'gather' groups of at most CANDIDATES_MAX_QUERIES queries and CANDIDATES_MAX_ROWS allowed rows: together ONE
        'candidates' part;
      every other 'gather' group: a 'gather' part of its own.
    Where the two bounds come from: candidate lists re-read a row once per query, Q_g * C * d * s bytes; gathering moves about
    3 * C * d * s (read, write, scan once), after which the queries share one MFMA scan.  That byte count put the split at 3 queries;
    the measurement put it at 8 for 1 000 rows and found no query count at which lists win for 20 000."""
    if route not in (None, "scan", "candidates"):
        raise ValueError("route must be None, 'scan' or 'candidates'")
    groups = [tuple(int(v) for v in g) for g in groups]
    if unfiltered and ntotal is None:
        raise ValueError("ntotal is needed to place the unfiltered queries")
    if not groups and not unfiltered:
        return []

    def scan_part(members):
        part = {"route": "scan", "groups": members, "unfiltered": bool(unfiltered), "rows": None, "n_allowed_min": 0}
        live = [groups[g] for g in members if groups[g][1] > 0]
        if unfiltered:
            lo, hi = 0, int(ntotal)
        elif live:
            lo, hi = min(g[2] for g in live) // 256 * 256, max(g[3] for g in live) + 1
        else:
            lo, hi = 0, 0
        part["rows"] = (lo, hi)
        part["n_allowed_min"] = min([groups[g][1] for g in members], default=hi - lo)
        return part

    if route is None and len(groups) == 1 and not unfiltered:
        return [{"route": "single", "groups": [0], "unfiltered": False, "rows": None, "n_allowed_min": groups[0][1]}]
    if route == "scan":
        return [scan_part(list(range(len(groups))))]
    if route == "candidates":
        if unfiltered:
            raise ValueError("route='candidates': a query under no filter has no candidate list")
        return [{"route": "candidates", "groups": list(range(len(groups))), "unfiltered": False, "rows": None, "n_allowed_min": 0}]
    scan, lists, parts = [], [], []
    for g, (nq, n_allowed, first, last) in enumerate(groups):
        way = filter_route(precision, k, first, last, n_allowed)
        if way in ("scan", "range"):
            scan.append(g)
        elif way == "empty" or (nq <= CANDIDATES_MAX_QUERIES and n_allowed <= CANDIDATES_MAX_ROWS):
            lists.append(g)
        else:
            parts.append({"route": "gather", "groups": [g], "unfiltered": False, "rows": None, "n_allowed_min": n_allowed})
    if scan or unfiltered:
        parts.insert(0, scan_part(scan))
    if lists:
        parts.append({"route": "candidates", "groups": lists, "unfiltered": False, "rows": None, "n_allowed_min": 0})
    return parts


def prepare_candidates(cand: torch.Tensor, ntotal: int):
    """The candidate tensor of `om_sim_topk_candidates` from a caller's [Q, C] ids padded with -1 (pure: any device): every row sorted,
    a repeated id kept once and its repeats set to -1 (the kernel would return a repeated row twice), int32.  Returns (cand int32 [Q, C],
    bad: a 0-d tensor counting ids >= ntotal or < -1, not read here)."""
    if cand.dim() != 2:
        raise ValueError("cand must be [Q, C] row ids, padded with -1")
    c = cand.to(torch.int64)
    bad = ((c < -1) | (c >= ntotal)).sum()
    c, _ = torch.sort(torch.where((c < 0) | (c >= ntotal), torch.full_like(c, -1), c), dim=1)      # out of range: a hole, whoever reads `bad`
    if c.shape[1] > 1:
        repeat = c[:, 1:] == c[:, :-1]
        c = torch.cat([c[:, :1], torch.where(repeat, torch.full_like(c[:, 1:], -1), c[:, 1:])], dim=1)
    return c.to(torch.int32).contiguous(), bad


EXCLUDE_MAX = 4096         # include/openmatch_hip.h OM_EXCLUDE_MAX: the ids of one query's exclusion list


def prepare_exclusions(excl, ntotal: int, device=None):
    """The exclusion table of `om_sim_topk_excluding` from a caller's lists: a [Q, E] integer tensor or array padded with -1, or a sequence
    of per-query id sequences (ragged; a Python loop over the queries pads them, the tensor form has none).  Returns int32 [Q, pitch] on
    `device` (default: where the ids are): every row ascending, a repeated id kept once, negatives and the padding moved to the end as
    -1, `pitch` the longest cleaned list (0: nothing is excluded).  An id at or beyond `ntotal` is legal and matches no row; one at or
    beyond 2^31 cannot be named by the int32 table and is dropped, which is the same thing.  More than EXCLUDE_MAX ids for one query
    raise ValueError (a `RowFilter(..., invert=True)` serves longer lists).  Torch ops only; reading `pitch` back is the one
    synchronisation on a device tensor."""
    if int(ntotal) >= 2 ** 31:
        raise ValueError("exclusion lists name rows as int32: the index holds 2^31 rows or more")
    if isinstance(excl, np.ndarray):
        excl = torch.from_numpy(excl)
    elif not isinstance(excl, torch.Tensor):
        rows = [[int(v) for v in (r.tolist() if hasattr(r, "tolist") else r)] for r in excl]
        width = max([len(r) for r in rows], default=0)
        excl = torch.tensor([r + [-1] * (width - len(r)) for r in rows], dtype=torch.int64).reshape(len(rows), width)
    if excl.dim() != 2 or excl.dtype.is_floating_point or excl.dtype == torch.bool:
        raise ValueError("excl must be [Q, E] integer row ids padded with -1, or a sequence of per-query id sequences")
    c = excl.to(torch.int64)
    if device is not None:
        c = c.to(device)
    big = 2 ** 31                                      # sorts behind every id an int32 can name
    c, _ = torch.sort(torch.where((c < 0) | (c >= big), torch.full_like(c, big), c), dim=1)
    if c.shape[1] > 1:                                 # a repeat becomes padding, and a second sort moves it to the end
        repeat = c[:, 1:] == c[:, :-1]
        c, _ = torch.sort(torch.cat([c[:, :1], torch.where(repeat, torch.full_like(c[:, 1:], big), c[:, 1:])], dim=1), dim=1)
    pitch = int((c < big).sum(1).max().item()) if c.numel() else 0
    if pitch > EXCLUDE_MAX:
        raise ValueError(f"{pitch} ids excluded for one query: at most EXCLUDE_MAX = {EXCLUDE_MAX} (RowFilter(..., invert=True) serves longer lists)")
    c = c[:, :pitch]
    return torch.where(c >= big, torch.full_like(c, -1), c).to(torch.int32).contiguous()


def _as_queries(x):
    """What the faiss-style methods take: a numpy array becomes a float32 CPU tensor, a tensor stays as it is."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) else x


def _no_hits(D, I):
    """The result of a search that can return no row, padded as faiss pads."""
    D.fill_(torch.finfo(torch.float32).min)
    I.fill_(-1)


class RowFilter:
    """The rows of one index a filtered search may return: a bitmap over [0, ntotal) shared by all queries of a call.
    allowed: a bool mask [ntotal], or a tensor / array / sequence of row ids (`invert=True`: the ids are an exclusion list).
    Construction packs the bitmap on the index's device and reads `n_allowed` and the first and last allowed row back: ONE host
    synchronisation.  A filter names ROW NUMBERS, not contents: it serves any index of `ntotal` rows on its device, and an index that
    was reset and filled again with as many rows is searched over the same row numbers of its new contents.  The planes of the
    'gather' route are cached here on first use, for one index as it then was: an `add` or `reset` of that index since (its
    generation count) or another index makes the next gather search build them anew."""

    def __init__(self, index, allowed, invert: bool = False):
        self.ntotal = int(index.ntotal)
        self.device = index.device
        if isinstance(allowed, np.ndarray):
            allowed = torch.from_numpy(allowed)
        elif not isinstance(allowed, torch.Tensor):
            allowed = torch.as_tensor(list(allowed), dtype=torch.int64)
        allowed = allowed.to(self.device)
        bad = torch.zeros((), dtype=torch.int64, device=self.device)
        if allowed.dtype == torch.bool:
            if allowed.dim() != 1 or allowed.shape[0] != self.ntotal:
                raise ValueError(f"the mask has {tuple(allowed.shape)} entries, the index {self.ntotal} rows")
            mask = ~allowed if invert else allowed
        else:
            ids = allowed.reshape(-1).to(torch.int64)
            mask = torch.zeros(self.ntotal, dtype=torch.bool, device=self.device)
            if ids.numel() and not self.ntotal:
                raise ValueError("row ids for an empty index")
            if ids.numel():
                bad = ((ids < 0) | (ids >= self.ntotal)).sum()          # read back with the counts below
                mask[ids.clamp(0, self.ntotal - 1)] = True
            if invert:
                mask = ~mask
        self.mask = mask
        self.words = self.pack(mask)
        if self.ntotal:
            pos = torch.arange(self.ntotal, device=self.device)
            big = torch.full_like(pos, self.ntotal)
            n, first, last, bad = torch.stack([mask.sum(), torch.where(mask, pos, big).min(), torch.where(mask, pos, -big).max(), bad]).tolist()
            if bad:
                raise ValueError(f"{bad} row id(s) outside [0, {self.ntotal})")
        else:
            n, first, last = 0, 0, -1
        self.n_allowed, self.first, self.last = int(n), int(first), int(last)
        self._gathered = None              # (index it was built from, that index's generation then, ids, sub-index over the allowed rows)

    @staticmethod
    def pack(mask: torch.Tensor) -> torch.Tensor:
        """bool [n] -> int32 words [(n + 31) // 32]: bit r & 31 of word r >> 5 is mask[r] (the uint32 words of om_sim_topk_filtered, in
        torch's int32); the bits of the last word beyond n are 0.  Pure: any device."""
        n = mask.shape[0]
        words = (n + 31) // 32
        m = torch.zeros(words * 32, dtype=torch.int64, device=mask.device)
        m[:n] = mask.to(torch.int64)
        v = (m.view(words, 32) << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(1)
        return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)

    def ids(self):
        """The allowed rows, ascending (int64, on the device)."""
        return self.mask.nonzero().reshape(-1)


class FlatIPIndex:
    def __init__(self, d: int, device=None, precision: str = "f16_rescore"):
        """precision: 'f16_rescore' (f16 MFMA scan with a certified margin + exact f32 re-score;
        same ids as the f32 scan), 'f32' (exact f32 MFMA scan) or 'f16' (alias 'f16_only': the rows are STORED in float16, as
        faiss's IndexScalarQuantizer(QT_fp16) stores them, and searched exactly -- the top-k of <q, widen(row)> with float32 queries, bit
        for bit what an 'f16_rescore' index built from the widened rows returns; no float32 plane is allocated.  A query the certified
        margin cannot serve is recomputed on the device by a radix select over all rows, which is far slower than a scan:
        `last_search_info["margin_too_wide_queries"]` / `SearchHandle.info()` tell when that was paid)."""
        if precision in ("bf16_rescore", "fp16_rescore"):     # accepted aliases
            precision = "f16_rescore"
        if precision == "f16_only":
            precision = "f16"
        if precision not in ("f16_rescore", "f32", "f16"):
            raise ValueError("precision must be 'f16_rescore', 'f32' or 'f16'")
        self.d = int(d)
        self.dpad = (self.d + 63) // 64 * 64      # kernels need d % 64 == 0; zero columns are free
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.precision = precision
        self.ntotal = 0
        self._generation = 0                       # counts `add`s and `reset`s: what a RowFilter was built against
        self._f32 = None
        self._f16 = None
        self._stats = torch.zeros(2, dtype=torch.float32, device=self.device)

    # -- storage ---------------------------------------------------------------------------
    @property
    def capacity(self):
        """Rows the planes hold without growing."""
        return 0 if self._f16 is None else self._f16.shape[0]

    def _reserve(self, n, exact=False):
        cap = self.capacity
        if n <= cap:
            return
        new_cap = n if exact else max(n, int(cap * _GROW), 1024)
        b16 = torch.zeros(new_cap, self.dpad, dtype=torch.float16, device=self.device)
        if self.ntotal:
            b16[:self.ntotal].copy_(self._f16[:self.ntotal])
        self._f16 = b16
        if self.precision == "f16":                # the float16 plane is the index: nothing else to grow
            return
        f32 = torch.zeros(new_cap, self.dpad, dtype=torch.float32, device=self.device)
        if self.ntotal:
            f32[:self.ntotal].copy_(self._f32[:self.ntotal])
        self._f32 = f32

    def reserve(self, n: int):
        """Room for `n` rows in all, in ONE allocation of exactly that size: called before the first `add`, a large index never holds an
        old and a new copy of its planes while it grows (growing on demand peaks at 2.5x the rows stored).  Never shrinks."""
        self._reserve(int(n), exact=True)

    def _add_f16(self, x):
        """`add` of a float16-only index: rows in float32 or float16 (bfloat16 goes through float32) straight into the float16 plane
        (om_index_add_f16), a device-side float16 tensor without a float32 round trip."""
        n = x.shape[0]
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.to(self.device)
        if self.dpad != self.d:                    # the kernel converts whole rows of the plane's width: zero columns behind d
            xp = torch.zeros(n, self.dpad, dtype=x.dtype, device=self.device)
            xp[:, :self.d].copy_(x)
            x = xp
        x = x.contiguous()
        self._reserve(self.ntotal + n)
        stats = self._stats.clone()                # committed only when every stored value is finite
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().om_index_add_f16(N.OM_F32 if x.dtype == torch.float32 else N.OM_F16, N.ptr(x), n, self.dpad,
                                              N.ptr(self._f16[self.ntotal:self.ntotal + n]), N.ptr(stats), N.ptr(bad),
                                              N.stream_ptr(self.device)))
        n_bad = int(bad.item())                    # the one synchronisation of an add
        if n_bad:
            self._f16[self.ntotal:self.ntotal + n].zero_()      # rows beyond ntotal stay what an allocation leaves: zeros
            raise ValueError(f"{n_bad} value(s) of the added rows are not finite in float16 (inf, NaN, or beyond the float16 range "
                             f"of +-65504): a precision='f16' index stores float16 rows; nothing was added")
        self._stats = stats
        self.ntotal += n
        self._generation += 1

    def add(self, x):
        """Append rows (numpy array or tensor, any device) in insertion order.
        precision='f16': float32, float16 or bfloat16 rows; float32 is rounded to nearest even (`torch.Tensor.half()`), float16 is stored bit
        for bit.  The add reads a counter of non-finite stored values back -- ONE host synchronisation per `add` -- and raises
        ValueError, leaving `ntotal` and the stored rows as they were, when a value is inf, NaN or beyond the float16 range."""
        if isinstance(x, np.ndarray):
            keep = self.precision == "f16" and x.dtype == np.float16
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16 if keep else np.float32))
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"expected [n,{self.d}] rows")
        n = x.shape[0]
        if n == 0:
            return
        if self.precision == "f16":
            return self._add_f16(x)
        self._reserve(self.ntotal + n)
        dst = self._f32[self.ntotal:self.ntotal + n]
        dst[:, :self.d].copy_(x.to(device=self.device, dtype=torch.float32), non_blocking=True)
        with torch.cuda.device(self.device):
            N.check(N.lib().om_index_to_f16(N.ptr(dst), n, self.dpad,
                                             N.ptr(self._f16[self.ntotal:self.ntotal + n]),
                                             N.ptr(self._stats), N.stream_ptr(self.device)))
        self.ntotal += n
        self._generation += 1

    def reset(self):
        self.ntotal = 0
        self._generation += 1
        self._f32 = self._f16 = None
        self._stats.zero_()

    # -- search ----------------------------------------------------------------------------
    def _search_args(self, queries, k):
        """What both searches start from: the float32 query panel [Q, dpad] on the index's device, the outputs D [Q,k] f32 and
        I [Q,k] int64, and the native mode."""
        if queries.dim() != 2 or queries.shape[1] != self.d:
            raise ValueError(f"expected [q,{self.d}] queries")
        q = queries.to(device=self.device, dtype=torch.float32)
        if self.dpad != self.d:            # zero-padded to the kernels' K step
            qp = torch.zeros(q.shape[0], self.dpad, dtype=torch.float32, device=self.device)
            qp[:, :self.d].copy_(q)
            q = qp
        q = q.contiguous()
        D = torch.empty(q.shape[0], k, dtype=torch.float32, device=self.device)
        I = torch.empty(q.shape[0], k, dtype=torch.int64, device=self.device)
        return q, D, I, {"f16_rescore": N.SEARCH_F16_RESCORE, "f32": N.SEARCH_F32, "f16": N.SEARCH_F16_ONLY}[self.precision]

    def search_device(self, queries: torch.Tensor, k: int, id_offset: int = 0):
        """Local-shard search on device tensors: returns (D [Q,k] f32, I [Q,k] int64) on the GPU."""
        q, D, I, mode = self._search_args(queries, k)
        nq = q.shape[0]
        lib = N.lib()
        step = 32768                       # the kernel takes <= 65535 queries per call
        with torch.cuda.device(self.device):
            for s in range(0, nq, step):
                n = min(step, nq - s)
                # (the float16-only mode runs the stream-ordered chain behind the synchronous entry too: that chain's workspace)
                nbytes = (lib.om_sim_topk_async_workspace_bytes if mode == N.SEARCH_F16_ONLY else lib.om_sim_topk_workspace_bytes)(n, self.dpad, k)
                _buf, ws = N.Workspace.get(self.device, nbytes, "search")
                N.check(lib.om_sim_topk(mode, N.ptr(q[s:s + n]), n, N.ptr(self._f32), N.ptr(self._f16),
                                        N.ptr(self._stats), self.ntotal, self.dpad, k, int(id_offset),
                                        N.ptr(D[s:s + n]), N.ptr(I[s:s + n]), N.c_void_p(ws), nbytes,
                                        N.stream_ptr(self.device)))
        info = (N.c_int64 * 8)()
        lib.om_sim_topk_info(info)
        self.last_search_info = {"scan": "f16+rescore" if info[0] == 1 else "f32", "rounds": int(info[1]),
                                 "overflow_fallbacks": int(info[2]), "max_list": int(info[3]),
                                 "margin_too_wide": bool(info[4]), "kernel": N.SCAN_FAMILY_NAME[int(info[5])],
                                 "launch": N.SCAN_KERNEL_NAME[int(info[6])]}
        if mode == N.SEARCH_F16_ONLY:      # no float32 retry: the queries the margin could not certify were redone on the device
            self.last_search_info.update(margin_too_wide_queries=int(info[4]), redone=int(info[7]))
        return D, I

    def search_device_async(self, queries: torch.Tensor, k: int, id_offset: int = 0):
        """`search_device` without the host in the loop (`om_sim_topk_async`): only enqueues on the current stream and returns a
        `SearchHandle` whose `.D` / `.I` are valid in the order of that stream.  The handle owns its workspace, its status words and
        its padded query copy, so several searches can be in flight (back to back, on several streams, or captured in a graph: the
        handle then has to outlive the graph).  The index must not be added to or reset while a search is in flight."""
        q, D, I, mode = self._search_args(queries, k)
        return SearchHandle(D, I, q, self._enqueue(q, D, I, mode, k, self._f32, self._f16, self.ntotal, id_offset), self.device)

    def _enqueue_chunks(self, nq, nbytes_of, call, status=True):
        """The loop of every stream-ordered entry: `nq` queries in chunks of at most 32 768 (an entry takes 65 535), on the index's device.
        Per chunk: nbytes_of(n) bytes of 256-aligned workspace, 8 zeroed status words for the entries that report through them, and
        call(rows, n, ws, nbytes, status) -- the native entry over queries `rows` (a slice), its return code checked.  Returns what a
        handle keeps alive: the (workspace, status) pairs, or the workspaces alone."""
        keep = []
        with torch.cuda.device(self.device):
            for s in range(0, nq, 32768):
                n = min(32768, nq - s)
                nbytes = nbytes_of(n)
                buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=self.device)
                ws = N.c_void_p(buf.data_ptr() + (-buf.data_ptr()) % 256)
                st = torch.zeros(8, dtype=torch.int64, device=self.device) if status else None
                N.check(call(slice(s, s + n), n, ws, nbytes, st))
                keep.append((buf, st) if status else buf)
        return keep

    def _waited(self, h):
        """A search in flight, waited for: `last_search_info` from the handle, (D, I) on the GPU."""
        self.last_search_info = h.info()
        return h.D, h.I

    def _planes(self, lo, hi):
        """Rows [lo, hi) of the float32 and the float16 plane (None where the index has no such plane)."""
        return tuple(None if plane is None else plane[lo:hi] for plane in (self._f32, self._f16))

    def _enqueue(self, q, D, I, mode, k, f32, f16, nrows, id_offset, words=None, n_allowed=0):
        """The stream-ordered chain over rows [0, nrows) of the planes `f32` / `f16`, in chunks of at most 32 768 queries: om_sim_topk_async,
        or with `words` (the bitmap over those rows) om_sim_topk_filtered.  Returns the (workspace, status) pairs a handle keeps alive."""
        lib = N.lib()
        entry, nbytes_of, own = ((lib.om_sim_topk_async, lib.om_sim_topk_async_workspace_bytes, ()) if words is None else
                                 (lib.om_sim_topk_filtered, lib.om_sim_topk_filtered_workspace_bytes, (N.ptr(words), int(n_allowed))))

        def call(rows, n, ws, nbytes, status):
            return entry(mode, N.ptr(q[rows]), n, N.ptr(f32), N.ptr(f16), N.ptr(self._stats), nrows, self.dpad, k, int(id_offset), *own,
                         N.ptr(D[rows]), N.ptr(I[rows]), N.ptr(status), ws, nbytes, N.stream_ptr(self.device))
        return self._enqueue_chunks(q.shape[0], lambda n: nbytes_of(n, self.dpad, k), call)

    # -- filtered search ---------------------------------------------------------------------
    def search_device_filtered_async(self, queries: torch.Tensor, k: int, row_filter: "RowFilter", id_offset: int = 0, route=None):
        """The exact top-k over the rows `row_filter` allows, stream-ordered: per query what an index of the same precision holding
        only the allowed rows (in their order) returns, with the ORIGINAL row numbers (+ `id_offset`), (-3.4028235e38, -1) padded when
        fewer than k rows are allowed.  Returns a `SearchHandle`; its `info()` adds `route` (see `filter_route`) and `n_allowed`.
        route: None, or 'scan' / 'gather' to force one (tests, benchmarks: the result is exact either way -- where a forced scan of a
        sparse filter overflows its lists the on-device redo recomputes the queries, `redone` tells how many)."""
        if not isinstance(row_filter, RowFilter):
            raise TypeError("row_filter must be a RowFilter")
        if row_filter.ntotal != self.ntotal or row_filter.device != self.device:
            raise ValueError(f"the filter was built for an index of {row_filter.ntotal} rows on {row_filter.device}, "
                             f"this one holds {self.ntotal} on {self.device}")
        rf = row_filter
        q, D, I, mode = self._search_args(queries, k)
        way = filter_route(self.precision, k, rf.first, rf.last, rf.n_allowed, route)
        extra = {"route": way, "n_allowed": rf.n_allowed, "_filter": rf}
        if way == "empty" or q.shape[0] == 0:
            _no_hits(D, I)
            return SearchHandle(D, I, q, [], self.device, extra)
        if way == "range":                 # a slice of the planes is an index: the unfiltered chain, ids shifted by the slice's first row
            lo, hi = rf.first, rf.last + 1
            chunks = self._enqueue(q, D, I, mode, k, *self._planes(lo, hi), hi - lo, int(id_offset) + lo)
        elif way == "scan":                # the bitmap's word of row lo is whole: lo is a multiple of 256
            lo, hi = rf.first // 256 * 256, rf.last + 1
            chunks = self._enqueue(q, D, I, mode, k, *self._planes(lo, hi), hi - lo, int(id_offset) + lo,
                                   words=rf.words[lo // 32:], n_allowed=rf.n_allowed)
        else:
            ids, sub = self._gathered(rf)
            Is = torch.empty_like(I)       # rows of the gathered planes, mapped back through the id list on the same stream
            chunks = sub._enqueue(q, D, Is, mode, k, sub._f32, sub._f16, sub.ntotal, 0)
            torch.where(Is >= 0, ids[Is.clamp(min=0)] + int(id_offset), Is, out=I)
            extra["_rows"] = Is
        return SearchHandle(D, I, q, chunks, self.device, extra)

    def _gathered(self, rf):
        """The 'gather' route's index over the allowed rows, cached on the filter: `index_select` of the planes (n_allowed * dpad * 2 or 6
        bytes) under THIS index's rounding statistics -- maxima over all rows, so still valid bounds for the certified margin."""
        if rf._gathered is None or rf._gathered[0] is not self or rf._gathered[1] != self._generation:
            ids = rf.ids()
            sub = FlatIPIndex(self.d, device=self.device, precision=self.precision)
            sub._f16 = self._f16.index_select(0, ids)
            sub._f32 = None if self._f32 is None else self._f32.index_select(0, ids)
            sub._stats = self._stats
            sub.ntotal = int(ids.shape[0])
            rf._gathered = (self, self._generation, ids, sub)
        return rf._gathered[2], rf._gathered[3]

    def search_device_filtered(self, queries: torch.Tensor, k: int, row_filter: "RowFilter", id_offset: int = 0, route=None):
        """`search_device_filtered_async`, waited for: (D [Q,k] f32, I [Q,k] int64) on the GPU, and `last_search_info` with `route`,
        `n_allowed` and `redone`."""
        return self._waited(self.search_device_filtered_async(queries, k, row_filter, id_offset=id_offset, route=route))

    def search_filtered(self, x, k: int, row_filter: "RowFilter"):
        """faiss-style, as `search`: numpy in, (D, I) numpy out."""
        D, I = self.search_device_filtered(_as_queries(x), k, row_filter)
        return D.cpu().numpy(), I.cpu().numpy()

    # -- candidate lists: every query scored over its own rows --------------------------------
    def _enqueue_candidates(self, q, D, I, mode, k, cand, id_offset):
        """om_sim_topk_candidates over `cand` (int32 [Q, C] on the device, distinct rows per query, holes -1), in chunks of at most 32 768
        queries.  Returns the workspaces a handle keeps alive."""
        lib = N.lib()
        if cand.dtype != torch.int32 or cand.device != self.device or cand.shape[0] != q.shape[0]:
            raise ValueError("candidates must be int32 [Q, C] on the index's device")
        cand = cand.contiguous()
        if cand.shape[1] == 0 or self.ntotal == 0:
            _no_hits(D, I)
            return [cand]

        def call(rows, n, ws, nbytes, _status):
            return lib.om_sim_topk_candidates(mode, N.ptr(q[rows]), n, N.ptr(self._f32), N.ptr(self._f16), self.ntotal, self.dpad, k,
                                              int(id_offset), N.ptr(cand[rows]), cand.shape[1], N.ptr(D[rows]), N.ptr(I[rows]), ws, nbytes,
                                              N.stream_ptr(self.device))
        return [cand] + self._enqueue_chunks(q.shape[0], lambda n: lib.om_sim_topk_candidates_workspace_bytes(n, self.dpad, k), call, status=False)

    def search_device_candidates_async(self, queries: torch.Tensor, k: int, cand, id_offset: int = 0):
        """The exact top-k of query q over ITS OWN candidate rows `cand[q]` (an int tensor or array [Q, C], padded with -1), stream-ordered:
        scores are the re-score's (in the 16-bit precisions the bits a filtered search returns for those rows), ties to the ascending row,
        ids the row numbers + `id_offset`, (-3.4028235e38, -1) padded when a query has fewer than k candidates.  The cost is Q * C * d,
        whatever `ntotal`.  Repeats within a row are removed on the device (sort, equal neighbours to -1).
        Ids >= ntotal or < -1 raise ValueError: candidates given on the HOST (array, list, CPU tensor) are checked there, without any
        synchronisation; a DEVICE tensor is checked by a count read back once -- the call's only synchronisation -- except while the
        current stream is capturing, where nothing may be read: such ids are then holes, like -1 (the kernel never follows them)."""
        q, D, I, mode = self._search_args(queries, k)
        if isinstance(cand, np.ndarray):
            cand = torch.from_numpy(cand)
        elif not isinstance(cand, torch.Tensor):
            cand = torch.as_tensor(cand, dtype=torch.int64)
        if cand.dim() != 2 or cand.shape[0] != q.shape[0] or cand.dtype.is_floating_point or cand.dtype == torch.bool:
            raise ValueError(f"cand must be [{q.shape[0]}, C] integer row ids, padded with -1")
        if self.ntotal >= 2 ** 31:
            raise ValueError("candidate lists name rows as int32: the index holds 2^31 rows or more")
        on_host = not cand.is_cuda
        c32, bad = prepare_candidates(cand, self.ntotal)      # (where the candidates are: host ids are prepared and checked on the host)
        if on_host or not torch.cuda.is_current_stream_capturing():
            n_bad = int(bad.item())
            if n_bad:
                raise ValueError(f"{n_bad} candidate id(s) outside [-1, {self.ntotal})")
        c32 = c32.to(self.device)
        keep = self._enqueue_candidates(q, D, I, mode, k, c32, id_offset)
        return SearchHandle(D, I, q, [], self.device, {"route": "candidates", "candidates": int(cand.shape[1]), "_keep": keep})

    def search_device_candidates(self, queries: torch.Tensor, k: int, cand, id_offset: int = 0):
        """`search_device_candidates_async`, waited for: (D, I) on the GPU, and `last_search_info`."""
        return self._waited(self.search_device_candidates_async(queries, k, cand, id_offset=id_offset))

    def search_candidates(self, x, k: int, cand):
        """faiss-style, as `search`: numpy in, (D, I) numpy out."""
        D, I = self.search_device_candidates(_as_queries(x), k, cand)
        return D.cpu().numpy(), I.cpu().numpy()

    # -- exclusion lists: every row but a few that differ per query ----------------------------
    def _enqueue_excluding(self, q, D, I, mode, k, table, id_offset):
        """om_sim_topk_excluding over all rows under `table` (int32 [Q, pitch] on the device, as `prepare_exclusions` leaves it), in
        chunks of at most 32 768 queries.  Returns the (workspace, status) pairs a handle keeps alive."""
        lib = N.lib()
        if table.dtype != torch.int32 or table.device != self.device or table.dim() != 2 or table.shape[0] != q.shape[0]:
            raise ValueError("the exclusion table must be int32 [Q, pitch] on the index's device")
        table = table.contiguous()
        pitch = int(table.shape[1])

        def call(rows, n, ws, nbytes, status):
            return lib.om_sim_topk_excluding(mode, N.ptr(q[rows]), n, N.ptr(self._f32), N.ptr(self._f16), N.ptr(self._stats), self.ntotal,
                                             self.dpad, k, int(id_offset), N.ptr(table[rows]) if pitch else None, pitch, N.ptr(D[rows]),
                                             N.ptr(I[rows]), N.ptr(status), ws, nbytes, N.stream_ptr(self.device))
        return self._enqueue_chunks(q.shape[0], lambda n: lib.om_sim_topk_excluding_workspace_bytes(n, self.dpad, k, pitch), call)

    def search_device_excluding_async(self, queries: torch.Tensor, k: int, excl, id_offset: int = 0):
        """The exact top-k of query q over every row but those of ITS OWN exclusion list `excl[q]`, stream-ordered: per query what an index
        of the same precision without those rows returns, with the ORIGINAL row numbers (+ `id_offset`), (-3.4028235e38, -1) padded when
        fewer than k rows remain.  excl: what `prepare_exclusions` takes -- [Q, E] integer ids padded with -1, or a sequence of per-query
        id sequences; at most EXCLUDE_MAX ids a query; ids the index does not hold match nothing.  Preparing the table reads its pitch
        back (one synchronisation); an int32 [Q, pitch] tensor on the index's device is taken as ALREADY prepared and nothing is read,
        which is the form a graph captures.  Returns a `SearchHandle`; its `info()` adds `route` = 'exclude' and `pitch`."""
        q, D, I, mode = self._search_args(queries, k)
        prepared = isinstance(excl, torch.Tensor) and excl.dtype == torch.int32 and excl.device == self.device and excl.dim() == 2
        table = excl if prepared else prepare_exclusions(excl, self.ntotal, device=self.device)
        if table.shape[0] != q.shape[0]:
            raise ValueError(f"{table.shape[0]} exclusion lists for {q.shape[0]} queries")
        if table.shape[1] > EXCLUDE_MAX:
            raise ValueError(f"{table.shape[1]} ids excluded for one query: at most EXCLUDE_MAX = {EXCLUDE_MAX}")
        chunks = self._enqueue_excluding(q, D, I, mode, k, table, id_offset)
        return SearchHandle(D, I, q, chunks, self.device, {"route": "exclude", "pitch": int(table.shape[1]), "_keep": table})

    def search_device_excluding(self, queries: torch.Tensor, k: int, excl, id_offset: int = 0):
        """`search_device_excluding_async`, waited for: (D, I) on the GPU, and `last_search_info` with `route`, `pitch` and `redone`."""
        return self._waited(self.search_device_excluding_async(queries, k, excl, id_offset=id_offset))

    def search_excluding(self, x, k: int, excl):
        """faiss-style, as `search`: numpy in, (D, I) numpy out."""
        D, I = self.search_device_excluding(_as_queries(x), k, excl)
        return D.cpu().numpy(), I.cpu().numpy()

    # -- a filter per query --------------------------------------------------------------------
    def _multi_plan(self, k, filters, filter_of, nq, route):
        """Everything of a multi-filter search that does not depend on the queries: the parts (`multi_filter_route`), the permutation that
        makes each part a contiguous slice, and per part its device tensors (stacked bitmaps and filter_of, or candidate lists).  The
        last plan is kept on the index: the same call again -- the one a graph captures after its eager run -- uploads and reads nothing."""
        filters = list(filters)
        for rf in filters:
            if rf is None:
                continue
            if not isinstance(rf, RowFilter):
                raise TypeError("filters must hold RowFilter objects or None")
            if rf.ntotal != self.ntotal or rf.device != self.device:
                raise ValueError(f"a filter was built for an index of {rf.ntotal} rows on {rf.device}, "
                                 f"this one holds {self.ntotal} on {self.device}")
        if filter_of is None:
            if len(filters) != nq:
                raise ValueError(f"{len(filters)} filters for {nq} queries: give one per query, or filter_of")
            of = list(range(nq))
        else:
            of = [int(v) for v in (filter_of.tolist() if hasattr(filter_of, "tolist") else filter_of)]
            if len(of) != nq:
                raise ValueError(f"filter_of has {len(of)} entries for {nq} queries")
            if any(v >= len(filters) for v in of):
                raise ValueError(f"filter_of names a filter at or beyond {len(filters)}")
        of = [v if v >= 0 and filters[v] is not None else -1 for v in of]
        key = (self._generation, k, route, tuple(of))
        last = getattr(self, "_multi_last", None)
        if last is not None and last["key"] == key and len(last["filters"]) == len(filters) and all(a is b for a, b in zip(last["filters"], filters)):
            return last
        distinct, members, free = [], [], []        # distinct filters in use (by identity), their queries, the unfiltered queries
        slot = {}
        for qi, v in enumerate(of):
            if v < 0:
                free.append(qi)
                continue
            g = slot.setdefault(id(filters[v]), len(distinct))
            if g == len(distinct):
                distinct.append(filters[v])
                members.append([])
            members[g].append(qi)
        groups = [(len(m), rf.n_allowed, rf.first, rf.last) for rf, m in zip(distinct, members)]
        parts = multi_filter_route(self.precision, k, groups, unfiltered=len(free), ntotal=self.ntotal, route=route)
        dev = self.device
        order = []
        for part in parts:
            qs = [qi for g in part["groups"] for qi in members[g]] + (free if part["unfiltered"] else [])
            part["start"], part["queries"] = len(order), len(qs)
            order += qs
            if part["route"] == "scan":
                lo, hi = part["rows"]
                used = [distinct[g] for g in part["groups"]]
                words = [rf.words[lo // 32:] for rf in used] or [torch.zeros(max(1, (self.ntotal + 31) // 32 - lo // 32), dtype=torch.int32, device=dev)]
                part["words"] = torch.stack(words).contiguous()
                fo = [i for i, g in enumerate(part["groups"]) for _ in members[g]] + [-1] * (len(free) if part["unfiltered"] else 0)
                # one bitmap per query, in the queries' order, in one native call: the entry's NULL filter_of says just that
                direct = fo == list(range(len(used))) and len(fo) <= 32768
                part["filter_of"] = None if direct else torch.tensor(fo, dtype=torch.int32).to(dev)
            elif part["route"] == "candidates":
                used = [distinct[g] for g in part["groups"]]
                width = max([rf.n_allowed for rf in used] + [1])
                lists = torch.full((len(used), width), -1, dtype=torch.int32, device=dev)
                for i, rf in enumerate(used):
                    if rf.n_allowed:
                        lists[i, :rf.n_allowed] = rf.ids().to(torch.int32)
                rows = torch.tensor([i for i, g in enumerate(part["groups"]) for _ in members[g]], dtype=torch.int64).to(dev)
                part["cand"] = lists.index_select(0, rows)
            else:
                part["filter"] = distinct[part["groups"][0]]
        inverse = [0] * nq
        for pos, qi in enumerate(order):
            inverse[qi] = pos
        identity = order == list(range(nq))
        plan = {"key": key, "filters": filters, "parts": parts, "identity": identity,
                "order": None if identity else torch.tensor(order, dtype=torch.int64).to(dev),
                "inverse": None if identity else torch.tensor(inverse, dtype=torch.int64).to(dev)}
        self._multi_last = plan
        return plan

    def search_device_filtered_multi_async(self, queries: torch.Tensor, k: int, filters, filter_of=None, id_offset: int = 0, route=None):
        """The exact top-k of every query over the rows ITS OWN filter allows, stream-ordered: per query what
        `search_device_filtered_async` returns for it alone under its filter.
        filters: a sequence of `RowFilter` or None (no filter) -- one per query, or indexed by `filter_of` ([Q] host ints: a list, an
        array or a CPU tensor; -1 is "no filter"; a device tensor is read back, which costs a synchronisation and cannot be captured).
        `multi_filter_route` splits the work: queries are permuted so that every part is a contiguous slice, every part enqueues on the
        current stream, and one `index_select` puts D and I back in the caller's order.  Nothing is read back beyond what building the
        filters cost; the first call with a set of filters uploads the plan (and reads the id lists of sparse filters), the same call
        again reuses it.  route: None, or 'scan' / 'candidates' to force ONE part for everything (tests, benchmarks; a forced scan of a
        sparse filter stays exact: the on-device redo serves it).  The handle's `info()` adds `parts` and sums `redone`."""
        q, D, I, mode = self._search_args(queries, k)
        nq = q.shape[0]
        plan = self._multi_plan(int(k), filters, filter_of, nq, route)
        parts = plan["parts"]
        if len(parts) == 1 and parts[0]["route"] == "single":
            h = self.search_device_filtered_async(queries, k, parts[0]["filter"], id_offset=id_offset)
            h._extra["parts"] = [{"route": h._extra["route"], "queries": nq, "n_filters": 1}]
            return h
        if nq == 0:
            return MultiSearchHandle(D, I, q, [], self.device)
        qp = q if plan["identity"] else q.index_select(0, plan["order"])
        Dp, Ip = (D, I) if plan["identity"] else (torch.empty_like(D), torch.empty_like(I))
        handles = []
        for part in parts:
            s, n = part["start"], part["queries"]
            qs, Ds, Is = qp[s:s + n], Dp[s:s + n], Ip[s:s + n]
            if part["route"] == "scan":
                lo, hi = part["rows"]
                h = SearchHandle(Ds, Is, qs, self._enqueue_multi(qs, Ds, Is, mode, k, *self._planes(lo, hi), hi - lo, int(id_offset) + lo,
                                                                 part["words"], part["filter_of"], part["n_allowed_min"]),
                                 self.device)
                n_filters = len(part["groups"])
            elif part["route"] == "candidates":
                keep = self._enqueue_candidates(qs, Ds, Is, mode, k, part["cand"], id_offset)
                h = SearchHandle(Ds, Is, qs, [], self.device, {"_keep": keep})
                n_filters = len(part["groups"])
            else:
                h = self.search_device_filtered_async(qs[:, :self.d], k, part["filter"], id_offset=id_offset, route="gather")
                Ds.copy_(h.D)
                Is.copy_(h.I)
                n_filters = 1
            handles.append((part["route"], h, n, n_filters))
        if not plan["identity"]:
            torch.index_select(Dp, 0, plan["inverse"], out=D)
            torch.index_select(Ip, 0, plan["inverse"], out=I)
        return MultiSearchHandle(D, I, q, handles, self.device, keep=(plan, qp, Dp, Ip))

    def _enqueue_multi(self, q, D, I, mode, k, f32, f16, nrows, id_offset, words, filter_of, n_allowed_min):
        """om_sim_topk_filtered_multi over rows [0, nrows) of the planes: `words` [F, pitch] int32 bitmaps over those rows, `filter_of`
        int32 [Q] on the device (None: F == Q <= 32 768 and query q is under bitmap q).  Chunks of at most 32 768 queries; returns the (workspace, status) pairs a handle keeps alive."""
        lib = N.lib()
        n_filters, pitch = words.shape

        def call(rows, n, ws, nbytes, status):
            return lib.om_sim_topk_filtered_multi(mode, N.ptr(q[rows]), n, N.ptr(f32), N.ptr(f16), N.ptr(self._stats), nrows, self.dpad, k,
                                                  int(id_offset), N.ptr(words), pitch, n_filters,
                                                  N.ptr(None if filter_of is None else filter_of[rows]), int(n_allowed_min), N.ptr(D[rows]),
                                                  N.ptr(I[rows]), N.ptr(status), ws, nbytes, N.stream_ptr(self.device))
        return self._enqueue_chunks(q.shape[0], lambda n: lib.om_sim_topk_filtered_multi_workspace_bytes(n, self.dpad, k, n_filters), call)

    def search_device_filtered_multi(self, queries: torch.Tensor, k: int, filters, filter_of=None, id_offset: int = 0, route=None):
        """`search_device_filtered_multi_async`, waited for: (D, I) on the GPU, and `last_search_info` with `parts` and `redone`."""
        return self._waited(self.search_device_filtered_multi_async(queries, k, filters, filter_of=filter_of, id_offset=id_offset, route=route))

    def search_filtered_multi(self, x, k: int, filters, filter_of=None):
        """faiss-style, as `search`: numpy in, (D, I) numpy out."""
        D, I = self.search_device_filtered_multi(_as_queries(x), k, filters, filter_of=filter_of)
        return D.cpu().numpy(), I.cpu().numpy()

    def search(self, x, k: int):
        """faiss-style: numpy in, (D, I) numpy out, I = insertion indices, -1 padded."""
        D, I = self.search_device(_as_queries(x), k)
        return D.cpu().numpy(), I.cpu().numpy()


def merge_topk(part_scores: torch.Tensor, part_ids: torch.Tensor, k_out: int):
    """[W,Q,k] per-shard results -> merged [Q,k_out] on the GPU (om_topk_merge)."""
    W, Q, k_in = part_scores.shape
    if W * k_in > 8192:        # one workgroup sorts at most 8192 keys: merge in groups first
        g = max(2, 8192 // k_in)
        if g * k_in > 8192:
            raise ValueError("k too large to merge")
        outs = [merge_topk(part_scores[i:i + g], part_ids[i:i + g], min(k_out, g * k_in)) for i in range(0, W, g)]
        kk = min(o[0].shape[1] for o in outs)
        return merge_topk(torch.stack([o[0][:, :kk] for o in outs]), torch.stack([o[1][:, :kk] for o in outs]), k_out)
    ps = part_scores.to(torch.float32).contiguous()
    pi = part_ids.to(torch.int64).contiguous()
    N.require_device(ps, pi)
    D = torch.empty(Q, k_out, dtype=torch.float32, device=ps.device)
    I = torch.empty(Q, k_out, dtype=torch.int64, device=ps.device)
    with torch.cuda.device(ps.device):
        N.check(N.lib().om_topk_merge(N.ptr(ps), N.ptr(pi), W, Q, k_in, k_out, N.ptr(D), N.ptr(I),
                                      N.stream_ptr(ps.device)))
    return D, I


def sharded_topk(index, queries: torch.Tensor, k: int, id_offset: int, merge=None):
    """Exact top-k of `queries` (the SAME [Q,d] tensor on every rank) over an index row-sharded across the ranks of the
    default process group: search the local shard, exchange candidates BY QUERY RANGE with one all-to-all (rank r
    receives every shard's [Q/W, k] candidates for its slice -- point-to-point xGMI traffic, no rank collects W full
    result sets), merge the W lists of the slice on the GPU.  Returns (D [blk,k], I [blk,k], blk): this rank's slice
    rows [rank*blk, (rank+1)*blk) of the merged result (rows past Q are padding)."""
    import torch.distributed as dist
    W = dist.get_world_size()
    dev = queries.device
    Q = queries.shape[0]
    D, I = index.search_device(queries, k, id_offset=id_offset)
    D, I = D.to(dev), I.to(dev)
    blk = (Q + W - 1) // W
    pad = blk * W - Q
    if pad:
        D = torch.cat([D, torch.full((pad, k), torch.finfo(torch.float32).min, dtype=D.dtype, device=dev)])
        I = torch.cat([I, torch.full((pad, k), -1, dtype=I.dtype, device=dev)])
    from .comm import native_comm
    comm = native_comm(dev) if D.is_cuda else None
    if comm is not None:                         # OPENMATCH_AMD_COMM=native: om_exchange_topk behind the C ABI
        recv_D, recv_I = comm.exchange_topk(D, I)
    else:
        # ONE all-to-all: per destination rank a block of [blk*k f32 score bits | blk*k int32 SHARD-LOCAL row ids | the
        # sender's 64-bit id offset as two int32] -- 8 bytes per candidate instead of 12 (int64 global ids in a second
        # call): 56 MB instead of 84 MB per GPU at Q = 6980, k = 1000, and one ring set-up instead of two
        n = blk * k
        payload = torch.empty(W, 2 * n + 2, dtype=torch.int32, device=dev)
        payload[:, :n] = D.contiguous().view(W, n).view(torch.int32)
        payload[:, n:2 * n] = torch.where(I >= 0, I - id_offset, I).to(torch.int32).view(W, n)
        payload[:, 2 * n:] = torch.tensor([id_offset], dtype=torch.int64).view(torch.int32).to(dev)
        recv = torch.empty_like(payload)
        dist.all_to_all_single(recv, payload)                   # block w of recv = shard w's candidates for MY queries
        recv_D = recv[:, :n].view(torch.float32).contiguous()
        loc = recv[:, n:2 * n].to(torch.int64)
        offs = recv[:, 2 * n:].contiguous().view(torch.int64)   # [W, 1]: shard w's first global row id
        recv_I = torch.where(loc >= 0, loc + offs, loc)
    Dm, Im = (merge or merge_topk)(recv_D.view(W, blk, k), recv_I.view(W, blk, k), k)
    return Dm.to(dev), Im.to(dev), blk
