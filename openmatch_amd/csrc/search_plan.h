// What a filtered scan round launches: scan_plan() maps (index format, queries, width, switches) to a ScanPlan -- the kernel family and,
// for the stream kernels, the instantiation -- and scan_round() maps (plan, rows of the round, CUs) to the round's launches: kernel id,
// rows, grid and `group` argument of a main launch and of a ragged tail.  Neither does anything else -- no launch, no HIP call, no global
// read or written, no pointer dereferenced.  Scan::filter_step (search.hip) asks for the round and launches it from the kernel table (search_scan.hip, through scan_launch);
// om_debug_scan_plan / om_debug_scan_round return the plan / the round alone, so the rules are testable on a machine without a GPU, and
// om_debug_sim_stream launches the stream instantiation a plan names over a caller's buffers, om_debug_scan_kernel one tile kernel with
// the grid and group of a ScanLaunch.  DESIGN.md 4f lists the rules in the order they are tested here.
#pragma once
#include <algorithm>

#include "gemm_plan.h"      // g7_ring_ok
#include "kernels.h"

struct ScanSwitches {
  int gen7;         // OM_OPT_SCAN_GEN7: 1 the persistent kernels (generation 7 for wide batches, the register-resident stream for small
                    // ones); 0 the tile-at-a-time kernels of generations 2 and 6
  int growth_set;   // OM_OPT_SCAN_GROWTH was given by the caller (else 33-128 queries take their own measured value)
  int growth;       // OM_OPT_SCAN_GROWTH: rows per round of the fast schedule, in percent of the rows already scanned
  int qgroup;       // OM_OPT_SCAN_QGROUP: query tiles an XCD keeps resident while the generation-7 scan sweeps the index rows
  int nt;           // OM_OPT_SEARCH_DEBUG bit 2 clear: the stream kernels fetch the index with non-temporal loads
  int probe;        // OM_OPT_SEARCH_DEBUG bits 3-4: the timing variant of the stream kernel (probe builds only; 0 the real one)
};

// every switch the planner reads, read once per entry call
static ScanSwitches scan_switches() {
  const int debug = om_option(OM_OPT_SEARCH_DEBUG);
  return ScanSwitches{om_option(OM_OPT_SCAN_GEN7), om_option_is_set(OM_OPT_SCAN_GROWTH) ? 1 : 0, om_option(OM_OPT_SCAN_GROWTH),
                      om_option(OM_OPT_SCAN_QGROUP), (debug & 4) ? 0 : 1, (debug >> 3) & 3};
}

// OM_SEARCH_* -> `half` of scan_plan, scan_round and search_schedule: OM_SEARCH_F16_ONLY scans the same 16-bit plane with the same certified
// margin as OM_SEARCH_F16_RESCORE, so its plan, its launches and its schedule are that mode's; only what the re-score reads differs.
static inline bool search_mode_half(int mode) { return mode == OM_SEARCH_F16_RESCORE || mode == OM_SEARCH_F16_ONLY; }

#define SCAN_KSTEP 64            // index columns per K step of the stream kernels (one 128-byte LDS row of 16-bit values)
#define SCAN_NKMAX32_NARROW 12   // K steps compiled into the 32-query stream kernel: 256 <= d <= 768 ...
#define SCAN_NKMAX32_WIDE 16     // ... and 832 <= d <= 1024
#define SCAN_NKMAX16 32          // K steps compiled into the 16-query stream kernel: 1088 <= d <= 2048

// What the planner decided.  family: OM_SCAN_FAMILY_*.  For the two stream families: qblock = queries per resident block (32: on
// 32 x 32 x 16 MFMAs, 16: on 16 x 16 x 32), nb = resident blocks per workgroup (1 | 2 | 4: 4 / nb waves share a block and a unit's 128
// rows), nkmax = K steps compiled in (query registers: qblock * nkmax * 64 * 2 bytes per wave).  The other families leave them 0.
struct ScanPlan { int family, qblock, nb, nkmax; };

static ScanPlan scan_plan(bool half, int64_t nq, int d, const ScanSwitches sw) {
  ScanPlan p = {OM_SCAN_FAMILY_GENERIC, 0, 0, 0};
  auto stream = [&](int family, int qblock, int nkmax) {
    const int64_t blocks = (nq + qblock - 1) / qblock;
    p.family = family; p.qblock = qblock; p.nb = blocks <= 1 ? 1 : blocks <= 2 ? 2 : 4; p.nkmax = nkmax;
    return p;
  };
  // 1. more than one 128-query tile: the 256 x 256 kernels, in both index formats (which of them: scan_round)
  if (nq > 128) { p.family = OM_SCAN_FAMILY_WIDE; return p; }
  // 2. the float32 index, the switch off, no whole K step: the 128-query tile of generation 2
  if (!half || !sw.gen7 || nq < 1 || d < SCAN_KSTEP || d % SCAN_KSTEP != 0) return p;
  const int nk = d / SCAN_KSTEP;
  // 3. fewer than four K steps: the split append of the stream kernels has no retire point inside a tile
  if (nk < 4) return p;
  // 4. the query block(s) of a workgroup resident in registers, one pass over the index at stream speed
  if (nk <= SCAN_NKMAX32_NARROW) return stream(OM_SCAN_FAMILY_STREAM32, 32, SCAN_NKMAX32_NARROW);
  if (nk <= SCAN_NKMAX32_WIDE) return stream(OM_SCAN_FAMILY_STREAM32, 32, SCAN_NKMAX32_WIDE);
  // 5. wider rows: a 32-query block no longer fits a wave's registers, a 16-query block does up to d = 2048 -- at most 64 queries
  if (nk <= SCAN_NKMAX16 && nq <= 64) return stream(OM_SCAN_FAMILY_STREAM16, 16, SCAN_NKMAX16);
  return p;
}

// One launch of a round: kernel OM_SCAN_KERNEL_* (the stream instantiation is the plan's qblock / nb / nkmax), rows [row0, row0 + rows) of
// the round on `grid` workgroups; group: the kernel's last argument -- group_m | qgroup << 8 of the tile walk, for the stream kernel 1
// when it fetches the index with non-temporal loads.  rows == 0: no launch (kernel 0).
struct ScanLaunch { int kernel; int64_t row0, rows, grid; int group; };
struct ScanRound { bool ok; ScanLaunch main, tail; };      // !ok: a grid above 2^31 - 1 workgroups

// The launches of one filtered round over `rows` index rows on a device of `cus` compute units.  The persistent kernels take the whole
// tiles on at most one workgroup per CU and leave the ragged rest to a tile-at-a-time kernel; either part may be empty.
static ScanRound scan_round(const ScanPlan& plan, bool half, int64_t nq, int d, int64_t rows, int cus, const ScanSwitches& sw) {
  ScanRound r = {true, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
  const int64_t tiles256 = (rows + 255) / 256, q256 = (nq + 255) / 256, q128 = (nq + 127) / 128;
  auto split = [&](int kernel, int64_t unit, int64_t grid_per_unit, int group, int tail_kernel, int64_t tail_grid) {
    const int64_t whole = rows - rows % unit;
    if (whole) r.main = {kernel, 0, whole, std::min<int64_t>(cus, whole / unit * grid_per_unit), group};
    if (rows > whole) r.tail = {tail_kernel, whole, rows - whole, tail_grid, 8};
  };
  if (plan.family == OM_SCAN_FAMILY_WIDE && half && sw.gen7) {
    // 1. wide batches on the 16-bit index: generation 7 over the whole 256-row tiles -- on the continuous ring where the rows hold its
    //    three K steps -- and generation 6 over the ragged tail
    split(g7_ring_ok(d) ? OM_SCAN_KERNEL_WIDE7C : OM_SCAN_KERNEL_WIDE7, 256, q256, 8 | (std::max(1, sw.qgroup) << 8), OM_SCAN_KERNEL_TILE6, q256);
  } else if (plan.family == OM_SCAN_FAMILY_WIDE) {
    // 2. wide batches with the switch off, or on the float32 index: generation 6, one workgroup per (row tile, query tile)
    r.main = {OM_SCAN_KERNEL_TILE6, 0, rows, tiles256 * q256, 8};
    r.ok = r.main.grid <= 0x7fffffffLL;
  } else if (plan.family == OM_SCAN_FAMILY_STREAM32 || plan.family == OM_SCAN_FAMILY_STREAM16) {
    // 3. the stream kernels over the whole 128-row tiles, the generic tile over the ragged tail
    split(OM_SCAN_KERNEL_STREAM, 128, 1, sw.nt, OM_SCAN_KERNEL_TILE2, q128);
  } else {
    // 4. the generic tile, one workgroup per (256 rows, 128 queries)
    r.main = {OM_SCAN_KERNEL_TILE2, 0, rows, tiles256 * q128, 8};
  }
  if (!r.main.rows) r.main = {0, 0, 0, 0, 0};
  return r;
}

// ---- the fast schedule's chunk arithmetic (one function for om_sim_topk and om_sim_topk_async, so the two cannot drift apart) --------
// Bootstrap on the first SEARCH_DENSE_CHUNK rows, scored densely; then filtered rounds over chunks whose sizes are fixed on the host from
// an ESTIMATE of the list length after a selection (it hardly moves: k plus ties / the certified margin).  Expected survivors of a chunk
// ~ list * chunk / at.  Few queries: the scan is one HBM pass whatever the thresholds, the per-round launches are what costs -- few, long
// rounds; many queries: an append costs the scan a slow path, the selection ~0.3 ms -- many short rounds with tight thresholds
// (profiles/r02_scan_trace_*.log; 33-128 queries, one index pass per round set on the register-resident stream kernel: 100 % measured
// best of 60 / 100 / 200).  Pure: no launch, no HIP call, no global read (om_debug_search_schedule returns it alone).
#define SEARCH_SORT_CAP 8192        // keys of one candidate list (search_keys.h SORT_CAP)
#define SEARCH_DENSE_CHUNK 4096     // rows of the dense bootstrap (search.hip DENSE_CHUNK)
#define SEARCH_SCHED_MAX 1024       // rounds a schedule can have: at the smallest growth (5 %) 2^32 rows take fewer than 320

struct SearchSchedule {
  int64_t list;     // estimated list length after a selection (certified: + the margin's ties)
  int sel_cap;      // keys the LDS copy of the rounds' selection holds: 4096 when twice the expected growth fits, else SEARCH_SORT_CAP
  int n;            // filtered rounds; chunks[0 .. min(n, cap)) are their sizes in rows, the first starts at row SEARCH_DENSE_CHUNK
};

// The list estimate after a selection for k: certified scans keep the margin's ties too.
static int64_t search_list_estimate(bool half, int64_t k) { return half ? k * 13 / 10 + 64 : k + 16; }

// The round loop of both schedules: rounds from row `first` to N, `list` the estimate the re-score covers, `list_grow` the estimate the
// lists fill by between two selections (the same number without a filter; that of k_eff under one).
static SearchSchedule search_schedule_rounds(int64_t list, int64_t list_grow, int64_t first, int64_t nq, int64_t N, const ScanSwitches sw,
                                             int64_t* chunks, int cap) {
  SearchSchedule p;
  p.list = list;
  const double growth = nq <= 32 ? 400.0 : (nq <= 128 && !sw.growth_set ? 100.0 : (double)(sw.growth > 5 ? sw.growth : 5));
  const double room = 0.75 * (double)(SEARCH_SORT_CAP - list_grow);
  const double grow = (double)list_grow * growth / 100.0;
  // never below 5 % a round, the least `growth` asks for: without a filter room is far above it (list_grow <= 2726 at k = 2048) and this
  // changes nothing; a forced scan of a sparse filter (list_grow near or beyond SEARCH_SORT_CAP, room <= 0) still ends within
  // SEARCH_SCHED_MAX rounds, and a list that overflows all the same is the redo's
  const double want = std::max(room < grow ? room : grow, (double)list_grow * 5.0 / 100.0);      // (`grow` at growth = 5: never above it)
  // selection launches of the rounds: lists are ~list_grow + want keys long; when twice that margin fits 4096 keys the
  // LDS copy is sized for 4096 (four workgroups per CU instead of two); a longer list is read from global memory
  p.sel_cap = (double)list_grow + 2.0 * want + 256.0 < 4096.0 ? 4096 : SEARCH_SORT_CAP;
  p.n = 0;
  int64_t at = first;
  while (at < N) {
    int64_t chunk = (int64_t)((double)at * want / (double)list_grow);
    if (chunk < SEARCH_DENSE_CHUNK) chunk = SEARCH_DENSE_CHUNK;
    chunk &= ~(int64_t)255;                                   // whole tiles (SEARCH_DENSE_CHUNK is one)
    if (chunk > N - at) chunk = N - at;
    if (N - at - chunk < chunk / 4) chunk = N - at;           // no sliver of a last round
    if (chunks && p.n < cap) chunks[p.n] = chunk;
    ++p.n;
    at += chunk;
  }
  return p;
}

static SearchSchedule search_schedule(bool half, int64_t nq, int64_t N, int k, const ScanSwitches sw, int64_t* chunks, int cap) {
  const int64_t list = search_list_estimate(half, k);
  return search_schedule_rounds(list, list, SEARCH_DENSE_CHUNK, nq, N, sw, chunks, cap);
}

// ---- the same schedule under a row filter (om_sim_topk_filtered) ----------------------------------------------------------------------
// Only n_allowed of the N rows may be returned.  The scan kernels do not know the filter: a selection keeps about k ALLOWED keys, so its
// threshold is the k-th best allowed score -- which about k_eff = ceil(k N / n_allowed) rows of any kind reach -- and the lists fill
// between two selections as those of an unfiltered search for k_eff would.  So the growth per round (and the selection's LDS copy) is
// sized from the list estimate of k_eff, and the dense bootstrap covers `boot` chunks of SEARCH_DENSE_CHUNK rows: the smallest count
// whose EXPECTED allowed rows reach 2 k (a threshold exists only once k allowed rows were seen; until then every scanned row is appended),
// at most all the rows.  The first round starts at row boot * SEARCH_DENSE_CHUNK.  `list` stays the estimate for k: after the last
// drop and selection a list holds allowed keys only, and that is what the re-score has to cover.
// n_allowed >= N returns exactly search_schedule (boot = 1); n_allowed < 1 counts as 1 (everything is scored densely).  Pure.
// Rule for a bitmap per query (om_sim_topk_filtered_multi): ONE schedule serves the call, this function's for n_allowed = the count of
// the SPARSEST bitmap any query of the call is under (N when every query is unfiltered).  The bootstrap and the rounds are then long
// enough for that query; the lists of a query under a denser bitmap -- or under none -- reach their threshold earlier and fill more
// slowly than planned, which costs nothing.  The count is a planning number only: the redo's rank is counted per bitmap on the device.
static int64_t search_k_eff(int64_t k, int64_t N, int64_t n_allowed) {                 // N < 2^32, k <= 2048: no overflow
  const int64_t na = n_allowed < 1 ? 1 : n_allowed;
  return na >= N ? k : (k * N + na - 1) / na;
}

static SearchSchedule search_schedule_filtered(bool half, int64_t nq, int64_t N, int k, int64_t n_allowed, const ScanSwitches sw,
                                               int64_t* chunks, int cap, int64_t* boot) {
  if (n_allowed >= N) {
    if (boot) *boot = 1;
    return search_schedule(half, nq, N, k, sw, chunks, cap);
  }
  const int64_t na = n_allowed < 1 ? 1 : n_allowed;
  const int64_t all = (N + SEARCH_DENSE_CHUNK - 1) / SEARCH_DENSE_CHUNK;
  int64_t b = (2 * (int64_t)k * N + SEARCH_DENSE_CHUNK * na - 1) / (SEARCH_DENSE_CHUNK * na);
  b = b < 1 ? 1 : (b > all ? all : b);
  if (boot) *boot = b;
  return search_schedule_rounds(search_list_estimate(half, k), search_list_estimate(half, search_k_eff(k, N, na)), b * SEARCH_DENSE_CHUNK,
                                nq, N, sw, chunks, cap);
}

// ---- the same schedule under an exclusion list per query (om_sim_topk_excluding) ------------------------------------------------------
// Every query may drop up to `pitch` rows, the width of the call's exclusion table (at most SEARCH_EXCLUDE_MAX ids a query), so at least
// N - pitch rows may be returned to each: the filtered schedule for that count -- a planning number only, as the bitmaps' count is (the
// redo's rank comes from a count of every list taken on the device).  pitch == 0 is search_schedule; N - pitch < 1 scores everything
// densely, as n_allowed < 1 does.  What defeats it is what defeats a clustered bitmap: lists that exclude most of the head of the index
// leave no threshold behind the bootstrap, the lists overflow and the queries are redone.  Pure.
#define SEARCH_EXCLUDE_MAX 4096     // ids of one query's exclusion list: 16 KiB, what the drop stages in LDS
static SearchSchedule search_schedule_excluding(bool half, int64_t nq, int64_t N, int k, int64_t pitch, const ScanSwitches sw, int64_t* chunks,
                                                int cap, int64_t* boot) {
  const int64_t left = N - (pitch < 0 ? 0 : pitch);
  return search_schedule_filtered(half, nq, N, k, left < 0 ? 0 : left, sw, chunks, cap, boot);
}
