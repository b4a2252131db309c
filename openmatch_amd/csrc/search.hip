// Exact inner-product top-k over a resident index shard (K12 + K13 + K14), gfx950.
// Replaces faiss.IndexFlatIP.search and the faiss-GPU shard merge
// (retriever/dense_retriever.py:38-58,180; utils.py:215-229).
//
// The [Q x N] score matrix is never materialised.  The scan is a threshold-filtered GEMM:
//   1. bootstrap: score the first few thousand rows densely, sort, theta_q = k-th best so far
//      (the k-th best of ANY subset is a lower bound of the final k-th best);
//   2. scan the remaining rows in geometrically growing chunks with the MFMA main loop of
//      gemm_core.h (A = index rows, B = queries -> every lane owns one query column); the
//      epilogue appends (score,row) to the query's candidate list only if score >= theta_q
//      -- the expected number of survivors per chunk is k * chunk / rows_seen;
//   3. after each chunk a per-query bitonic sort (LDS, 8192 keys) keeps the best k and
//      raises theta_q.  If a list overflows (adversarial row order) the chunk is redone
//      through the dense path, which is always exact.
// Scores in OM_SEARCH_F32 mode come from the exact-f32 MFMA (k-ordered fmaf chain).
// In OM_SEARCH_F16_RESCORE mode the scan runs on the IEEE-f16 shadow index with a CERTIFIED
// margin: |s_f16 - s_f32| <= E_q = ||q||*max||p-f16(p)|| + ||q-f16(q)||*max||f16(p)|| (+ f32
// accumulation slop), the list keeps everything within 2*E_q of the running k-th best, and
// the survivors are re-scored with exact f32 dot products before the final top-k -- so the
// returned ids are those of the f32 scan.
#include <stdlib.h>

#include <algorithm>

#include "gemm_core2.h"
#include "gemm_core6.h"
#include "gemm_wide7.h"
#include "kernels.h"
#include "search_plan.h"

#define SORT_CAP 8192      // keys one workgroup sorts in LDS (64 KiB)
#define DENSE_CHUNK 4096   // rows scored densely per bootstrap / fallback step
#define LIST_MAX (SORT_CAP - DENSE_CHUNK)
#define K_MAX 2048
#define SORT_THREADS 512
static_assert(SORT_CAP == SEARCH_SORT_CAP && DENSE_CHUNK == SEARCH_DENSE_CHUNK, "search_plan.h schedules for these list and bootstrap sizes");

// Per-query sticky status of the asynchronous entry (`qstat`, nullptr on om_sim_topk's path): a query with any bit set is recomputed by the
// on-device redo.  The global flags (flag[0] overflow, flag[1] longest list, flag[2] margin too wide or not finite) stay as they are: they
// are all om_sim_topk's path has.
#define QSTAT_OVERFLOW 1u    // the list exceeded SORT_CAP in some round: appends were dropped
#define QSTAT_WIDE 2u        // a certified list outgrew LIST_MAX (or the certified margin is not finite)
#define QSTAT_COVER 4u       // the final list is longer than the re-score cover

typedef unsigned long long u64;
static thread_local int64_t g_info[8];   // last om_sim_topk call: see om_sim_topk_info()

__host__ __device__ inline u64 pack_key(float score, uint32_t payload) {
  return ((u64)f32_orderable(score) << 32) | (u64)(uint32_t)~payload;
}
__host__ __device__ inline float key_score(u64 k) { return orderable_f32((uint32_t)(k >> 32)); }
__host__ __device__ inline uint32_t key_payload(u64 k) { return ~(uint32_t)k; }

// ---- filtered scan: A = index rows [row0, row0+nrows), B = queries ----------------------
template <typename T>
__global__ __launch_bounds__(G2_THREADS) void sim_filter_kernel(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries,
    int64_t nq, int64_t d, const float* __restrict__ thr, u64* __restrict__ keys,
    unsigned* __restrict__ cnt, int group_m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t m0, n0;
  g2_tile_coords(nrows, nq, group_m, m0, n0);       // 256 index rows x 128 queries per workgroup
  f32x16_t acc[2][2];
  gemm_mainloop2<T>(rows, d, queries, d, nrows, nq, d, m0, n0, smem, acc);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int64_t q = n0 + wn * 64 + ni * 32 + (lane & 31);
    if (q >= nq) continue;
    const float th = thr[q];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int64_t mbase = m0 + wm * 64 + mi * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
        const float v = acc[mi][ni][r];
        if (m < nrows && v >= th) {
          const unsigned pos = atomicAdd(cnt + q, 1u);
          if (pos < SORT_CAP) keys[q * SORT_CAP + pos] = pack_key(v, row_base + (uint32_t)m);
        }
      }
    }
  }
}

// The scan for query batches wider than one 128 tile: 256 queries x 256 index rows per workgroup on
// the one-wave-per-SIMD main loop of gemm_core6.h.  The QUERIES are its A operand, so (operands
// swapped inside, see there) a lane owns one query and its registers walk index rows:
//   acc[mi][ni][r] = <query q0 + wm*128 + mi*32 + (lane&31),  row r0 + wn*128 + ni*32 + 8*(r>>2) + 4*(lane>>5) + (r&3)>
// The filter first takes the maximum of each 16-register tile (8 v_max3) and only walks the tile
// when some lane of the wave has a survivor -- survivors are rare by construction of theta.
template <typename T>
__global__ __launch_bounds__(G6_THREADS) void sim_filter_kernel6(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries,
    int64_t nq, int64_t d, const float* __restrict__ thr, u64* __restrict__ keys,
    unsigned* __restrict__ cnt, int group_m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // `group_m` index-row tiles stay resident (L2) while every query tile sweeps over them
  const int64_t ntr = (nrows + G6_BN - 1) / G6_BN, ntq = (nq + G6_BM - 1) / G6_BM;
  int64_t tr_, tq_;
  gemm_tile_coords(ntr, ntq, group_m, tr_, tq_);
  const int64_t q0 = tq_ * G6_BM, r0 = tr_ * G6_BN;
  f32x16_t acc[4][4];
  {
    f32x16_t zero[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) zero[i][r] = 0.f;
    gemm_mainloop6<T>(queries, d, rows, d, nq, nrows, d, q0, r0, smem, acc, zero);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t q = q0 + wm * 128 + mi * 32 + (lane & 31);
    const float th = q < nq ? thr[q] : __builtin_inff();
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const f32x16_t a = acc[mi][ni];
      float mx = fmaxf(fmaxf(a[0], a[1]), a[2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, a[r]), a[r + 1]);
      mx = fmaxf(mx, a[15]);
      if (mx >= th) {
        const int64_t nbase = r0 + wn * 128 + ni * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t n = nbase + (r & 3) + 8 * (r >> 2);
          const float v = a[r];
          if (n < nrows && v >= th) {
            const unsigned pos = atomicAdd(cnt + q, 1u);
            if (pos < SORT_CAP) keys[q * SORT_CAP + pos] = pack_key(v, row_base + (uint32_t)n);
          }
        }
      }
    }
  }
}

// Survivors of the generation-7 scan.  A score passes its list's threshold about once in a thousand, but with 1024
// scores per 32 x 32 block most blocks hold one: appending from inside the block walk (returning atomic on the list
// counter -> wait -> store, per survivor, as generation 6 does) serialises ~7 L2 round trips per wave and tile
// (profiles/r02_scan_trace_v0.log: 11.2k cycles of a 44.9k-cycle tile).  Instead the walk only STAGES survivors in
// wave-private LDS -- position from the wave's ballot, no atomics.  Staging: keys in the wave's OWN DMA slices of units 2
// and 3 (only this wave ever writes them, and not before its next tile starts), 2048 of them; their query numbers in
// unit 4 behind the threshold tables.  A block adds at most 1024 records, so one capacity check per block suffices.
//
// Round 3 (the tile trace had 12k of a tile's 40k cycles outside the K loop, and the four waves meet at the next tile's
// first barrier, so the slowest filter sets the pace):
//  * two-level walk: the block test keeps the maxima of its four register quads; a block with a survivor tests the
//    quads and walks only the (one, almost always) quad that holds it -- ~8 ballot + branch steps instead of 16;
//  * the append is split around the NEXT tile's K loop: at the end of a tile's filter its (<= 64, one per lane)
//    records move from the staging area into registers; after the next K loop the list-counter atomics are issued,
//    their return is consumed half a filter later and the key stores leave half a filter before the tile start that
//    would otherwise wait for their acknowledgement (vmcnt retires in order).  Neither round trip is exposed.  More
//    than 64 records in a tile, or a full staging area, take the synchronous flush (rare);
//  * the tile walk advances incrementally (no division per tile), and the DMA lane offsets are computed once: the
//    query panel is padded with zero rows to a whole tile (query_prep_kernel), so no tile needs clamped rows.
#define SC7_STAGE_CAP 2048
#define SC7_QIDX_OFF (G7_TAB_OFF + 4096)
__device__ __forceinline__ char* sc7_key_slot(char* smem, int wave, unsigned pos) {
  return smem + (2 + (pos >> 10)) * G7_UNIT_BYTES + wave * 1024 + ((pos >> 7) & 7) * 4096 + (pos & 127) * 8;
}
__device__ __forceinline__ uint16_t* sc7_q_slot(char* smem, int wave, unsigned pos) {
  return (uint16_t*)(smem + SC7_QIDX_OFF + wave * (SC7_STAGE_CAP * 2) + pos * 2);
}
// synchronous append of staged records [from, wcount): one atomic round trip, then the stores
__device__ __forceinline__ void sc7_flush(char* smem, int wave, unsigned from, unsigned wcount, int lane, int64_t q0,
                                          u64* __restrict__ keys, unsigned* __restrict__ cnt) {
  for (unsigned i = from + (unsigned)lane; i < wcount; i += 64) {
    const u64 key = *(const u64*)sc7_key_slot(smem, wave, i);
    const int64_t q = q0 + *sc7_q_slot(smem, wave, i);
    const unsigned pos = atomicAdd(cnt + q, 1u);
    if (pos < SORT_CAP) keys[q * SORT_CAP + pos] = key;
  }
}
// query blocks MI0 .. MI1-1 of the wave's 128 x 128 scores; whole tiles only: every row of the tile exists
template <int MI0, int MI1>
__device__ __forceinline__ void sc7_filter(f32x16_t (&acc)[4][4], const float (&th)[4], uint32_t id0, uint32_t ql0,
                                           int lane, char* smem, int wave, unsigned& wcount, int64_t q0,
                                           u64* __restrict__ keys, unsigned* __restrict__ cnt) {
#pragma unroll
  for (int mi = MI0; mi < MI1; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      asm volatile("" : "+a"(acc[mi][ni]));            // stays in its AGPRs until this point
      const f32x16_t a = acc[mi][ni];
      float gm[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) gm[g] = fmaxf(fmaxf(fmaxf(a[4 * g], a[4 * g + 1]), a[4 * g + 2]), a[4 * g + 3]);
      const float mx = fmaxf(fmaxf(fmaxf(gm[0], gm[1]), gm[2]), gm[3]);
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx >= th[mi]) != 0, 0)) {          // wave-uniform: some lane holds a survivor (cold: laid out behind the 16 block tests)
        if (wcount > SC7_STAGE_CAP - 1024) { sc7_flush(smem, wave, 0u, wcount, lane, q0, keys, cnt); wcount = 0; }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (__builtin_amdgcn_ballot_w64(gm[g] >= th[mi]) == 0) continue;
#pragma unroll
          for (int r = 4 * g; r < 4 * g + 4; ++r) {
            const uint32_t off = (uint32_t)(ni * 32 + (r & 3) + 8 * (r >> 2));
            const bool pass = a[r] >= th[mi];
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
            if (m != 0) {
              if (pass) {
                const unsigned pos = wcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                *(u64*)sc7_key_slot(smem, wave, pos) = pack_key(a[r], id0 + off);
                *sc7_q_slot(smem, wave, pos) = (uint16_t)(ql0 + mi * 32);
              }
              wcount += (unsigned)__builtin_popcountll(m);
            }
          }
        }
      }
      G7_FENCE_();
    }
  }
}

// Work id -> (row tile, query tile) of the generation-7 scan.  With the GEMM's walk (g7_tile: groups of row tiles swept by
// ALL query tiles, 32 consecutive tiles per XCD and round) every XCD touches 4 query panels and 8 row panels per
// round and hops to another group next round: nothing is reused across rounds, and the L2 -> fabric traffic of one
// 6980-query search measured 441 GB, 32x the 13.6 GB index (FETCH_SIZE, profiles/r02_hbm_traffic_search.json) -- 4.7 TB/s,
// close to what the memory system delivers at all.  Here every XCD OWNS a group of at most 8 query tiles (<= 3 MiB of
// query panels, resident in its 4 MiB L2 for the whole launch) and a share of the row tiles, and walks its rows with
// the query tile running fastest: a row panel is fetched once per query GROUP instead of once per 4 query tiles.
// The walk is an iterator: work item w = it * nslots + slot of the XCD's (row, query tile) grid, advanced by nslots per
// tile with one compare instead of a division.
struct Sc7Walk {
  bool owned;                      // XCD-owned query groups (else the GEMM's walk, by index)
  int it;
  int64_t ntr, ntq; int group_m;
  uint32_t q_lo, qn, r_lo, rn, row, qi, d_row, d_qi;
  __device__ __forceinline__ bool init(int64_t ntr_, int64_t ntq_, int group_m_, int qgroup, int64_t& r0, int64_t& q0) {
    ntr = ntr_; ntq = ntq_; group_m = group_m_; it = 0;
    owned = (gridDim.x & 7) == 0 && ntq <= 8 * qgroup;
    if (!owned) return g7_tile(0, ntr, ntq, group_m, r0, q0);
    const uint32_t x = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
    const uint32_t tq = (uint32_t)ntq, tr = (uint32_t)ntr;
    uint32_t ng = 1;                                        // query groups: 1, 2, 4 or 8 -- at most 8 query tiles each
    while (ng < 8 && (tq + ng - 1) / ng > (uint32_t)qgroup) ng <<= 1;
    const uint32_t g = x % ng, part = x / ng, nparts = 8 / ng;
    q_lo = g * tq / ng; qn = (g + 1) * tq / ng - q_lo;
    r_lo = (uint32_t)((uint64_t)part * tr / nparts); rn = (uint32_t)((uint64_t)(part + 1) * tr / nparts) - r_lo;
    if (qn == 0) return false;
    row = slot / qn; qi = slot - row * qn;
    d_row = nslots / qn; d_qi = nslots - d_row * qn;
    if (row >= rn) return false;
    r0 = (int64_t)(r_lo + row) * 256; q0 = (int64_t)(q_lo + qi) * 256;
    return true;
  }
  __device__ __forceinline__ bool next(int64_t& r0, int64_t& q0) {
    ++it;
    if (!owned) return g7_tile(it, ntr, ntq, group_m, r0, q0);
    qi += d_qi; row += d_row;
    if (qi >= qn) { qi -= qn; ++row; }
    if (row >= rn) return false;
    r0 = (int64_t)(r_lo + row) * 256; q0 = (int64_t)(q_lo + qi) * 256;
    return true;
  }
};

// The same scan on generation 7 (gemm_core7.h / gemm_wide7.h): 128-byte K steps (whole-line LDS-DMA requests) in a
// PERSISTENT kernel -- one workgroup per CU walks (query tile, row tile) pairs, the first K step of the next pair and its
// 256 thresholds are fetched while the current pair is filtered.  The only wait at a tile start is vmcnt(16): K step 1
// may be outstanding, everything older -- the prefetch, and the appends of the tile before, issued half a filter
// earlier -- has landed.  16-bit inputs only (the f32 scan stays on generation 6).
// `thr` must be readable up to round_up(nq, 256) + 256 entries (+inf beyond nq: carve_search / init_lists_kernel);
// `queries` holds round_up(nq, 256) rows, zeros beyond nq (query_prep_kernel).
template <typename T>
__global__ __launch_bounds__(G6_THREADS) void sim_filter_kernel7(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries,
    int64_t nq, int64_t d, const float* __restrict__ thr, u64* __restrict__ keys,
    unsigned* __restrict__ cnt, int group_m, unsigned long long* __restrict__ trace) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t ntr = (nrows + 255) / 256, ntq = (nq + 255) / 256;
  const int nk = (int)((d * 2) / G7_ROW_BYTES);
  unsigned wcount = 0;                     // records in this wave's staging area (wave-uniform)
  unsigned pend_n = 0;                     // records of the previous tile held in registers, one per lane (wave-uniform)
  u64 pend_key = 0; uint32_t pend_q = 0;
  int64_t r0, q0;
  const int qgroup = group_m >> 8;                 // (the host packs both walk parameters into one argument)
  group_m &= 255;
  Sc7Walk walk;
  if (!walk.init(ntr, ntq, group_m, qgroup, r0, q0)) return;
  G7Src src;
  g7_offsets<T>(src, d, d, wave, lane0);           // every row of every tile exists (padded query panel, whole row tiles)
  src.a = (const char*)(queries + q0 * d);
  src.b = (const char*)(rows + r0 * d);
  g7_dma((const char*)(thr + q0 + wm * 128), lane0 * 16, g7_lds_addr(smem + G7_TAB_OFF + wave * 1024));
  g7_fill(src.a, src.oa, smem, wave);
  g7_fill(src.b, src.ob, smem + G7_UNIT_BYTES, wave);
  for (;;) {
    unsigned long long* tr = nullptr;          // debug: phase stamps of the first 8192 tiles (om_debug_gemm_trace)
    if (trace) {
      const int64_t tile_id = (r0 / 256) * ntq + q0 / 256;
      if (tile_id < 8192) tr = trace + tile_id * 32;
    }
    if (tr && threadIdx.x == 0) { tr[0] = clock64(); tr[30] = wall_clock64(); }
    if (nk > 1) {
      g7_fill(src.a + G7_ROW_BYTES, src.oa, smem + 2 * G7_UNIT_BYTES, wave);
      g7_fill(src.b + G7_ROW_BYTES, src.ob, smem + 3 * G7_UNIT_BYTES, wave);
      G7_WAIT_VM(16);
    } else {
      G7_WAIT_VM(0);
    }
    if (tr && threadIdx.x == 0) tr[1] = clock64();
    float th[4];
    f32x16_t acc[4][4];
    {
      int lane_i = lane0;
      asm volatile("" : "+v"(lane_i));
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) th[mi] = *(const float*)(smem + G7_TAB_OFF + wave * 1024 + (mi * 32 + (lane_i & 31)) * 4);
      const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
      const frag_t zf = __builtin_bit_cast(frag_t, z4);
      const f32x16_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 16; ++q) {       // zero by the matrix core, one MFMA per accumulator tile: with ONE shared zero fragment the
        frag_t zq = zf;                    // compiler issues one product and copies it into the other fifteen tiles with 240
        asm volatile("" : "+v"(zq));       // v_accvgpr_mov (~1 k of the 1.5 k cycles this block took per pair)
        acc[q >> 2][q & 3] = zero;
        MmaOps<T>::mma(zq, zq, acc[q >> 2][q & 3]);
      }
    }
    gemm_mainloop7_run<T>(src, nk, smem, acc, tr, false);
    if (tr && threadIdx.x == 0) tr[15] = clock64();
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    // the previous tile's records: list positions requested now, consumed half a filter later
    unsigned pend_pos = 0;
    if (pend_n && (unsigned)lane < pend_n) pend_pos = atomicAdd(cnt + pend_q, 1u);
    // next pair: its first K step and its thresholds are fetched under the filter below
    const int64_t rc = r0, qc = q0;
    const bool has_next = walk.next(r0, q0);       // (r0, q0 unchanged when there is none: a harmless re-fetch)
    src.a = (const char*)(queries + q0 * d);
    src.b = (const char*)(rows + r0 * d);
    g7_dma((const char*)(thr + q0 + wm * 128), lane0 * 16, g7_lds_addr(smem + G7_TAB_OFF + wave * 1024));
    g7_fill(src.a, src.oa, smem, wave);
    g7_fill(src.b, src.ob, smem + G7_UNIT_BYTES, wave);
    G7_FENCE_();
    {
      const uint32_t id0 = row_base + (uint32_t)rc + (uint32_t)(wn * 128 + 4 * (lane >> 5));    // row id of (ni = 0, r = 0)
      const uint32_t ql0 = (uint32_t)(wm * 128 + (lane & 31));
      sc7_filter<0, 2>(acc, th, id0, ql0, lane, smem, wave, wcount, qc, keys, cnt);
      if (pend_n) {
        if ((unsigned)lane < pend_n && pend_pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pend_pos] = pend_key;
        pend_n = 0;
      }
      G7_FENCE_();
      sc7_filter<2, 4>(acc, th, id0, ql0, lane, smem, wave, wcount, qc, keys, cnt);
      if (wcount > 64) sc7_flush(smem, wave, 64u, wcount, lane, qc, keys, cnt);
      pend_n = wcount < 64u ? wcount : 64u;
      if ((unsigned)lane < pend_n) {
        pend_key = *(const u64*)sc7_key_slot(smem, wave, (unsigned)lane);
        pend_q = (uint32_t)qc + *sc7_q_slot(smem, wave, (unsigned)lane);
      }
      wcount = 0;
    }
    if (tr && threadIdx.x == 0) { tr[28] = clock64(); tr[29] = blockIdx.x; tr[31] = wall_clock64(); }
    if (!has_next) break;
  }
  if (pend_n && (unsigned)lane0 < pend_n) {
    const unsigned pos = atomicAdd(cnt + pend_q, 1u);
    if (pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pos] = pend_key;
  }
  G7_WAIT_VM(0);
}

// ---- the same scan on the CONTINUOUS ring (round 4; gemm_core7.h gemm_mainloop7_cont, gemm_wide7.h kernels 7c / 7r) ------
// What the kernel above pays per tile beside its 12 k-cycle filter: 16 wave-uniform branches in every K step (one around each
// DMA issue: ~800 of a step's ~3200 cycles -- the branch-free loop runs 2400), 16 DMA issues of K step 1 at every tile start
// and a cold first step.  Here the K loop of a pair prefetches step 0 of the next pair (its last step issues nothing else:
// TAIL_EMPTY), A(1) of the next pair is issued right behind the K loop and lands under the filter, the first half of B(1)
// behind the filter.  The filter's staging lives in the units the last step frees -- this wave's own slices of them, so no
// barrier brackets the filter:
//     ring.bn (the unit A(nk - 1) left)   slices 0-7   keys 0 .. 1023
//     ring.sp (the unit B(nk - 1) left)   slices 0-3   keys 1024 .. 1535;  4-6 query numbers;  7 the next pair's thresholds
//     ring.an (the spare of the last step)              A(1) of the next pair
#define SC7C_CAP 1536
struct Sc7cStage { char* bn; char* sp; };
__device__ __forceinline__ char* sc7c_key_slot(const Sc7cStage& st, unsigned pos) {
  const unsigned sl = pos >> 7;
  return (sl < 8 ? st.bn + sl * 4096 : st.sp + (sl - 8) * 4096) + (pos & 127) * 8;
}
__device__ __forceinline__ uint16_t* sc7c_q_slot(const Sc7cStage& st, unsigned pos) { return (uint16_t*)(st.sp + (4 + (pos >> 9)) * 4096 + (pos & 511) * 2); }
__device__ __forceinline__ void sc7c_flush(const Sc7cStage& st, unsigned from, unsigned wcount, int lane, int64_t q0, u64* __restrict__ keys,
                                           unsigned* __restrict__ cnt) {
  for (unsigned i = from + (unsigned)lane; i < wcount; i += 64) {
    const u64 key = *(const u64*)sc7c_key_slot(st, i);
    const int64_t q = q0 + *sc7c_q_slot(st, i);
    const unsigned pos = atomicAdd(cnt + q, 1u);
    if (pos < SORT_CAP) keys[q * SORT_CAP + pos] = key;
  }
}
__device__ __forceinline__ float sc7c_max3(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float sc7c_max16(const f32x16_t& a) {      // eight v_max3 (the compiler's fmaxf tree: 13 v_max + 5 v_max3)
  const float t0 = sc7c_max3(a[0], a[1], a[2]), t1 = sc7c_max3(a[3], a[4], a[5]), t2 = sc7c_max3(a[6], a[7], a[8]);
  const float t3 = sc7c_max3(a[9], a[10], a[11]), t4 = sc7c_max3(a[12], a[13], a[14]);
  return sc7c_max3(sc7c_max3(t0, t1, t2), sc7c_max3(t3, t4, a[15]), t0);
}
// One row block of queries (mi) against the wave's 128 index rows: the common case -- no score of the block's 64 per lane reaches
// its query's threshold -- is 64 accumulator reads, 33 v_max3, ONE compare and ONE branch; the survivor path is laid out as cold
// code behind the straight line.  Tile trace at the benchmark's size (profiles/r04_probe16_scan_filter_phases.log): filter 5.4 k
// cycles per tile with one test per column block and the survivor code inline (each test 5 KB from the next), 4.7 k like this;
// 3.4 survivors per wave and tile cost ~850 cycles each, the 16 block tests ~1.8 k.  A COMPACT survivor path (scores parked in LDS,
// run-time loop over the score indices: 70 KB of code down to 12) measured 8.9 k -- the unrolled per-score code is the faster one,
// the instruction cache is not what it waits for.
template <int MI0, int MI1>
__device__ __forceinline__ void sc7c_filter(f32x16_t (&acc)[4][4], const float (&th)[4], uint32_t id0, uint32_t ql0, int lane, const Sc7cStage& st,
                                            unsigned& wcount, int64_t q0, u64* __restrict__ keys, unsigned* __restrict__ cnt) {
#pragma unroll
  for (int mi = MI0; mi < MI1; ++mi) {
    f32x16_t a[4];
    float bm[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      asm volatile("" : "+a"(acc[mi][ni]));            // stays in its AGPRs until this point
      a[ni] = acc[mi][ni];
      bm[ni] = sc7c_max16(a[ni]);
    }
    const float mx = sc7c_max3(sc7c_max3(bm[0], bm[1], bm[2]), bm[3], bm[3]);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx >= th[mi]) != 0, 0)) {          // wave-uniform: some lane holds a survivor
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        if (__builtin_amdgcn_ballot_w64(bm[ni] >= th[mi]) == 0) continue;
        if (wcount > SC7C_CAP - 1024) { sc7c_flush(st, 0u, wcount, lane, q0, keys, cnt); wcount = 0; }      // a block adds at most 1024
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float gm = fmaxf(fmaxf(a[ni][4 * g], a[ni][4 * g + 1]), fmaxf(a[ni][4 * g + 2], a[ni][4 * g + 3]));
          if (__builtin_amdgcn_ballot_w64(gm >= th[mi]) == 0) continue;
#pragma unroll
          for (int r = 4 * g; r < 4 * g + 4; ++r) {
            const uint32_t off = (uint32_t)(ni * 32 + (r & 3) + 8 * (r >> 2));
            const bool pass = a[ni][r] >= th[mi];
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
            if (m != 0) {
              if (pass) {
                const unsigned pos = wcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                *(u64*)sc7c_key_slot(st, pos) = pack_key(a[ni][r], id0 + off);
                *sc7c_q_slot(st, pos) = (uint16_t)(ql0 + mi * 32);
              }
              wcount += (unsigned)__builtin_popcountll(m);
            }
          }
        }
      }
    }
    G7_FENCE_();
  }
}

template <typename T>
__global__ __launch_bounds__(G6_THREADS) void sim_filter_kernel7c(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries,
    int64_t nq, int64_t d, const float* __restrict__ thr, u64* __restrict__ keys,
    unsigned* __restrict__ cnt, int group_m, unsigned long long* __restrict__ trace) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t ntr = (nrows + 255) / 256, ntq = (nq + 255) / 256;
  const int nk = (int)((d * 2) / G7_ROW_BYTES);
  unsigned wcount = 0;                     // records in this wave's staging area (wave-uniform)
  unsigned pend_n = 0;                     // records of the previous tile held in registers, one per lane (wave-uniform)
  u64 pend_key = 0; uint32_t pend_q = 0;
  int64_t r0, q0;
  const int qgroup = group_m >> 8;
  group_m &= 255;
  Sc7Walk walk;
  if (!walk.init(ntr, ntq, group_m, qgroup, r0, q0)) return;
  G7SrcU src;
  g7_offsets_u<T>(src, d, d, wave, lane0);         // every row of every tile exists (padded query panel, whole row tiles)
  G7Ring ring;
  g7_ring_reset(ring);
  const uint32_t lds_base = g7_lds_addr(smem);
  const char* cur_a = (const char*)(queries + q0 * d);
  const char* cur_b = (const char*)(rows + r0 * d);
  g7_dma((const char*)(thr + q0 + wm * 128), lane0 * 16, lds_base + ring.sp + (7 * 4 + wave) * 1024);
  g7_fill_a(src, cur_a, smem + ring.ac, wave);
  g7_fill_b(src, cur_b, smem + ring.bc, wave);
  g7_fill_a(src, cur_a + G7_ROW_BYTES, smem + ring.an, wave);
#pragma unroll
  for (int i = 0; i < 4; ++i) g7_issue_b(src, cur_b + G7_ROW_BYTES, i, lds_base + ring.bn + (i * 4 + wave) * 1024);
  G7_WAIT_VM(12);                                  // the thresholds and K step 0 (A(1) and half of B(1) may be outstanding)
  __builtin_amdgcn_s_barrier();                    // first pair only: K step 0 published
  int64_t r1 = r0, q1 = q0;
  bool has_next = walk.next(r1, q1);
  for (;;) {
    unsigned long long* tr = nullptr;
    if (trace) {
      const int64_t tile_id = (r0 / 256) * ntq + q0 / 256;
      if (tile_id < 8192) tr = trace + tile_id * 32;
    }
    if (tr && threadIdx.x == 0) { tr[0] = tr[1] = clock64(); tr[30] = wall_clock64(); }
    float th[4];
    f32x16_t acc[4][4];          // (starts from zero inside the K loop: ZERO_FIRST -- no initialising pass)
    {
      int lane_i = lane0;
      asm volatile("" : "+v"(lane_i));
      const char* const tab = smem + ring.sp + (7 * 4 + wave) * 1024;      // this pair's thresholds (fetched under the previous filter)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) th[mi] = *(const float*)(tab + (mi * 32 + (lane_i & 31)) * 4);
    }
    const char* const next_a = (const char*)(queries + q1 * d);      // (no next pair: this one again -- a harmless prefetch)
    const char* const next_b = (const char*)(rows + r1 * d);
    gemm_mainloop7_cont<T, true, G7NoTail, true, true>(src, cur_a, cur_b, next_a, next_b, nk, smem, ring, acc, tr);
    if (tr && threadIdx.x == 0) tr[15] = clock64();
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const Sc7cStage st = {smem + ring.bn + wave * 1024, smem + ring.sp + wave * 1024};
    // the previous tile's records: list positions requested now, consumed half a filter later
    unsigned pend_pos = 0;
    if (pend_n && (unsigned)lane < pend_n) pend_pos = atomicAdd(cnt + pend_q, 1u);
    // under the filter: A(1) of the next pair (into the unit the filter does not use) and its thresholds
    g7_fill_a(src, next_a + G7_ROW_BYTES, smem + ring.an, wave);
    g7_dma((const char*)(thr + q1 + wm * 128), lane0 * 16, g7_lds_addr(st.sp) + 7 * 4096);
    G7_FENCE_();
    if (tr && threadIdx.x == 0) tr[16] = clock64();
    {
      const uint32_t id0 = row_base + (uint32_t)r0 + (uint32_t)(wn * 128 + 4 * (lane >> 5));    // row id of (ni = 0, r = 0)
      const uint32_t ql0 = (uint32_t)(wm * 128 + (lane & 31));
      sc7c_filter<0, 2>(acc, th, id0, ql0, lane, st, wcount, q0, keys, cnt);
      if (pend_n) {
        if ((unsigned)lane < pend_n && pend_pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pend_pos] = pend_key;
        pend_n = 0;
      }
      G7_FENCE_();
      if (tr && threadIdx.x == 0) tr[17] = clock64();
      sc7c_filter<2, 4>(acc, th, id0, ql0, lane, st, wcount, q0, keys, cnt);
      if (tr && threadIdx.x == 0) { tr[18] = clock64(); tr[20] = wcount; }
      if (wcount > 64) sc7c_flush(st, 64u, wcount, lane, q0, keys, cnt);
      pend_n = wcount < 64u ? wcount : 64u;
      if ((unsigned)lane < pend_n) {
        pend_key = *(const u64*)sc7c_key_slot(st, (unsigned)lane);
        pend_q = (uint32_t)q0 + *sc7c_q_slot(st, (unsigned)lane);
      }
      wcount = 0;
    }
    // A(1) and the thresholds were fetched a whole filter ago; everything issued since (the key stores of the pending records,
    // half a filter old; a synchronous flush, rare) is older than any DMA of the next K loop.  The staging area has been read
    // (lgkmcnt): the first half of B(1) may overwrite it.
    if (tr && threadIdx.x == 0) tr[19] = clock64();
    G7_WAIT_VM(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (tr && threadIdx.x == 0) tr[21] = clock64();
#pragma unroll
    for (int i = 0; i < 4; ++i) g7_issue_b(src, next_b + G7_ROW_BYTES, i, lds_base + ring.bn + (i * 4 + wave) * 1024);
    if (tr && threadIdx.x == 0) { tr[28] = clock64(); tr[29] = blockIdx.x; tr[31] = wall_clock64(); }
    if (!has_next) break;
    cur_a = next_a; cur_b = next_b; r0 = r1; q0 = q1;
    has_next = walk.next(r1, q1);
  }
  if (pend_n && (unsigned)lane0 < pend_n) {
    const unsigned pos = atomicAdd(cnt + pend_q, 1u);
    if (pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pos] = pend_key;
  }
  G7_WAIT_VM(0);
}

// Small query batches (<= 128 queries): the scan is a pass over the whole f16 index (13.6 GB at 8.8 M x 768) that has to
// run at HBM speed.  The generic 128-query tile spends 1.7 PFLOP of matrix-core time on padding at Q = 1 (3.99 ms per
// search in round 1, profiles/r01_search_shapes.jsonl).  Round 2 kept one or two 32-query blocks resident in LDS beside a
// three- / four-slot ring (2.56 ms at Q = 1, 3.35 at Q = 64, nothing for 65-128 queries: 4.6 ms on the generation-2 filter
// kernel) -- LDS shared between the resident blocks (48 KiB each) and the ring had no room for a third block.  Round 3 moves
// the queries into registers.  A wave's B operand never changes: its 32-query block is 12 K steps x 4 MFMA sub-steps x 16 bytes per lane = 192
// VGPRs of the 512 this one-wave-per-SIMD kernel owns, loaded once from global memory in fragment order.  The whole LDS
// (160 KiB) is the ring: ten slots of 128 rows x 128 bytes, nine units = 144 KiB per CU in flight.
//     NB = 1 (Q <= 32)    the four waves share the block and take 32 rows of a unit each
//     NB = 2 (Q <= 64)    waves 0, 2 / 1, 3 hold block 0 / 1 and take 64 rows each
//     NB = 4 (Q <= 128)   one block per wave, every wave takes all 128 rows (each reads the whole unit: 64 KiB of fragment
//                         reads + 16 KiB of DMA per unit is the LDS port's limit at ~15 TB/s, above what HBM delivers)
// Persistent over 128-row tiles (blockIdx, blockIdx + grid, ...); whole tiles only; 256 <= d <= 768 (K steps past d / 64 are
// compiled but skipped: the K loop is unrolled so that the query fragments are indexed statically).  The index stream is
// fetched with the non-temporal policy (read once, by one CU).  Measured (8 841 823 x 768, k = 1000, profiles/r03_search_small_batches.log):
// Q = 1 2.42-2.62 ms (round 2: 2.56-2.65 on like boxes), Q = 64 3.14-3.22 (3.35), Q = 128 3.59-3.68 (4.63).  What more
// bytes in flight did NOT buy: the kernel's own time still grows with the resident blocks (2.15 / 2.9 / 3.3 ms for one / two /
// four, rocprofv3) although neither the matrix core (16 MFMAs per 16 KiB unit at most) nor the LDS port is near a limit.
#define SR_RING 10
#define SR_UROWS 128
#define SR_UBYTES (SR_UROWS * G7_ROW_BYTES)
#define SR_LDS (SR_RING * SR_UBYTES)
#define SR_IPU (SR_UROWS / 32)                  // DMA instructions per wave and unit

// The pass of sim_stream_reg_kernel (below) for 1088 <= d <= 2048 (round 7), its QB = 16 body.  A 32-query block at d = 2048 is 128 KiB, a
// wave's whole register file; a SIXTEEN-query block on 16 x 16 x 32 MFMAs is d / 8 registers, 256 at d = 2048, and its accumulators are 4
// registers per 16-row block:
//     NB = 1 (Q <= 16)    the four waves share the block and take 32 rows of a unit each (two 16-row blocks)
//     NB = 2 (Q <= 32)    waves 0, 2 / 1, 3 hold block 0 / 1 and take 64 rows each
//     NB = 4 (Q <= 64)    one block per wave, every wave takes all 128 rows
// Operand A = index rows (lane: row lane & 15, k 8 (lane >> 4) + j of the 32-wide sub-step), B = the query block (same map), so
// acc[rt][r] = <row 16 rt + 4 (lane >> 4) + r of the wave's share, query 16 nb + (lane & 15)>: the 16 x 16 x 32 MFMA's own layout.
// Ring, DMA swizzle (row r keeps source chunk c at c ^ ((r >> 1) & 7); r & 15 = lane & 15 here), non-temporal stream, split append and
// end-of-launch retire are those of the 32-query body; a K step is two sub-steps instead of four, and a lane has ONE list (its query) for
// all its 8 NB scores of a tile, so one atomic per lane and tile.  Registers: the 4 RB accumulators are pinned into the accumulation half
// with the fragments of the first 32 - NB K steps (8 registers each), the last NB K steps' fragments into the other half.
template <typename T, int NB>
__device__ __forceinline__ void sim_stream_reg16_body(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries, int64_t nq, int64_t d,
    const float* __restrict__ thr, u64* __restrict__ keys, unsigned* __restrict__ cnt, int nt) {
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int NKMAX = SCAN_NKMAX16;
  constexpr int RB = 2 * NB;                     // 16-row blocks per wave and unit: 4 / NB waves share a query block
  constexpr int NVK = NB;                        // K steps whose query fragments live in VGPRs: 8 registers each, 4 RB accumulators
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nk = (int)((d * 2) / G7_ROW_BYTES);
  const int64_t ntiles = nrows / SR_UROWS;
  const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
  if (my_tiles <= 0) return;
  const int units = my_tiles * nk;
  const uint32_t lds0 = g7_lds_addr(smem);
  const int quad = lane >> 4, l15 = lane & 15, key = l15 >> 1;
  const int nb = wave % NB, rgroup = wave / NB;   // this wave's query block and its share of a unit's rows

  frag_t bq[NKMAX][2];
  {
    const int qr = nb * 16 + l15;
    const int rr = qr < nq ? qr : (int)nq - 1;                  // padding rows repeat the last query (their threshold is +inf)
    const T* qrow = queries + (int64_t)rr * d + quad * 8;
#pragma unroll
    for (int ks = 0; ks < NKMAX; ++ks)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
        bq[ks][kk] = ks < nk ? *(const frag_t*)(qrow + ks * 64 + kk * 32) : __builtin_bit_cast(frag_t, z4);
      }
  }
  const float th = nb * 16 + l15 < nq ? thr[nb * 16 + l15] : __builtin_inff();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // before the first hand-counted DMA: nothing of the compiler's is in flight
#pragma unroll
  for (int ks = 0; ks < NKMAX - NVK; ++ks)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) asm volatile("" : "+a"(bq[ks][kk]));
#pragma unroll
  for (int ks = NKMAX - NVK; ks < NKMAX; ++ks)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) asm volatile("" : "+v"(bq[ks][kk]));

  uint32_t off[SR_IPU];
#pragma unroll
  for (int i = 0; i < SR_IPU; ++i) {
    const int r = (i * 4 + wave) * 8 + (lane >> 3);
    off[i] = (uint32_t)(r * d * 2) + ((((lane & 7) ^ ((r >> 1) & 7))) << 4);
  }
  const char* i_base = (const char*)(rows + (int64_t)blockIdx.x * SR_UROWS * d);
  const int64_t i_tile_step = (int64_t)gridDim.x * SR_UROWS * d * 2 - (int64_t)nk * G7_ROW_BYTES;   // last K step of a tile -> first of the next
  int i_ks = 0, i_slot = 0, issued = 0;
  auto issue = [&]() {
    const char* base = i_base;
    const uint32_t dst = lds0 + i_slot * SR_UBYTES + wave * 1024;
    if (nt) {
#pragma unroll
      for (int i = 0; i < SR_IPU; ++i) g7_dma_nt(base, off[i], dst + i * 4096);
    } else {
#pragma unroll
      for (int i = 0; i < SR_IPU; ++i) g7_dma(base, off[i], dst + i * 4096);
    }
    i_base += G7_ROW_BYTES;
    if (++i_ks == nk) { i_ks = 0; i_base += i_tile_step; }
    if (++i_slot == SR_RING) i_slot = 0;
    ++issued;
  };
  for (int u = 0; u < SR_RING - 1; ++u)
    if (u < units) issue();

  const int arow = (rgroup * (16 * RB) + l15) * G7_ROW_BYTES;    // + rt * 16 rows
  f32x4_t acc[RB];
#pragma unroll
  for (int rt = 0; rt < RB; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[rt][r] = 0.f;
  f32x4_t sh[RB];                                                // the previous tile's scores while its list position is in flight
  unsigned pn = 0, ppos = 0;
  bool pend = false;                                             // (wave-uniform) a tile's appends are in flight
  int64_t ptile = 0;
  int since = 0;                                                 // units issued since its atomics
  const int qi = nb * 16 + l15;
  auto retire = [&]() {
    if (since >= 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(ppos));                               // (the result is read after the wait)
    if (pn) {
      const uint32_t id0 = row_base + (uint32_t)(ptile * SR_UROWS) + rgroup * (16 * RB) + 4 * quad;
      unsigned pos = ppos;
      u64* const kq = keys + (int64_t)qi * SORT_CAP;
#pragma unroll
      for (int rt = 0; rt < RB; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (sh[rt][r] >= th) {
            if (pos < SORT_CAP) kq[pos] = pack_key(sh[rt][r], id0 + rt * 16 + r);
            ++pos;
          }
    }
    pend = false;
  };
  int c_slot = 0, u = 0;
  int64_t tile = blockIdx.x;
  frag_t a[2][RB];
  for (int ti = 0; ti < my_tiles; ++ti) {
#pragma unroll
    for (int ks = 0; ks < NKMAX; ++ks) {
      if (ks < nk) {                                             // wave-uniform
        const int younger = issued - 1 - u;
        if (younger == SR_RING - 2) G7_WAIT_VM((SR_RING - 2) * SR_IPU);
        else G7_WAIT_VM(0);
        __builtin_amdgcn_s_barrier();                            // ... for every wave; and unit u - 1 has been read by all
        if (issued < units) { issue(); ++since; }                // into the slot of unit u - 1
        const char* ua = smem + c_slot * SR_UBYTES + arow;
#pragma unroll
        for (int rt = 0; rt < RB; ++rt) a[0][rt] = *(const frag_t*)(ua + rt * 16 * G7_ROW_BYTES + ((quad ^ key) << 4));
        G7_FENCE_();
#pragma unroll
        for (int rt = 0; rt < RB; ++rt) a[1][rt] = *(const frag_t*)(ua + rt * 16 * G7_ROW_BYTES + (((4 | quad) ^ key) << 4));
        G7_FENCE_();
#pragma unroll
        for (int rt = 0; rt < RB; ++rt) Mma16c<T>::mma(a[0][rt], bq[ks][0], acc[rt]);
        G7_FENCE_();
#pragma unroll
        for (int rt = 0; rt < RB; ++rt) Mma16c<T>::mma(a[1][rt], bq[ks][1], acc[rt]);
        G7_FENCE_();
#pragma unroll
        for (int rt = 0; rt < RB; ++rt) asm volatile("" : "+a"(acc[rt]));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (++c_slot == SR_RING) c_slot = 0;
        ++u;
        if (ks == 3 && pend) retire();                           // the previous tile's appends: positions are back by now
      }
#pragma unroll
      for (int rt = 0; rt < RB; ++rt) asm volatile("" : "+a"(acc[rt]));   // (also where the skipped and the taken K step meet)
    }
    unsigned n = 0;
#pragma unroll
    for (int rt = 0; rt < RB; ++rt) {
      sh[rt] = acc[rt];
#pragma unroll
      for (int r = 0; r < 4; ++r) { n += sh[rt][r] >= th ? 1u : 0u; acc[rt][r] = 0.f; }
    }
    pn = n;
    if (n) {
      unsigned* const cp = cnt + qi;
      asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=&v"(ppos) : "v"(cp), "v"(n) : "memory");
    }
    if (__builtin_amdgcn_ballot_w64(n != 0) != 0) { pend = true; ptile = tile; since = 0; }
    tile += gridDim.x;
  }
  if (pend) { since = 0; retire(); }
  G7_WAIT_VM(0);
}

// DBG (timing probes only, OM_OPT_SEARCH_DEBUG bits 3 / 4; the results are wrong): 1 = every second MFMA sub-step skipped (does
// the pass's time follow its matrix-core work?), 2 = no MFMA at all
// NKMAX (round 7): the K steps compiled in.  12 serves 256 <= d <= 768 and is the kernel above, instruction for instruction.  16 serves
// 832 <= d <= 1024: the query block is then 256 registers, the whole accumulation half, and the accumulators pinned there as well would
// have no home.  So the fragments of the last NVK = NB K steps (16 registers each, as many as the 16 NB accumulators need) are pinned into
// the OTHER half -- the matrix core reads B from either -- which holds 8 NB row-fragment and 16 NB shadow registers besides: 64 / 106 /
// 192 VGPRs and 256 AGPRs for NB = 1 / 2 / 4, no scratch, and no v_accvgpr move in the unit loop.
// QB (round 7): queries per resident block.  16 with NKMAX = 32 is the body above (1088 <= d <= 2048), 32 the one below.
template <typename T, int NB, int DBG = 0, int NKMAX = SCAN_NKMAX32_NARROW, int QB = 32>
__global__ __launch_bounds__(G6_THREADS) void sim_stream_reg_kernel(
    const T* __restrict__ rows, int64_t nrows, uint32_t row_base, const T* __restrict__ queries, int64_t nq, int64_t d,
    const float* __restrict__ thr, u64* __restrict__ keys, unsigned* __restrict__ cnt, int nt) {
  if constexpr (QB == 16) {
    static_assert(NKMAX == SCAN_NKMAX16 && DBG == 0, "the 16-query body compiles 32 K steps and has no probe variants");
    sim_stream_reg16_body<T, NB>(rows, nrows, row_base, queries, nq, d, thr, keys, cnt, nt);
    return;
  }
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int RBW = NB;                        // 32-row blocks per wave and unit: 4 / NB waves share a query block
  constexpr int NVK = NKMAX * 16 + RBW * 16 > 256 ? (NKMAX * 16 + RBW * 16 - 256) / 16 : 0;      // K steps whose query fragments live in VGPRs
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nk = (int)((d * 2) / G7_ROW_BYTES);
  const int64_t ntiles = nrows / SR_UROWS;
  const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
  if (my_tiles <= 0) return;
  const int units = my_tiles * nk;
  const uint32_t lds0 = g7_lds_addr(smem);
  const int half = lane >> 5, l31 = lane & 31, key = (l31 >> 1) & 7;
  const int nb = wave % NB, rgroup = wave / NB;   // this wave's query block and its share of a unit's rows

  // the wave's query block, in MFMA fragment order, straight from global memory (once per launch)
  frag_t bq[NKMAX][4];
  {
    const int qr = nb * 32 + l31;
    const int rr = qr < nq ? qr : (int)nq - 1;                  // padding rows repeat the last query (their threshold is +inf)
    const T* qrow = queries + (int64_t)rr * d + half * 8;
#pragma unroll
    for (int ks = 0; ks < NKMAX; ++ks)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
        bq[ks][kk] = ks < nk ? *(const frag_t*)(qrow + ks * 64 + kk * 16) : __builtin_bit_cast(frag_t, z4);
      }
  }
  const float th = thr[nb * 32 + l31];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // before the first hand-counted DMA: nothing of the compiler's is in flight
#pragma unroll
  for (int ks = 0; ks < NKMAX - NVK; ++ks)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+a"(bq[ks][kk]));    // in the accumulation half of the register file (the matrix core
                                                                            // reads B from there as well): 192 + 16 NB of its 256; the other half stays free for the row fragments
#pragma unroll
  for (int ks = NKMAX - NVK; ks < NKMAX; ++ks)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(bq[ks][kk]));    // (NKMAX = 16 only: see above)

  // DMA offsets of a unit: instruction i of this wave moves rows (i*4 + wave)*8 .. +7, lane -> row (lane >> 3),
  // physical chunk (lane & 7) <- source chunk (lane & 7) ^ ((row >> 1) & 7)
  uint32_t off[SR_IPU];
#pragma unroll
  for (int i = 0; i < SR_IPU; ++i) {
    const int r = (i * 4 + wave) * 8 + (lane >> 3);
    off[i] = (uint32_t)(r * d * 2) + ((((lane & 7) ^ ((r >> 1) & 7))) << 4);
  }
  // issue cursor: (source address, K step, slot) of the next unit to fetch -- advanced incrementally (the per-unit scalar
  // work counts: at two and four resident blocks a unit's instruction path is as long as its share of the HBM stream)
  const char* i_base = (const char*)(rows + (int64_t)blockIdx.x * SR_UROWS * d);
  const int64_t i_tile_step = (int64_t)gridDim.x * SR_UROWS * d * 2 - (int64_t)nk * G7_ROW_BYTES;   // last K step of a tile -> first of the next
  int i_ks = 0, i_slot = 0, issued = 0;
  auto issue = [&]() {
    const char* base = i_base;
    const uint32_t dst = lds0 + i_slot * SR_UBYTES + wave * 1024;
    if (nt) {                                                    // (wave-uniform) the index is read once per pass, by one CU
#pragma unroll
      for (int i = 0; i < SR_IPU; ++i) g7_dma_nt(base, off[i], dst + i * 4096);
    } else {
#pragma unroll
      for (int i = 0; i < SR_IPU; ++i) g7_dma(base, off[i], dst + i * 4096);
    }
    i_base += G7_ROW_BYTES;
    if (++i_ks == nk) { i_ks = 0; i_base += i_tile_step; }
    if (++i_slot == SR_RING) i_slot = 0;
    ++issued;
  };
  for (int u = 0; u < SR_RING - 1; ++u)
    if (u < units) issue();

  const int arow = (rgroup * (32 * RBW) + l31) * G7_ROW_BYTES;   // + rt * 32 rows
  f32x16_t acc[RBW];
#pragma unroll
  for (int rt = 0; rt < RBW; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
  // Appends are split around the next tile.  A 32 x 32 score block holds a survivor about once per tile and query block, and
  // the list position comes from a returning atomic: ~1.1 us under a streaming load (MI355X_MICROARCH.md "dequeue"), during
  // which this wave issues nothing -- written in line (returning atomic, then the stores) that was RBW round trips per
  // 8-12 us tile, and the compiler's wait for the result is vmcnt(0): the whole ring.  Instead the tile's scores move to a
  // shadow register set, the atomics of all its blocks leave together (inline assembly: invisible to the compiler's
  // counting), and four units into the NEXT tile -- 16 younger DMA instructions in the in-order queue -- the positions are
  // there and the keys are stored.
  f32x16_t sh[RBW];
  unsigned pn[RBW], ppos[RBW];
#pragma unroll
  for (int rt = 0; rt < RBW; ++rt) { pn[rt] = 0; ppos[rt] = 0; }
  bool pend = false;                                             // (wave-uniform) a tile's appends are in flight
  int64_t ptile = 0;
  int since = 0;                                                 // units issued since its atomics
  const int qi = nb * 32 + l31;
  auto retire = [&]() {
    // every atomic has returned once at most the younger operations are outstanding
    if (since >= 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int rt = 0; rt < RBW; ++rt) asm volatile("" : "+v"(ppos[rt]));      // (the results are read after the wait)
#pragma unroll
    for (int rt = 0; rt < RBW; ++rt) {
      if (pn[rt]) {
        const uint32_t id0 = row_base + (uint32_t)(ptile * SR_UROWS) + rgroup * (32 * RBW) + rt * 32 + 4 * half;
        unsigned pos = ppos[rt];
        u64* const kq = keys + (int64_t)qi * SORT_CAP;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (sh[rt][r] >= th) {
            if (pos < SORT_CAP) kq[pos] = pack_key(sh[rt][r], id0 + (r & 3) + 8 * (r >> 2));
            ++pos;
          }
      }
    }
    pend = false;
  };
  int c_slot = 0, u = 0;
  int64_t tile = blockIdx.x;
  // Round 4, what the pass's time is made of (timing probes with half / none of the MFMAs compiled out, DBG above;
  // profiles/r04_probe9_small_batch_mfma_share.log): with HALF the matrix-core work the pass runs at the no-MFMA time (2.16-2.40 ms
  // whatever the batch: the HBM stream), with all of it +0.2 ms (Q = 1) to +1.0 ms (Q = 64, 128) -- a threshold, not a slope,
  // and not the clock round 3 suspected.  Reading the first fragments of unit u + 1 under the last MFMAs of unit u (the
  // barrier of u certifying u + 1 as well, eight units in flight instead of nine) changed nothing (Q = 64 3.20, Q = 128 3.32 ms:
  // profiles/r04_probe10_small_batch_cross_unit_prefetch.log) and was removed: the chain that is too long for a unit's share of
  // the stream is the four dependent read -> MFMA stages themselves.
  frag_t a[2][RBW];
  for (int ti = 0; ti < my_tiles; ++ti) {
#pragma unroll
    for (int ks = 0; ks < NKMAX; ++ks) {
      if (ks < nk) {                                             // wave-uniform
        // unit u landed; up to RING - 1 younger units may be in flight
        const int younger = issued - 1 - u;
        // steady state: the eight units behind unit u are in flight (the ninth is issued behind the barrier below).  While
        // the ring drains -- the last units of a launch -- everything outstanding is waited for: a ladder of exact counts
        // compiled to ~40 scalar instructions and a dozen taken branches per unit, a third of what a unit may cost at all
        if (younger == SR_RING - 2) G7_WAIT_VM((SR_RING - 2) * SR_IPU);
        else G7_WAIT_VM(0);
        __builtin_amdgcn_s_barrier();                            // ... for every wave; and unit u - 1 has been read by all
        if (issued < units) { issue(); ++since; }                // into the slot of unit u - 1
        const char* ua = smem + c_slot * SR_UBYTES + arow;
        // the row fragments of sub-step kk + 1 are read under the MFMAs of sub-step kk (order pinned: left alone the
        // compiler reads two fragments, waits, multiplies, reads two ... and every LDS round trip is exposed)
#pragma unroll
        for (int rt = 0; rt < RBW; ++rt) a[0][rt] = *(const frag_t*)(ua + rt * 32 * G7_ROW_BYTES + ((half ^ key) << 4));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          G7_FENCE_();
          if (kk < 3) {
            const int slot = ((((kk + 1) << 1) | half) ^ key) << 4;
#pragma unroll
            for (int rt = 0; rt < RBW; ++rt) a[(kk + 1) & 1][rt] = *(const frag_t*)(ua + rt * 32 * G7_ROW_BYTES + slot);
          }
          G7_FENCE_();
#pragma unroll
          for (int rt = 0; rt < RBW; ++rt)
            if (DBG == 0 || (DBG == 1 && !(kk & 1))) MmaOps<T>::mma(a[kk & 1][rt], bq[ks][kk], acc[rt]); // acc[rt][r]: row 8(r>>2) + 4 half + (r&3) of the 32-row block, query 32 nb + l31
        }
        G7_FENCE_();
        // the accumulators' home is the AGPR file: without the pin the compiler keeps them in VGPRs across the (wave-uniform)
        // K-step branches and copies all of them in and out around every unit's MFMAs -- 32 RBW v_accvgpr moves per unit that
        // also wait for the matrix core to drain (rocprofv3: 88 VALU instructions per unit, the pass 35 / 55 % longer with two /
        // four resident blocks than with one)
#pragma unroll
        for (int rt = 0; rt < RBW; ++rt) asm volatile("" : "+a"(acc[rt]));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (++c_slot == SR_RING) c_slot = 0;
        ++u;
        if (ks == 3 && pend) retire();                           // the previous tile's appends: positions are back by now
      }
#pragma unroll
      for (int rt = 0; rt < RBW; ++rt) asm volatile("" : "+a"(acc[rt]));   // (also where the skipped and the taken K step meet)
    }
    // (the dispatcher sends d < 256 -- fewer than four K steps, no retire point inside a tile -- to the generic kernels)
    bool any = false;
#pragma unroll
    for (int rt = 0; rt < RBW; ++rt) {
      sh[rt] = acc[rt];
      unsigned n = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) n += sh[rt][r] >= th ? 1u : 0u;
      pn[rt] = n;
      // one atomic per lane and block, not per survivor (with one query every append of a round lands on one counter)
      if (n) {
        unsigned* const cp = cnt + qi;
        asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=&v"(ppos[rt]) : "v"(cp), "v"(n) : "memory");
      }
      any = any || __builtin_amdgcn_ballot_w64(n != 0) != 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
    }
    if (any) { pend = true; ptile = tile; since = 0; }
    tile += gridDim.x;
  }
  if (pend) { since = 0; retire(); }
  G7_WAIT_VM(0);
}

// append a dense score block S[q, 0:n] (rows row_base..) to every list
__global__ void append_dense_kernel(const float* __restrict__ S, int64_t ldS, int n,
                                    uint32_t row_base, u64* __restrict__ keys,
                                    unsigned* __restrict__ cnt) {
  const int64_t q = blockIdx.x;
  const unsigned base = cnt[q];
  for (int j = threadIdx.x; j < n; j += blockDim.x)
    if (base + j < SORT_CAP) keys[q * SORT_CAP + base + j] = pack_key(S[q * ldS + j], row_base + j);
  __syncthreads();
  if (threadIdx.x == 0) cnt[q] = base + n;
}

// flag[0] |= any list overflowed; with qstat also the per-query bits: overflow, and a list longer than the `cover` slots a re-score reaches
__global__ void check_overflow_kernel(const unsigned* __restrict__ cnt, int64_t nq,
                                      unsigned* __restrict__ flag, unsigned* __restrict__ qstat, unsigned cover) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const unsigned n = cnt[q];
  if (n > SORT_CAP) atomicOr(flag, 1u);
  if (qstat) {
    const unsigned bits = (n > SORT_CAP ? QSTAT_OVERFLOW : 0u) | (n > cover ? QSTAT_COVER : 0u);
    if (bits) atomicOr(qstat + q, bits);
  }
}
__global__ void restore_cnt_kernel(unsigned* __restrict__ cnt, const unsigned* __restrict__ prev,
                                   int64_t nq) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) cnt[q] = prev[q];
}

// descending bitonic sort of P (power of two) keys in LDS
__device__ inline void bitonic_sort_desc(u64* s, int P, int tid, int nthr) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += nthr) {
        const int x = i ^ j;
        if (x > i) {
          const u64 a = s[i], b = s[x];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) { s[i] = b; s[x] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// Sort one list, keep the best k (exact mode) or everything within margin[q] of the k-th
// best (certified f16 mode), publish the new threshold.  flag[1] = max list length,
// flag[2] |= a certified list outgrew LIST_MAX, or the certified margin is not finite.
__global__ __launch_bounds__(SORT_THREADS) void select_kernel(
    u64* __restrict__ keys, unsigned* __restrict__ cnt, unsigned* __restrict__ cnt_prev,
    float* __restrict__ thr, const float* __restrict__ margin, int k, unsigned* __restrict__ flag,
    unsigned* __restrict__ qstat) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* s = (u64*)smem;
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  unsigned n = cnt[q];
  if (n > SORT_CAP) {
    n = SORT_CAP;
    if (qstat && tid == 0) atomicOr(qstat + q, QSTAT_OVERFLOW);
  }
  int P = 2;
  while (P < (int)n) P <<= 1;
  u64* list = keys + q * SORT_CAP;
  for (int i = tid; i < P; i += SORT_THREADS) s[i] = i < (int)n ? list[i] : 0ull;
  __syncthreads();
  bitonic_sort_desc(s, P, tid, SORT_THREADS);

  unsigned& keep_s = *(unsigned*)(smem + SORT_CAP * 8);  // all LDS in the one dynamic array
  if (tid == 0) keep_s = 0;
  __syncthreads();
  float th = -INFINITY;
  unsigned keep;
  if (!margin) {
    keep = n < (unsigned)k ? n : (unsigned)k;
    if (n >= (unsigned)k) th = key_score(s[k - 1]);
  } else {
    if (n >= (unsigned)k) {
      th = key_score(s[k - 1]) - 2.0f * margin[q];
      unsigned local = 0;
      for (int i = tid; i < (int)n; i += SORT_THREADS) local += key_score(s[i]) >= th ? 1u : 0u;
      atomicAdd(&keep_s, local);
      __syncthreads();
      keep = keep_s;
    } else {
      keep = n;
    }
  }
  for (int i = tid; i < (int)keep; i += SORT_THREADS) list[i] = s[i];
  if (tid == 0) {
    cnt[q] = keep;
    cnt_prev[q] = keep;
    thr[q] = th;
    atomicMax(flag + 1, keep);
    const bool wide = keep > LIST_MAX || (margin && !(margin[q] < INFINITY));
    if (wide) atomicOr(flag + 2, 1u);
    if (qstat && margin && wide) atomicOr(qstat + q, QSTAT_WIDE);
  }
}

// The per-round selection WITHOUT a sort: a round only needs the new threshold (the k-th best score so far) and the
// list cut down to what can still matter; order is irrelevant until the very end.  Radix select over the 32 score bits
// of the keys (4 passes of a 256-bin histogram in LDS, suffix sums by wave shuffles), then an unordered compaction of
// everything >= the cut (exact mode: the k-th score, ties included; certified mode: k-th - 2 margin).  ~30x cheaper
// than the 8192-key bitonic sort it replaces between rounds (profiles/r01_bench_v8_kernel_stats.csv: 8 x 2.3 ms).
__global__ __launch_bounds__(256) void select_radix_kernel(
    u64* __restrict__ keys, unsigned* __restrict__ cnt, float* __restrict__ thr, const float* __restrict__ margin,
    int k, unsigned* __restrict__ flag, int cap, unsigned* __restrict__ qstat) {
  // cap: keys the LDS copy holds (SORT_CAP, or less when the host expects short lists: 64 KiB of LDS per workgroup
  // leaves two workgroups per CU, 32 KiB four -- this kernel is a chain of barriers and wants the occupancy)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* s = (u64*)smem;
  unsigned* hist = (unsigned*)(smem + (size_t)cap * 8);       // 256 bins
  unsigned* misc = hist + 256;                                // [0] bucket, [1] remaining, [2] keep counter, [4..7] wave totals
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned n = cnt[q];
  if (n > SORT_CAP) {                                        // appends beyond the capacity were dropped: the round is void
    if (tid == 0) {
      atomicOr(flag, 1u);                                    // (sticky; the step-by-step loop uses check_overflow_kernel)
      if (qstat) atomicOr(qstat + q, QSTAT_OVERFLOW);
    }
    n = SORT_CAP;
  }
  // (a margin that is not finite -- a value of the index or of the query beyond f16 -- certifies nothing: inf - inf is a NaN cut that
  // keeps no key.  flag[2] as well: om_sim_topk has no qstat, and a list cut down to nothing would never outgrow LIST_MAX)
  if (margin && tid == 0 && !(margin[q] < INFINITY)) {
    atomicOr(flag + 2, 1u);
    if (qstat) atomicOr(qstat + q, QSTAT_WIDE);
  }
  u64* list = keys + q * SORT_CAP;
  // a list longer than the LDS copy (rare: the host sizes `cap` with a 2x margin) is read from global memory in every
  // pass (64 KiB, L2-resident) and only the survivors are staged
  const bool staged = n <= (unsigned)cap;
  const u64* src = staged ? (const u64*)s : (const u64*)list;
  if (staged)
    for (unsigned i = tid; i < n; i += 256) s[i] = list[i];
  if (tid == 0) misc[2] = 0;
  __syncthreads();
  if (n <= (unsigned)k) {                                     // nothing to cut: keep everything
    float mn = INFINITY;
    for (unsigned i = tid; i < n; i += 256) mn = fminf(mn, key_score(src[i]));
    mn = -wave_max(-mn);
    float* wmin = (float*)(misc + 4);
    if (lane == 0) wmin[wave] = mn;
    __syncthreads();
    if (tid == 0) {
      float th = -INFINITY;                                   // fewer than k candidates so far: no threshold yet
      if (n == (unsigned)k) {                                 // exactly k: the k-th best is the minimum
        const float m4 = fminf(fminf(wmin[0], wmin[1]), fminf(wmin[2], wmin[3]));
        th = margin ? m4 - 2.0f * margin[q] : m4;
      }
      thr[q] = th;
      atomicMax(flag + 1, n);
    }
    return;
  }
  uint32_t prefix = 0, mask = 0;
  unsigned remaining = (unsigned)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    // (round 6 probe: one LDS atomic per DISTINCT bin of a wave for the two high bytes -- where nearly every lane names the same bin -- ran
    // 170 us per launch against 152: the same-address atomics are not what this kernel waits for; it is 3 % of a search)
    for (unsigned i = tid; i < n; i += 256) {
      const uint32_t v = (uint32_t)(src[i] >> 32);
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    // suffix sums S[t] = sum_{b >= t} hist[b]: inside each wave by shuffles, across waves through misc[4..7]
    const unsigned c = hist[tid];
    unsigned suf = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += up;
    }
    if (lane == 0) misc[4 + wave] = suf;                      // total of this wave's 64 bins
    __syncthreads();
    unsigned above = 0;                                       // bins of higher waves
    for (int w = wave + 1; w < 4; ++w) above += misc[4 + w];
    const unsigned S = suf + above, Snext = S - c;            // S[t] and S[t+1]
    if (S >= remaining && Snext < remaining) { misc[0] = (unsigned)tid; misc[1] = remaining - Snext; }
    __syncthreads();
    prefix |= misc[0] << shift;
    mask |= 255u << shift;
    remaining = misc[1];
    __syncthreads();
  }
  const float kth = orderable_f32(prefix);
  const float cut = margin ? kth - 2.0f * margin[q] : kth;
  if (staged) {
    for (unsigned i = tid; i < n; i += 256) {
      const u64 key = s[i];
      if (key_score(key) >= cut) list[atomicAdd(&misc[2], 1u)] = key;
    }
    __syncthreads();
  } else {                                                    // in place is not safe without the copy: survivors via LDS
    for (unsigned i = tid; i < n; i += 256) {
      const u64 key = list[i];
      if (key_score(key) >= cut) {
        const unsigned pos = atomicAdd(&misc[2], 1u);
        if (pos < (unsigned)cap) s[pos] = key;
      }
    }
    __syncthreads();
    unsigned kept = misc[2];                                  // one value for the whole workgroup (no writer until the barrier below)
    if (kept > (unsigned)cap) {                               // masses of ties (duplicated rows): treated as an overflow
      if (tid == 0) {
        atomicOr(flag, 1u);
        if (qstat) atomicOr(qstat + q, QSTAT_OVERFLOW);
      }
      kept = (unsigned)cap;
    }
    for (unsigned i = tid; i < kept; i += 256) list[i] = s[i];
    __syncthreads();
    if (tid == 0) misc[2] = kept;                             // read back by this same thread below
  }
  if (tid == 0) {
    const unsigned keep = misc[2];
    cnt[q] = keep;
    thr[q] = cut;
    atomicMax(flag + 1, keep);
    if (margin && keep > LIST_MAX) {
      atomicOr(flag + 2, 1u);
      if (qstat) atomicOr(qstat + q, QSTAT_WIDE);
    }
  }
}

// per-query certified margin and bf16 copy of the queries
__global__ __launch_bounds__(256) void query_prep_kernel(const float* __restrict__ q,
                                                         f16_t* __restrict__ qb,
                                                         float* __restrict__ margin,
                                                         const float* __restrict__ stats,
                                                         int64_t nq, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq) {            // padding of the query panel up to a whole 256-query tile: zero rows (the generation-7 scan reads them)
    if (row < (nq + 255) / 256 * 256)
      for (int c = lane; c < d; c += 64) qb[row * d + c] = (f16_t)0.f;
    return;
  }
  float n2 = 0.f, e2 = 0.f, b2 = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = q[row * d + c];
    const f16_t r = (f16_t)v;
    const float rv = (float)r;
    qb[row * d + c] = r;
    n2 += v * v; e2 += (v - rv) * (v - rv); b2 += rv * rv;
  }
  n2 = wave_sum(n2); e2 = wave_sum(e2); b2 = wave_sum(b2);
  if (lane == 0) {
    const float qn = sqrtf(n2), qe = sqrtf(e2), qbn = sqrtf(b2);
    const float Ep = stats[0], Pn = stats[1];
    // f32 accumulation of the 16-bit scan and of the f32 re-score, bounded by DEPTH (the additions one product takes part in), not by
    // the d additions of the whole sum -- 3 d 2^-24 was 46 % of the margin at d = 2048 and sent searches a 16-bit scan serves to the
    // float32 one.  Products of two f16 values are exact in f32.  Scan (and the dense bootstrap's GEMM): at most the 32 k values of one
    // MFMA (16 x 16 x 32; 16 of 32 x 32 x 16), then one addition per later MFMA of the chain (d / 16 at most), each taken at 2^-23 -- a
    // matrix core may truncate where the VALU rounds.  Re-score: a lane's chain of d / 64 fmaf, six butterfly additions, + 2 spare.
    const float depth = 2.0f * (32.0f + (float)d / 16.0f) + ((float)d / 64.0f + 8.0f);
    const float slop = depth * 5.9604645e-8f * fmaxf(qn, qbn) * (Pn + Ep);
    margin[row] = 1.01f * (qn * Ep + qe * Pn) + slop;
  }
}

// The exact f32 score of the re-score and of the on-device redo: each lane's fmaf chain over columns c = lane * 4, step 256, then the
// butterfly sum -- every lane returns the same value, and the same (query, row) gives the same bits wherever it is computed.
// TRow: the row's storage, float or f16_t (OM_SEARCH_F16_ONLY: one 8-byte load of four halves, widened -- exactly -- to float32; the
// column -> lane map and the chain are the float32 form's, so a float16 row and a float32 row holding the same values give the same bits).
__device__ __forceinline__ float4 rescore_load4(const float* __restrict__ p) { return *(const float4*)p; }
__device__ __forceinline__ float4 rescore_load4(const f16_t* __restrict__ p) {
  typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
  const f16x4_t h = *(const f16x4_t*)p;
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
template <typename TRow>
__device__ __forceinline__ float rescore_dot(const float* __restrict__ qv, const TRow* __restrict__ pv, int d, int lane) {
  float acc = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 a = *(const float4*)(qv + c);
    const float4 b = rescore_load4(pv + c);
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
  }
  return wave_sum(acc);
}

// exact f32 re-score of every surviving candidate: one wavefront per (query, slot)
template <typename TRow>
__global__ __launch_bounds__(256) void rescore_kernel(const float* __restrict__ q,
                                                      const TRow* __restrict__ index,
                                                      u64* __restrict__ keys,
                                                      const unsigned* __restrict__ cnt, int d) {
  const int64_t qi = blockIdx.y;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (slot >= (int)cnt[qi]) return;
  u64* kp = keys + qi * SORT_CAP + slot;
  const uint32_t row = key_payload(*kp);
  const float acc = rescore_dot(q + qi * d, index + (int64_t)row * d, d, lane);
  if (lane == 0) *kp = pack_key(acc, row);
}

// The same re-score on a FIXED grid (the asynchronous entry above 128 queries: the host does not know the list lengths, and a grid of
// nq x cover workgroups sized for the longest list the estimate allows would launch millions of empty ones).  Work item (query, j) is
// the slots j, j + RESCORE_SPLIT, ... < cnt[query]; the grid's wavefronts stride over the items.
#define RESCORE_SPLIT 32
template <typename TRow>
__global__ __launch_bounds__(256) void rescore_strided_kernel(const float* __restrict__ q, const TRow* __restrict__ index,
                                                              u64* __restrict__ keys, const unsigned* __restrict__ cnt, int64_t nq, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < nq * RESCORE_SPLIT; item += nwaves) {
    const int64_t qi = item / RESCORE_SPLIT;
    unsigned n = cnt[qi];
    if (n > SORT_CAP) n = SORT_CAP;
    for (unsigned slot = (unsigned)(item % RESCORE_SPLIT); slot < n; slot += RESCORE_SPLIT) {
      u64* kp = keys + qi * SORT_CAP + slot;
      const uint32_t row = key_payload(*kp);
      const float acc = rescore_dot(q + qi * d, index + (int64_t)row * d, d, lane);
      if (lane == 0) *kp = pack_key(acc, row);
    }
  }
}

// om_sim_topk_candidates: one wavefront per (query, candidate column) of the columns [col0, col0 + ncols) of cand [nq][pitch] -- the key
// pack_key(rescore_dot(query, row), row) appended to list q.  A value outside [0, N) is a hole: skipped, never followed.  The host keeps
// ncols <= CAND_BLOCK with at most K_MAX keys already in the list, so a slot always exists (the test on pos guards the memory all the same).
#define CAND_BLOCK 4096
static_assert(K_MAX + CAND_BLOCK <= SORT_CAP, "a list holds the kept k and one block of candidates");
template <typename TRow>
__global__ __launch_bounds__(256) void score_candidates_kernel(const float* __restrict__ q, const TRow* __restrict__ index, int64_t N, int d,
                                                               const int32_t* __restrict__ cand, int64_t pitch, int64_t col0, int ncols,
                                                               u64* __restrict__ keys, unsigned* __restrict__ cnt) {
  const int64_t qi = blockIdx.y;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= ncols) return;
  const int64_t row = cand[qi * pitch + col0 + j];     // (wave-uniform)
  if (row < 0 || row >= N) return;
  const float acc = rescore_dot(q + qi * d, index + row * d, d, lane);
  if (lane != 0) return;
  const unsigned pos = atomicAdd(cnt + qi, 1u);
  if (pos < SORT_CAP) keys[qi * SORT_CAP + pos] = pack_key(acc, (uint32_t)row);
}

__global__ void emit_kernel(const u64* __restrict__ keys, const unsigned* __restrict__ cnt, int k,
                            int64_t id_offset, float* __restrict__ out_scores,
                            int64_t* __restrict__ out_ids) {
  const int64_t q = blockIdx.x;
  const unsigned n = cnt[q];
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    if (j < (int)n) {
      const u64 key = keys[q * SORT_CAP + j];
      out_scores[q * k + j] = key_score(key);
      out_ids[q * k + j] = id_offset + (int64_t)key_payload(key);
    } else {
      out_scores[q * k + j] = -3.4028235e38f;  // faiss pads (D,I) with (-FLT_MAX, -1)
      out_ids[q * k + j] = -1;
    }
  }
}

__global__ void init_lists_kernel(unsigned* cnt, unsigned* cnt_prev, float* thr, int64_t nq, unsigned* flag) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < 16) flag[q] = 0;                                            // the 64-byte flag block (one launch less than a memset)
  if (q < nq) { cnt[q] = 0; cnt_prev[q] = 0; thr[q] = -INFINITY; }
  else if (q < (nq + 255) / 256 * 256 + 256) thr[q] = INFINITY;       // queries that do not exist never have survivors
}

// ---- the row filters of om_sim_topk_filtered and om_sim_topk_filtered_multi ---------------------------------------------------------------
// A bitmap: bit r & 31 of word r >> 5 is row r of the shard; bits at and beyond N are never read as rows (count_allowed_kernel masks them,
// no scan names such a row, the redo stops at N).
__device__ __forceinline__ bool row_allowed(const uint32_t* __restrict__ allow, uint32_t row) { return (allow[row >> 5] >> (row & 31u)) & 1u; }

// Which bitmap a query is under.  bits == nullptr: no filter in the call.  per_query == 0 (om_sim_topk_filtered): every query under the one
// bitmap at `bits`.  per_query == 1 (om_sim_topk_filtered_multi): bitmap f is the words at bits + f * pitch, query q is under bitmap of[q]
// (of == nullptr: bitmap q); a value below 0 is "every row", one at or beyond n is "no row" and is never used as an address.
struct RowFilters {
  const uint32_t* bits;
  int64_t pitch, n;
  const int32_t* of;
  int per_query;
};
#define FILTER_EVERY_ROW (-1)
#define FILTER_NO_ROW (-2)
__device__ __forceinline__ int64_t filter_index(const RowFilters& F, int64_t q) {
  if (!F.bits) return FILTER_EVERY_ROW;
  if (!F.per_query) return 0;
  const int64_t f = F.of ? (int64_t)F.of[q] : q;
  return f < 0 ? FILTER_EVERY_ROW : (f >= F.n ? FILTER_NO_ROW : f);
}

// out[f] += rows bitmap f = blockIdx.y allows among [0, N): the rank of the redo's select is min(k, this), whatever count the host was told
__global__ __launch_bounds__(256) void count_allowed_kernel(const RowFilters F, int64_t N, unsigned* __restrict__ out) {
  const uint32_t* __restrict__ allow = F.bits + (int64_t)blockIdx.y * F.pitch;
  const int64_t words = (N + 31) / 32;
  unsigned c = 0;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t v = allow[w];
    if (w == words - 1 && (N & 31)) v &= (1u << (N & 31)) - 1u;
    c += (unsigned)__builtin_popcount(v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out + blockIdx.y, c);
}

// Drop before every selection: list q compacted IN PLACE to the keys whose row (the low 32 bits, complemented) the query's filter allows, in
// their order, so thresholds, margins, the LIST_MAX test and the re-score only ever see allowed rows.  One workgroup per query, 256 keys
// per step: every key of a step is in a register before the barrier, and a step writes only below what it has read (out <= base), so
// no staging copy is needed.  Position inside a step: wave ballot + the totals of the lower waves.  A list beyond SORT_CAP lost
// appends: clamped and marked here as the selections do, or the compaction would hide it from them.
// A query under no filter keeps its list (clamped and marked all the same); one whose filter allows no row ends with an empty list.
__global__ __launch_bounds__(256) void drop_disallowed_kernel(u64* __restrict__ keys, unsigned* __restrict__ cnt, const RowFilters F,
                                                              uint32_t nrows, unsigned* __restrict__ flag, unsigned* __restrict__ qstat) {
  __shared__ unsigned wtot[4];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f = filter_index(F, q);              // (workgroup-uniform)
  const uint32_t* __restrict__ allow = F.bits + (f > 0 ? f : 0) * F.pitch;
  unsigned n = cnt[q];
  if (n > SORT_CAP) {
    if (tid == 0) {
      atomicOr(flag, 1u);
      if (qstat) atomicOr(qstat + q, QSTAT_OVERFLOW);
    }
    n = SORT_CAP;
  }
  if (f < 0) {
    __syncthreads();                                 // every thread has read cnt[q]
    if (tid == 0) cnt[q] = f == FILTER_NO_ROW ? 0u : n;
    return;
  }
  u64* list = keys + q * SORT_CAP;
  unsigned out = 0;
  for (unsigned base = 0; base < n; base += 256) {
    const unsigned i = base + (unsigned)tid;
    u64 key = 0ull;
    bool ok = false;
    if (i < n) {
      key = list[i];
      const uint32_t row = key_payload(key);
      ok = row < nrows && row_allowed(allow, row);
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    const unsigned below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wtot[wave] = (unsigned)__builtin_popcountll(m);
    __syncthreads();                               // the step's keys are read, the wave totals written
    unsigned off = out;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (ok) list[off + below] = key;
    out += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();                               // the totals are read
  }
  __syncthreads();                                 // (an empty list: every thread has read cnt[q])
  if (tid == 0) cnt[q] = out;
}

// ---- on-device redo of the asynchronous entry ----------------------------------------------------------------------------------------
// The exact top-k of every query whose qstat is not zero, without a word to the host: an MSB-first radix select over the 64-bit keys
// pack_key(score, row) of ALL rows.  Ordering by that key is score descending, then row ascending, and no two keys tie -- so the k-th
// key T is unique, exactly min(k, N) keys are >= T whatever ties the scores have, and the number of tied groups does not matter.
// The host enqueues a FIXED chain (it does not know n_bad): compact -> begin -> REDO_PASSES x (histogram pass over the index -> pick)
// -> collect pass.  Every kernel reads n_bad first and returns at once when it is 0: with nothing to redo the chain is 15 empty launches.
// No device-wide barrier, no spin on a flag, no cooperative launch: the stream orders the passes.
//   pass      one launch on a fixed grid streams the f32 index once for ALL bad queries: a workgroup stages a tile of rows in LDS, then
//             loops over the bad queries (their vectors come from L2); a wavefront scores one (row, query) at a time with rescore_dot --
//             the same bits in every pass -- and counts the current digit of the keys whose higher digits equal the query's prefix;
//   pick      one workgroup: per bad query the digit that holds the remaining rank (suffix sums over the histogram, highest digit
//             first), the rank left inside it, and the histogram zeroed for the next pass;
//   collect   after the last pick the prefix IS T: one more pass writes every key >= T into the query's list from slot 0 and leaves
//             cnt = min(k, N).  The final select_kernel sorts the list like any other.
// Digits of 11 bits (the last one 9): six histogram passes and one collect pass over the index, 8 KiB of histogram per bad query.
#define REDO_BINS 2048
#define REDO_PASSES 6
#define REDO_TILE_BYTES 32768
#define REDO_RS_BAD 0         // rs[0]: queries to redo;  rs[1]: of those, with QSTAT_WIDE
#define REDO_RS_WIDE 1
#define REDO_RS_ALLOWED 2     // rs[2]: rows the filter allows among [0, N) (om_sim_topk_filtered: count_allowed_kernel; the multi entry counts into its own words)
__host__ __device__ inline int redo_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }      // 53, 42, 31, 20, 9, 0
__host__ __device__ inline int redo_width(int pass) { return pass < 5 ? 11 : 9; }

__global__ void async_init_kernel(unsigned* __restrict__ qstat, unsigned* __restrict__ rs, int64_t* __restrict__ status, int64_t nq) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) qstat[q] = 0;
  if (q < 16) rs[q] = 0;
  if (status && q < 8) status[q] = 0;            // status[6] turns 1 when the chain has finished (nullptr: om_sim_topk in OM_SEARCH_F16_ONLY reads flag / rs itself)
}

__global__ void redo_compact_kernel(const unsigned* __restrict__ qstat, int64_t nq, unsigned* __restrict__ rs, unsigned* __restrict__ bad) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const unsigned st = qstat[q];
  if (!st) return;
  bad[atomicAdd(rs + REDO_RS_BAD, 1u)] = (unsigned)q;
  if (st & QSTAT_WIDE) atomicAdd(rs + REDO_RS_WIDE, 1u);
}

// F, n_allowed: the call's row filters and the device's count of every bitmap's rows (F.bits == nullptr: no filter, neither is read)
__global__ __launch_bounds__(256) void redo_begin_kernel(const unsigned* __restrict__ rs, const unsigned* __restrict__ bad, u64* __restrict__ prefix,
                                                         unsigned* __restrict__ remaining, unsigned* __restrict__ hist, unsigned want,
                                                         const RowFilters F, const unsigned* __restrict__ n_allowed) {
  const unsigned n_bad = rs[REDO_RS_BAD];
  if (!n_bad) return;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < (int64_t)n_bad * REDO_BINS; i += step) hist[i] = 0;
  for (int64_t b = i0; b < n_bad; b += step) {
    // under a row filter the rank is min(k, rows the query's bitmap allows), counted on the device
    const int64_t f = filter_index(F, bad[b]);
    const unsigned have = f == FILTER_EVERY_ROW ? want : (f == FILTER_NO_ROW ? 0u : n_allowed[f]);
    prefix[b] = 0;
    remaining[b] = have < want ? have : want;
  }
}

// F: the call's row filters (F.bits == nullptr: every row counts for every query).
// COLLECT = false: hist[b][digit at `shift`] += 1 for every row whose key agrees with prefix[b] above the digit;
// COLLECT = true: every key >= prefix[b] (= T) appended to list bad[b].  Rows [0, N) of `index`, tiles of R rows (R * d * 4 bytes of LDS).
// TRow = f16_t (OM_SEARCH_F16_ONLY): the tile is filled from 16-byte loads of eight halves and staged WIDENED to float32, so R, the LDS
// bytes and the scoring loop are those of the float32 rows.
template <bool COLLECT, typename TRow>
__global__ __launch_bounds__(256) void redo_pass_kernel(const float* __restrict__ q32, const TRow* __restrict__ index, int64_t N, int d, int R,
                                                        const unsigned* __restrict__ rs, const unsigned* __restrict__ bad,
                                                        const u64* __restrict__ prefix, unsigned* __restrict__ hist, int shift, int width,
                                                        u64* __restrict__ keys, unsigned* __restrict__ cnt, const RowFilters F) {
  const unsigned n_bad = rs[REDO_RS_BAD];
  if (!n_bad) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = (N + R - 1) / R;
  const int hi = shift + width;                   // bits [hi, 64) are decided
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t r0 = t * R;
    const int nr = (int)(N - r0 < R ? N - r0 : R);
    __syncthreads();                              // the tile before has been read
    if constexpr (sizeof(TRow) == 4) {
      const float4* src = (const float4*)(index + r0 * d);
      for (int i = tid; i < nr * (d / 4); i += 256) ((float4*)tile)[i] = src[i];
    } else {
      const f16x8_t* src = (const f16x8_t*)(index + r0 * d);
      for (int i = tid; i < nr * (d / 8); i += 256) {
        const f16x8_t h = src[i];
        ((float4*)tile)[2 * i] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        ((float4*)tile)[2 * i + 1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
      }
    }
    __syncthreads();
    for (unsigned b = 0; b < n_bad; ++b) {
      const unsigned q = bad[b];
      const float* qv = q32 + (int64_t)q * d;
      const u64 P = prefix[b];
      const int64_t f = filter_index(F, q);                                  // (workgroup-uniform) the bad query's own bitmap
      if (f == FILTER_NO_ROW) continue;
      const uint32_t* __restrict__ allow = f < 0 ? nullptr : F.bits + f * F.pitch;
      for (int r = wave; r < nr; r += 4) {
        if (allow && !row_allowed(allow, (uint32_t)(r0 + r))) continue;      // (wave-uniform) a row the filter drops has no key
        const float sc = rescore_dot(qv, tile + (int64_t)r * d, d, lane);
        if (lane != 0) continue;
        const u64 key = pack_key(sc, (uint32_t)(r0 + r));
        if (COLLECT) {
          if (key >= P) {
            const unsigned pos = atomicAdd(cnt + q, 1u);
            if (pos < SORT_CAP) keys[(int64_t)q * SORT_CAP + pos] = key;
          }
        } else if (hi >= 64 || (key >> hi) == (P >> hi)) {
          atomicAdd(hist + (int64_t)b * REDO_BINS + (unsigned)((key >> shift) & ((1u << width) - 1u)), 1u);
        }
      }
    }
  }
}

// one workgroup, bad query after bad query: thread t owns bins [8 t, 8 t + 8)
__global__ __launch_bounds__(256) void redo_pick_kernel(const unsigned* __restrict__ rs, const unsigned* __restrict__ bad, u64* __restrict__ prefix,
                                                        unsigned* __restrict__ remaining, unsigned* __restrict__ hist, int shift,
                                                        unsigned* __restrict__ cnt, int last) {
  const unsigned n_bad = rs[REDO_RS_BAD];
  if (!n_bad) return;
  __shared__ unsigned wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned b = 0; b < n_bad; ++b) {
    unsigned* h = hist + (int64_t)b * REDO_BINS + tid * 8;
    unsigned c[8], own = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { c[i] = h[i]; h[i] = 0; own += c[i]; }
    unsigned suf = own;                           // own bins and those of the higher lanes of this wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += up;
    }
    if (lane == 0) wtot[wave] = suf;
    const unsigned rem = remaining[b];
    __syncthreads();
    unsigned above = suf - own;                   // keys in bins above this thread's
    for (int w = wave + 1; w < 4; ++w) above += wtot[w];
    if (rem == 0) {                               // a row filter that allows no row: no key is wanted, T = the largest key
      if (tid == 0) { prefix[b] = ~0ull; if (last) cnt[bad[b]] = 0; }
    } else if (above < rem && above + own >= rem) {      // the digit is one of this thread's: exactly one thread gets here
      unsigned acc = above;
      int digit = 0;
#pragma unroll
      for (int i = 7; i >= 0; --i) {
        if (acc < rem && acc + c[i] >= rem) { digit = i; remaining[b] = rem - acc; }
        acc += c[i];
      }
      prefix[b] |= (u64)(unsigned)(tid * 8 + digit) << shift;
      if (last) cnt[bad[b]] = 0;                  // the collect pass fills the list from slot 0
    }
    __syncthreads();
  }
}

// the last kernel of the chain: status[6] = 1 is written behind everything else
__global__ void async_status_kernel(const unsigned* __restrict__ flag, const unsigned* __restrict__ rs, int64_t* __restrict__ status, int scan,
                                    int rounds, int family) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  status[0] = scan;
  status[1] = rounds;
  status[2] = rs[REDO_RS_BAD];
  status[3] = flag[1];
  status[4] = rs[REDO_RS_WIDE];
  status[5] = family;
  status[7] = 0;
  __threadfence();
  *(volatile int64_t*)(status + 6) = 1;
}

// ---- K14: merge W sorted partial lists per query ------------------------------------------
__global__ __launch_bounds__(SORT_THREADS) void merge_kernel(
    const float* __restrict__ ps, const int64_t* __restrict__ pi, int W, int64_t nq, int k_in,
    int k_out, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* s = (u64*)smem;
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = W * k_in;
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += SORT_THREADS) {
    u64 key = 0ull;
    if (i < n) {
      const int w = i / k_in, j = i % k_in;
      const int64_t src = ((int64_t)w * nq + q) * k_in + j;
      if (pi[src] >= 0) key = pack_key(ps[src], (uint32_t)i);  // ties: (part, position) order
    }
    s[i] = key;
  }
  __syncthreads();
  bitonic_sort_desc(s, P, tid, SORT_THREADS);
  for (int j = tid; j < k_out; j += SORT_THREADS) {
    const u64 key = j < P ? s[j] : 0ull;
    if (key != 0ull) {
      const int i = (int)key_payload(key);
      const int w = i / k_in, jj = i % k_in;
      const int64_t src = ((int64_t)w * nq + q) * k_in + jj;
      out_scores[q * k_out + j] = ps[src];
      out_ids[q * k_out + j] = pi[src];
    } else {
      out_scores[q * k_out + j] = -3.4028235e38f;
      out_ids[q * k_out + j] = -1;
    }
  }
}

extern "C" int om_topk_merge(const float* part_scores, const int64_t* part_ids, int W,
                             int64_t n_queries, int k_in, int k_out, float* out_scores,
                             int64_t* out_ids, void* stream) {
  if (n_queries <= 0 || k_out <= 0) return 0;
  if (W <= 0 || k_in <= 0) OM_FAIL("W and k_in must be positive");
  if ((int64_t)W * k_in > SORT_CAP) OM_FAIL("W*k_in exceeds the 8192-key merge capacity");
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    OM_HIP(hipFuncSetAttribute((const void*)merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               SORT_CAP * 8));
    attr_set = true;
  }
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n_queries), dim3(SORT_THREADS), SORT_CAP * 8,
                     (hipStream_t)stream, part_scores, part_ids, W, n_queries, k_in, k_out,
                     out_scores, out_ids);
  OM_LAUNCH_CHECK();
  return 0;
}

// ---- host orchestration -------------------------------------------------------------------
struct SearchWs {
  u64* keys; unsigned *cnt, *cnt_prev, *flag; float *thr, *margin, *dense; f16_t* qb;
  size_t total;
};
static SearchWs carve_search(int64_t nq, int d, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  SearchWs w;
  w.keys = (u64*)take((size_t)nq * SORT_CAP * 8);
  w.cnt = (unsigned*)take((size_t)nq * 4);
  w.cnt_prev = (unsigned*)take((size_t)nq * 4);
  w.flag = (unsigned*)take(64);
  w.thr = (float*)take(((size_t)(nq + 255) / 256 * 256 + 256) * 4);      // +inf beyond nq: the generation-7 scan reads whole tiles of thresholds
  w.margin = (float*)take((size_t)nq * 4);
  w.dense = (float*)take((size_t)nq * DENSE_CHUNK * 4);
  w.qb = (f16_t*)take((size_t)((nq + 255) / 256 * 256) * d * 2);            // whole query tiles, zero rows beyond nq
  w.total = off;
  return w;
}

// what the asynchronous entry needs behind om_sim_topk's own workspace
struct AsyncWs {
  unsigned *qstat, *rs, *bad, *remaining, *hist; u64* prefix;
  size_t total;
};
static AsyncWs carve_async(int64_t nq, int d, char* base) {
  size_t off = carve_search(nq, d, nullptr).total;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  AsyncWs w;
  w.qstat = (unsigned*)take((size_t)nq * 4);
  w.rs = (unsigned*)take(64);
  w.bad = (unsigned*)take((size_t)nq * 4);
  w.remaining = (unsigned*)take((size_t)nq * 4);
  w.prefix = (u64*)take((size_t)nq * 8);
  w.hist = (unsigned*)take((size_t)nq * REDO_BINS * 4);
  w.total = off;
  return w;
}

extern "C" void om_sim_topk_info(int64_t out[8]) {
  for (int i = 0; i < 8; ++i) out[i] = g_info[i];
}

extern "C" int om_debug_scan_plan(int half, int64_t nq, int d, int out[4]) {
  if (!out) OM_FAIL("null argument");
  const ScanPlan p = scan_plan(half != 0, nq, d, scan_switches());
  out[0] = p.family; out[1] = p.qblock; out[2] = p.nb; out[3] = p.nkmax;
  return 0;
}

extern "C" int om_debug_scan_round(int half, int64_t nq, int d, int64_t rows, int cus, int64_t out[8]) {
  if (!out) OM_FAIL("null argument");
  if (nq < 1 || d < 1 || rows < 0 || cus < 1) OM_FAIL("nq >= 1, d >= 1, rows >= 0 and cus >= 1");
  const ScanSwitches sw = scan_switches();
  const ScanRound r = scan_round(scan_plan(half != 0, nq, d, sw), half != 0, nq, d, rows, cus, sw);
  if (!r.ok) OM_FAIL("scan grid too large");
  const ScanLaunch* const part[2] = {&r.main, &r.tail};
  for (int i = 0; i < 2; ++i) {
    out[4 * i] = part[i]->kernel; out[4 * i + 1] = part[i]->rows; out[4 * i + 2] = part[i]->grid; out[4 * i + 3] = part[i]->group;
  }
  return 0;
}

extern "C" size_t om_sim_topk_workspace_bytes(int64_t n_queries, int d, int k) {
  (void)k;
  if (n_queries <= 0 || d <= 0) return 0;
  return carve_search(n_queries, d, nullptr).total;
}

extern "C" size_t om_sim_topk_async_workspace_bytes(int64_t n_queries, int d, int k) {
  (void)k;
  if (n_queries <= 0 || d <= 0) return 0;
  return carve_async(n_queries, d, nullptr).total;
}

extern "C" int om_debug_search_schedule(int mode, int64_t nq, int64_t N, int k, int64_t* chunks, int cap, int* n) {
  if (!n || (cap > 0 && !chunks)) OM_FAIL("null argument");
  if (nq < 1 || N < 0 || k < 1 || k > K_MAX) OM_FAIL("nq >= 1, N >= 0 and k in [1,2048]");
  *n = search_schedule(search_mode_half(mode), nq, N, k, scan_switches(), chunks, cap < 0 ? 0 : cap).n;
  return 0;
}

// ---- the scan kernels: one table for their LDS attributes and their launches ---------------------------------------------------------
// The tile kernels by [OM_SCAN_KERNEL_*][index format: 0 float32, 1 16-bit], the stream kernel by [instantiation][nb: 1 | 2 | 4].  All
// take (rows, nrows, row_base, queries, nq, d, thr, keys, cnt, int); generation 7 appends the trace buffer.  fn == nullptr: no such kernel.
struct ScanKernel { const void* fn; int threads; int lds; bool trace; };
#define SCAN_KERNEL_(FN, THREADS, LDS, TRACE) {(const void*)FN, THREADS, LDS, TRACE}
#define SCAN_NONE_ {nullptr, 0, 0, false}
static const ScanKernel g_tile_kernels[OM_SCAN_KERNEL_WIDE7C + 1][2] = {
    {SCAN_NONE_, SCAN_NONE_},
    {SCAN_KERNEL_(sim_filter_kernel<float>, G2_THREADS, G2_LDS_BYTES, false), SCAN_KERNEL_(sim_filter_kernel<f16_t>, G2_THREADS, G2_LDS_BYTES, false)},
    {SCAN_KERNEL_(sim_filter_kernel6<float>, G6_THREADS, G6_LDS_BYTES, false), SCAN_KERNEL_(sim_filter_kernel6<f16_t>, G6_THREADS, G6_LDS_BYTES, false)},
    {SCAN_NONE_, SCAN_KERNEL_(sim_filter_kernel7<f16_t>, G6_THREADS, G7_LDS_BYTES, true)},
    {SCAN_NONE_, SCAN_KERNEL_(sim_filter_kernel7c<f16_t>, G6_THREADS, G7_LDS_BYTES, true)},
};
#define STREAM_ROW_(...)                                                                                                            \
  {SCAN_KERNEL_((sim_stream_reg_kernel<f16_t, 1, __VA_ARGS__>), G6_THREADS, SR_LDS, false),                                          \
   SCAN_KERNEL_((sim_stream_reg_kernel<f16_t, 2, __VA_ARGS__>), G6_THREADS, SR_LDS, false),                                          \
   SCAN_KERNEL_((sim_stream_reg_kernel<f16_t, 4, __VA_ARGS__>), G6_THREADS, SR_LDS, false)}
static const ScanKernel g_stream_kernels[][3] = {
    STREAM_ROW_(0, SCAN_NKMAX32_NARROW, 32),      // 256 <= d <= 768
    STREAM_ROW_(0, SCAN_NKMAX32_WIDE, 32),        // 832 <= d <= 1024
    STREAM_ROW_(0, SCAN_NKMAX16, 16),             // 1088 <= d <= 2048, 16-query blocks
#ifdef OM_PROBE_KERNELS      // timing variants with MFMAs compiled out (WRONG results): probe builds only (python -m openmatch_amd._build --probe)
    STREAM_ROW_(1, SCAN_NKMAX32_NARROW, 32),
    STREAM_ROW_(2, SCAN_NKMAX32_NARROW, 32),
#endif
};
#undef STREAM_ROW_
#undef SCAN_NONE_
#undef SCAN_KERNEL_

// the table row of a planned launch
static const ScanKernel& scan_kernel(int kernel, bool half, const ScanPlan& plan, const ScanSwitches& sw) {
  if (kernel != OM_SCAN_KERNEL_STREAM) return g_tile_kernels[kernel][half ? 1 : 0];
  int inst = plan.family == OM_SCAN_FAMILY_STREAM16 ? 2 : plan.nkmax == SCAN_NKMAX32_WIDE ? 1 : 0;
#ifdef OM_PROBE_KERNELS
  if (inst == 0 && (sw.probe == 1 || sw.probe == 2)) inst = 2 + sw.probe;
#endif
  (void)sw;
  return g_stream_kernels[inst][plan.nb == 1 ? 0 : plan.nb == 2 ? 1 : 2];
}

// dynamic-LDS attribute of every scan kernel: host calls, made once (a capturing stream must not meet them)
static int scan_attrs() {
  static std::atomic<bool> done{false};
  if (done) return 0;
  for (const auto& row : g_tile_kernels)
    for (const ScanKernel& kn : row)
      if (kn.fn) OM_HIP(hipFuncSetAttribute(kn.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kn.lds));
  for (const auto& row : g_stream_kernels)
    for (const ScanKernel& kn : row) OM_HIP(hipFuncSetAttribute(kn.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kn.lds));
  done = true;
  return 0;
}

// The one launcher of the scan kernels: rows [nrows, d] with ids from row_base against the queries, survivors appended to keys / cnt.
static int scan_launch(const ScanKernel& kn, const void* rows, int64_t nrows, uint32_t row_base, const void* queries, int64_t nq, int d,
                       const float* thr, u64* keys, unsigned* cnt, int64_t grid, int group, hipStream_t s) {
  if (!kn.fn) OM_FAIL("the scan plan names a kernel that does not exist");
  int64_t d64 = d;
  unsigned long long* trace = kn.trace ? omk_debug_trace() : nullptr;
  void* args[] = {&rows, &nrows, &row_base, &queries, &nq, &d64, &thr, &keys, &cnt, &group, &trace};      // (trace: generation 7 only)
  OM_HIP(hipLaunchKernel(kn.fn, dim3((unsigned)grid), dim3((unsigned)kn.threads), args, (size_t)kn.lds, s));
  return 0;
}

namespace {
struct Scan {
  int mode; const float* q32; const float* idx32; const f16_t* idx16; int64_t nq, N; int d, k;
  SearchWs ws; hipStream_t s;
  unsigned* qstat = nullptr;      // per-query sticky status: the asynchronous entry only
  ScanSwitches sw;                // the thread's switches, read once by the entry
  // om_sim_topk_filtered only (nullptr: no filter, and not one launch differs): the bitmap over rows [0, N) and the host's count of its bits
  // (om_sim_topk_filtered_multi: the bitmaps of the call, n_allowed the count of the sparsest one in use, fcount one device count per bitmap)
  RowFilters filt = {nullptr, 0, 0, nullptr, 0};
  int64_t n_allowed = 0;
  unsigned* fcount = nullptr;
  // diagnostics, accumulated over the 16-bit run and the float32 retry (om_sim_topk publishes them, the asynchronous entry's status
  // kernel takes rounds and family): rounds, chunks redone densely or schedules started over, longest list seen by the host,
  // OM_SCAN_FAMILY_* and OM_SCAN_KERNEL_* of the last filtered round (its tail's where the round had no whole tile)
  int64_t rounds = 0, fallbacks = 0, max_list = 0;
  int family = 0, launch = 0;

  // under a row filter every selection is preceded by the drop of the keys it does not allow
  // (mark: as the selection it precedes -- the last one of the chain, behind the redo, marks no query: nothing reads the marks any more)
  int drop(bool mark = true) {
    if (!filt.bits) return 0;
    hipLaunchKernelGGL(drop_disallowed_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, filt, (uint32_t)N, ws.flag,
                       mark ? qstat : nullptr);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int select(bool certified, bool mark = true) {
    if (drop(mark)) return 1;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)nq), dim3(SORT_THREADS), SORT_CAP * 8 + 16, s,
                       ws.keys, ws.cnt, ws.cnt_prev, ws.thr, certified ? ws.margin : nullptr, k,
                       ws.flag, mark ? qstat : nullptr);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int select_radix(bool certified, int cap = SORT_CAP) {
    if (drop()) return 1;
    hipLaunchKernelGGL(select_radix_kernel, dim3((unsigned)nq), dim3(256), (size_t)cap * 8 + 1024 + 64, s,
                       ws.keys, ws.cnt, ws.thr, certified ? ws.margin : nullptr, k, ws.flag, cap, qstat);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int read_flags(unsigned (&f)[4]) {
    static thread_local unsigned* pinned = nullptr;        // page-locked: the copy is one DMA, no staging through the runtime
    if (!pinned) OM_HIP(hipHostMalloc((void**)&pinned, 64, hipHostMallocPortable));
    OM_HIP(hipMemcpyAsync(pinned, ws.flag, sizeof(f), hipMemcpyDeviceToHost, s));
    OM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) f[i] = pinned[i];
    return 0;
  }
  bool rows16() const { return mode == OM_SEARCH_F16_ONLY; }      // the re-score and the redo read the float16 rows: there are no others
  int rescore(unsigned maxlist) {
    if (rows16())
      hipLaunchKernelGGL(rescore_kernel<f16_t>, dim3((maxlist + 3) / 4, (unsigned)nq), dim3(256), 0, s, q32, idx16, ws.keys, ws.cnt, d);
    else
      hipLaunchKernelGGL(rescore_kernel<float>, dim3((maxlist + 3) / 4, (unsigned)nq), dim3(256), 0, s, q32,
                         idx32, ws.keys, ws.cnt, d);
    OM_LAUNCH_CHECK();
    return 0;
  }
  // one pass of the on-device redo over the rows the mode stores (COLLECT: the last one, which fills the lists)
  template <bool COLLECT>
  void redo_pass(const AsyncWs& aw, dim3 grid, size_t lds, int R, int shift, int width) {
    if (rows16())
      hipLaunchKernelGGL((redo_pass_kernel<COLLECT, f16_t>), grid, dim3(256), lds, s, q32, idx16, N, d, R, aw.rs, aw.bad, aw.prefix, aw.hist,
                         shift, width, ws.keys, ws.cnt, filt);
    else
      hipLaunchKernelGGL((redo_pass_kernel<COLLECT, float>), grid, dim3(256), lds, s, q32, idx32, N, d, R, aw.rs, aw.bad, aw.prefix, aw.hist,
                         shift, width, ws.keys, ws.cnt, filt);
  }
  // dense-score rows [r0, r0+n) and merge them into the lists (always exact, HBM heavy)
  int dense_gemm_append(int64_t r0, int n, bool bf16) {
    if (bf16) {
      if (om_gemm_nt(OM_F16, ws.qb, d, idx16 + r0 * d, d, OM_F32, ws.dense, DENSE_CHUNK, nq, n, d,
                     nullptr, nullptr, 0, OM_ACT_NONE, s)) return 1;
    } else {
      if (om_gemm_nt(OM_F32, q32, d, idx32 + r0 * d, d, OM_F32, ws.dense, DENSE_CHUNK, nq, n, d,
                     nullptr, nullptr, 0, OM_ACT_NONE, s)) return 1;
    }
    hipLaunchKernelGGL(append_dense_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.dense,
                       (int64_t)DENSE_CHUNK, n, (uint32_t)r0, ws.keys, ws.cnt);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int dense_step(int64_t r0, int n, bool bf16) {
    if (dense_gemm_append(r0, n, bf16)) return 1;
    return select(bf16);
  }
  // one filtered round over rows [r0, r0 + n): what scan_round plans, launched from the kernel table
  int filter_step(int64_t r0, int64_t n, bool bf16, bool check = true /* false: the selection that follows flags overflows */) {
    const ScanPlan plan = scan_plan(bf16, nq, d, sw);
    const ScanRound round = scan_round(plan, bf16, nq, d, n, g7_num_cus(), sw);
    if (!round.ok) OM_FAIL("scan grid too large");
    family = plan.family;
    launch = round.main.rows ? round.main.kernel : round.tail.kernel;
    const char* const rows = bf16 ? (const char*)idx16 : (const char*)idx32;
    const void* const queries = bf16 ? (const void*)ws.qb : (const void*)q32;
    const int64_t row_bytes = (int64_t)d * (bf16 ? 2 : 4);
    const bool timing = om_timing_on();
    if (timing) om_timing_begin(OM_TIMING_SCAN, s);
    for (const ScanLaunch* l : {&round.main, &round.tail})
      if (l->rows && scan_launch(scan_kernel(l->kernel, bf16, plan, sw), rows + (r0 + l->row0) * row_bytes, l->rows, (uint32_t)(r0 + l->row0),
                                 queries, nq, d, ws.thr, ws.keys, ws.cnt, l->grid, l->group, s)) return 1;
    if (timing) om_timing_end(OM_TIMING_SCAN, s, 2.0 * (double)n * (double)nq * (double)d);
    OM_LAUNCH_CHECK();
    if (!check) return 0;
    hipLaunchKernelGGL(check_overflow_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s,
                       ws.cnt, nq, ws.flag, (unsigned*)nullptr, 0u);
    OM_LAUNCH_CHECK();
    return 0;
  }

  // empty lists, thresholds at -inf (+inf beyond nq, a whole query tile further: the generation-7 scan reads whole tiles), flags cleared
  int init_lists() {
    hipLaunchKernelGGL(init_lists_kernel, dim3((unsigned)((nq + 255) / 256 + 2)), dim3(256), 0, s,
                       ws.cnt, ws.cnt_prev, ws.thr, nq, ws.flag);
    OM_LAUNCH_CHECK();
    return 0;
  }
  // What every search starts with: the lists, the asynchronous entry's status words (aw != nullptr) and, for the 16-bit scan of a
  // non-empty shard, the 16-bit query panel with its certified margins.
  int begin(bool bf16, const AsyncWs* aw = nullptr, int64_t* status = nullptr) {
    if (init_lists()) return 1;
    if (aw) {
      hipLaunchKernelGGL(async_init_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, aw->qstat, aw->rs, status, nq);
      OM_LAUNCH_CHECK();
      if (filt.bits && N > 0) {                    // behind the kernel that zeroes rs
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((N + 31) / 32 + 255) / 256, 1024));
        // one bitmap: counted into rs[REDO_RS_ALLOWED]; a bitmap per query: one grid row and one word of the entry's own counts per bitmap
        if (filt.per_query) OM_HIP(hipMemsetAsync(fcount, 0, (size_t)filt.n * 4, s));
        hipLaunchKernelGGL(count_allowed_kernel, dim3((unsigned)blocks, (unsigned)(filt.per_query ? filt.n : 1)), dim3(256), 0, s, filt, N, fcount);
        OM_LAUNCH_CHECK();
      }
    }
    if (bf16 && N > 0) {
      hipLaunchKernelGGL(query_prep_kernel, dim3((unsigned)(((nq + 255) / 256 * 256 + 3) / 4)), dim3(256), 0, s, q32,
                         ws.qb, ws.margin, stats, nq, d);
      OM_LAUNCH_CHECK();
    }
    return 0;
  }
  // The fast schedule's rounds, for both entries (N > DENSE_CHUNK): the dense bootstrap and its selection, then per round the filtered
  // scan and a radix selection, which also flags overflows -- back to back, nothing read by the host.  The list estimate, the growth
  // per round, the selection's LDS copy and the chunks are search_plan.h's search_schedule, returned in `sched`.
  // Under a row filter the schedule is search_schedule_filtered's: `boot` dense chunks, each with its drop and selection, then the rounds.
  int fast_rounds(bool bf16, SearchSchedule& sched) {
    int64_t chunks[SEARCH_SCHED_MAX];
    int64_t boot = 1;
    sched = filt.bits ? search_schedule_filtered(bf16, nq, N, k, n_allowed, sw, chunks, SEARCH_SCHED_MAX, &boot)
                  : search_schedule(bf16, nq, N, k, sw, chunks, SEARCH_SCHED_MAX);
    if (sched.n > SEARCH_SCHED_MAX) OM_FAIL("schedule has too many rounds");
    for (int64_t b = 0; b < boot && b * DENSE_CHUNK < N; ++b) {
      if (dense_gemm_append(b * DENSE_CHUNK, (int)std::min<int64_t>(DENSE_CHUNK, N - b * DENSE_CHUNK), bf16)) return 1;
      if (select_radix(bf16, b == 0 && DENSE_CHUNK <= 4096 ? 4096 : SORT_CAP)) return 1;
      rounds++;
    }
    int64_t at = boot * DENSE_CHUNK;
    for (int i = 0; i < sched.n; ++i) {
      if (filter_step(at, chunks[i], bf16, false)) return 1;
      if (select_radix(bf16, sched.sel_cap)) return 1;
      rounds++;
      at += chunks[i];
    }
    return 0;
  }

  void trace(const char* what, int64_t done, int64_t chunk, const unsigned (&f)[4]) {
    rounds++;
    max_list = std::max<int64_t>(max_list, f[1]);
    const bool dbg = (om_option(OM_OPT_SEARCH_DEBUG) & 1) != 0;
    if (dbg) fprintf(stderr, "[om_sim_topk] %-8s done=%ld chunk=%ld overflow=%u max_list=%u too_wide=%u\n",
                     what, (long)done, (long)chunk, f[0], f[1], f[2]);
  }

  // returns 0 ok, 1 error, 2 certified margin too wide (caller retries in f32)
  int run(bool bf16) {
    if (begin(bf16)) return 1;
    int64_t done = 0;
    unsigned f[4] = {0, 0, 0, 0};
    bool unsorted = false;
    // Fast schedule (default): bootstrap on a dense-scored chunk, then filtered scan -> overflow check (sticky flag) ->
    // radix selection per round, back to back with NO host synchronisation at all -- the list length after a selection
    // hardly moves (k plus ties / the certified margin), so the chunk sizes are fixed on the host from an ESTIMATE of
    // it.  One read of the flags at the very end; an overflow or a too-wide margin anywhere (adversarial row order,
    // heavily duplicated rows) falls back to the step-by-step loop below from scratch, which is always exact.
    bool careful = true;
    if (sw.gen7 && N > DENSE_CHUNK) {
      SearchSchedule sched;
      if (fast_rounds(bf16, sched)) return 1;
      const int64_t list = sched.list;
      // Few queries: the exact re-score and the final sort are queued BEHIND the last round before the flags are read, so
      // the host's wake-up overlaps them instead of idling the device (a 34 us hole per search at one query).  They
      // cover lists up to twice the estimate; a longer list (never seen) counts as a failed fast schedule.
      // (round 6: up to 128 queries, the whole small-batch regime of the register-resident stream kernel -- a search of 2.6-3.3 ms; at
      // thousands of queries the one wake-up per 90 ms search is nothing, and a re-score grid sized for twice the estimate would launch
      // millions of empty workgroups.  om_sim_topk has exactly ONE host synchronisation per search on this schedule: this read)
      const bool spec = bf16 && nq <= 128;
      const unsigned spec_cover = (unsigned)std::min<int64_t>(2 * list, SORT_CAP);
      if (spec) {
        if (rescore(spec_cover)) return 1;
        if (select(false)) return 1;
      }
      unsigned g[4];
      if (read_flags(g)) return 1;
      max_list = std::max<int64_t>(max_list, g[1]);
      if (!g[0] && !g[2] && !(spec && g[1] > spec_cover)) {
        if (spec) return 0;                      // everything is done
        done = N;
        f[1] = g[1];
        unsorted = true;                         // the lists are cut but not ordered: one sort at the very end
        careful = false;
      } else {                                   // rare: start over on the careful path
        fallbacks++;
        if (init_lists()) return 1;
      }
    }
    if (careful) {                               // bootstrap of the step-by-step loop
      const int n = (int)std::min<int64_t>(N, DENSE_CHUNK);
      if (dense_step(0, n, bf16)) return 1;
      done = n;
      if (read_flags(f)) return 1;
      trace("boot", 0, n, f);
      if (f[2]) return 2;
    }
    while (done < N) {
      const int64_t list = std::max<unsigned>(f[1], 1u);
      // expected survivors of a chunk ~ list * chunk / done.  The per-query sort pads its list to the next
      // power of two, so aim just under 4096 keys (list + survivors) while the list is short enough --
      // filling half the free slots lands at ~4700 and sorts 8192 every round -- else half the free slots.
      const double want = list <= 2048 ? 3800.0 - (double)list : (double)(SORT_CAP - list) / 2.0;
      int64_t chunk = (int64_t)((double)done * want / (double)list);
      chunk = std::max<int64_t>(chunk, DENSE_CHUNK);
      chunk = std::min<int64_t>(chunk, N - done);
      OM_HIP(hipMemsetAsync(ws.flag, 0, 64, s));
      if (filter_step(done, chunk, bf16)) return 1;
      if (read_flags(f)) return 1;
      if (!f[0]) {
        if (select(bf16)) return 1;
      } else {
        fallbacks++;
        // a list overflowed: rewind to the pre-chunk lists and redo the chunk densely
        hipLaunchKernelGGL(restore_cnt_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s,
                           ws.cnt, ws.cnt_prev, nq);
        OM_LAUNCH_CHECK();
        for (int64_t r = done; r < done + chunk; r += DENSE_CHUNK) {
          OM_HIP(hipMemsetAsync(ws.flag, 0, 64, s));
          if (dense_step(r, (int)std::min<int64_t>(DENSE_CHUNK, done + chunk - r), bf16)) return 1;
          if (bf16) {
            if (read_flags(f)) return 1;
            if (f[2]) return 2;
          }
        }
      }
      if (read_flags(f)) return 1;
      trace("scan", done, chunk, f);
      if (f[2]) return 2;
      done += chunk;
    }
    if (bf16) {
      // exact f32 re-score of the certified candidate set, then the true top-k
      if (rescore(std::max<unsigned>(f[1], 1u))) return 1;
      if (select(false)) return 1;
    } else if (unsorted) {
      if (select(false)) return 1;               // exact mode after the radix rounds: best k, in order
    }
    return 0;
  }
  const float* stats;

  // The asynchronous chain (om_sim_topk_async): the fast schedule above with every decision the host used to take from the flags moved
  // to the device.  Enqueues only: no synchronisation, no copy to the host, no allocation.  Order: init -> query prep -> dense bootstrap
  // -> rounds -> re-score -> redo of every query with a sticky bit -> ONE final sort of all lists -> emit -> status.
  int run_async(bool bf16, const AsyncWs& aw, int64_t id_offset, float* out_scores, int64_t* out_ids, int64_t* status) {
    const unsigned qblocks = (unsigned)((nq + 255) / 256);
    if (begin(bf16, &aw, status)) return 1;
    if (N > 0) {
      SearchSchedule sched;
      if (N <= DENSE_CHUNK) {                      // one dense step, no rounds (what om_sim_topk does for a shard this small)
        sched = search_schedule(bf16, nq, N, k, sw, nullptr, 0);      // (its list estimate alone)
        if (dense_step(0, (int)N, bf16)) return 1;
        rounds++;
      } else if (fast_rounds(bf16, sched)) return 1;
      const int64_t list = sched.list;
      if (bf16) {
        // exact f32 re-score of the certified candidates.  Up to 128 queries: om_sim_topk's own launch, covering lists up to twice the
        // estimate -- a longer list is marked (QSTAT_COVER) and redone; above: the fixed grid, which reaches every slot below cnt.
        // A marked query's list is still well-formed here: cnt <= SORT_CAP after a selection, and every key below cnt names a row.
        if (nq <= 128) {
          const unsigned cover = (unsigned)std::min<int64_t>(2 * list, SORT_CAP);
          hipLaunchKernelGGL(check_overflow_kernel, dim3(qblocks), dim3(256), 0, s, ws.cnt, nq, ws.flag, qstat, cover);
          OM_LAUNCH_CHECK();
          if (rescore(cover)) return 1;
        } else {
          const dim3 rgrid((unsigned)(g7_num_cus() * 8));
          if (rows16()) hipLaunchKernelGGL(rescore_strided_kernel<f16_t>, rgrid, dim3(256), 0, s, q32, idx16, ws.keys, ws.cnt, nq, d);
          else hipLaunchKernelGGL(rescore_strided_kernel<float>, rgrid, dim3(256), 0, s, q32, idx32, ws.keys, ws.cnt, nq, d);
          OM_LAUNCH_CHECK();
        }
      }
      // redo: a fixed chain, empty launches when no query is marked
      hipLaunchKernelGGL(redo_compact_kernel, dim3(qblocks), dim3(256), 0, s, qstat, nq, aw.rs, aw.bad);
      hipLaunchKernelGGL(redo_begin_kernel, dim3(256), dim3(256), 0, s, aw.rs, aw.bad, aw.prefix, aw.remaining, aw.hist,
                         (unsigned)std::min<int64_t>(k, N), filt, (const unsigned*)fcount);
      OM_LAUNCH_CHECK();
      const int R = (int)std::max<int64_t>(1, std::min<int64_t>(32, REDO_TILE_BYTES / ((int64_t)d * 4)));
      const size_t lds = (size_t)R * d * 4;
      const dim3 pgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>((N + R - 1) / R, (int64_t)g7_num_cus() * 4)));
      for (int p = 0; p < REDO_PASSES; ++p) {
        redo_pass<false>(aw, pgrid, lds, R, redo_shift(p), redo_width(p));
        hipLaunchKernelGGL(redo_pick_kernel, dim3(1), dim3(256), 0, s, aw.rs, aw.bad, aw.prefix, aw.remaining, aw.hist, redo_shift(p), ws.cnt,
                           p == REDO_PASSES - 1 ? 1 : 0);
        OM_LAUNCH_CHECK();
      }
      redo_pass<true>(aw, pgrid, lds, R, 0, 0);
      OM_LAUNCH_CHECK();
      if (select(false, false)) return 1;          // best k of every list, in order
    }
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, k, id_offset, out_scores, out_ids);
    if (status) hipLaunchKernelGGL(async_status_kernel, dim3(1), dim3(64), 0, s, ws.flag, aw.rs, status, bf16 ? 1 : 0, (int)rounds, family);
    OM_LAUNCH_CHECK();
    return 0;
  }

  // om_sim_topk in OM_SEARCH_F16_ONLY: there is no float32 plane to retry on, so the entry enqueues the asynchronous chain -- whose redo
  // serves every query the margin does not certify -- without status words, and reads the chain's own counters back: ONE synchronisation.
  // out: {queries redone, of those with a too-wide margin, longest list}
  int run_sync16(const AsyncWs& aw, int64_t id_offset, float* out_scores, int64_t* out_ids, unsigned (&out)[3]) {
    if (run_async(true, aw, id_offset, out_scores, out_ids, nullptr)) return 1;
    static thread_local unsigned* pinned = nullptr;
    if (!pinned) OM_HIP(hipHostMalloc((void**)&pinned, 128, hipHostMallocPortable));
    OM_HIP(hipMemcpyAsync(pinned, ws.flag, 64, hipMemcpyDeviceToHost, s));
    OM_HIP(hipMemcpyAsync(pinned + 16, aw.rs, 64, hipMemcpyDeviceToHost, s));
    OM_HIP(hipStreamSynchronize(s));
    out[0] = pinned[16 + REDO_RS_BAD]; out[1] = pinned[16 + REDO_RS_WIDE]; out[2] = pinned[1];
    return 0;
  }

  // om_sim_topk behind its checks: the 16-bit scan, the float32 one when that was asked for or the certified margin is too wide, emit
  int run_sync(int64_t id_offset, float* out_scores, int64_t* out_ids) {
    if (N > 0) {
      int rc = 2;
      if (mode == OM_SEARCH_F16_RESCORE) {
        rc = run(true);
        if (rc == 1) return 1;
        precision = 1;
        if (rc == 2) too_wide = 1;
      }
      if (rc == 2) {                           // f32 scan (requested, or margin too wide)
        precision = 0;
        if (run(false)) return 1;
      }
    } else {
      hipLaunchKernelGGL(init_lists_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s,
                         ws.cnt, ws.cnt_prev, ws.thr, nq, ws.flag);
      OM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, k, id_offset, out_scores, out_ids);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int precision = 0, too_wide = 0;      // om_sim_topk_info [0] and [4]
};

// The argument checks and the set-up the two entries share (n_queries > 0).  Returns the refusal, nullptr when there is none: the entry
// fails with it under its own name.
const char* scan_setup(Scan& sc, int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                       const float* stats, int64_t N, int d, int k, const float* out_scores, const int64_t* out_ids, void* workspace,
                       void* stream) {
  if (k < 1 || k > K_MAX) return "k must be in [1,2048]";
  if (N < 0 || N > 0xffffffffLL) return "shard rows must fit in 32 bits";
  if (d <= 0 || (d * 2) % GEMM_ROW_BYTES != 0) return "d must be a multiple of 64 (pad with zeros)";
  if (n_queries > 65535) return "at most 65535 queries per call";
  if (!queries || !out_scores || !out_ids) return "null argument";
  if (!workspace || ((uintptr_t)workspace & 255)) return "workspace must be 256-byte aligned";
  if (N > 0 && mode != OM_SEARCH_F16_ONLY && !index_f32) return "index_f32 is null";
  if (N > 0 && mode == OM_SEARCH_F16_RESCORE && (!index_f16 || !stats)) return "f16 mode needs index_f16 and stats";
  if (N > 0 && mode == OM_SEARCH_F16_ONLY && !index_f16) return "OM_SEARCH_F16_ONLY: index_f16 is null (the float16 rows are the index)";
  if (N > 0 && mode == OM_SEARCH_F16_ONLY && !stats) return "OM_SEARCH_F16_ONLY: stats is null (om_index_add_f16 leaves them)";
  sc.ws = carve_search(n_queries, d, (char*)workspace);
  sc.mode = mode; sc.q32 = queries; sc.idx32 = index_f32; sc.idx16 = (const f16_t*)index_f16;
  sc.nq = n_queries; sc.N = N; sc.d = d; sc.k = k; sc.s = (hipStream_t)stream; sc.stats = stats;
  sc.sw = scan_switches();
  return nullptr;
}

// What OM_SEARCH_F16_ONLY refuses in BOTH entries: it always runs the stream-ordered chain, and neither entry has another path to offer.
const char* f16_only_refusal(const Scan& sc) {
  if (sc.d > 16384) return "OM_SEARCH_F16_ONLY: d above 16384: a row does not fit the redo's LDS tile, and the mode has no float32 scan to fall back to";
  if (!sc.sw.gen7)
    return "OM_SEARCH_F16_ONLY: OM_OPT_SCAN_GEN7 is 0: the fast schedule this mode runs is switched off, and it has no step-by-step path";
  return nullptr;
}
}  // namespace

// dynamic-LDS attributes of every kernel a search launches: host calls, made once (a capturing stream must not meet them)
static int search_attrs() {
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    OM_HIP(hipFuncSetAttribute((const void*)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               SORT_CAP * 8 + 16));
    if (scan_attrs()) return 1;
    OM_HIP(hipFuncSetAttribute((const void*)select_radix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               SORT_CAP * 8 + 1024 + 64));
    attr_set = true;
  }
  return 0;
}

extern "C" int om_sim_topk(int mode, const float* queries, int64_t n_queries,
                           const float* index_f32, const void* index_f16, const float* stats,
                           int64_t N, int d, int k, int64_t id_offset, float* out_scores,
                           int64_t* out_ids, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (n_queries <= 0) return 0;
  Scan sc;
  if (const char* why = scan_setup(sc, mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, stream))
    OM_FAIL(why);
  if (mode == OM_SEARCH_F16_ONLY) {
    if (const char* why = f16_only_refusal(sc)) OM_FAIL(why);
    const AsyncWs aw = carve_async(n_queries, d, (char*)workspace);
    if (aw.total > workspace_bytes) OM_FAIL("workspace too small: OM_SEARCH_F16_ONLY needs om_sim_topk_async_workspace_bytes");
    sc.qstat = aw.qstat;
    if (search_attrs()) return 1;
    for (auto& v : g_info) v = 0;
    unsigned redo[3] = {0, 0, 0};
    const int rc = sc.run_sync16(aw, id_offset, out_scores, out_ids, redo);
    g_info[0] = 1; g_info[1] = sc.rounds; g_info[3] = redo[2]; g_info[4] = redo[1]; g_info[5] = sc.family; g_info[6] = sc.launch;
    g_info[7] = redo[0];
    return rc;
  }
  if (sc.ws.total > workspace_bytes) OM_FAIL("workspace too small");
  if (search_attrs()) return 1;
  for (auto& v : g_info) v = 0;
  const int rc = sc.run_sync(id_offset, out_scores, out_ids);
  g_info[0] = sc.precision; g_info[1] = sc.rounds; g_info[2] = sc.fallbacks; g_info[3] = sc.max_list;
  g_info[4] = sc.too_wide; g_info[5] = sc.family; g_info[6] = sc.launch;
  return rc;
}

// The asynchronous search: om_sim_topk's arguments, checks and output; everything on `stream`, nothing read back, and the thread's
// om_sim_topk_info left as it is.
extern "C" int om_sim_topk_async(int mode, const float* queries, int64_t n_queries,
                                 const float* index_f32, const void* index_f16, const float* stats,
                                 int64_t N, int d, int k, int64_t id_offset, float* out_scores,
                                 int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (n_queries <= 0) return 0;
  Scan sc;
  if (const char* why = scan_setup(sc, mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, stream))
    OM_FAIL(why);
  if (mode == OM_SEARCH_F16_ONLY) {
    if (const char* why = f16_only_refusal(sc)) OM_FAIL(why);
  }
  if (d > 16384) OM_FAIL("d above 16384: a row does not fit the redo's LDS tile (use om_sim_topk)");
  if (!status) OM_FAIL("status is null: the asynchronous entry reports through 8 x int64 of device memory");
  if (!sc.sw.gen7)
    OM_FAIL("OM_OPT_SCAN_GEN7 is 0: the fast schedule this entry runs is switched off (use om_sim_topk)");
  const AsyncWs aw = carve_async(n_queries, d, (char*)workspace);
  if (aw.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_async_workspace_bytes)");
  sc.qstat = aw.qstat;
  if (search_attrs()) return 1;
  return sc.run_async(search_mode_half(mode), aw, id_offset, out_scores, out_ids, status);
}

// The stream-ordered search under a row filter: om_sim_topk_async's chain (Scan::run_async itself) with the bitmap set, which adds the
// count of the allowed rows behind the init, the drop in front of every selection, the filtered schedule and the redo's row test.
extern "C" int om_sim_topk_filtered(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                                    const float* stats, int64_t N, int d, int k, int64_t id_offset, const uint32_t* allow_bits,
                                    int64_t n_allowed, float* out_scores, int64_t* out_ids, int64_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (n_queries <= 0) return 0;
  Scan sc;
  if (const char* why = scan_setup(sc, mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, stream))
    OM_FAIL(why);
  if (mode == OM_SEARCH_F16_ONLY) {
    if (const char* why = f16_only_refusal(sc)) OM_FAIL(why);
  }
  if (d > 16384) OM_FAIL("d above 16384: a row does not fit the redo's LDS tile");
  if (!sc.sw.gen7) OM_FAIL("OM_OPT_SCAN_GEN7 is 0: the fast schedule this entry runs is switched off");
  if (!allow_bits) OM_FAIL("allow_bits is null: the filtered search needs the bitmap of the allowed rows (om_sim_topk_async searches all rows)");
  if (n_allowed < 0 || n_allowed > N) OM_FAIL("n_allowed must be in [0, N]");
  const AsyncWs aw = carve_async(n_queries, d, (char*)workspace);
  if (aw.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_filtered_workspace_bytes)");
  sc.qstat = aw.qstat;
  sc.filt = RowFilters{allow_bits, 0, 1, nullptr, 0};
  sc.n_allowed = n_allowed;
  sc.fcount = aw.rs + REDO_RS_ALLOWED;
  if (search_attrs()) return 1;
  return sc.run_async(search_mode_half(mode), aw, id_offset, out_scores, out_ids, status);
}

// The same chain with a bitmap per query: the three kernels that read a bitmap -- the drop, the count, the redo -- take it from
// filter_of[q]; one count per bitmap lives in n_filters words behind the asynchronous workspace.  The schedule is the single-filter one of
// the sparsest bitmap in use (search_plan.h).
static size_t multi_counts_offset(int64_t n_queries, int d) { return carve_async(n_queries, d, nullptr).total; }
extern "C" size_t om_sim_topk_filtered_multi_workspace_bytes(int64_t n_queries, int d, int k, int64_t n_filters) {
  (void)k;
  if (n_queries <= 0 || d <= 0 || n_filters < 1) return 0;
  return multi_counts_offset(n_queries, d) + align_up((size_t)n_filters * 4, 256);
}

extern "C" int om_sim_topk_filtered_multi(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                                          const float* stats, int64_t N, int d, int k, int64_t id_offset, const uint32_t* allow_bits,
                                          int64_t words_pitch, int64_t n_filters, const int32_t* filter_of, int64_t n_allowed_min,
                                          float* out_scores, int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (n_queries <= 0) return 0;
  Scan sc;
  if (const char* why = scan_setup(sc, mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, stream))
    OM_FAIL(why);
  if (mode == OM_SEARCH_F16_ONLY) {
    if (const char* why = f16_only_refusal(sc)) OM_FAIL(why);
  }
  if (d > 16384) OM_FAIL("d above 16384: a row does not fit the redo's LDS tile");
  if (!sc.sw.gen7) OM_FAIL("OM_OPT_SCAN_GEN7 is 0: the fast schedule this entry runs is switched off");
  if (!allow_bits) OM_FAIL("allow_bits is null: the filtered search needs the bitmaps of the allowed rows (om_sim_topk_async searches all rows)");
  if (n_filters < 1 || n_filters > 65535) OM_FAIL("n_filters must be in [1, 65535]");
  if (words_pitch < (N + 31) / 32) OM_FAIL("words_pitch is below (N + 31) / 32, the words of one bitmap");
  if (!filter_of && n_filters != n_queries) OM_FAIL("filter_of is null: query q is under bitmap q, which needs n_filters == n_queries");
  if (n_allowed_min < 0 || n_allowed_min > N) OM_FAIL("n_allowed_min must be in [0, N]");
  const AsyncWs aw = carve_async(n_queries, d, (char*)workspace);
  if (om_sim_topk_filtered_multi_workspace_bytes(n_queries, d, k, n_filters) > workspace_bytes)
    OM_FAIL("workspace too small (om_sim_topk_filtered_multi_workspace_bytes)");
  sc.qstat = aw.qstat;
  sc.filt = RowFilters{allow_bits, words_pitch, n_filters, filter_of, 1};
  sc.n_allowed = n_allowed_min;
  sc.fcount = (unsigned*)((char*)workspace + multi_counts_offset(n_queries, d));
  if (search_attrs()) return 1;
  return sc.run_async(search_mode_half(mode), aw, id_offset, out_scores, out_ids, status);
}

// ---- om_sim_topk_candidates: the exact top-k of every query over its OWN candidate rows ------------------------------------------------
// No scan, no margin, no redo: init -> per block of CAND_BLOCK candidate columns (score_candidates_kernel -> select_kernel in exact mode,
// which keeps the best k by the 64-bit key) -> emit.  A list never holds more than k + CAND_BLOCK <= SORT_CAP keys, and keys of distinct
// rows never tie, so there is nothing to overflow and nothing to redo.  The chain is fixed by cand_pitch alone; the cost is
// n_queries * cand_pitch * d, whatever N.
struct CandWs { u64* keys; unsigned *cnt, *cnt_prev, *flag; float* thr; size_t total; };
static CandWs carve_candidates(int64_t nq, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  CandWs w;
  w.keys = (u64*)take((size_t)nq * SORT_CAP * 8);
  w.cnt = (unsigned*)take((size_t)nq * 4);
  w.cnt_prev = (unsigned*)take((size_t)nq * 4);
  w.flag = (unsigned*)take(64);
  w.thr = (float*)take(((size_t)(nq + 255) / 256 * 256 + 256) * 4);      // init_lists_kernel writes a whole tile beyond nq
  w.total = off;
  return w;
}

extern "C" size_t om_sim_topk_candidates_workspace_bytes(int64_t n_queries, int d, int k) {
  (void)d; (void)k;
  if (n_queries <= 0) return 0;
  return carve_candidates(n_queries, nullptr).total;
}

extern "C" int om_sim_topk_candidates(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16, int64_t N,
                                      int d, int k, int64_t id_offset, const int32_t* cand, int64_t cand_pitch, float* out_scores,
                                      int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_queries <= 0) return 0;
  if (mode != OM_SEARCH_F32 && mode != OM_SEARCH_F16_RESCORE && mode != OM_SEARCH_F16_ONLY) OM_FAIL("mode must be one of OM_SEARCH_*");
  if (k < 1 || k > K_MAX) OM_FAIL("k must be in [1,2048]");
  if (N < 0 || N > 0x7fffffffLL) OM_FAIL("N: a candidate is an int32 row number, the shard holds at most 2^31 - 1 rows");
  if (d <= 0 || (d * 2) % GEMM_ROW_BYTES != 0) OM_FAIL("d must be a multiple of 64 (pad with zeros)");
  if (n_queries > 65535) OM_FAIL("at most 65535 queries per call");
  if (!queries || !out_scores || !out_ids) OM_FAIL("null argument");
  if (!cand) OM_FAIL("cand is null: the candidate rows of every query");
  if (cand_pitch < 1) OM_FAIL("cand_pitch must be at least 1");
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  const bool rows16 = mode == OM_SEARCH_F16_ONLY;
  if (N > 0 && rows16 && !index_f16) OM_FAIL("OM_SEARCH_F16_ONLY: index_f16 is null (the float16 rows are the index)");
  if (N > 0 && !rows16 && !index_f32) OM_FAIL("index_f32 is null: the candidates are scored on the float32 rows");
  const CandWs ws = carve_candidates(n_queries, (char*)workspace);
  if (ws.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_candidates_workspace_bytes)");
  if (search_attrs()) return 1;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned nq = (unsigned)n_queries;
  hipLaunchKernelGGL(init_lists_kernel, dim3((unsigned)((n_queries + 255) / 256 + 2)), dim3(256), 0, s, ws.cnt, ws.cnt_prev, ws.thr, n_queries,
                     ws.flag);
  OM_LAUNCH_CHECK();
  for (int64_t col0 = 0; col0 < cand_pitch; col0 += CAND_BLOCK) {
    const int ncols = (int)std::min<int64_t>(CAND_BLOCK, cand_pitch - col0);
    const dim3 grid((unsigned)((ncols + 3) / 4), nq);
    if (rows16)
      hipLaunchKernelGGL(score_candidates_kernel<f16_t>, grid, dim3(256), 0, s, queries, (const f16_t*)index_f16, N, d, cand, cand_pitch, col0,
                         ncols, ws.keys, ws.cnt);
    else
      hipLaunchKernelGGL(score_candidates_kernel<float>, grid, dim3(256), 0, s, queries, index_f32, N, d, cand, cand_pitch, col0, ncols, ws.keys,
                         ws.cnt);
    OM_LAUNCH_CHECK();
    hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(SORT_THREADS), SORT_CAP * 8 + 16, s, ws.keys, ws.cnt, ws.cnt_prev, ws.thr,
                       (const float*)nullptr, k, ws.flag, (unsigned*)nullptr);
    OM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(emit_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, k, id_offset, out_scores, out_ids);
  OM_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t om_sim_topk_filtered_workspace_bytes(int64_t n_queries, int d, int k) {
  return om_sim_topk_async_workspace_bytes(n_queries, d, k);
}

extern "C" int om_debug_search_schedule_filtered(int mode, int64_t nq, int64_t N, int k, int64_t n_allowed, int64_t* chunks, int cap, int* n,
                                                 int64_t* boot) {
  if (!n || !boot || (cap > 0 && !chunks)) OM_FAIL("null argument");
  if (nq < 1 || N < 0 || k < 1 || k > K_MAX) OM_FAIL("nq >= 1, N >= 0 and k in [1,2048]");
  if (n_allowed < 0 || n_allowed > N) OM_FAIL("n_allowed must be in [0, N]");
  *n = search_schedule_filtered(search_mode_half(mode), nq, N, k, n_allowed, scan_switches(), chunks, cap < 0 ? 0 : cap, boot).n;
  return 0;
}

extern "C" int om_debug_search_filter_estimate(int mode, int64_t N, int k, int64_t n_allowed, int64_t* list_eff, int64_t* list_max) {
  if (!list_eff || !list_max) OM_FAIL("null argument");
  if (N < 1 || k < 1 || k > K_MAX) OM_FAIL("N >= 1 and k in [1,2048]");
  if (n_allowed < 1 || n_allowed > N) OM_FAIL("n_allowed must be in [1, N]");
  *list_eff = search_list_estimate(search_mode_half(mode), search_k_eff(k, N, n_allowed));
  *list_max = LIST_MAX;
  return 0;
}

extern "C" int om_debug_sim_stream(const void* rows16, int64_t nrows, uint32_t row_base, const void* queries16, int64_t nq, int d, const float* thr,
                                   uint64_t* keys, unsigned* cnt, int grid, void* stream) {
  if (!rows16 || !queries16 || !thr || !keys || !cnt) OM_FAIL("null argument");
  if (nrows <= 0 || nrows % SR_UROWS != 0) OM_FAIL("whole 128-row tiles only");
  if (grid < 1 || grid > 65535) OM_FAIL("grid must be in [1,65535]");
  const ScanSwitches sw = scan_switches();
  const ScanPlan plan = scan_plan(true, nq, d, sw);
  if (plan.family != OM_SCAN_FAMILY_STREAM32 && plan.family != OM_SCAN_FAMILY_STREAM16)
    OM_FAIL("the scan plan sends this (nq, d) to no stream kernel");
  if (scan_attrs()) return 1;
  if (scan_launch(scan_kernel(OM_SCAN_KERNEL_STREAM, true, plan, sw), rows16, nrows, row_base, queries16, nq, d, thr, (u64*)keys, cnt, grid, sw.nt,
                  (hipStream_t)stream)) return 1;
  OM_LAUNCH_CHECK();
  return 0;
}

// One launch of a tile kernel of g_tile_kernels over a caller's buffers, through scan_kernel / scan_attrs / scan_launch as
// Scan::filter_step launches a planned round: `grid` and `group` are what scan_round would hand over (generation 7: group_m | qgroup << 8).
// What is refused: below.  What CANNOT be checked here and is the caller's to keep, from the kernels' own comments:
//   * generations 6 and 7 read whole 256-query tiles: `queries` holds round_up(nq, 256) rows, zero beyond nq (query_prep_kernel);
//   * generation 7 fetches 256 thresholds from the middle of a query tile on: `thr` is readable for round_up(nq, 256) + 256 entries and
//     +inf beyond nq (init_lists_kernel) -- a finite value there appends keys of the zero rows to lists that do not exist;
//   * keys is [nq][SORT_CAP], cnt is [nq] and is NOT cleared: survivors are appended behind the cnt[q] keys a list already holds, cnt
//     counts every survivor and keys holds those whose position is below SORT_CAP.
extern "C" int om_debug_scan_kernel(int kernel, int half, const void* rows, int64_t nrows, uint32_t row_base, const void* queries, int64_t nq,
                                    int d, const float* thr, uint64_t* keys, unsigned* cnt, int64_t grid, int group, void* stream) {
  if (!rows || !queries || !thr || !keys || !cnt) OM_FAIL("null argument");
  if (kernel < OM_SCAN_KERNEL_TILE2 || kernel > OM_SCAN_KERNEL_WIDE7C)
    OM_FAIL("kernel must be OM_SCAN_KERNEL_TILE2, TILE6, WIDE7 or WIDE7C (the stream kernel: om_debug_sim_stream)");
  const ScanSwitches sw = scan_switches();
  const ScanKernel& kn = scan_kernel(kernel, half != 0, ScanPlan{OM_SCAN_FAMILY_GENERIC, 0, 0, 0}, sw);
  if (!kn.fn) OM_FAIL("no such scan kernel: generation 7 scans the 16-bit index only");
  if (d <= 0 || d % SCAN_KSTEP != 0) OM_FAIL("d must be a positive multiple of 64");
  if (nrows < 1 || nq < 1) OM_FAIL("nrows >= 1 and nq >= 1");
  if (grid < 1 || grid > 0x7fffffffLL) OM_FAIL("grid must be in [1, 2^31 - 1]");
  if ((group & 255) < 1) OM_FAIL("group_m (the low byte of group) must be at least 1");
  if (kernel >= OM_SCAN_KERNEL_WIDE7) {
    if (nrows % 256 != 0) OM_FAIL("generation 7 takes whole 256-row tiles only");
    if (kernel == OM_SCAN_KERNEL_WIDE7C && !g7_ring_ok(d)) OM_FAIL("the continuous ring needs three 128-byte K steps: d >= 192");
  } else {
    // a tile-at-a-time workgroup takes its tile from its block index and tests no bound: one workgroup per (row tile, query tile)
    const int64_t qt = kernel == OM_SCAN_KERNEL_TILE2 ? (nq + 127) / 128 : (nq + 255) / 256;
    if ((nrows + 255) / 256 > 0x7fffffffLL / qt || grid != (nrows + 255) / 256 * qt)
      OM_FAIL("generations 2 and 6 take one workgroup per (256-row tile, query tile): grid must be their number");
  }
  if (scan_attrs()) return 1;
  if (scan_launch(kn, rows, nrows, row_base, queries, nq, d, thr, (u64*)keys, cnt, grid, group, (hipStream_t)stream)) return 1;
  OM_LAUNCH_CHECK();
  return 0;
}

// ---- om_debug_rescore_rows: the row-typed kernels (re-score, strided re-score, the redo's collect pass) over a caller's candidates ----
// cand -> lists: list q = rows cand[q][0 .. m) in order, scores 0.  A row number beyond the index is not followed (its score comes back NaN).
__global__ void debug_fill_lists_kernel(const uint32_t* __restrict__ cand, int m, int64_t N, u64* __restrict__ keys, unsigned* __restrict__ cnt) {
  const int64_t q = blockIdx.x;
  for (int j = threadIdx.x; j < m; j += blockDim.x) {
    const uint32_t row = cand[q * m + j];
    keys[q * SORT_CAP + j] = pack_key(0.f, (int64_t)row < N ? row : 0u);
  }
  if (threadIdx.x == 0) cnt[q] = (unsigned)m;
}
// every query marked for the redo with prefix 0 (every key passes the collect pass), lists emptied
__global__ void debug_mark_all_kernel(int64_t nq, unsigned* __restrict__ rs, unsigned* __restrict__ bad, u64* __restrict__ prefix,
                                      unsigned* __restrict__ cnt) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < 16) rs[q] = q == REDO_RS_BAD ? (unsigned)nq : 0u;
  if (q < nq) { bad[q] = (unsigned)q; prefix[q] = 0; cnt[q] = 0; }
}
// by_row = 0: out[q][j] = score of slot j (cand[q][j] beyond the index: NaN);  by_row = 1: out[q][row] = score of the slot that names row
__global__ void debug_read_lists_kernel(const u64* __restrict__ keys, const unsigned* __restrict__ cnt, const uint32_t* __restrict__ cand, int m,
                                        int64_t N, int by_row, float* __restrict__ out) {
  const int64_t q = blockIdx.x;
  const unsigned n = cnt[q] < (unsigned)m ? cnt[q] : (unsigned)m;
  for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
    const u64 key = keys[q * SORT_CAP + j];
    if (by_row) {
      if (key_payload(key) < (uint32_t)m) out[q * m + key_payload(key)] = key_score(key);
    } else {
      out[q * m + j] = (int64_t)cand[q * m + j] < N ? key_score(key) : __builtin_nanf("");
    }
  }
}

extern "C" int om_debug_rescore_rows(int kernel, int row_dtype, const void* rows, int64_t N, int d, const float* queries, int64_t n_queries,
                                     const uint32_t* cand, int m, float* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
  if (row_dtype != OM_F32 && row_dtype != OM_F16) OM_FAIL("om_debug_rescore_rows: row dtype must be OM_F32 or OM_F16");
  if (kernel < 0 || kernel > 2) OM_FAIL("om_debug_rescore_rows: kernel must be 0 (re-score), 1 (strided re-score) or 2 (redo collect pass)");
  if (!rows || !queries || !out_scores || (kernel != 2 && !cand)) OM_FAIL("om_debug_rescore_rows: null argument");
  if (N < 1 || N > 0xffffffffLL || n_queries < 1 || n_queries > 65535) OM_FAIL("om_debug_rescore_rows: N in [1, 2^32) and 1 to 65535 queries");
  if (d <= 0 || d % 64 != 0 || d > 16384) OM_FAIL("om_debug_rescore_rows: d must be a multiple of 64, at most 16384");
  if (m < 1 || m > SORT_CAP) OM_FAIL("om_debug_rescore_rows: 1 to 8192 candidates per query");
  if (kernel == 2 && (int64_t)m != N) OM_FAIL("om_debug_rescore_rows: the redo pass scores every row: m must be N (at most 8192)");
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("om_debug_rescore_rows: workspace must be 256-byte aligned");
  const SearchWs ws = carve_search(n_queries, d, (char*)workspace);
  const AsyncWs aw = carve_async(n_queries, d, (char*)workspace);
  if (aw.total > workspace_bytes) OM_FAIL("om_debug_rescore_rows: workspace too small (om_sim_topk_async_workspace_bytes)");
  const hipStream_t s = (hipStream_t)stream;
  const bool h = row_dtype == OM_F16;
  const f16_t* r16 = (const f16_t*)rows;
  const float* r32 = (const float*)rows;
  const unsigned nq = (unsigned)n_queries;
  if (kernel == 2) {
    hipLaunchKernelGGL(debug_mark_all_kernel, dim3((nq + 255) / 256 + 1), dim3(256), 0, s, n_queries, aw.rs, aw.bad, aw.prefix, ws.cnt);
    const int R = (int)std::max<int64_t>(1, std::min<int64_t>(32, REDO_TILE_BYTES / ((int64_t)d * 4)));
    const size_t lds = (size_t)R * d * 4;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((N + R - 1) / R, (int64_t)g7_num_cus() * 4)));
    if (h) hipLaunchKernelGGL((redo_pass_kernel<true, f16_t>), grid, dim3(256), lds, s, queries, r16, N, d, R, aw.rs, aw.bad, aw.prefix, aw.hist, 0, 0, ws.keys, ws.cnt, RowFilters{nullptr, 0, 0, nullptr, 0});
    else hipLaunchKernelGGL((redo_pass_kernel<true, float>), grid, dim3(256), lds, s, queries, r32, N, d, R, aw.rs, aw.bad, aw.prefix, aw.hist, 0, 0, ws.keys, ws.cnt, RowFilters{nullptr, 0, 0, nullptr, 0});
  } else {
    hipLaunchKernelGGL(debug_fill_lists_kernel, dim3(nq), dim3(256), 0, s, cand, m, N, ws.keys, ws.cnt);
    if (kernel == 0) {
      const dim3 grid(((unsigned)m + 3) / 4, nq);
      if (h) hipLaunchKernelGGL(rescore_kernel<f16_t>, grid, dim3(256), 0, s, queries, r16, ws.keys, ws.cnt, d);
      else hipLaunchKernelGGL(rescore_kernel<float>, grid, dim3(256), 0, s, queries, r32, ws.keys, ws.cnt, d);
    } else {
      const dim3 grid((unsigned)(g7_num_cus() * 8));
      if (h) hipLaunchKernelGGL(rescore_strided_kernel<f16_t>, grid, dim3(256), 0, s, queries, r16, ws.keys, ws.cnt, n_queries, d);
      else hipLaunchKernelGGL(rescore_strided_kernel<float>, grid, dim3(256), 0, s, queries, r32, ws.keys, ws.cnt, n_queries, d);
    }
  }
  OM_LAUNCH_CHECK();
  hipLaunchKernelGGL(debug_read_lists_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, cand, m, N, kernel == 2 ? 1 : 0, out_scores);
  OM_LAUNCH_CHECK();
  return 0;
}

// ---- om_debug_select_lists / om_debug_query_prep: the list kernels (selections, drop, dense append, emit) and the query preparation -------
// over a caller's lists, launched as Scan launches them
#define DEBUG_STALE_ROW 0xf0000000u      // stale slots: score +inf, row DEBUG_STALE_ROW + slot
__global__ void debug_put_lists_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ counts,
                                       const float* __restrict__ margin_in, int m, u64* __restrict__ keys, unsigned* __restrict__ cnt,
                                       unsigned* __restrict__ cnt_prev, float* __restrict__ thr, float* __restrict__ margin,
                                       unsigned* __restrict__ flag, unsigned* __restrict__ qstat) {
  const int64_t q = blockIdx.x;
  for (int j = threadIdx.x; j < SORT_CAP; j += blockDim.x)
    keys[q * SORT_CAP + j] = j < m ? pack_key(scores[q * m + j], rows[q * m + j]) : pack_key(INFINITY, DEBUG_STALE_ROW + (uint32_t)j);
  if (threadIdx.x == 0) {
    cnt[q] = counts[q] < 2u * SORT_CAP ? counts[q] : 2u * SORT_CAP;
    cnt_prev[q] = 0xffffffffu;
    thr[q] = __builtin_nanf("");
    margin[q] = margin_in ? margin_in[q] : 0.f;
    qstat[q] = 0u;
  }
  if (q == 0 && threadIdx.x < 16) flag[threadIdx.x] = 0u;
}
__global__ void debug_get_lists_kernel(const u64* __restrict__ keys, const unsigned* __restrict__ cnt, const unsigned* __restrict__ cnt_prev,
                                       const float* __restrict__ thr, const unsigned* __restrict__ flag, const unsigned* __restrict__ qstat,
                                       float* __restrict__ out_scores, uint32_t* __restrict__ out_rows, uint32_t* __restrict__ out_state) {
  const int64_t q = blockIdx.x, nq = gridDim.x;
  for (int j = threadIdx.x; j < SORT_CAP; j += blockDim.x) {
    const u64 key = keys[q * SORT_CAP + j];
    if (out_scores) out_scores[q * SORT_CAP + j] = key_score(key);
    if (out_rows) out_rows[q * SORT_CAP + j] = key_payload(key);
  }
  if (out_state && threadIdx.x == 0) {
    out_state[q * 4] = cnt[q]; out_state[q * 4 + 1] = cnt_prev[q];
    out_state[q * 4 + 2] = __builtin_bit_cast(uint32_t, thr[q]); out_state[q * 4 + 3] = qstat[q];
  }
  if (out_state && q == 0 && threadIdx.x < 4) out_state[nq * 4 + threadIdx.x] = flag[threadIdx.x];
}

extern "C" int om_debug_select_lists(int op, int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int k,
                                     const float* margin, int use_qstat, int cap, const uint32_t* allow, uint32_t nrows, const float* S,
                                     int64_t ldS, int n, uint32_t row_base, uint32_t cover, int64_t id_offset, float* emit_scores,
                                     int64_t* emit_ids, float* out_scores, uint32_t* out_rows, uint32_t* out_state, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (op < OM_DEBUG_LISTS_RADIX || op > OM_DEBUG_LISTS_EMIT)
    OM_FAIL("op must be 0 (radix selection), 1 (sorting selection), 2 (drop), 3 (dense append + overflow check) or 4 (emit)");
  if (!scores || !rows || !counts) OM_FAIL("null argument: scores, rows and counts describe the lists");
  if (n_queries < 1 || n_queries > 65535) OM_FAIL("1 to 65535 queries");
  if (m < 1 || m > SORT_CAP) OM_FAIL("m must be in [1, 8192]");
  if (k < 1 || k > K_MAX) OM_FAIL("k must be in [1, 2048]");
  if (op == OM_DEBUG_LISTS_RADIX && cap != 4096 && cap != SORT_CAP) OM_FAIL("cap must be 4096 or 8192");
  if (op == OM_DEBUG_LISTS_DROP && (!allow || nrows < 1)) OM_FAIL("the drop needs the bitmap (null argument) and nrows >= 1");
  if (op == OM_DEBUG_LISTS_APPEND && (!S || n < 1 || n > DENSE_CHUNK || ldS < n)) OM_FAIL("the dense append needs S (null argument), n in [1, 4096] and ldS >= n");
  if (op == OM_DEBUG_LISTS_EMIT && (!emit_scores || !emit_ids)) OM_FAIL("null argument: emit writes emit_scores and emit_ids");
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  const SearchWs ws = carve_search(n_queries, 64, (char*)workspace);
  const AsyncWs aw = carve_async(n_queries, 64, (char*)workspace);
  if (aw.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_async_workspace_bytes(n_queries, 64, 1))");
  if (search_attrs()) return 1;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned nq = (unsigned)n_queries;
  unsigned* const qstat = use_qstat ? aw.qstat : nullptr;
  const float* const mg = margin ? ws.margin : nullptr;
  hipLaunchKernelGGL(debug_put_lists_kernel, dim3(nq), dim3(256), 0, s, scores, rows, counts, margin, m, ws.keys, ws.cnt, ws.cnt_prev, ws.thr,
                     ws.margin, ws.flag, aw.qstat);
  OM_LAUNCH_CHECK();
  switch (op) {
    case OM_DEBUG_LISTS_RADIX:
      hipLaunchKernelGGL(select_radix_kernel, dim3(nq), dim3(256), (size_t)cap * 8 + 1024 + 64, s, ws.keys, ws.cnt, ws.thr, mg, k, ws.flag, cap,
                         qstat);
      break;
    case OM_DEBUG_LISTS_SORT:
      hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(SORT_THREADS), SORT_CAP * 8 + 16, s, ws.keys, ws.cnt, ws.cnt_prev, ws.thr, mg, k, ws.flag,
                         qstat);
      break;
    case OM_DEBUG_LISTS_DROP:
      hipLaunchKernelGGL(drop_disallowed_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, RowFilters{allow, 0, 1, nullptr, 0}, nrows, ws.flag, qstat);
      break;
    case OM_DEBUG_LISTS_APPEND:
      hipLaunchKernelGGL(append_dense_kernel, dim3(nq), dim3(256), 0, s, S, ldS, n, row_base, ws.keys, ws.cnt);
      OM_LAUNCH_CHECK();
      hipLaunchKernelGGL(check_overflow_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, ws.cnt, n_queries, ws.flag, qstat, cover);
      break;
    default:
      hipLaunchKernelGGL(emit_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, k, id_offset, emit_scores, emit_ids);
      break;
  }
  OM_LAUNCH_CHECK();
  hipLaunchKernelGGL(debug_get_lists_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, ws.cnt_prev, ws.thr, ws.flag, aw.qstat, out_scores,
                     out_rows, out_state);
  OM_LAUNCH_CHECK();
  return 0;
}

// om_debug_select_lists' OM_DEBUG_LISTS_DROP with the bitmaps of om_sim_topk_filtered_multi: the drop as that entry launches it
extern "C" int om_debug_drop_lists_multi(int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int use_qstat,
                                         const uint32_t* allow, uint32_t nrows, int64_t words_pitch, int64_t n_filters, const int32_t* filter_of,
                                         float* out_scores, uint32_t* out_rows, uint32_t* out_state, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  if (!scores || !rows || !counts) OM_FAIL("null argument: scores, rows and counts describe the lists");
  if (n_queries < 1 || n_queries > 65535) OM_FAIL("1 to 65535 queries");
  if (m < 1 || m > SORT_CAP) OM_FAIL("m must be in [1, 8192]");
  if (!allow || nrows < 1) OM_FAIL("the drop needs the bitmaps (allow is null) and nrows >= 1");
  if (n_filters < 1) OM_FAIL("n_filters must be at least 1");
  if (words_pitch < ((int64_t)nrows + 31) / 32) OM_FAIL("words_pitch is below (nrows + 31) / 32, the words of one bitmap");
  if (!filter_of && n_filters != n_queries) OM_FAIL("filter_of is null: query q is under bitmap q, which needs n_filters == n_queries");
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  const SearchWs ws = carve_search(n_queries, 64, (char*)workspace);
  const AsyncWs aw = carve_async(n_queries, 64, (char*)workspace);
  if (aw.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_async_workspace_bytes(n_queries, 64, 1))");
  const hipStream_t s = (hipStream_t)stream;
  const unsigned nq = (unsigned)n_queries;
  hipLaunchKernelGGL(debug_put_lists_kernel, dim3(nq), dim3(256), 0, s, scores, rows, counts, (const float*)nullptr, m, ws.keys, ws.cnt,
                     ws.cnt_prev, ws.thr, ws.margin, ws.flag, aw.qstat);
  OM_LAUNCH_CHECK();
  hipLaunchKernelGGL(drop_disallowed_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, RowFilters{allow, words_pitch, n_filters, filter_of, 1},
                     nrows, ws.flag, use_qstat ? aw.qstat : (unsigned*)nullptr);
  OM_LAUNCH_CHECK();
  hipLaunchKernelGGL(debug_get_lists_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, ws.cnt_prev, ws.thr, ws.flag, aw.qstat, out_scores,
                     out_rows, out_state);
  OM_LAUNCH_CHECK();
  return 0;
}

extern "C" int om_debug_query_prep(const float* queries, int64_t n_queries, int d, const float* stats, void* out_q16, float* out_margin,
                                   void* stream) {
  if (!queries || !stats || !out_q16 || !out_margin) OM_FAIL("null argument");
  if (n_queries < 1 || n_queries > 65535 || d < 1 || d > 16384) OM_FAIL("1 to 65535 queries, d in [1, 16384]");
  hipLaunchKernelGGL(query_prep_kernel, dim3((unsigned)(((n_queries + 255) / 256 * 256 + 3) / 4)), dim3(256), 0, (hipStream_t)stream, queries,
                     (f16_t*)out_q16, out_margin, stats, n_queries, d);
  OM_LAUNCH_CHECK();
  return 0;
}
