// The scan kernels of the exact inner-product search (search.hip has the method, the list kernels and the host chain), gfx950: the
// threshold-filtered GEMM of generations 2, 6, 7 and 7c for query tiles and the register-resident stream scan for small batches, one
// table for their LDS attributes and launches, and the two debug hooks that launch them alone.  The rest of the search code reaches them
// through search_scan.h only.
#include "search_scan.h"

#include "gemm_core2.h"
#include "gemm_core6.h"
#include "gemm_wide7.h"

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
//  * two-level walk: a block with a survivor tests its four register quads and walks only the (one, almost always) quad that
//    holds it -- ~8 ballot + branch steps instead of 16 (round 4 put one test per ROW block in front: scan7_filter below);
//  * the append is split around the NEXT tile's K loop: at the end of a tile's filter its (<= 64, one per lane)
//    records move from the staging area into registers; after the next K loop the list-counter atomics are issued,
//    their return is consumed half a filter later and the key stores leave half a filter before the tile start that
//    would otherwise wait for their acknowledgement (vmcnt retires in order).  Neither round trip is exposed.  More
//    than 64 records in a tile, or a full staging area, take the synchronous flush (rare);
//  * the tile walk advances incrementally (no division per tile), and the DMA lane offsets are computed once: the
//    query panel is padded with zero rows to a whole tile (query_prep_kernel), so no tile needs clamped rows.
//
// Both generation-7 kernels (the one below and the continuous ring behind it) share the staged append; what differs is WHERE a wave stages,
// which a Stage policy carries: key_slot(pos) / q_slot(pos) of staged record pos, and CAP, the records the area holds.
#define SC7_QIDX_OFF (G7_TAB_OFF + 4096)
struct Sc7Stage {      // the restart-per-tile kernel: the layout described above
  char* smem; int wave;
  static constexpr unsigned CAP = 2048;
  __device__ __forceinline__ char* key_slot(unsigned pos) const {
    return smem + (2 + (pos >> 10)) * G7_UNIT_BYTES + wave * 1024 + ((pos >> 7) & 7) * 4096 + (pos & 127) * 8;
  }
  __device__ __forceinline__ uint16_t* q_slot(unsigned pos) const { return (uint16_t*)(smem + SC7_QIDX_OFF + wave * (CAP * 2) + pos * 2); }
};
// synchronous append of staged records [from, wcount): one atomic round trip, then the stores
template <typename Stage>
__device__ __forceinline__ void scan7_flush(const Stage& st, unsigned from, unsigned wcount, int lane, int64_t q0, u64* __restrict__ keys,
                                            unsigned* __restrict__ cnt) {
  for (unsigned i = from + (unsigned)lane; i < wcount; i += 64) {
    const u64 key = *(const u64*)st.key_slot(i);
    const int64_t q = q0 + *st.q_slot(i);
    const unsigned pos = atomicAdd(cnt + q, 1u);
    if (pos < SORT_CAP) keys[q * SORT_CAP + pos] = key;
  }
}
__device__ __forceinline__ float scan7_max3(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float scan7_max16(const f32x16_t& a) {      // eight v_max3 (the compiler's fmaxf tree: 13 v_max + 5 v_max3)
  const float t0 = scan7_max3(a[0], a[1], a[2]), t1 = scan7_max3(a[3], a[4], a[5]), t2 = scan7_max3(a[6], a[7], a[8]);
  const float t3 = scan7_max3(a[9], a[10], a[11]), t4 = scan7_max3(a[12], a[13], a[14]);
  return scan7_max3(scan7_max3(t0, t1, t2), scan7_max3(t3, t4, a[15]), t0);
}
// Query blocks MI0 .. MI1-1 of the wave's 128 x 128 scores; whole tiles only: every row of the tile exists.
// One row block of queries (mi) against the wave's 128 index rows: the common case -- no score of the block's 64 per lane reaches
// its query's threshold -- is 64 accumulator reads, 33 v_max3, ONE compare and ONE branch; the survivor path is laid out as cold
// code behind the straight line.  Tile trace at the benchmark's size (profiles/r04_probe16_scan_filter_phases.log): filter 5.4 k
// cycles per tile with one test per column block and the survivor code inline (each test 5 KB from the next), 4.7 k like this;
// 3.4 survivors per wave and tile cost ~850 cycles each, the 16 block tests ~1.8 k.  A COMPACT survivor path (scores parked in LDS,
// run-time loop over the score indices: 70 KB of code down to 12) measured 8.9 k -- the unrolled per-score code is the faster one,
// the instruction cache is not what it waits for.
template <int MI0, int MI1, typename Stage>
__device__ __forceinline__ void scan7_filter(f32x16_t (&acc)[4][4], const float (&th)[4], uint32_t id0, uint32_t ql0, int lane, const Stage& st,
                                             unsigned& wcount, int64_t q0, u64* __restrict__ keys, unsigned* __restrict__ cnt) {
#pragma unroll
  for (int mi = MI0; mi < MI1; ++mi) {
    f32x16_t a[4];
    float bm[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      asm volatile("" : "+a"(acc[mi][ni]));            // stays in its AGPRs until this point
      a[ni] = acc[mi][ni];
      bm[ni] = scan7_max16(a[ni]);
    }
    const float mx = scan7_max3(scan7_max3(bm[0], bm[1], bm[2]), bm[3], bm[3]);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx >= th[mi]) != 0, 0)) {          // wave-uniform: some lane holds a survivor
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        if (__builtin_amdgcn_ballot_w64(bm[ni] >= th[mi]) == 0) continue;
        if (wcount > Stage::CAP - 1024) { scan7_flush(st, 0u, wcount, lane, q0, keys, cnt); wcount = 0; }      // a block adds at most 1024
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
                *(u64*)st.key_slot(pos) = pack_key(a[ni][r], id0 + off);
                *st.q_slot(pos) = (uint16_t)(ql0 + mi * 32);
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
      const Sc7Stage st = {smem, wave};
      scan7_filter<0, 2>(acc, th, id0, ql0, lane, st, wcount, qc, keys, cnt);
      if (pend_n) {
        if ((unsigned)lane < pend_n && pend_pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pend_pos] = pend_key;
        pend_n = 0;
      }
      G7_FENCE_();
      scan7_filter<2, 4>(acc, th, id0, ql0, lane, st, wcount, qc, keys, cnt);
      if (wcount > 64) scan7_flush(st, 64u, wcount, lane, qc, keys, cnt);
      pend_n = wcount < 64u ? wcount : 64u;
      if ((unsigned)lane < pend_n) {
        pend_key = *(const u64*)st.key_slot((unsigned)lane);
        pend_q = (uint32_t)qc + *st.q_slot((unsigned)lane);
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
struct Sc7cStage {
  char* bn; char* sp;
  static constexpr unsigned CAP = 1536;
  __device__ __forceinline__ char* key_slot(unsigned pos) const {
    const unsigned sl = pos >> 7;
    return (sl < 8 ? bn + sl * 4096 : sp + (sl - 8) * 4096) + (pos & 127) * 8;
  }
  __device__ __forceinline__ uint16_t* q_slot(unsigned pos) const { return (uint16_t*)(sp + (4 + (pos >> 9)) * 4096 + (pos & 511) * 2); }
};

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
      scan7_filter<0, 2>(acc, th, id0, ql0, lane, st, wcount, q0, keys, cnt);
      if (pend_n) {
        if ((unsigned)lane < pend_n && pend_pos < SORT_CAP) keys[(int64_t)pend_q * SORT_CAP + pend_pos] = pend_key;
        pend_n = 0;
      }
      G7_FENCE_();
      if (tr && threadIdx.x == 0) tr[17] = clock64();
      scan7_filter<2, 4>(acc, th, id0, ql0, lane, st, wcount, q0, keys, cnt);
      if (tr && threadIdx.x == 0) { tr[18] = clock64(); tr[20] = wcount; }
      if (wcount > 64) scan7_flush(st, 64u, wcount, lane, q0, keys, cnt);
      pend_n = wcount < 64u ? wcount : 64u;
      if ((unsigned)lane < pend_n) {
        pend_key = *(const u64*)st.key_slot((unsigned)lane);
        pend_q = (uint32_t)q0 + *st.q_slot((unsigned)lane);
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
int scan_attrs() {
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

// The one launcher of the scan kernels: rows [l.rows, d] with ids from row_base against the queries, survivors appended to keys / cnt.
int scan_launch(const ScanPlan& plan, const ScanLaunch& l, bool half, const ScanSwitches& sw, const void* rows, uint32_t row_base,
                const void* queries, int64_t nq, int d, const float* thr, u64* keys, unsigned* cnt, hipStream_t s) {
  const ScanKernel& kn = scan_kernel(l.kernel, half, plan, sw);
  if (!kn.fn) OM_FAIL("the scan plan names a kernel that does not exist");
  int64_t nrows = l.rows, d64 = d;
  int group = l.group;
  unsigned long long* trace = kn.trace ? omk_debug_trace() : nullptr;
  void* args[] = {&rows, &nrows, &row_base, &queries, &nq, &d64, &thr, &keys, &cnt, &group, &trace};      // (trace: generation 7 only)
  OM_HIP(hipLaunchKernel(kn.fn, dim3((unsigned)l.grid), dim3((unsigned)kn.threads), args, (size_t)kn.lds, s));
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
  if (scan_launch(plan, ScanLaunch{OM_SCAN_KERNEL_STREAM, 0, nrows, grid, sw.nt}, true, sw, rows16, row_base, queries16, nq, d, thr, (u64*)keys,
                  cnt, (hipStream_t)stream)) return 1;
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
  const ScanPlan plan = {OM_SCAN_FAMILY_GENERIC, 0, 0, 0};
  if (!scan_kernel(kernel, half != 0, plan, sw).fn) OM_FAIL("no such scan kernel: generation 7 scans the 16-bit index only");
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
  if (scan_launch(plan, ScanLaunch{kernel, 0, nrows, grid, group}, half != 0, sw, rows, row_base, queries, nq, d, thr, (u64*)keys, cnt,
                  (hipStream_t)stream)) return 1;
  OM_LAUNCH_CHECK();
  return 0;
}
