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
// This unit holds the list kernels and the host chain; the scan kernels of step 2 are search_scan.hip, reached through the two functions
// of search_scan.h.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "gemm_wide7.h"       // g7_num_cus, GEMM_ROW_BYTES
#include "search_scan.h"      // the scan kernels (search_scan.hip): their attributes and their one launcher

#define DENSE_CHUNK 4096   // rows scored densely per bootstrap / fallback step
#define LIST_MAX (SORT_CAP - DENSE_CHUNK)
#define K_MAX 2048
#define SORT_THREADS 512
static_assert(DENSE_CHUNK == SEARCH_DENSE_CHUNK, "search_plan.h schedules for this bootstrap size");

// Per-query sticky status of the asynchronous entry (`qstat`, nullptr on om_sim_topk's path): a query with any bit set is recomputed by the
// on-device redo.  The global flags (flag[0] overflow, flag[1] longest list, flag[2] margin too wide or not finite) stay as they are: they
// are all om_sim_topk's path has.
#define QSTAT_OVERFLOW 1u    // the list exceeded SORT_CAP in some round: appends were dropped
#define QSTAT_WIDE 2u        // a certified list outgrew LIST_MAX (or the certified margin is not finite)
#define QSTAT_COVER 4u       // the final list is longer than the re-score cover

static thread_local int64_t g_info[8];   // last om_sim_topk call: see om_sim_topk_info()

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
// drop_compact is the compaction itself over the predicate keep(row) -- the bitmaps' here, the exclusion lists' in drop_excluded_kernel:
// keys [0, n) of `list`, by all 256 threads of the workgroup; wtot: 4 words of LDS.  Returns the number of keys kept.
template <typename Keep>
__device__ __forceinline__ unsigned drop_compact(u64* __restrict__ list, unsigned n, unsigned* wtot, Keep keep) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned out = 0;
  for (unsigned base = 0; base < n; base += 256) {
    const unsigned i = base + (unsigned)tid;
    u64 key = 0ull;
    bool ok = false;
    if (i < n) {
      key = list[i];
      ok = keep(key_payload(key));
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
  return out;
}

__global__ __launch_bounds__(256) void drop_disallowed_kernel(u64* __restrict__ keys, unsigned* __restrict__ cnt, const RowFilters F,
                                                              uint32_t nrows, unsigned* __restrict__ flag, unsigned* __restrict__ qstat) {
  __shared__ unsigned wtot[4];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
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
  const unsigned out = drop_compact(keys + q * SORT_CAP, n, wtot, [&](uint32_t row) { return row < nrows && row_allowed(allow, row); });
  __syncthreads();                                 // (an empty list: every thread has read cnt[q])
  if (tid == 0) cnt[q] = out;
}

// ---- the exclusion lists of om_sim_topk_excluding -----------------------------------------------------------------------------------------
// excl [n_queries][pitch] int32: row q is the rows query q must not return -- ascending, no repeats, padded at the end with -1; pitch is at
// most EXCLUDE_MAX.  Read as unsigned the whole row is ascending (the padding is the largest word), so one binary search over all `n`
// words serves every list length.  An id at or beyond N names no row and matches nothing.  A row that breaks the contract (unsorted,
// repeats, a negative other than the padding) may drop the wrong keys or leave a short result; every probe stays inside [list, list + n),
// and no value of the list is ever used as an address.
#define EXCLUDE_MAX SEARCH_EXCLUDE_MAX
struct RowExclusions {
  const int32_t* ids;      // nullptr: no exclusion list in the call
  int64_t pitch;
};
__device__ __forceinline__ bool row_excluded(const int32_t* list, int n, uint32_t row) {
  if (row > 0x7fffffffu) return false;               // an int32 list cannot name it (and the padding must not match it)
  int lo = 0, hi = n;                                // the first word >= row is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)list[mid] < row) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && (uint32_t)list[lo] == row;
}

// out[q] = N - e_q, the rows list q leaves, e_q its entries in [0, N) (the words below N in the unsigned order): the rank of the redo's
// select is min(k, this).  One thread and one binary search per query.
__global__ void count_excluded_kernel(const RowExclusions X, int64_t nq, int64_t N, unsigned* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int32_t* list = X.ids + q * X.pitch;
  const uint32_t bound = N > 0x7fffffffLL ? 0x80000000u : (uint32_t)N;
  int lo = 0, hi = (int)X.pitch;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)list[mid] < bound) lo = mid + 1;
    else hi = mid;
  }
  out[q] = (unsigned)(N - lo);
}

// drop_disallowed_kernel under the list predicate: list q compacted in place to the keys whose row is NOT in the query's exclusion list --
// the same order, clamp and mark.  The exclusion list is staged in LDS once (at most 16 KiB) and every key costs one binary search there.
// A query whose list is empty keeps its candidates (clamped and marked all the same), as a query under no bitmap does.
__global__ __launch_bounds__(256) void drop_excluded_kernel(u64* __restrict__ keys, unsigned* __restrict__ cnt, const RowExclusions X,
                                                            uint32_t nrows, unsigned* __restrict__ flag, unsigned* __restrict__ qstat) {
  __shared__ unsigned wtot[4];
  __shared__ int32_t ex[EXCLUDE_MAX];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int ne = (int)X.pitch;                       // (the entry refuses a pitch above EXCLUDE_MAX)
  const int32_t* __restrict__ src = X.ids + q * X.pitch;
  for (int i = tid; i < ne; i += 256) ex[i] = src[i];
  unsigned n = cnt[q];
  if (n > SORT_CAP) {
    if (tid == 0) {
      atomicOr(flag, 1u);
      if (qstat) atomicOr(qstat + q, QSTAT_OVERFLOW);
    }
    n = SORT_CAP;
  }
  __syncthreads();                                   // the list is staged, every thread has read cnt[q]
  if (ne == 0 || ex[0] < 0) {                        // (workgroup-uniform) nothing to exclude
    if (tid == 0) cnt[q] = n;
    return;
  }
  const unsigned out = drop_compact(keys + q * SORT_CAP, n, wtot, [&](uint32_t row) { return row < nrows && !row_excluded(ex, ne, row); });
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
// X: the call's exclusion lists (om_sim_topk_excluding; F has no bitmap then): n_allowed[q] is count_excluded_kernel's count for query q
__global__ __launch_bounds__(256) void redo_begin_kernel(const unsigned* __restrict__ rs, const unsigned* __restrict__ bad, u64* __restrict__ prefix,
                                                         unsigned* __restrict__ remaining, unsigned* __restrict__ hist, unsigned want,
                                                         const RowFilters F, const unsigned* __restrict__ n_allowed, const RowExclusions X) {
  const unsigned n_bad = rs[REDO_RS_BAD];
  if (!n_bad) return;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < (int64_t)n_bad * REDO_BINS; i += step) hist[i] = 0;
  for (int64_t b = i0; b < n_bad; b += step) {
    // under a row filter the rank is min(k, rows the query's bitmap allows), counted on the device
    const int64_t f = filter_index(F, bad[b]);
    const unsigned have = X.ids ? n_allowed[bad[b]] : (f == FILTER_EVERY_ROW ? want : (f == FILTER_NO_ROW ? 0u : n_allowed[f]));
    prefix[b] = 0;
    remaining[b] = have < want ? have : want;
  }
}

// F: the call's row filters (F.bits == nullptr: every row counts for every query).  X: its exclusion lists (X.ids == nullptr: none).
// COLLECT = false: hist[b][digit at `shift`] += 1 for every row whose key agrees with prefix[b] above the digit;
// COLLECT = true: every key >= prefix[b] (= T) appended to list bad[b].  Rows [0, N) of `index`, tiles of R rows (R * d * 4 bytes of LDS).
// TRow = f16_t (OM_SEARCH_F16_ONLY): the tile is filled from 16-byte loads of eight halves and staged WIDENED to float32, so R, the LDS
// bytes and the scoring loop are those of the float32 rows.
template <bool COLLECT, typename TRow>
__global__ __launch_bounds__(256) void redo_pass_kernel(const float* __restrict__ q32, const TRow* __restrict__ index, int64_t N, int d, int R,
                                                        const unsigned* __restrict__ rs, const unsigned* __restrict__ bad,
                                                        const u64* __restrict__ prefix, unsigned* __restrict__ hist, int shift, int width,
                                                        u64* __restrict__ keys, unsigned* __restrict__ cnt, const RowFilters F,
                                                        const RowExclusions X) {
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
      const int32_t* __restrict__ excl = X.ids ? X.ids + (int64_t)q * X.pitch : nullptr;      // the bad query's own list, served from L2
      for (int r = wave; r < nr; r += 4) {
        if (allow && !row_allowed(allow, (uint32_t)(r0 + r))) continue;      // (wave-uniform) a row the filter drops has no key
        if (excl && row_excluded(excl, (int)X.pitch, (uint32_t)(r0 + r))) continue;      // (wave-uniform) nor has a row the list excludes
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
// lists_only (om_sim_topk_candidates: no scan, no margin): the lists and their thresholds alone, the rest null
static SearchWs carve_search(int64_t nq, int d, char* base, bool lists_only = false) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  SearchWs w = {};
  w.keys = (u64*)take((size_t)nq * SORT_CAP * 8);
  w.cnt = (unsigned*)take((size_t)nq * 4);
  w.cnt_prev = (unsigned*)take((size_t)nq * 4);
  w.flag = (unsigned*)take(64);
  w.thr = (float*)take(((size_t)(nq + 255) / 256 * 256 + 256) * 4);      // +inf beyond nq: the generation-7 scan reads whole tiles of thresholds
  w.total = off;
  if (lists_only) return w;
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

// The one place that knows the exact scores read float16 or float32 rows: f(rows), typed, and RowOf names the kernel instantiation for it
template <typename P> using RowOf = std::remove_const_t<std::remove_pointer_t<P>>;
template <typename F>
static void with_rows(bool rows16, const f16_t* r16, const float* r32, F f) {
  if (rows16) f(r16);
  else f(r32);
}

// The thread's page-locked words for what the host reads back (a copy into them is one DMA, no staging through the runtime): 32 of them
static int pinned_words(unsigned*& out) {
  static thread_local unsigned* pinned = nullptr;
  if (!pinned) OM_HIP(hipHostMalloc((void**)&pinned, 128, hipHostMallocPortable));
  out = pinned;
  return 0;
}

namespace {
// Which rows a query may return: everything the chain knows about the restriction of a call.  Three encodings, at most one in a call: one
// bitmap for every query (om_sim_topk_filtered), a bitmap per query (om_sim_topk_filtered_multi), an exclusion list per query
// (om_sim_topk_excluding); the default rule restricts nothing, and not one launch differs under it.  filt and excl are what the kernels
// take.  drop, count, schedule and place are the only places that ask which kind a rule is.
struct RowRule {
  RowFilters filt = {};          // (bits == nullptr: no bitmap)
  RowExclusions excl = {};       // (ids == nullptr: no lists)
  int64_t planned = 0;           // what the schedule is planned from: the rows the (sparsest) bitmap allows, or the pitch of the lists
  unsigned* fcount = nullptr;    // the device's counts of the rows left, set by place: one word, one per bitmap, or one per query (lists)
  size_t extra_bytes = 0;        // what those counts need behind the asynchronous workspace

  static RowRule bitmap(const uint32_t* bits, int64_t n_allowed) { return {{bits, 0, 1, nullptr, 0}, {}, n_allowed, nullptr, 0}; }
  static RowRule bitmaps(const uint32_t* bits, int64_t pitch, int64_t n, const int32_t* of, int64_t n_allowed_min) {
    return {{bits, pitch, n, of, 1}, {}, n_allowed_min, nullptr, align_up((size_t)n * 4, 256)};
  }
  // (pitch == 0: no list, the unrestricted chain itself -- the entry's workspace is sized for the counts all the same)
  static RowRule exclusions(const int32_t* ids, int64_t pitch, int64_t nq) {
    return {{}, {pitch > 0 ? ids : nullptr, pitch}, pitch, nullptr, align_up((size_t)nq * 4, 256)};
  }

  // the drop in front of a selection: list q compacted to the keys whose row the rule leaves query q; qstat: the marks, or nullptr
  int drop(const SearchWs& ws, int64_t nq, uint32_t nrows, unsigned* qstat, hipStream_t s) const {
    if (!excl.ids && !filt.bits) return 0;
    if (excl.ids)
      hipLaunchKernelGGL(drop_excluded_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, excl, nrows, ws.flag, qstat);
    else
      hipLaunchKernelGGL(drop_disallowed_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, filt, nrows, ws.flag, qstat);
    OM_LAUNCH_CHECK();
    return 0;
  }
  // fcount = the rows the rule leaves among [0, N), counted on the device behind the kernel that zeroes rs: the ranks of the redo
  int count(int64_t nq, int64_t N, hipStream_t s) const {
    if (N <= 0 || (!excl.ids && !filt.bits)) return 0;
    // bitmaps: one grid row and one word per bitmap, added to -- the words of per-query bitmaps are the entry's own, zeroed here
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((N + 31) / 32 + 255) / 256, 1024));
    if (filt.per_query) OM_HIP(hipMemsetAsync(fcount, 0, (size_t)filt.n * 4, s));
    if (excl.ids)
      hipLaunchKernelGGL(count_excluded_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, excl, nq, N, fcount);
    else
      hipLaunchKernelGGL(count_allowed_kernel, dim3((unsigned)blocks, (unsigned)(filt.per_query ? filt.n : 1)), dim3(256), 0, s, filt, N, fcount);
    OM_LAUNCH_CHECK();
    return 0;
  }
  // the fast schedule under the rule (search_plan.h): `boot` dense chunks, then the rounds in `chunks` [SEARCH_SCHED_MAX]
  SearchSchedule schedule(bool bf16, int64_t nq, int64_t N, int k, const ScanSwitches& sw, int64_t* chunks, int64_t* boot) const {
    return excl.ids    ? search_schedule_excluding(bf16, nq, N, k, planned, sw, chunks, SEARCH_SCHED_MAX, boot)
           : filt.bits ? search_schedule_filtered(bf16, nq, N, k, planned, sw, chunks, SEARCH_SCHED_MAX, boot)
                       : search_schedule(bf16, nq, N, k, sw, chunks, SEARCH_SCHED_MAX);
  }
  // where the counts live: one bitmap's in the redo's own words, per-query bitmaps' and lists' behind the asynchronous workspace
  void place(void* workspace, const AsyncWs& aw) {
    fcount = excl.ids || filt.per_query ? (unsigned*)((char*)workspace + aw.total) : filt.bits ? aw.rs + REDO_RS_ALLOWED : nullptr;
  }
};

struct Scan {
  int mode; const float* q32; const float* idx32; const f16_t* idx16; int64_t nq, N; int d, k;
  SearchWs ws; hipStream_t s;
  unsigned* qstat = nullptr;      // per-query sticky status: the asynchronous entry only
  ScanSwitches sw;                // the thread's switches, read once by the entry
  RowRule rule;                   // which rows a query may return (the default: every row)
  // diagnostics, accumulated over the 16-bit run and the float32 retry (om_sim_topk publishes them, the asynchronous entry's status
  // kernel takes rounds and family): rounds, chunks redone densely or schedules started over, longest list seen by the host,
  // OM_SCAN_FAMILY_* and OM_SCAN_KERNEL_* of the last filtered round (its tail's where the round had no whole tile)
  int64_t rounds = 0, fallbacks = 0, max_list = 0;
  int family = 0, launch = 0;

  // under a row rule every selection is preceded by the drop of the keys it does not allow
  // (mark: the drop as the selection -- the last one of the chain, behind the redo, marks no query: nothing reads the marks any more)
  int select(bool certified, bool mark = true) {
    if (rule.drop(ws, nq, (uint32_t)N, mark ? qstat : nullptr, s)) return 1;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)nq), dim3(SORT_THREADS), SORT_CAP * 8 + 16, s,
                       ws.keys, ws.cnt, ws.cnt_prev, ws.thr, certified ? ws.margin : nullptr, k,
                       ws.flag, mark ? qstat : nullptr);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int select_radix(bool certified, int cap = SORT_CAP) {
    if (rule.drop(ws, nq, (uint32_t)N, qstat, s)) return 1;
    hipLaunchKernelGGL(select_radix_kernel, dim3((unsigned)nq), dim3(256), (size_t)cap * 8 + 1024 + 64, s,
                       ws.keys, ws.cnt, ws.thr, certified ? ws.margin : nullptr, k, ws.flag, cap, qstat);
    OM_LAUNCH_CHECK();
    return 0;
  }
  int read_flags(unsigned (&f)[4]) {
    unsigned* pinned;
    if (pinned_words(pinned)) return 1;
    OM_HIP(hipMemcpyAsync(pinned, ws.flag, sizeof(f), hipMemcpyDeviceToHost, s));
    OM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) f[i] = pinned[i];
    return 0;
  }
  bool rows16() const { return mode == OM_SEARCH_F16_ONLY; }      // the re-score and the redo read the float16 rows: there are no others
  template <typename F> void with_rows(F f) const { ::with_rows(rows16(), idx16, idx32, f); }
  int rescore(unsigned maxlist) {
    with_rows([&](auto* rows) {
      hipLaunchKernelGGL(rescore_kernel<RowOf<decltype(rows)>>, dim3((maxlist + 3) / 4, (unsigned)nq), dim3(256), 0, s, q32, rows, ws.keys, ws.cnt, d);
    });
    OM_LAUNCH_CHECK();
    return 0;
  }
  // one pass of the on-device redo over the rows the mode stores (COLLECT: the last one, which fills the lists)
  template <bool COLLECT>
  void redo_pass(const AsyncWs& aw, dim3 grid, size_t lds, int R, int shift, int width) {
    with_rows([&](auto* rows) {
      hipLaunchKernelGGL((redo_pass_kernel<COLLECT, RowOf<decltype(rows)>>), grid, dim3(256), lds, s, q32, rows, N, d, R, aw.rs, aw.bad, aw.prefix,
                         aw.hist, shift, width, ws.keys, ws.cnt, rule.filt, rule.excl);
    });
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
      if (l->rows && scan_launch(plan, *l, bf16, sw, rows + (r0 + l->row0) * row_bytes, (uint32_t)(r0 + l->row0), queries, nq, d, ws.thr,
                                 ws.keys, ws.cnt, s)) return 1;
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
  // what every search ends with: the best k of every list as (D, I), padded as faiss pads
  int emit(int64_t id_offset, float* out_scores, int64_t* out_ids) {
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)nq), dim3(256), 0, s, ws.keys, ws.cnt, k, id_offset, out_scores, out_ids);
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
      if (rule.count(nq, N, s)) return 1;
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
  // Under a row rule the schedule is the rule's: `boot` dense chunks, each with its drop and selection, then the rounds.
  int fast_rounds(bool bf16, SearchSchedule& sched) {
    int64_t chunks[SEARCH_SCHED_MAX];
    int64_t boot = 1;
    sched = rule.schedule(bf16, nq, N, k, sw, chunks, &boot);
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
          with_rows([&](auto* rows) {
            hipLaunchKernelGGL(rescore_strided_kernel<RowOf<decltype(rows)>>, rgrid, dim3(256), 0, s, q32, rows, ws.keys, ws.cnt, nq, d);
          });
          OM_LAUNCH_CHECK();
        }
      }
      // redo: a fixed chain, empty launches when no query is marked
      hipLaunchKernelGGL(redo_compact_kernel, dim3(qblocks), dim3(256), 0, s, qstat, nq, aw.rs, aw.bad);
      hipLaunchKernelGGL(redo_begin_kernel, dim3(256), dim3(256), 0, s, aw.rs, aw.bad, aw.prefix, aw.remaining, aw.hist,
                         (unsigned)std::min<int64_t>(k, N), rule.filt, (const unsigned*)rule.fcount, rule.excl);
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
    if (emit(id_offset, out_scores, out_ids)) return 1;
    if (status) hipLaunchKernelGGL(async_status_kernel, dim3(1), dim3(64), 0, s, ws.flag, aw.rs, status, bf16 ? 1 : 0, (int)rounds, family);
    OM_LAUNCH_CHECK();
    return 0;
  }

  // om_sim_topk in OM_SEARCH_F16_ONLY: there is no float32 plane to retry on, so the entry enqueues the asynchronous chain -- whose redo
  // serves every query the margin does not certify -- without status words, and reads the chain's own counters back: ONE synchronisation.
  // out: {queries redone, of those with a too-wide margin, longest list}
  int run_sync16(const AsyncWs& aw, int64_t id_offset, float* out_scores, int64_t* out_ids, unsigned (&out)[3]) {
    if (run_async(true, aw, id_offset, out_scores, out_ids, nullptr)) return 1;
    unsigned* pinned;
    if (pinned_words(pinned)) return 1;
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
    } else if (init_lists()) {
      return 1;
    }
    return emit(id_offset, out_scores, out_ids);
  }
  // om_sim_topk_candidates behind its checks: init -> per block of CAND_BLOCK candidate columns (score, then the exact-mode selection,
  // which keeps the best k by the 64-bit key) -> emit
  int run_candidates(const int32_t* cand, int64_t cand_pitch, int64_t id_offset, float* out_scores, int64_t* out_ids) {
    if (init_lists()) return 1;
    for (int64_t col0 = 0; col0 < cand_pitch; col0 += CAND_BLOCK) {
      const int ncols = (int)std::min<int64_t>(CAND_BLOCK, cand_pitch - col0);
      with_rows([&](auto* rows) {
        hipLaunchKernelGGL(score_candidates_kernel<RowOf<decltype(rows)>>, dim3((unsigned)((ncols + 3) / 4), (unsigned)nq), dim3(256), 0, s, q32,
                           rows, N, d, cand, cand_pitch, col0, ncols, ws.keys, ws.cnt);
      });
      OM_LAUNCH_CHECK();
      if (select(false)) return 1;
    }
    return emit(id_offset, out_scores, out_ids);
  }
  int precision = 0, too_wide = 0;      // om_sim_topk_info [0] and [4]
};

// The arguments every scanning entry takes, as scan_setup and chain_setup read them
struct SearchArgs {
  int mode; const float* queries; int64_t n_queries; const float* index_f32; const void* index_f16; const float* stats; int64_t N; int d, k;
  float* out_scores; int64_t* out_ids; void* workspace; size_t workspace_bytes; void* stream;
};

// The argument checks and the set-up the entries share (n_queries > 0).  Returns the refusal, nullptr when there is none: the entry
// fails with it under its own name.
const char* scan_setup(Scan& sc, const SearchArgs& a) {
  if (a.k < 1 || a.k > K_MAX) return "k must be in [1,2048]";
  if (a.N < 0 || a.N > 0xffffffffLL) return "shard rows must fit in 32 bits";
  if (a.d <= 0 || (a.d * 2) % GEMM_ROW_BYTES != 0) return "d must be a multiple of 64 (pad with zeros)";
  if (a.n_queries > 65535) return "at most 65535 queries per call";
  if (!a.queries || !a.out_scores || !a.out_ids) return "null argument";
  if (!a.workspace || ((uintptr_t)a.workspace & 255)) return "workspace must be 256-byte aligned";
  if (a.N > 0 && a.mode != OM_SEARCH_F16_ONLY && !a.index_f32) return "index_f32 is null";
  if (a.N > 0 && a.mode == OM_SEARCH_F16_RESCORE && (!a.index_f16 || !a.stats)) return "f16 mode needs index_f16 and stats";
  if (a.N > 0 && a.mode == OM_SEARCH_F16_ONLY && !a.index_f16) return "OM_SEARCH_F16_ONLY: index_f16 is null (the float16 rows are the index)";
  if (a.N > 0 && a.mode == OM_SEARCH_F16_ONLY && !a.stats) return "OM_SEARCH_F16_ONLY: stats is null (om_index_add_f16 leaves them)";
  sc.ws = carve_search(a.n_queries, a.d, (char*)a.workspace);
  sc.mode = a.mode; sc.q32 = a.queries; sc.idx32 = a.index_f32; sc.idx16 = (const f16_t*)a.index_f16;
  sc.nq = a.n_queries; sc.N = a.N; sc.d = a.d; sc.k = a.k; sc.s = (hipStream_t)a.stream; sc.stats = a.stats;
  sc.sw = scan_switches();
  return nullptr;
}

// What OM_SEARCH_F16_ONLY refuses in EVERY entry: it always runs the stream-ordered chain, and no entry has another path to offer.
const char* f16_only_refusal(const Scan& sc) {
  if (sc.d > 16384) return "OM_SEARCH_F16_ONLY: d above 16384: a row does not fit the redo's LDS tile, and the mode has no float32 scan to fall back to";
  if (!sc.sw.gen7)
    return "OM_SEARCH_F16_ONLY: OM_OPT_SCAN_GEN7 is 0: the fast schedule this mode runs is switched off, and it has no step-by-step path";
  return nullptr;
}
const char* no_own_checks() { return nullptr; }
}  // namespace

// The dynamic-LDS attributes of every kernel a search launches, set at this one site: host calls, made once per unit (a capturing stream
// must not meet them)
static int search_attrs() {
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    OM_HIP(hipFuncSetAttribute((const void*)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               SORT_CAP * 8 + 16));
    OM_HIP(hipFuncSetAttribute((const void*)select_radix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               SORT_CAP * 8 + 1024 + 64));
    attr_set = true;
  }
  return scan_attrs();
}

// What the four entries that run the stream-ordered chain (Scan::run_async) do before it, in the order of their refusals: scan_setup; what
// OM_SEARCH_F16_ONLY refuses; d above the redo's tile and OM_OPT_SCAN_GEN7 = 0, both ending in `tail` (`early`: a refusal the entry has
// already found, or nullptr -- it is reported between the two); own(), the entry's other argument checks, a refusal or nullptr; the
// asynchronous workspace with what sc.rule needs behind it (`ws_refusal` when it does not fit); qstat and the rule's counts placed; the
// kernel attributes.  A refusal fails under the entry's name, as OM_FAIL would in its body.
template <typename Own>
static int chain_setup(const char* entry, Scan& sc, AsyncWs& aw, const SearchArgs& a, const char* tail, const char* early, Own own,
                       const char* ws_refusal) {
  auto fail = [&](const std::string& why) { om_set_error(std::string(entry) + ": " + why); return 1; };
  if (const char* why = scan_setup(sc, a)) return fail(why);
  if (a.mode == OM_SEARCH_F16_ONLY)
    if (const char* why = f16_only_refusal(sc)) return fail(why);
  if (a.d > 16384) return fail(std::string("d above 16384: a row does not fit the redo's LDS tile") + tail);
  if (early) return fail(early);
  if (!sc.sw.gen7) return fail(std::string("OM_OPT_SCAN_GEN7 is 0: the fast schedule this entry runs is switched off") + tail);
  if (const char* why = own()) return fail(why);
  aw = carve_async(a.n_queries, a.d, (char*)a.workspace);
  if (aw.total + sc.rule.extra_bytes > a.workspace_bytes) return fail(ws_refusal);
  sc.qstat = aw.qstat;
  sc.rule.place(a.workspace, aw);
  return search_attrs();
}

// The stream-ordered search under `rule`, for the entries below (n_queries > 0): chain_setup, then the chain.  The rule adds the count
// of the rows it leaves behind the init, the drop in front of every selection, its own schedule and the redo's row test.
template <typename Own>
static int chain_entry(const char* entry, const SearchArgs& a, int64_t id_offset, int64_t* status, const RowRule& rule, const char* tail,
                       const char* early, Own own, const char* ws_refusal) {
  Scan sc;
  sc.rule = rule;
  AsyncWs aw;
  if (chain_setup(entry, sc, aw, a, tail, early, own, ws_refusal)) return 1;
  return sc.run_async(search_mode_half(a.mode), aw, id_offset, a.out_scores, a.out_ids, status);
}
// the workspace of such an entry: the asynchronous one and the rule's counts behind it
static size_t chain_workspace_bytes(int64_t nq, int d, const RowRule& rule) { return carve_async(nq, d, nullptr).total + rule.extra_bytes; }

extern "C" int om_sim_topk(int mode, const float* queries, int64_t n_queries,
                           const float* index_f32, const void* index_f16, const float* stats,
                           int64_t N, int d, int k, int64_t id_offset, float* out_scores,
                           int64_t* out_ids, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (n_queries <= 0) return 0;
  const SearchArgs a = {mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, workspace_bytes, stream};
  Scan sc;
  if (mode == OM_SEARCH_F16_ONLY) {
    AsyncWs aw;
    if (chain_setup(__func__, sc, aw, a, "", nullptr, no_own_checks, "workspace too small: OM_SEARCH_F16_ONLY needs om_sim_topk_async_workspace_bytes"))
      return 1;
    for (auto& v : g_info) v = 0;
    unsigned redo[3] = {0, 0, 0};
    const int rc = sc.run_sync16(aw, id_offset, out_scores, out_ids, redo);
    g_info[0] = 1; g_info[1] = sc.rounds; g_info[3] = redo[2]; g_info[4] = redo[1]; g_info[5] = sc.family; g_info[6] = sc.launch;
    g_info[7] = redo[0];
    return rc;
  }
  if (const char* why = scan_setup(sc, a)) OM_FAIL(why);
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
  const SearchArgs a = {mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, workspace_bytes, stream};
  return chain_entry(__func__, a, id_offset, status, RowRule{}, " (use om_sim_topk)",
                     status ? nullptr : "status is null: the asynchronous entry reports through 8 x int64 of device memory", no_own_checks,
                     "workspace too small (om_sim_topk_async_workspace_bytes)");
}

// The stream-ordered search under a row filter: one bitmap over rows [0, N) for every query, n_allowed the host's count of its bits.
extern "C" int om_sim_topk_filtered(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                                    const float* stats, int64_t N, int d, int k, int64_t id_offset, const uint32_t* allow_bits,
                                    int64_t n_allowed, float* out_scores, int64_t* out_ids, int64_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (n_queries <= 0) return 0;
  const SearchArgs a = {mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, workspace_bytes, stream};
  auto own = [&]() -> const char* {
    if (!allow_bits) return "allow_bits is null: the filtered search needs the bitmap of the allowed rows (om_sim_topk_async searches all rows)";
    if (n_allowed < 0 || n_allowed > N) return "n_allowed must be in [0, N]";
    return nullptr;
  };
  return chain_entry(__func__, a, id_offset, status, RowRule::bitmap(allow_bits, n_allowed), "", nullptr, own,
                     "workspace too small (om_sim_topk_filtered_workspace_bytes)");
}

// The same chain with a bitmap per query: the three kernels that read a bitmap -- the drop, the count, the redo -- take it from
// filter_of[q].  The schedule is the single-filter one of the sparsest bitmap in use (search_plan.h).
extern "C" size_t om_sim_topk_filtered_multi_workspace_bytes(int64_t n_queries, int d, int k, int64_t n_filters) {
  (void)k;
  if (n_queries <= 0 || d <= 0 || n_filters < 1) return 0;
  return chain_workspace_bytes(n_queries, d, RowRule::bitmaps(nullptr, 0, n_filters, nullptr, 0));
}

extern "C" int om_sim_topk_filtered_multi(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                                          const float* stats, int64_t N, int d, int k, int64_t id_offset, const uint32_t* allow_bits,
                                          int64_t words_pitch, int64_t n_filters, const int32_t* filter_of, int64_t n_allowed_min,
                                          float* out_scores, int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (n_queries <= 0) return 0;
  const SearchArgs a = {mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, workspace_bytes, stream};
  auto own = [&]() -> const char* {
    if (!allow_bits) return "allow_bits is null: the filtered search needs the bitmaps of the allowed rows (om_sim_topk_async searches all rows)";
    if (n_filters < 1 || n_filters > 65535) return "n_filters must be in [1, 65535]";
    if (words_pitch < (N + 31) / 32) return "words_pitch is below (N + 31) / 32, the words of one bitmap";
    if (!filter_of && n_filters != n_queries) return "filter_of is null: query q is under bitmap q, which needs n_filters == n_queries";
    if (n_allowed_min < 0 || n_allowed_min > N) return "n_allowed_min must be in [0, N]";
    return nullptr;
  };
  return chain_entry(__func__, a, id_offset, status, RowRule::bitmaps(allow_bits, words_pitch, n_filters, filter_of, n_allowed_min), "", nullptr,
                     own, "workspace too small (om_sim_topk_filtered_multi_workspace_bytes)");
}

// The same chain with an exclusion list per query in the bitmaps' place: the drop (drop_excluded_kernel), the count and the redo read
// list q.  pitch == 0 is om_sim_topk_async's chain itself.
extern "C" size_t om_sim_topk_excluding_workspace_bytes(int64_t n_queries, int d, int k, int64_t pitch) {
  (void)k;
  if (n_queries <= 0 || d <= 0) return 0;
  return chain_workspace_bytes(n_queries, d, RowRule::exclusions(nullptr, pitch, n_queries));
}

extern "C" int om_sim_topk_excluding(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                                     const float* stats, int64_t N, int d, int k, int64_t id_offset, const int32_t* excl, int64_t pitch,
                                     float* out_scores, int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (n_queries <= 0) return 0;
  const SearchArgs a = {mode, queries, n_queries, index_f32, index_f16, stats, N, d, k, out_scores, out_ids, workspace, workspace_bytes, stream};
  auto own = [&]() -> const char* {
    if (pitch < 0 || pitch > EXCLUDE_MAX) return "pitch must be in [0, EXCLUDE_MAX = 4096]: the ids of one query's exclusion list (a RowFilter serves longer ones)";
    if (!excl && pitch > 0) return "excl is null: the exclusion table of the call (pitch 0 searches all rows)";
    return nullptr;
  };
  return chain_entry(__func__, a, id_offset, status, RowRule::exclusions(excl, pitch, n_queries), "", nullptr, own,
                     "workspace too small (om_sim_topk_excluding_workspace_bytes)");
}

// ---- om_sim_topk_candidates: the exact top-k of every query over its OWN candidate rows ------------------------------------------------
// No scan, no margin, no redo: Scan::run_candidates.  A list never holds more than k + CAND_BLOCK <= SORT_CAP keys, and keys of distinct
// rows never tie, so there is nothing to overflow and nothing to redo.  The chain is fixed by cand_pitch alone; the cost is
// n_queries * cand_pitch * d, whatever N.
extern "C" size_t om_sim_topk_candidates_workspace_bytes(int64_t n_queries, int d, int k) {
  (void)d; (void)k;
  if (n_queries <= 0) return 0;
  return carve_search(n_queries, 0, nullptr, true).total;
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
  Scan sc;
  sc.ws = carve_search(n_queries, d, (char*)workspace, true);
  if (sc.ws.total > workspace_bytes) OM_FAIL("workspace too small (om_sim_topk_candidates_workspace_bytes)");
  if (search_attrs()) return 1;
  sc.mode = mode; sc.q32 = queries; sc.idx32 = index_f32; sc.idx16 = (const f16_t*)index_f16;
  sc.nq = n_queries; sc.N = N; sc.d = d; sc.k = k; sc.s = (hipStream_t)stream;
  return sc.run_candidates(cand, cand_pitch, id_offset, out_scores, out_ids);
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

extern "C" int om_debug_search_exclude_schedule(int mode, int64_t nq, int64_t N, int k, int64_t pitch, int64_t* chunks, int cap, int* n,
                                                int64_t* boot) {
  if (!n || !boot || (cap > 0 && !chunks)) OM_FAIL("null argument");
  if (nq < 1 || N < 0 || k < 1 || k > K_MAX) OM_FAIL("nq >= 1, N >= 0 and k in [1,2048]");
  if (pitch < 0 || pitch > EXCLUDE_MAX) OM_FAIL("pitch must be in [0, EXCLUDE_MAX = 4096]");
  *n = search_schedule_excluding(search_mode_half(mode), nq, N, k, pitch, scan_switches(), chunks, cap < 0 ? 0 : cap, boot).n;
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
    with_rows(h, r16, r32, [&](auto* r) {
      hipLaunchKernelGGL((redo_pass_kernel<true, RowOf<decltype(r)>>), grid, dim3(256), lds, s, queries, r, N, d, R, aw.rs, aw.bad, aw.prefix, aw.hist,
                         0, 0, ws.keys, ws.cnt, RowFilters{nullptr, 0, 0, nullptr, 0}, RowExclusions{nullptr, 0});
    });
  } else {
    hipLaunchKernelGGL(debug_fill_lists_kernel, dim3(nq), dim3(256), 0, s, cand, m, N, ws.keys, ws.cnt);
    with_rows(h, r16, r32, [&](auto* r) {
      if (kernel == 0)
        hipLaunchKernelGGL(rescore_kernel<RowOf<decltype(r)>>, dim3(((unsigned)m + 3) / 4, nq), dim3(256), 0, s, queries, r, ws.keys, ws.cnt, d);
      else
        hipLaunchKernelGGL(rescore_strided_kernel<RowOf<decltype(r)>>, dim3((unsigned)(g7_num_cus() * 8)), dim3(256), 0, s, queries, r, ws.keys,
                           ws.cnt, n_queries, d);
    });
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

// What the three drop hooks share: the caller's lists put in place, the drop under `rule` as the chain launches it (RowRule::drop), the
// lists read back.  hook: the name refusals fail under; own: the hook's refusal of its other arguments (nullptr: none), reported
// between the checks of the lists and those of the workspace.
static int debug_drop_lists(const char* hook, const RowRule& rule, const char* own, int64_t n_queries, int m, const float* scores,
                            const uint32_t* rows, const uint32_t* counts, int use_qstat, uint32_t nrows, float* out_scores, uint32_t* out_rows,
                            uint32_t* out_state, void* workspace, size_t workspace_bytes, void* stream) {
  auto fail = [&](const char* why) { om_set_error(std::string(hook) + ": " + why); return 1; };
  if (!scores || !rows || !counts) return fail("null argument: scores, rows and counts describe the lists");
  if (n_queries < 1 || n_queries > 65535) return fail("1 to 65535 queries");
  if (m < 1 || m > SORT_CAP) return fail("m must be in [1, 8192]");
  if (own) return fail(own);
  if (!workspace || ((uintptr_t)workspace & 255)) return fail("workspace must be 256-byte aligned");
  const SearchWs ws = carve_search(n_queries, 64, (char*)workspace);
  const AsyncWs aw = carve_async(n_queries, 64, (char*)workspace);
  if (aw.total > workspace_bytes) return fail("workspace too small (om_sim_topk_async_workspace_bytes(n_queries, 64, 1))");
  const hipStream_t s = (hipStream_t)stream;
  const unsigned nq = (unsigned)n_queries;
  hipLaunchKernelGGL(debug_put_lists_kernel, dim3(nq), dim3(256), 0, s, scores, rows, counts, (const float*)nullptr, m, ws.keys, ws.cnt,
                     ws.cnt_prev, ws.thr, ws.margin, ws.flag, aw.qstat);
  OM_LAUNCH_CHECK();
  if (rule.drop(ws, n_queries, nrows, use_qstat ? aw.qstat : nullptr, s)) return 1;
  hipLaunchKernelGGL(debug_get_lists_kernel, dim3(nq), dim3(256), 0, s, ws.keys, ws.cnt, ws.cnt_prev, ws.thr, ws.flag, aw.qstat, out_scores,
                     out_rows, out_state);
  OM_LAUNCH_CHECK();
  return 0;
}

extern "C" int om_debug_select_lists(int op, int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int k,
                                     const float* margin, int use_qstat, int cap, const uint32_t* allow, uint32_t nrows, const float* S,
                                     int64_t ldS, int n, uint32_t row_base, uint32_t cover, int64_t id_offset, float* emit_scores,
                                     int64_t* emit_ids, float* out_scores, uint32_t* out_rows, uint32_t* out_state, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (op < OM_DEBUG_LISTS_RADIX || op > OM_DEBUG_LISTS_EMIT)
    OM_FAIL("op must be 0 (radix selection), 1 (sorting selection), 2 (drop), 3 (dense append + overflow check) or 4 (emit)");
  const char* const k_refusal = k < 1 || k > K_MAX ? "k must be in [1, 2048]" : nullptr;
  if (op == OM_DEBUG_LISTS_DROP)      // the one bitmap of om_sim_topk_filtered
    return debug_drop_lists(__func__, RowRule::bitmap(allow, 0),
                            k_refusal ? k_refusal : !allow || nrows < 1 ? "the drop needs the bitmap (null argument) and nrows >= 1" : nullptr,
                            n_queries, m, scores, rows, counts, use_qstat, nrows, out_scores, out_rows, out_state, workspace, workspace_bytes, stream);
  if (!scores || !rows || !counts) OM_FAIL("null argument: scores, rows and counts describe the lists");
  if (n_queries < 1 || n_queries > 65535) OM_FAIL("1 to 65535 queries");
  if (m < 1 || m > SORT_CAP) OM_FAIL("m must be in [1, 8192]");
  if (k_refusal) OM_FAIL(k_refusal);
  if (op == OM_DEBUG_LISTS_RADIX && cap != 4096 && cap != SORT_CAP) OM_FAIL("cap must be 4096 or 8192");
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
  const char* const own = !allow || nrows < 1                           ? "the drop needs the bitmaps (allow is null) and nrows >= 1"
                          : n_filters < 1                               ? "n_filters must be at least 1"
                          : words_pitch < ((int64_t)nrows + 31) / 32    ? "words_pitch is below (nrows + 31) / 32, the words of one bitmap"
                          : !filter_of && n_filters != n_queries        ? "filter_of is null: query q is under bitmap q, which needs n_filters == n_queries"
                                                                        : nullptr;
  return debug_drop_lists(__func__, RowRule::bitmaps(allow, words_pitch, n_filters, filter_of, 0), own, n_queries, m, scores, rows, counts,
                          use_qstat, nrows, out_scores, out_rows, out_state, workspace, workspace_bytes, stream);
}

// The drop under the exclusion lists of om_sim_topk_excluding: drop_excluded_kernel as that entry launches it
extern "C" int om_debug_drop_lists_excluding(int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts,
                                             int use_qstat, const int32_t* excl, int64_t pitch, uint32_t nrows, float* out_scores,
                                             uint32_t* out_rows, uint32_t* out_state, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const own = !excl || nrows < 1                  ? "the drop needs the exclusion table (excl is null) and nrows >= 1"
                          : pitch < 1 || pitch > EXCLUDE_MAX  ? "pitch must be in [1, EXCLUDE_MAX = 4096]"
                                                              : nullptr;
  return debug_drop_lists(__func__, RowRule::exclusions(excl, pitch, n_queries), own, n_queries, m, scores, rows, counts, use_qstat, nrows,
                          out_scores, out_rows, out_state, workspace, workspace_bytes, stream);
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
