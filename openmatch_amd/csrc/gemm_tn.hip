// Weight-gradient contraction for the training backward (stands in for autograd's  dW = dY^T X  of every nn.Linear in
// HF BertModel / T5 under DRModel.forward + loss.backward(); reference: modeling/dense_retrieval_model.py:89-131):
//
//     C[n, k] += sum_m A[m, n] * B[m, k]          A = dY [M, N],  B = X [M, K],  both ROW-major as the forward /
//     bias[n] += sum_m A[m, n]                     backward kernels leave them, bf16;  C, bias f32 (accumulated)
//
// The contraction index m is the SLOW index of both operands, so neither tile has the k-contiguous fragment layout the
// matrix core wants.  Round 1 transposed both operands in HBM first (transpose_kernel x2 + colsum_kernel + an NT
// split-K GEMM: 10 of the 26.7 ms of a training step, profiles/r01_train_kernel_stats_v1.csv).  Here the tiles are staged
// row-major and read back through gfx950's transposing LDS read (ds_read_b64_tr_b16): a 16-lane group fetches a
// [4 m][16 col] block, 8 bytes per lane, and each lane receives the four m values of ITS column -- two such reads
// are one 32x32x16 MFMA fragment.  LDS image per operand tile (64 m x 128 col): eight [64 m][16 col] sub-tiles of
// 32-byte rows, sub-tile stride 2048 + 128 bytes (the two column blocks a half-wave reads land on disjoint banks).
//
// Workgroup: 128 (n) x 128 (k) output tile, four waves of 64 x 64, over one slice of the token axis (split-M, f32
// atomics into the caller-zeroed / caller-accumulated C).  Two kernels share that shape: `gemm_tn_dma_kernel` (whole
// 64-token steps brought in by LDS-DMA, the default) and `gemm_tn_kernel` (register-staged, zero-fills: ragged tails and
// short token axes).  The bias column sums are taken from the A fragments themselves (eight tokens of one column per
// lane) by the vector ALU under the MFMAs, in the waves that own k columns 0..63 of k tile 0.
#include <string.h>

#include <atomic>
#include <string>

#include "gemm_core7.h"
#include "gemm_tn_plan.h"
#include "kernels.h"

namespace {
constexpr int TN_BM = 64;                       // tokens per step
constexpr int TN_SUB = TN_BM * 32 + 128;        // bytes per [64][16] sub-tile, padded
constexpr int TN_OPER = 8 * TN_SUB;             // one operand tile (64 tokens x 128 columns)
constexpr int TN_LDS = 4 * TN_OPER;             // A, B double-buffered: 69 632 bytes, two workgroups per CU
constexpr int TN_THREADS = 256;

typedef short v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s tn_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(p));
}

// Measured on the way here (profiles/r02_gemm_tn_variants.log, M = 9216):
//  * the f32 atomics of the split-M flush execute at the memory side, ~0.35 M/us: 16 384 per workgroup, so the number of
//    WORKGROUPS sets that cost -- ~320 of them (one wave of two per CU) instead of ~1000 took 104 -> 77 us at 768 x 3072;
//  * a 256 x 256 tile (one workgroup per CU, 65 536 atomics each) was slower than 128 x 128 at every shape;
//  * with one step of prefetch the token loop ran at ~30 % of the MFMA rate, parked on the global loads (SQ_WAIT_ANY
//    42 %, no LDS bank conflicts): the loads of step t + 2 are now issued before step t is computed (two register sets).
// T = bf16_t | f16_t (round 5: float16 training).  The kernels move raw 16-bit words (bf16x8_t = eight shorts); only the MFMA opcode
// and the value of a word (the bias column sums) depend on the format.
template <typename T> __device__ __forceinline__ void tn_mma(const bf16x8_t& a, const bf16x8_t& b, f32x16_t& c);
template <> __device__ __forceinline__ void tn_mma<bf16_t>(const bf16x8_t& a, const bf16x8_t& b, f32x16_t& c) { MmaOps<bf16_t>::mma(a, b, c); }
template <> __device__ __forceinline__ void tn_mma<f16_t>(const bf16x8_t& a, const bf16x8_t& b, f32x16_t& c) {
  MmaOps<f16_t>::mma(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c);
}
// sum of the eight values of a fragment
template <typename T> __device__ __forceinline__ float tn_sum8(const uint4& w) {
  return (Half16<T>::lo(w.x) + Half16<T>::hi(w.x)) + (Half16<T>::lo(w.y) + Half16<T>::hi(w.y)) +
         (Half16<T>::lo(w.z) + Half16<T>::hi(w.z)) + (Half16<T>::lo(w.w) + Half16<T>::hi(w.w));
}
template <typename T>
__global__ __launch_bounds__(TN_THREADS, 2) void gemm_tn_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb, float* __restrict__ C,
    int64_t ldc, float* __restrict__ bias, int64_t M, int N, int K, int rows_per_slice, int dbg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int ntk = K / 128;
  const int n0 = (blockIdx.x / ntk) * 128, k0 = (blockIdx.x % ntk) * 128;
  const int64_t m_begin = (int64_t)blockIdx.y * rows_per_slice;
  int64_t m_end = m_begin + rows_per_slice < M ? m_begin + rows_per_slice : M;
  if (m_begin >= m_end) return;
  if (dbg & 4) m_end = m_begin + 1;          // measurement only: one step of the token loop
  const int nsteps = (int)((m_end - m_begin + TN_BM - 1) / TN_BM);
  const bool do_bias = bias != nullptr && k0 == 0 && wk == 0;

  // staging: wave instruction j = wave * 4 + i covers rows (j >> 1) * 8 .. + 7 and column blocks (j & 1) * 4 .. + 3
  // (64 columns = one 128-byte line of each row); lane -> (half h of the 32-byte sub-tile row, row r8, column block
  // cbl): 16 lanes write 256 contiguous LDS bytes.  Addresses = one per-lane 32-bit part + a wave-uniform part.
  const int h = lane & 1, r8 = (lane >> 1) & 7, cbl = lane >> 4;
  const int row0 = wave * 16 + r8;                    // + (i >> 1) * 8
  const uint32_t a_lane = (uint32_t)((row0 * lda + cbl * 16 + h * 8) * 2);
  const uint32_t b_lane = (uint32_t)((row0 * ldb + cbl * 16 + h * 8) * 2);
  const int lds_lane = cbl * TN_SUB + row0 * 32 + h * 16;
  const uint32_t col_lane = (uint32_t)((cbl * 16 + h * 8) * 2);   // row 0 of the step: the stand-in for rows past m_end
  const char* const a_base = (const char*)(A + m_begin * lda + n0);      // wave-uniform
  const char* const b_base = (const char*)(B + m_begin * ldb + k0);
  const size_t a_step = (size_t)TN_BM * lda * 2, b_step = (size_t)TN_BM * ldb * 2;
  // two register sets (X, Y) of 4 + 4 x 16 bytes: named registers, not arrays -- hipcc leaves a uint4 array that lives
  // across the barrier in scratch, and a conditionally filled one too (hence the clamped, unconditional fetches)
  uint4 raX0, raX1, raX2, raX3, rbX0, rbX1, rbX2, rbX3, raY0, raY1, raY2, raY3, rbY0, rbY1, rbY2, rbY3;
  // rows past the end of the slice: no branches -- the load goes to row 0 of the step (always valid) and the A value is
  // zeroed on its way into LDS (0 x finite = 0; the B stand-in is real data)
#define TN_FETCH1(S, I, STEP)                                                                          \
  {                                                                                                    \
    const bool ok = m_begin + (int64_t)(STEP) * TN_BM + row0 + ((I) >> 1) * 8 < m_end;                  \
    const uint32_t ua = (uint32_t)(((I) >> 1) * 8 * lda * 2), ub = (uint32_t)(((I) >> 1) * 8 * ldb * 2); \
    ra##S##I = *(const uint4*)(a_base + (STEP) * a_step + ((I) & 1) * 128 + (ok ? a_lane + ua : col_lane)); \
    rb##S##I = *(const uint4*)(b_base + (STEP) * b_step + ((I) & 1) * 128 + (ok ? b_lane + ub : col_lane)); \
  }
#define TN_FETCH(S, STEP_)                                                                             \
  do {                                                                                                 \
    const int st_ = (STEP_) < nsteps ? (STEP_) : nsteps - 1;      /* past the end: re-fetch the last tile, never used */ \
    TN_FETCH1(S, 0, st_) TN_FETCH1(S, 1, st_) TN_FETCH1(S, 2, st_) TN_FETCH1(S, 3, st_)                \
  } while (0)
#define TN_STASH1(S, I, BUF, STEP)                                                                     \
  {                                                                                                    \
    const bool ok = m_begin + (int64_t)(STEP) * TN_BM + row0 + ((I) >> 1) * 8 < m_end;                  \
    const int off = ((I) & 1) * 4 * TN_SUB + ((I) >> 1) * 8 * 32;                                      \
    uint4 va = ra##S##I;                                                                               \
    if (!ok) va = make_uint4(0u, 0u, 0u, 0u);                                                          \
    *(uint4*)((BUF) + lds_lane + off) = va;                                                            \
    *(uint4*)((BUF) + TN_OPER + lds_lane + off) = rb##S##I;                                            \
  }
#define TN_STASH(S, BUF, STEP)                                                                         \
  do { TN_STASH1(S, 0, BUF, STEP) TN_STASH1(S, 1, BUF, STEP) TN_STASH1(S, 2, BUF, STEP) TN_STASH1(S, 3, BUF, STEP) } while (0)

  // fragment reads: 16-lane group g -> column block (g & 1) of the 32-column fragment, m half (g >> 1) of the k16 step
  const int g = lane >> 4;
  const int frag_off = (g & 1) * TN_SUB + (g >> 1) * 8 * 32 + (lane & 15) * 8;
  f32x16_t acc[2][2];
  float bsum[2] = {0.f, 0.f};               // bias: this lane's share of the column sum of A column (i*32 + lane&31)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[i][0][r] = 0.f; acc[i][1][r] = 0.f; }

  // one 64-token step from LDS buffer CUR: fragments of k16 step ks + 1 are read while the MFMAs of step ks run
#define TN_READ(KS, SET)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
    const v4s a0 = tn_read(ia + i * 2 * TN_SUB + (KS) * 512), a1 = tn_read(ia + i * 2 * TN_SUB + (KS) * 512 + 128); \
    const v4s b0 = tn_read(ib + i * 2 * TN_SUB + (KS) * 512), b1 = tn_read(ib + i * 2 * TN_SUB + (KS) * 512 + 128); \
    fa[SET][i] = (bf16x8_t){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};                   \
    fb[SET][i] = (bf16x8_t){b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};                   \
  }
  // acc[i][j][r]: n = n0 + wn*64 + i*32 + 8*(r>>2) + 4*(lane>>5) + (r&3),  k = k0 + wk*64 + j*32 + (lane & 31)
  // (k, the contiguous index of C, runs along the lanes: every atomic instruction of the flush covers whole 128-byte rows)
#define TN_COMPUTE(CUR)                                                                                \
  do {                                                                                                 \
    const char* ia = smem + (CUR) * 2 * TN_OPER + (wn * 4) * TN_SUB + frag_off;                        \
    const char* ib = smem + (CUR) * 2 * TN_OPER + TN_OPER + (wk * 4) * TN_SUB + frag_off;              \
    bf16x8_t fa[2][2], fb[2][2];                                                                       \
    TN_READ(0, 0)                                                                                      \
    _Pragma("unroll") for (int ks = 0; ks < TN_BM / 16; ++ks) {                                        \
      __builtin_amdgcn_sched_barrier(0);                                                               \
      if (ks + 1 < TN_BM / 16) { TN_READ(ks + 1, (ks + 1) & 1) }                                       \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                  \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) tn_mma<T>(fa[ks & 1][i], fb[ks & 1][j], acc[i][j]); \
        if (do_bias) {      /* the fragment holds 8 tokens of column (lane & 31): add them up under the MFMAs */ \
          const uint4 w = __builtin_bit_cast(uint4, fa[ks & 1][i]);                                    \
          bsum[i] += tn_sum8<T>(w); \
        }                                                                                              \
      }                                                                                                \
    }                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)

  // pipeline: LDS holds step t, set Y holds step t + 1 (in flight), set X receives step t + 2 -- and the roles swap
  TN_FETCH(X, 0);
  TN_FETCH(Y, 1);
  TN_STASH(X, smem, 0);
  __syncthreads();
  for (int t = 0; t < nsteps; t += 2) {
    TN_FETCH(X, t + 2);
    TN_COMPUTE(0);
    if (t + 1 >= nsteps) break;
    TN_STASH(Y, smem + 2 * TN_OPER, t + 1);
    __syncthreads();
    TN_FETCH(Y, t + 3);
    TN_COMPUTE(1);
    if (t + 2 >= nsteps) break;
    TN_STASH(X, smem, t + 2);
    __syncthreads();
  }

  const int kcol = k0 + wk * 64 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int nbase = n0 + wn * 64 + i * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nbase + 8 * (r >> 2) + (r & 3);
      float* crow = C + (int64_t)n * ldc + kcol;
#pragma unroll
      for (int j = 0; j < 2; ++j) { if (dbg & 2) crow[j * 32] = acc[i][j][r]; else atomicAdd(crow + j * 32, acc[i][j][r]); }   // (dbg 2: measurement only)
    }
    if (do_bias) {                          // lanes l and l + 32 hold the two token halves of column (l & 31)
      const float t = bsum[i] + __shfl_xor(bsum[i], 32, 64);
      if (lane < 32) atomicAdd(bias + n0 + wn * 64 + i * 32 + lane, t);
    }
  }
}

// ---- the same contraction with the tiles brought in by LDS-DMA --------------------------------------------------------
// The register-staged kernel above is bound by its own LDS writes: 8 ds_write_b128 per wave and step at ~13 LDS cycles
// each (MI355X_MICROARCH.md: 79 B/clk/CU) is 830 cycles per two resident workgroups against 512 cycles of MFMA.
// global_load_lds writes LDS without passing through registers.  Its destination is lane-linear (64 x 16 bytes
// contiguous), so the image is made of 1 KiB REGIONS, one per (32-column fragment f, 16-token k step ks), laid out as
// the transposing reads want them:  [read 0 | read 1][16-lane group g = (token half, column block)][4 tokens][16 columns]
//     DMA lane l = r*32 + g*8 + tl*2 + h  ->  token ks*16 + (g>>1)*8 + r*4 + tl,  columns f*32 + (g&1)*16 + h*8 .. + 7
//     read  r of lane l : region + r*512 + l*8   (each half-wave reads 256 contiguous bytes: no bank conflicts)
// Two stages of 32 KiB (A + B), two workgroups per CU; whole 64-token steps only (the launcher gives a ragged tail to
// the register-staged kernel, which can zero-fill).  vmcnt is counted by hand: the DMA is inline assembly.
constexpr int TD_STAGE = 32768;
template <typename T>
__global__ __launch_bounds__(TN_THREADS, 2) void gemm_tn_dma_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb, float* __restrict__ C,
    int64_t ldc, float* __restrict__ bias, int N, int K, int steps_per_slice, int total_steps, int dbg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  int lane = tid & 63;
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int ntk = K / 128;
  const int n0 = (blockIdx.x / ntk) * 128, k0 = (blockIdx.x % ntk) * 128;
  const int s_begin = blockIdx.y * steps_per_slice;
  int nsteps = total_steps - s_begin < steps_per_slice ? total_steps - s_begin : steps_per_slice;
  if (nsteps <= 0) return;
  if (dbg & 4) nsteps = 1;
  const bool do_bias = bias != nullptr && k0 == 0 && wk == 0;

  // DMA: instruction i of this wave fills region (f = i, ks = wave) of each operand
  const int dr = lane >> 5, dg = (lane >> 3) & 3, dtl = (lane >> 1) & 3, dh = lane & 1;
  const int drow = wave * 16 + (dg >> 1) * 8 + dr * 4 + dtl;
  const uint32_t a_off = (uint32_t)((drow * lda + (dg & 1) * 16 + dh * 8) * 2);
  const uint32_t b_off = (uint32_t)((drow * ldb + (dg & 1) * 16 + dh * 8) * 2);
  const char* a_at = (const char*)(A + (int64_t)s_begin * TN_BM * lda + n0);       // wave-uniform, advanced per step issued
  const char* b_at = (const char*)(B + (int64_t)s_begin * TN_BM * ldb + k0);
  const size_t a_step = (size_t)TN_BM * lda * 2, b_step = (size_t)TN_BM * ldb * 2;
  const uint32_t lds0 = g7_lds_addr(smem);
#define TD_ISSUE(STAGE)                                                                               \
  do {                                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
      g7_dma(a_at + i * 64, a_off, lds0 + (STAGE) * TD_STAGE + (i * 4 + wave) * 1024);                \
      g7_dma(b_at + i * 64, b_off, lds0 + (STAGE) * TD_STAGE + 16384 + (i * 4 + wave) * 1024);        \
    }                                                                                                 \
    a_at += a_step; b_at += b_step;                                                                   \
  } while (0)

  f32x16_t acc[2][2];
  float bsum[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[i][0][r] = 0.f; acc[i][1][r] = 0.f; }

#define TD_READ(KS, SET)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
    const char* pa_ = st + ((wn * 2 + i) * 4 + (KS)) * 1024 + lane * 8;                                \
    const char* pb_ = st + 16384 + ((wk * 2 + i) * 4 + (KS)) * 1024 + lane * 8;                        \
    fa[SET][i] = frag2(tn_read(pa_), tn_read(pa_ + 512));                                              \
    fb[SET][i] = frag2(tn_read(pb_), tn_read(pb_ + 512));                                              \
  }
  auto frag2 = [](v4s a, v4s b) { return (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; };

  TD_ISSUE(0);
  if (nsteps > 1) TD_ISSUE(1);
  for (int t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");      // step t has landed; step t + 1 may be in flight
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const char* st = smem + (t & 1) * TD_STAGE;
    bf16x8_t fa[2][2], fb[2][2];
    TD_READ(0, 0)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < 4) { TD_READ(ks + 1, (ks + 1) & 1) }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) tn_mma<T>(fa[ks & 1][i], fb[ks & 1][j], acc[i][j]);
        if (do_bias) {
          const uint4 w = __builtin_bit_cast(uint4, fa[ks & 1][i]);
          bsum[i] += tn_sum8<T>(w);}
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nsteps) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();                        // every wave has read stage t & 1
      TD_ISSUE(t & 1);
    }
  }
#undef TD_READ
#undef TD_ISSUE

  const int kcol = k0 + wk * 64 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int nbase = n0 + wn * 64 + i * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nbase + 8 * (r >> 2) + (r & 3);
      float* crow = C + (int64_t)n * ldc + kcol;
#pragma unroll
      for (int j = 0; j < 2; ++j) { if (dbg & 2) crow[j * 32] = acc[i][j][r]; else atomicAdd(crow + j * 32, acc[i][j][r]); }
    }
    if (do_bias) {
      const float t = bsum[i] + __shfl_xor(bsum[i], 32, 64);
      if (lane < 32) atomicAdd(bias + n0 + wn * 64 + i * 32 + lane, t);
    }
  }
}

// ---- many contractions in one launch, 256 x 256 tiles over the WHOLE token axis (round 3) ---------------------------------
// The kernels above split the token axis so that one contraction fills the chip: at the training batch (9 216 tokens) that
// is ~36 steps of 64 tokens per workgroup and 16 384 memory-side atomics to flush each 128 x 128 tile -- 290-590 TFLOP/s, and
// the atomics alone ~0.7 ms of a training step (profiles/r02_gemm_tn_variants.log, r02_train_kernel_stats_v8.csv).  The
// backward does not need a layer's dW before its end, so it now KEEPS the dY of every site (train.hip) and hands the
// weight gradients of a whole group of layers to one launch: 108 tiles of 256 x 256 per bert-base layer, each over all
// the tokens -- no split, no atomics (a tile has one owner: C is read, added to and written back with plain accesses), the
// epilogue amortised over 288 steps, and enough tiles to fill the chip.
//   workgroup   256 (n) x 256 (k) outputs, four waves of 128 x 128 (256 accumulators per lane), one per CU
//   step        32 tokens: per operand eight 32-column fragments x two 16-token k steps x two transposing reads = thirty-two
//               512-byte half regions in the read layout of gemm_tn_dma_kernel; stage = 32 KiB (A | B), FOUR stages (128 KiB).
//               A DMA instruction fills the 1 KiB WINDOW of read r of a fragment PAIR (f = 2p, 2p + 1): its lanes cover
//               8 tokens x 64 columns = eight whole 128-byte lines (a window per fragment, as the 128 x 128 kernel has it,
//               is sixteen HALF lines per instruction -- the request pattern that bounded the generation-6 GEMM)
//   pipeline    steps t+1 .. t+3 in flight while step t is computed; ONE barrier per step, in its middle: there every wave
//               has its part of step t+1 in LDS (vmcnt counted by hand) and has left step t-1, so step t+4 is issued into
//               that stage and the fragments of step t+1 are read under the second half's MFMAs.  (Four stages -- a lead of
//               two steps, ~3.9 k cycles -- left the waves parked 38 % of their time: SQ_WAIT_ANY, profiles/
//               r03_pmc_wgrad_batch_and_small_scan.txt; the loaded LDS-DMA latency is ~2.7 us.)
//   LDS port    per step 64 KiB of fragment reads + 32 KiB of DMA writes per 1024 MFMA cycles = 75 % (128 x 128 tiles: 150 %)
//   XCD         workgroup b runs on XCD b % 8: tile = (b % 8) * chunk + b / 8 -- each XCD walks a CONTIGUOUS run of
//               tiles, whose A (dY) panel is shared by the tiles of one row and stays in that L2
constexpr int TW_TOK = 32;
constexpr int TW_STAGE = 32768;
constexpr int TW_STAGES = 5;                   // 160 KiB: the whole LDS (one workgroup per CU anyway)
constexpr int TW_MAXP = 48;
struct TwProblem { const bf16_t* A; const bf16_t* B; float* C; float* bias; int lda, ldb, ldc, ntk; };
struct TwBatch { int n, chunk, total, steps; int tile_start[TW_MAXP + 1]; TwProblem p[TW_MAXP]; };

// acc + lo + hi of a packed bf16 pair (v_dot2c_f32_bf16 with a pair of ones)
typedef __bf16 tw_bf2 __attribute__((ext_vector_type(2)));
typedef _Float16 tw_h2 __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ float tw_sum2(uint32_t pair, float acc);
template <> __device__ __forceinline__ float tw_sum2<bf16_t>(uint32_t pair, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(tw_bf2, pair), __builtin_bit_cast(tw_bf2, 0x3f803f80u), acc, false);
}
template <> __device__ __forceinline__ float tw_sum2<f16_t>(uint32_t pair, float acc) {      // v_dot2_f32_f16 with (1, 1)
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(tw_h2, pair), __builtin_bit_cast(tw_h2, 0x3c003c00u), acc, false);
}
#define TW_WAIT(K_)                                                                                    \
  do {                                                                                                 \
    if ((K_) >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");                                   \
    else if ((K_) == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");                              \
    else if ((K_) == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                               \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                              \
  } while (0)

template <typename T>
__global__ __launch_bounds__(TN_THREADS, 1) void gemm_tn_wide_kernel(const TwBatch bt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  int lane = tid & 63;
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = (int)(blockIdx.x & 7) * bt.chunk + (int)(blockIdx.x >> 3);
  if (tile >= bt.total) return;
  int pi = 0;
  while (pi + 1 < bt.n && tile >= bt.tile_start[pi + 1]) ++pi;              // wave-uniform
  const bf16_t* const A = bt.p[pi].A;
  const bf16_t* const B = bt.p[pi].B;
  float* const C = bt.p[pi].C;
  float* const bias = bt.p[pi].bias;
  const int lda = bt.p[pi].lda, ldb = bt.p[pi].ldb, ldc = bt.p[pi].ldc, ntk = bt.p[pi].ntk;
  const int tl = tile - bt.tile_start[pi];
  const int n0 = (tl / ntk) * 256, k0 = (tl % ntk) * 256;
  const int nsteps = bt.steps;
  const bool do_bias = bias != nullptr && k0 == 0 && wk == 0;

  // DMA: this wave fills the four windows (k step ks, read r) of fragment pair p = wave of each operand.  Window
  // (p, ks, r) at ((p * 2 + ks) * 2 + r) KiB = [read r of fragment 2p | read r of fragment 2p + 1], 512 bytes each in the
  // lane order of gemm_tn_dma_kernel's reads:
  //     lane l = j*32 + g*8 + tl*2 + h  ->  token ks*16 + (g>>1)*8 + r*4 + tl,  columns (2p + j)*32 + (g&1)*16 + h*8 .. + 7
  // -- the eight lanes of a token (j, g & 1, h) read 128 contiguous bytes.
  const int dj = lane >> 5, dg = (lane >> 3) & 3, dtl = (lane >> 1) & 3, dh = lane & 1;
  const int drow = (dg >> 1) * 8 + dtl;                                    // + ks * 16 + r * 4 (per instruction, scalar)
  const uint32_t a_off = (uint32_t)((drow * lda + dj * 32 + (dg & 1) * 16 + dh * 8) * 2);
  const uint32_t b_off = (uint32_t)((drow * ldb + dj * 32 + (dg & 1) * 16 + dh * 8) * 2);
  const char* a_at = (const char*)(A + n0 + wave * 64);                    // wave-uniform, advanced per step issued
  const char* b_at = (const char*)(B + k0 + wave * 64);
  const size_t a_step = (size_t)TW_TOK * lda * 2, b_step = (size_t)TW_TOK * ldb * 2;
  const size_t a_row4 = (size_t)4 * lda * 2, b_row4 = (size_t)4 * ldb * 2;  // four tokens
  const uint32_t lds0 = g7_lds_addr(smem);
  const uint32_t dreg = (uint32_t)(wave * 4096);                           // the pair's four windows
  // instruction i = ks * 2 + r: tokens ks * 16 + r * 4 + ..  ->  window i of the pair
#define TW_ISSUE(STAGE)                                                                                \
  do {                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
      g7_dma(a_at + ((i >> 1) * 4 + (i & 1)) * a_row4, a_off, lds0 + (STAGE) * TW_STAGE + dreg + i * 1024); \
      g7_dma(b_at + ((i >> 1) * 4 + (i & 1)) * b_row4, b_off, lds0 + (STAGE) * TW_STAGE + 16384 + dreg + i * 1024); \
    }                                                                                                  \
    a_at += a_step; b_at += b_step;                                                                    \
  } while (0)

  f32x16_t acc[4][4];
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto frag2 = [](v4s a, v4s b) { return (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; };
  // fragment I of k step KS of the stage at ST: A fragments wn * 4 + I, B fragments wk * 4 + I (two transposing reads each)
  // (fragment f = 2p + j of k step KS: read r at window (p, KS, r), half j)
#define TW_FRAG_A(F, ST, KS, I) { const char* p_ = (ST) + ((wn * 2 + ((I) >> 1)) * 4 + (KS) * 2) * 1024 + ((I) & 1) * 512 + lane * 8; F[I] = frag2(tn_read(p_), tn_read(p_ + 1024)); }
#define TW_FRAG_B(F, ST, KS, I) { const char* p_ = (ST) + 16384 + ((wk * 2 + ((I) >> 1)) * 4 + (KS) * 2) * 1024 + ((I) & 1) * 512 + lane * 8; F[I] = frag2(tn_read(p_), tn_read(p_ + 1024)); }
#define TW_READ(FA, FB, ST, KS)                                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) { TW_FRAG_A(FA, ST, KS, i) TW_FRAG_B(FB, ST, KS, i) }
  // One k step of 16 tokens: 16 MFMAs from (FA, FB); behind each of the first eight, ONE fragment (two reads) of the next
  // k step goes into (NA, NB) from stage NST, in the order in which the next half consumes them.  Issue order pinned by
  // fences: left to itself the compiler put all 16 reads in front, and with more LDS operations in flight than lgkmcnt can
  // count (15) every MFMA of a half waited for reads issued just before it (2 200 cycles per step for 1 024 of MFMA).
#define TW_HALF(FA, FB, NA, NB, NST, NKS, DMA_COND, DMA_STAGE)                                         \
  _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                     \
    tn_mma<T>(FA[q >> 2], FB[q & 3], acc[q >> 2][q & 3]);                                    \
    if (q == 0) TW_FRAG_A(NA, NST, NKS, 0)                                                             \
    else if (q <= 4) TW_FRAG_B(NB, NST, NKS, q - 1)                                                    \
    else if (q <= 7) TW_FRAG_A(NA, NST, NKS, q - 4)                                                    \
    else if (DMA_COND) {                /* MFMAs 8-15 each cover one DMA issue of step t + 3 (wave-uniform branch) */ \
      const int i_ = (q - 8) >> 1;                                                                     \
      if (q & 1) g7_dma(b_at + ((i_ >> 1) * 4 + (i_ & 1)) * b_row4, b_off, lds0 + (DMA_STAGE) * TW_STAGE + 16384 + dreg + i_ * 1024); \
      else g7_dma(a_at + ((i_ >> 1) * 4 + (i_ & 1)) * a_row4, a_off, lds0 + (DMA_STAGE) * TW_STAGE + dreg + i_ * 1024); \
    }                                                                                                  \
    if (do_bias && (q & 3) == 3) {      /* the fragment holds 8 tokens of column (lane & 31): add them up under the MFMAs --  \
                                           four v_dot2c_f32_bf16 against (1, 1) instead of 14 shift / mask / add instructions: the \
                                           two waves that carry the bias sums reach the step's barrier with the other two */ \
      const uint4 w = __builtin_bit_cast(uint4, FA[q >> 2]);                                           \
      bsum[q >> 2] = tw_sum2<T>(w.x, tw_sum2<T>(w.y, bsum[q >> 2])) + tw_sum2<T>(w.z, tw_sum2<T>(w.w, 0.f));       \
    }                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  }

  const int pre = nsteps < TW_STAGES - 1 ? nsteps : TW_STAGES - 1;
  for (int sidx = 0; sidx < pre; ++sidx) TW_ISSUE(sidx);
  TW_WAIT(pre - 1);                                   // step 0 has landed; steps 1 .. 3 may be in flight
  __syncthreads();
  bf16x8_t fa0[4], fb0[4], fa1[4], fb1[4];
  TW_READ(fa0, fb0, smem, 0)
  int cs = 0;                                         // stage of step t; step t + 1 -> cs + 1, step t + 4 -> cs - 1 (mod 5)
  for (int t = 0; t < nsteps; ++t) {
    const char* st = smem + cs * TW_STAGE;
    __builtin_amdgcn_sched_barrier(0);
    TW_HALF(fa0, fb0, fa1, fb1, st, 1, false, 0)      // tokens 0-15 of step t; reads its tokens 16-31
    if (t + 1 < nsteps) {
      const int later = nsteps - 2 - t;               // steps behind t + 1 that exist
      TW_WAIT(later < 2 ? later : 2);                 // this wave's part of step t + 1 is in LDS (steps t + 2, t + 3 may be in flight)
      __syncthreads();                                // ... everyone's; and every wave has left step t - 1: its stage takes step t + 4
    }
    const bool issue = t + TW_STAGES - 1 < nsteps;
    const int istage = cs == 0 ? TW_STAGES - 1 : cs - 1;
    const int ns = cs + 1 == TW_STAGES ? 0 : cs + 1;
    const char* sn = smem + ns * TW_STAGE;            // (past the last step: a stage nobody writes any more; the fragments are not used)
    __builtin_amdgcn_sched_barrier(0);
    TW_HALF(fa1, fb1, fa0, fb0, sn, 0, issue, istage) // tokens 16-31 of step t; reads tokens 0-15 of step t + 1; issues step t + 4
    if (issue) { a_at += a_step; b_at += b_step; }
    cs = ns;
  }
#undef TW_READ
#undef TW_HALF
#undef TW_FRAG_A
#undef TW_FRAG_B
#undef TW_ISSUE

  // acc[i][j][r]: n = n0 + wn*128 + i*32 + 8*(r>>2) + 4*(lane>>5) + (r&3),  k = k0 + wk*128 + j*32 + (lane & 31): the tile
  // has one owner -- plain read-add-write, 128-byte rows per half-wave
  const int kcol = k0 + wk * 128 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nbase = n0 + wn * 128 + i * 32 + 4 * (lane >> 5);
    // eight rows at a time: all 32 loads of the batch are issued before its first store (C may alias itself as far as
    // the compiler knows: one read-add-write per element would wait for every load's round trip in turn)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));      // stays in its AGPRs until here (else all 256 are copied out at once: spills)
#pragma unroll
    for (int rb = 0; rb < 16; rb += 8) {
      float cv[8][4];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float* crow = C + (int64_t)(nbase + 8 * ((rb + r) >> 2) + ((rb + r) & 3)) * ldc + kcol;
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[r][j] = crow[j * 32];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float* crow = C + (int64_t)(nbase + 8 * ((rb + r) >> 2) + ((rb + r) & 3)) * ldc + kcol;
#pragma unroll
        for (int j = 0; j < 4; ++j) crow[j * 32] = cv[r][j] + acc[i][j][rb + r];
      }
    }
    if (do_bias) {                          // lanes l and l + 32 hold the two token halves of column (l & 31)
      const float tsum = bsum[i] + __shfl_xor(bsum[i], 32, 64);
      if (lane < 32) bias[n0 + wn * 128 + i * 32 + lane] += tsum;
    }
  }
}
}  // namespace

// ---- what the calling thread's last om_gemm_tn_acc / om_gemm_tn_acc_batch launched (om_debug_gemm_tn_last) ---------------------------------
// [0] bit mask: 1 gemm_tn_dma_kernel, 2 gemm_tn_kernel, 4 gemm_tn_wide_kernel; 0 after a call that launched nothing
// single call:  [1] DMA rows  [2] DMA slices  [3] DMA steps per slice  [4] register-staged rows  [5] its slices  [6] its rows per slice
// batch call:   [1] whole 32-token steps  [2] tiles (all problems)  [3] chunk of the last launch  [4] launches  [5] tail rows
//               [6] slices  [7] rows per slice of the last problem's tail
struct TnLast { int64_t v[8]; };
static thread_local TnLast g_tn_last = {{0, 0, 0, 0, 0, 0, 0, 0}};
extern "C" int om_debug_gemm_tn_last(int64_t out[8]) {
  if (!out) OM_FAIL("om_debug_gemm_tn_last: null argument");
  memcpy(out, g_tn_last.v, sizeof(g_tn_last.v));
  return 0;
}
static void tn_plan_words(const TnPlan& p, bool batch, int64_t n, int64_t v[8]) {
  for (int i = 0; i < 8; ++i) v[i] = 0;
  if (batch) {
    int64_t last = n % TN_PLAN_WIDE_MAXP ? n % TN_PLAN_WIDE_MAXP : TN_PLAN_WIDE_MAXP;      // n identical problems, 48 to a launch
    v[0] = 4 | (p.tail_rows ? 2 : 0); v[1] = p.wide_steps; v[2] = n * p.wide_tiles; v[3] = tn_plan_chunk(last * p.wide_tiles);
    v[4] = (n + TN_PLAN_WIDE_MAXP - 1) / TN_PLAN_WIDE_MAXP; v[5] = p.tail_rows; v[6] = p.reg_slices; v[7] = p.reg_per;
  } else {
    v[0] = (p.dma_rows ? 1 : 0) | (p.reg_rows ? 2 : 0);
    v[1] = p.dma_rows; v[2] = p.dma_slices; v[3] = p.dma_steps; v[4] = p.reg_rows; v[5] = p.reg_slices; v[6] = p.reg_per;
  }
}
// the shipped library keeps the selection bits of OM_OPT_WGRAD_DEBUG (3: register-staged kernel, >> 4: grid aim); bits 1 and 2 (plain stores
// instead of atomics, one step of the token loop) BREAK the result: timing probes, honoured only in a probe build (python -m openmatch_amd._build --probe)
static int tn_debug_word() {
#ifdef OM_PROBE_KERNELS
  return om_option(OM_OPT_WGRAD_DEBUG);
#else
  return om_option(OM_OPT_WGRAD_DEBUG) & ~6;
#endif
}
// host only: what om_gemm_tn_acc (batch == 0) or om_gemm_tn_acc_batch over `batch` problems of this shape would launch at the current
// switches, in the words of om_debug_gemm_tn_last; 0, all words zero, for an empty problem; -1 for a refusal (its reason in
// om_last_error).  Touches no GPU and leaves om_debug_gemm_tn_last as it is.
extern "C" int om_debug_gemm_tn_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int batch, int64_t out[8]) {
  if (!out) OM_FAIL("om_debug_gemm_tn_plan: null argument");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (batch < 0) { om_set_error(std::string(__func__) + ": batch must be 0 (a single call) or a problem count"); return -1; }
  if (M <= 0 || (!batch && (N <= 0 || K <= 0))) return 0;
  const TnPlan p = tn_plan(dtype, M, N, K, lda, ldb, tn_debug_word(), batch != 0);
  if (p.error) { om_set_error(std::string(__func__) + ": " + p.error); return -1; }
  tn_plan_words(p, batch != 0, batch, out);
  return 0;
}

bool omk_gemm_tn_ok(int dtype, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb) {
  return !tn_plan(dtype, M, N, K, lda, ldb, 0, false).error;
}

// the register-staged kernel over `slices` slices of `per` rows (tn_plan's reg_slices, reg_per)
template <typename T>
static int launch_tn_regs_t(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, float* bias, int64_t M,
                          int64_t N, int64_t K, int64_t slices, int64_t per, int dbg, hipStream_t s) {
  const int64_t tiles = (N / 128) * (K / 128);
  static std::atomic<bool> attr{false};
  if (!attr) {
    OM_HIP(hipFuncSetAttribute((const void*)gemm_tn_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS));
    attr = true;
  }
  hipLaunchKernelGGL(gemm_tn_kernel<T>, dim3((unsigned)tiles, (unsigned)slices), dim3(TN_THREADS), TN_LDS, s, (const bf16_t*)A, lda,
                     (const bf16_t*)B, ldb, C, ldc, bias, M, (int)N, (int)K, (int)per, dbg);
  OM_LAUNCH_CHECK();
  g_tn_last.v[0] |= 2;
  return 0;
}

static int launch_tn_regs(int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, float* bias, int64_t M,
                          int64_t N, int64_t K, int64_t slices, int64_t per, int dbg, hipStream_t s) {
  if (dtype == OM_F16) return launch_tn_regs_t<f16_t>(A, lda, B, ldb, C, ldc, bias, M, N, K, slices, per, dbg, s);
  return launch_tn_regs_t<bf16_t>(A, lda, B, ldb, C, ldc, bias, M, N, K, slices, per, dbg, s);
}

int omk_gemm_tn(int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, float* bias,
                int64_t M, int64_t N, int64_t K, hipStream_t s) {
  g_tn_last = TnLast{{0, 0, 0, 0, 0, 0, 0, 0}};
  const int dbg = tn_debug_word();
  const TnPlan p = tn_plan(dtype, M, N, K, lda, ldb, dbg, false);
  if (p.error) OM_FAIL(p.error);
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15)) OM_FAIL("gemm_tn: operands must be 16-byte aligned");
  const bool timing = om_timing_on();
  if (timing) om_timing_begin(OM_TIMING_GEMM_BF16, s);
  TnLast note;
  tn_plan_words(p, false, 0, note.v);
  note.v[0] = 0;                                       // the mask is set launch by launch
  g_tn_last = note;
  if (p.dma_rows) {
    const int64_t tiles = (N / 128) * (K / 128);
    const int64_t whole = p.dma_rows / TN_BM;
    static std::atomic<bool> attr{false};
    if (!attr) {
      OM_HIP(hipFuncSetAttribute((const void*)gemm_tn_dma_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * TD_STAGE));
      OM_HIP(hipFuncSetAttribute((const void*)gemm_tn_dma_kernel<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * TD_STAGE));
      attr = true;
    }
    if (dtype == OM_F16)
      hipLaunchKernelGGL(gemm_tn_dma_kernel<f16_t>, dim3((unsigned)tiles, (unsigned)p.dma_slices), dim3(TN_THREADS), 2 * TD_STAGE, s, (const bf16_t*)A, lda,
                         (const bf16_t*)B, ldb, C, ldc, bias, (int)N, (int)K, (int)p.dma_steps, (int)whole, dbg);
    else
      hipLaunchKernelGGL(gemm_tn_dma_kernel<bf16_t>, dim3((unsigned)tiles, (unsigned)p.dma_slices), dim3(TN_THREADS), 2 * TD_STAGE, s, (const bf16_t*)A, lda,
                         (const bf16_t*)B, ldb, C, ldc, bias, (int)N, (int)K, (int)p.dma_steps, (int)whole, dbg);
    OM_LAUNCH_CHECK();
    g_tn_last.v[0] |= 1;
  }
  const int64_t done = p.dma_rows;
  if (p.reg_rows && launch_tn_regs(dtype, (const bf16_t*)A + done * lda, lda, (const bf16_t*)B + done * ldb, ldb, C, ldc, bias, p.reg_rows, N, K,
                                   p.reg_slices, p.reg_per, dbg, s))
    return 1;
  if (timing) om_timing_end(OM_TIMING_GEMM_BF16, s, 2.0 * (double)M * (double)N * (double)K);
  return 0;
}

extern "C" int om_gemm_tn_acc(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc,
                              float* bias, int64_t M, int64_t N, int64_t K, void* stream) {
  g_tn_last = TnLast{{0, 0, 0, 0, 0, 0, 0, 0}};
  if (!A || !B || !C) OM_FAIL("null argument");
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return omk_gemm_tn(in_dtype, A, lda, B, ldb, C, ldc, bias, M, N, K, (hipStream_t)stream);
}

// ---- batched launch ----------------------------------------------------------------------------------------------------------
bool omk_gemm_tn_batch_ok(int dtype, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb) {
  return !tn_plan(dtype, M, N, K, lda, ldb, 0, true).error;
}

int omk_gemm_tn_batch(int dtype, const OmTnProblem* probs, int n, int64_t M, hipStream_t s) {
  g_tn_last = TnLast{{0, 0, 0, 0, 0, 0, 0, 0}};
  if (n <= 0 || M <= 0) return 0;
  if (!probs) OM_FAIL("gemm_tn_batch: null problem list");
  TnPlan tail = {nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const OmTnProblem& q = probs[i];
    if (!q.A || !q.B || !q.C) OM_FAIL("gemm_tn_batch: null operand");
    tail = tn_plan(dtype, M, q.N, q.K, q.lda, q.ldb, 0, true);
    if (tail.error) OM_FAIL(tail.error);
    if (q.ldc > 0x7fffffffLL) OM_FAIL("gemm_tn_batch: 16-bit operands with N and K multiples of 256 and at least 32 tokens only");
    if (((uintptr_t)q.A & 15) || ((uintptr_t)q.B & 15)) OM_FAIL("gemm_tn_batch: operands must be 16-byte aligned");
  }
  static std::atomic<bool> attr{false};
  if (!attr) {
    OM_HIP(hipFuncSetAttribute((const void*)gemm_tn_wide_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, TW_STAGES * TW_STAGE));
    OM_HIP(hipFuncSetAttribute((const void*)gemm_tn_wide_kernel<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, TW_STAGES * TW_STAGE));
    attr = true;
  }
  const bool timing = om_timing_on();
  const int64_t whole = tail.wide_steps;                 // M / 32: the same for every problem
  g_tn_last.v[1] = whole; g_tn_last.v[5] = tail.tail_rows;
  for (int first = 0; first < n; first += TW_MAXP) {
    const int cnt = n - first < TW_MAXP ? n - first : TW_MAXP;
    TwBatch bt;
    memset(&bt, 0, sizeof(bt));
    bt.n = cnt; bt.steps = (int)whole;
    int64_t total = 0;
    double flops = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const OmTnProblem& q = probs[first + i];
      bt.tile_start[i] = (int)total;
      bt.p[i].A = (const bf16_t*)q.A; bt.p[i].B = (const bf16_t*)q.B; bt.p[i].C = q.C; bt.p[i].bias = q.bias;
      bt.p[i].lda = (int)q.lda; bt.p[i].ldb = (int)q.ldb; bt.p[i].ldc = (int)q.ldc; bt.p[i].ntk = (int)(q.K / 256);
      total += (q.N / 256) * (q.K / 256);
      flops += 2.0 * (double)M * (double)q.N * (double)q.K;
      if (total > 0x3fffffffLL) OM_FAIL("gemm_tn_batch: too many tiles");
    }
    bt.tile_start[cnt] = (int)total;
    bt.total = (int)total;
    bt.chunk = (int)tn_plan_chunk(total);
    if (timing) om_timing_begin(OM_TIMING_GEMM_BF16, s);
    if (dtype == OM_F16) hipLaunchKernelGGL(gemm_tn_wide_kernel<f16_t>, dim3((unsigned)(bt.chunk * 8)), dim3(TN_THREADS), TW_STAGES * TW_STAGE, s, bt);
    else hipLaunchKernelGGL(gemm_tn_wide_kernel<bf16_t>, dim3((unsigned)(bt.chunk * 8)), dim3(TN_THREADS), TW_STAGES * TW_STAGE, s, bt);
    OM_LAUNCH_CHECK();
    g_tn_last.v[0] |= 4; g_tn_last.v[2] += total; g_tn_last.v[3] = bt.chunk; g_tn_last.v[4] += 1;
    if (timing) om_timing_end(OM_TIMING_GEMM_BF16, s, flops * (double)(whole * TW_TOK) / (double)M);
  }
  // tokens past the last whole 32-token step: the split kernels above (atomics; ordered behind the launch on the stream)
  const int64_t done = whole * TW_TOK;
  if (M > done) {
    for (int i = 0; i < n; ++i) {
      const OmTnProblem& q = probs[i];
      const TnPlan p = tn_plan(dtype, M, q.N, q.K, q.lda, q.ldb, 0, true);
      if (launch_tn_regs(dtype, (const bf16_t*)q.A + done * q.lda, q.lda, (const bf16_t*)q.B + done * q.ldb, q.ldb, q.C, q.ldc, q.bias,
                         p.reg_rows, q.N, q.K, p.reg_slices, p.reg_per, 0, s)) return 1;
      g_tn_last.v[6] = p.reg_slices; g_tn_last.v[7] = p.reg_per;
    }
  }
  return 0;
}

extern "C" int om_gemm_tn_acc_batch(int in_dtype, const OmTnProblem* problems, int n, int64_t M, void* stream) {
  return omk_gemm_tn_batch(in_dtype, problems, n, M, (hipStream_t)stream);
}
