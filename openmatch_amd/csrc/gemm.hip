// om_gemm_nt: C = act(A · B^T + bias) (+|*) resid  on MFMA (bf16 / f16 or exact-f32), gfx950.
// Stands in for the ATen/BLAS GEMM under every nn.Linear on the hot path
// (HF:models/bert/modeling_bert.py:175-177,289-293,334-351; linear.py:22-23).
//
// Four tile shapes, each with a job none of the others does:
//   v1  128x128 tile, 2-stage LDS, direct stores             any M, N: small / ragged problems, odd alignments (this file)
//   v2  256x128 tile, 3-deep LDS ring (gemm_core2.h)          M >= 512 with few column tiles: the training batch (this file)
//   v6  256x256 tile, 4 waves of 128x128, 64-byte K steps     f32 (3 x bf16 split), training epilogues (gemm_wide6_*.hip)
//   v7  256x256 tile, persistent, 128-byte K steps            16-bit inference: whole tiles, fused LayerNorm (gemm_wide7*.hip)
// (the eight-wave 256x256 generation 4 that v6 replaced is gone: what it still caught -- a bias that is not 16-byte
// aligned, an epilogue v6 does not instantiate -- runs on v2)
#include "gemm_core2.h"
#include "gemm_epilogue.h"
#include "gemm_plan.h"

// ---- v1: 128x128 tile, direct (scattered) stores; any M, N --------------------------------------
template <typename T, typename OutT>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_nt_kernel(
    const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, OutT* C,
    int64_t ldc, int64_t M, int64_t N, int64_t K, GemmEpilogue ep, int group_m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t ntm = (M + GEMM_BM - 1) / GEMM_BM, ntn = (N + GEMM_BN - 1) / GEMM_BN;
  int64_t tm, tn;
  gemm_tile_coords(ntm, ntn, group_m, tm, tn);
  const int64_t m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
  f32x16_t acc[2][2];
  gemm_mainloop<T>(A, lda, B, ldb, M, N, K, m0, n0, smem, acc);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const EpiScalars es(ep);
#define OM_V1_CALL(A, TR) store_direct<OutT, A, TR>(acc[0][0], acc[0][1], acc[1][0], acc[1][1], m0 + wm * 64, n0 + wn * 64, C, ldc, M, N, ep, es)
  OM_EPI_SWITCH(es.act, es.train, OM_V1_CALL)
#undef OM_V1_CALL
}

// ---- split-K: C (f32, zero-initialised by the caller) += A[:, ks] · B[:, ks]^T per K slice --------
// Weight-gradient contractions have a long K (the token count) and a small output (768 x 768 is
// 9 tiles of 256^2): slicing K over blockIdx.y fills the chip; partial sums meet in f32 atomics.
template <typename T>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_nt_splitk_kernel(
    const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, float* __restrict__ C,
    int64_t ldc, int64_t M, int64_t N, int64_t K, int steps_per_slice) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t ntn = (N + GEMM_BN - 1) / GEMM_BN;
  const int64_t m0 = (blockIdx.x / ntn) * GEMM_BM, n0 = (blockIdx.x % ntn) * GEMM_BN;
  f32x16_t acc[2][2];
  gemm_mainloop<T>(A, lda, B, ldb, M, N, K, m0, n0, smem, acc,
                   (int64_t)blockIdx.y * steps_per_slice * GEMM_ROW_BYTES, steps_per_slice);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int64_t n = n0 + wn * 64 + ni * 32 + (lane & 31);
    if (n >= N) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int64_t mbase = m0 + wm * 64 + mi * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
        if (m < M) atomicAdd(C + m * ldc + n, acc[mi][ni][r]);
      }
    }
  }
}

// ---- v2: 256x128 tile, 3-deep LDS ring -----------------------------------------------------------
template <typename T, typename OutT>
__global__ __launch_bounds__(G2_THREADS) void gemm_nt_kernel2(
    const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, OutT* C,
    int64_t ldc, int64_t M, int64_t N, int64_t K, GemmEpilogue ep, int group_m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t m0, n0;
  g2_tile_coords(M, N, group_m, m0, n0);
  f32x16_t acc[2][2];
  unsigned long long* tr = ep.trace ? ep.trace + (size_t)blockIdx.x * 32 : nullptr;
  if (tr && threadIdx.x == 0) tr[0] = clock64();
  gemm_mainloop2<T>(A, lda, B, ldb, M, N, K, m0, n0, smem, acc, tr);
  if (tr && threadIdx.x == 0) tr[15] = clock64();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const EpiScalars es(ep);
  const int64_t nc = n0 + wn * 64;
  const float b0 = (ep.bias && nc + (lane & 31) < N) ? ep.bias[nc + (lane & 31)] : 0.f;
  const float b1 = (ep.bias && nc + 32 + (lane & 31) < N) ? ep.bias[nc + 32 + (lane & 31)] : 0.f;
  char* region = smem + wave * (32 * PATCH_STRIDE);
  __syncthreads();                                  // every wave is done reading the ring
#define OM_V2_CALL(A, TR)                                                                                   \
  store_patch<OutT, A, TR>(acc[0][0], acc[0][1], b0, b1, m0 + wm * 64, nc, C, ldc, M, N, ep, es, region);    \
  store_patch<OutT, A, TR>(acc[1][0], acc[1][1], b0, b1, m0 + wm * 64 + 32, nc, C, ldc, M, N, ep, es, region)
  OM_EPI_SWITCH(es.act, es.train, OM_V2_CALL)
#undef OM_V2_CALL
  if (tr && threadIdx.x == 0) { tr[28] = clock64(); tr[29] = blockIdx.x; }
}

static thread_local int g_gemm_last = 0;
void omk_gemm_note(int family) { g_gemm_last = family; }
extern "C" int om_debug_gemm_last(void) { return g_gemm_last; }

OM_DEFINE_LAUNCHER(launch_gemm, gemm_nt_kernel, GEMM_THREADS, GEMM_LDS_BYTES, GEMM_BM, GEMM_BN, OM_GEMM_FAMILY_V1)
OM_DEFINE_LAUNCHER(launch_gemm2, gemm_nt_kernel2, G2_THREADS, G2_LDS_BYTES, G2_BM, G2_BN, OM_GEMM_FAMILY_V2)

static unsigned long long* g_trace = nullptr;
extern "C" void om_debug_gemm_trace(unsigned long long* buf) { g_trace = buf; }
unsigned long long* omk_debug_trace() { return g_trace; }      // the scan kernels of search_scan.hip stamp into the same buffer
static int g_debug_gen = 0;     // GemmSwitches::debug_gen
extern "C" void om_debug_gemm_gen(int gen) { g_debug_gen = gen; }

bool omk_gemm_ln_fusable(int dtype, int64_t M, int64_t N, int64_t K) { return g7_shape_ok(dtype, M, N, K, gemm_switches(g_debug_gen)); }

int omk_gemm_wide7_f16(const GemmPlan& p, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                       int64_t N, int64_t K, const GemmEpilogue& ep, hipStream_t s);
int omk_gemm_wide7(const GemmPlan& p, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                   int64_t N, int64_t K, const GemmEpilogue& ep, hipStream_t s);
int omk_gemm_skinny(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N,
                    int64_t K, const GemmEpilogue& ep, hipStream_t s);

int omk_gemm(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C, int64_t ldc, int64_t M,
             int64_t N, int64_t K, const GemmEpilogue& ep_in, hipStream_t s, int64_t plan_m) {
  GemmEpilogue ep = ep_in;
  ep.trace = g_trace, g_gemm_last = 0;
  GemmSwitches sw = gemm_switches(g_debug_gen);
  sw.plan_m = plan_m;
  const GemmPlan p = gemm_plan(in_dtype, (uintptr_t)A, lda, (uintptr_t)B, ldb, out_dtype, (uintptr_t)C, ldc, M, N, K, ep, sw);
  if (p.error) OM_FAIL(p.error);
#define OM_GEMM_GO(TI, TO)                                                                                      \
  return p.family == OM_GEMM_FAMILY_V2 ? launch_gemm2<TI, TO>(A, lda, B, ldb, C, ldc, M, N, K, ep, s)           \
                                       : launch_gemm<TI, TO>(A, lda, B, ldb, C, ldc, M, N, K, ep, s)
  switch (p.family) {
    case 0: return 0;                                   // an empty problem
    case OM_GEMM_FAMILY_SKINNY: return omk_gemm_skinny(in_dtype, A, lda, B, ldb, C, ldc, M, N, K, ep, s);
    case OM_GEMM_FAMILY_G7: case OM_GEMM_FAMILY_G7_ONE_TILE: case OM_GEMM_FAMILY_G7C16: case OM_GEMM_FAMILY_G7R16:
      return in_dtype == OM_F16 ? omk_gemm_wide7_f16(p, A, lda, B, ldb, C, ldc, M, N, K, ep, s)
                                : omk_gemm_wide7(p, A, lda, B, ldb, C, ldc, M, N, K, ep, s);
    case OM_GEMM_FAMILY_V6:
      return in_dtype == OM_F32 ? omk_gemm_wide6_f32(in_dtype, A, lda, B, ldb, out_dtype, C, ldc, M, N, K, ep, s)
                                : omk_gemm_wide6_b16(in_dtype, A, lda, B, ldb, out_dtype, C, ldc, M, N, K, ep, s);
    case OM_GEMM_FAMILY_V1: case OM_GEMM_FAMILY_V2:
      if (in_dtype == OM_F16 && out_dtype == OM_F16) OM_GEMM_GO(f16_t, f16_t);
      if (in_dtype == OM_BF16 && out_dtype == OM_BF16) OM_GEMM_GO(bf16_t, bf16_t);
      if (in_dtype == OM_BF16 && out_dtype == OM_F32) OM_GEMM_GO(bf16_t, float);
      if (in_dtype == OM_F32 && out_dtype == OM_F32) OM_GEMM_GO(float, float);
      if (in_dtype == OM_F16 && out_dtype == OM_F32) OM_GEMM_GO(f16_t, float);
      if (in_dtype == OM_F32 && out_dtype == OM_BF16) return launch_gemm<float, bf16_t>(A, lda, B, ldb, C, ldc, M, N, K, ep, s);
  }
#undef OM_GEMM_GO
  OM_FAIL("the plan names no launcher");
}

// the plan alone, for a caller that must know the family before it launches (encoder.hip encoder_fork)
int omk_gemm_family(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, const void* C, int64_t ldc, int64_t M,
                    int64_t N, int64_t K, const GemmEpilogue& ep, int64_t plan_m) {
  GemmSwitches sw = gemm_switches(g_debug_gen);
  sw.plan_m = plan_m;
  const GemmPlan p = gemm_plan(in_dtype, (uintptr_t)A, lda, (uintptr_t)B, ldb, out_dtype, (uintptr_t)C, ldc, M, N, K, ep, sw);
  return p.error ? -1 : p.family;
}

// test hook (openmatch_hip.h): the family om_gemm_nt would launch, -1 for a refusal; the pointers are addresses only
extern "C" int om_debug_gemm_plan(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C,
                                  int64_t ldc, int64_t M, int64_t N, int64_t K, const float* bias, const void* resid, int64_t ldr, int act) {
  GemmEpilogue ep = {};
  ep.bias = bias; ep.resid = resid; ep.ldr = ldr; ep.act = act;
  const GemmPlan p = gemm_plan(in_dtype, (uintptr_t)A, lda, (uintptr_t)B, ldb, out_dtype, (uintptr_t)C, ldc, M, N, K, ep, gemm_switches(g_debug_gen));
  return p.error ? -1 : p.family;
}

// test hooks (openmatch_hip.h): the whole GemmEpilogue from C, field by field (everything but the trace pointer, which omk_gemm sets)
static GemmEpilogue debug_epilogue(const OmDebugGemmEpilogue& d) {
  GemmEpilogue ep = {};
  ep.bias = d.bias; ep.resid = d.resid; ep.ldr = d.ldr; ep.act = d.act;
  ep.pre_act = d.pre_act; ep.ldp = d.ldp; ep.drop_p = d.drop_p; ep.seed = d.seed; ep.drop_rows = d.drop_rows;
  ep.ln_stats = d.ln_stats; ep.ln_colsum = d.ln_colsum; ep.rln_stats = d.rln_stats; ep.rln_g = d.rln_g; ep.rln_b = d.rln_b;
  ep.stats_out = d.stats_out;
  ep.resid_lo = d.resid_lo; ep.out_lo = d.out_lo;
  ep.resid32 = d.resid32; ep.out32 = d.out32;
  ep.a_ln32 = d.a_ln32; ep.a_ln_g = d.a_ln_g; ep.a_ln_b = d.a_ln_b; ep.a_ln_stats_out = d.a_ln_stats_out;
  ep.rln32 = d.rln32; ep.rln32_stats = d.rln32_stats;
  ep.lo8 = d.lo8; ep.ln_inv_h = d.ln_inv_h; ep.ln_eps = d.ln_eps; ep.ln_rms = d.ln_rms; ep.reverse = d.reverse;
  ep.rows_dev = d.rows_dev;
  return ep;
}
extern "C" int om_debug_gemm_ex(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C, int64_t ldc,
                                int64_t M, int64_t N, int64_t K, const OmDebugGemmEpilogue* ep, void* stream) {
  if (!ep) OM_FAIL("om_debug_gemm_ex: null epilogue");
  return omk_gemm(in_dtype, A, lda, B, ldb, out_dtype, C, ldc, M, N, K, debug_epilogue(*ep), (hipStream_t)stream);
}
extern "C" int om_debug_gemm_plan_ex(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C,
                                     int64_t ldc, int64_t M, int64_t N, int64_t K, const OmDebugGemmEpilogue* ep) {
  if (!ep) return -1;
  const GemmPlan p = gemm_plan(in_dtype, (uintptr_t)A, lda, (uintptr_t)B, ldb, out_dtype, (uintptr_t)C, ldc, M, N, K, debug_epilogue(*ep),
                               gemm_switches(g_debug_gen));
  return p.error ? -1 : p.family;
}

int omk_gemm_splitk(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int64_t es = in_dtype == OM_F32 ? 4 : 2;
  if ((K * es) % GEMM_ROW_BYTES != 0) OM_FAIL("K*sizeof(elem) must be a multiple of 128 bytes");
  const int64_t tiles = ((M + GEMM_BM - 1) / GEMM_BM) * ((N + GEMM_BN - 1) / GEMM_BN);
  const int nk = (int)(K * es / GEMM_ROW_BYTES);
  int slices = (int)((1024 + tiles - 1) / tiles);          // aim at ~4 workgroups per CU
  if (slices > nk / 4) slices = nk / 4 > 0 ? nk / 4 : 1;   // but at least 4 K steps per slice
  const int per = (nk + slices - 1) / slices;
  slices = (nk + per - 1) / per;
  static std::atomic<bool> attr_bf16{false}, attr_f32{false};
  const bool timing = om_timing_on();
  const int tclass = es == 2 ? OM_TIMING_GEMM_BF16 : OM_TIMING_GEMM_F32;
  if (timing) om_timing_begin(tclass, s);
  if (in_dtype == OM_BF16) {
    if (!attr_bf16) { OM_HIP(hipFuncSetAttribute((const void*)gemm_nt_splitk_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES)); attr_bf16 = true; }
    hipLaunchKernelGGL((gemm_nt_splitk_kernel<bf16_t>), dim3((unsigned)tiles, slices), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                       (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C, ldc, M, N, K, per);
  } else if (in_dtype == OM_F16) {
    static std::atomic<bool> attr_f16{false};
    if (!attr_f16) { OM_HIP(hipFuncSetAttribute((const void*)gemm_nt_splitk_kernel<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES)); attr_f16 = true; }
    hipLaunchKernelGGL((gemm_nt_splitk_kernel<f16_t>), dim3((unsigned)tiles, slices), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                       (const f16_t*)A, lda, (const f16_t*)B, ldb, C, ldc, M, N, K, per);
  } else if (in_dtype == OM_F32) {
    if (!attr_f32) { OM_HIP(hipFuncSetAttribute((const void*)gemm_nt_splitk_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES)); attr_f32 = true; }
    hipLaunchKernelGGL((gemm_nt_splitk_kernel<float>), dim3((unsigned)tiles, slices), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                       (const float*)A, lda, (const float*)B, ldb, C, ldc, M, N, K, per);
  } else {
    OM_FAIL("unsupported dtype");
  }
  if (timing) om_timing_end(tclass, s, 2.0 * (double)M * (double)N * (double)K);
  OM_LAUNCH_CHECK();
  return 0;
}
extern "C" int om_debug_gemm_splitk(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                                    int64_t N, int64_t K, void* stream) {
  return omk_gemm_splitk(in_dtype, A, lda, B, ldb, C, ldc, M, N, K, (hipStream_t)stream);
}

extern "C" int om_gemm_nt(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
                          int out_dtype, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          const float* bias, const void* resid, int64_t ldr, int act,
                          void* stream) {
  GemmEpilogue ep = {};
  ep.bias = bias; ep.resid = resid; ep.ldr = ldr; ep.act = act;
  return omk_gemm(in_dtype, A, lda, B, ldb, out_dtype, C, ldc, M, N, K, ep, (hipStream_t)stream);
}
