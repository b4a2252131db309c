// om_gemm_nt, tile generation 7 (gemm_wide7.h): bf16 -> bf16 inference epilogues without fused LayerNorm.
#include "gemm_wide7.h"

bool omk_gemm_wide7_has(int act, bool resid, int lnf) {
  if (lnf == 2 || lnf == 3) return act == OM_ACT_NONE && resid;
  switch (act) {
    case OM_ACT_NONE: return lnf == 0 || !resid;
    case OM_ACT_GELU_TANH: return true;
    case OM_ACT_GELU_ERF: case OM_ACT_RELU: return !resid;
  }
  return false;
}

int omk_gemm_wide7_ln(const GemmPlan& p, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, const GemmEpilogue& ep, hipStream_t s);

// The training forward's FFN1: C = gelu(A B^T + bias) and ep.pre_act = gelu'(A B^T + bias), both as whole lines (kernel 7c16, TRAIN;
// the planner gates it on bit 5 of the continuous-ring mask)
bool omk_gemm_wide7_train_ok(int64_t M, int64_t N, int64_t K, int64_t ldc, const GemmEpilogue& ep) {
  return gemm_whole_tiles(M, N, K) && K * 2 >= 3 * G7_ROW_BYTES &&
         (ep.act & 0xff) == OM_ACT_GELU_ERF && (ep.act & OM_ACT_PRE_GRAD) && !(ep.act & OM_ACT_MUL_RESID) && ep.pre_act && ep.ldp == ldc &&
         !ep.resid && ep.drop_p == 0.f && (((uintptr_t)ep.pre_act | (uintptr_t)ep.bias) & 15) == 0 && !ep.ln_stats && !ep.rln_stats && !ep.stats_out;
}

int omk_gemm_wide7(const GemmPlan& p, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                   int64_t N, int64_t K, const GemmEpilogue& ep, hipStream_t s) {
  if (p.train) return launch7c<bf16_t, OM_ACT_GELU_ERF, 0, true>(A, lda, B, ldb, C, ldc, M, N, K, ep, s);      // (its own checks: launch7c)
  if (g7_check(p, M, N, K, ep)) return 1;
  if (p.lnf) return omk_gemm_wide7_ln(p, A, lda, B, ldb, C, ldc, M, N, K, ep, s);
  const int act = p.act, resid = p.resid;
  if (p.family == OM_GEMM_FAMILY_G7_ONE_TILE) {      // one tile per workgroup (A/B measurements of the cross-tile prefetch; two variants only)
#define OM_L7NP(A_) return g7_launch<gemm_nt_kernel7<bf16_t, A_, false, 0, false>, bf16_t>(p.family, A, lda, B, ldb, C, ldc, M, N, K, ep, s)
    if (act == OM_ACT_NONE && !resid) OM_L7NP(OM_ACT_NONE);
    if (act == OM_ACT_GELU_ERF && !resid) OM_L7NP(OM_ACT_GELU_ERF);
#undef OM_L7NP
  }
#define OM_L7(A_, R_) return launch7<bf16_t, A_, R_, 0>(p.family, A, lda, B, ldb, C, ldc, M, N, K, ep, s)
  switch (act) {
    case OM_ACT_NONE:      if (resid) OM_L7(OM_ACT_NONE, true); else OM_L7(OM_ACT_NONE, false);
    case OM_ACT_GELU_TANH: if (resid) OM_L7(OM_ACT_GELU_TANH, true); else OM_L7(OM_ACT_GELU_TANH, false);
    case OM_ACT_GELU_ERF:  if (!resid) OM_L7(OM_ACT_GELU_ERF, false); break;
    case OM_ACT_RELU:      if (!resid) OM_L7(OM_ACT_RELU, false); break;
  }
#undef OM_L7
  OM_FAIL("no generation-7 kernel for this epilogue");
}
