// The token-axis split of the weight-gradient contraction (gemm_tn.hip): tn_plan() maps (format, shape, row pitches, the
// OM_OPT_WGRAD_DEBUG word, single call or one problem of a batch) to what is launched -- which kernels, over how many rows, in how many
// slices -- or to a refusal with its reason, as gemm_plan() does for om_gemm_nt.  It does nothing else: no launch, no HIP call, no
// global written.  omk_gemm_tn, omk_gemm_tn_batch and the two _ok predicates call it; om_debug_gemm_tn_plan returns its numbers, so the
// table is testable on a machine without a GPU.
#pragma once
#include <stdint.h>

#include "kernels.h"

constexpr int TN_PLAN_STEP = 64;        // tokens per step of the two 128 x 128 kernels (TN_BM)
constexpr int TN_PLAN_WIDE_STEP = 32;   // tokens per step of the 256 x 256 kernel (TW_TOK)
constexpr int TN_PLAN_WIDE_MAXP = 48;   // problems per launch of the 256 x 256 kernel (TW_MAXP)

struct TnPlan {
  const char* error;                    // non-null: the call is refused, nothing is launched
  // single call: whole 64-token steps to gemm_tn_dma_kernel, everything else to gemm_tn_kernel
  int64_t dma_rows, dma_slices, dma_steps;      // rows, slices (grid.y), 64-token steps per slice
  int64_t reg_rows, reg_slices, reg_per;        // rows, slices (grid.y), rows per slice (a multiple of 64)
  // one problem of a batch: whole 32-token steps to gemm_tn_wide_kernel, the tail (reg_*) to gemm_tn_kernel
  int64_t wide_steps, wide_tiles, tail_rows;
};

// slices of a token axis of `steps` steps for `tiles` output tiles: one round of two workgroups per CU (320, or the aim of
// OM_OPT_WGRAD_DEBUG >> 4 in units of 64) and no more -- every workgroup flushes 16 384 memory-side atomics -- and at least four steps
// per slice; the count is then what the rounded-up slice length leaves
static inline void tn_plan_split(int64_t steps, int64_t tiles, int dbg, int64_t* slices_out, int64_t* per_out) {
  const int64_t want = (dbg >> 4) ? (int64_t)(dbg >> 4) * 64 : 320;
  int64_t slices = (want + tiles - 1) / tiles;
  if (slices > steps / 4) slices = steps / 4 > 0 ? steps / 4 : 1;
  const int64_t per = (steps + slices - 1) / slices;
  *slices_out = (steps + per - 1) / per;
  *per_out = per;
}

// gemm_tn_kernel forms each lane's byte offset into a step in 32 bits (TN_FETCH1: a_lane + ua, likewise for B):
//     a_lane = (row0 * ld + cbl * 16 + h * 8) * 2     row0 = wave * 16 + r8 <= 55, cbl <= 3, h <= 1
//     ua     = (I >> 1) * 8 * ld * 2                  I <= 3: eight rows more
// so the largest offset is 63 * ld * 2 + 112 bytes, and the sum wraps unless 126 * ld + 112 < 2^32, i.e. ld <= 34 087 041.  The
// refusal uses the round figure below that, 64 * ld * 2 < 2^32 (ld < 2^25): a pitch of 64 MiB per row is no tensor of this library.
// The DMA and 256 x 256 kernels have their own, tighter conditions below (64 resp. 32 rows below 2^31 bytes).
static inline bool tn_plan_pitch_ok(int64_t lda, int64_t ldb) {
  const int64_t ld = lda > ldb ? lda : ldb;
  return 64 * ld * 2 < (1ll << 32);
}

static inline TnPlan tn_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int dbg, bool batch) {
  TnPlan p = {nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto refuse = [&](const char* why) { p.error = why; return p; };
  const bool b16 = dtype == OM_BF16 || dtype == OM_F16;
  if (batch) {
    if (!(b16 && M >= TN_PLAN_WIDE_STEP && N > 0 && K > 0 && N % 256 == 0 && K % 256 == 0 && lda % 8 == 0 && ldb % 8 == 0 && N <= (1 << 20) &&
          K <= (1 << 20) && (int64_t)TN_PLAN_WIDE_STEP * lda * 2 < (1ll << 31) && (int64_t)TN_PLAN_WIDE_STEP * ldb * 2 < (1ll << 31)))
      return refuse("gemm_tn_batch: 16-bit operands with N and K multiples of 256 and at least 32 tokens only");
    // (32 rows below 2^31 bytes is ld < 2^25: the tail's register-staged kernel is covered)
    p.wide_steps = M / TN_PLAN_WIDE_STEP;
    p.wide_tiles = (N / 256) * (K / 256);
    p.tail_rows = p.reg_rows = M - p.wide_steps * TN_PLAN_WIDE_STEP;
    dbg = 0;                                                       // the tail ignores the A/B switches
  } else {
    if (!(b16 && M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 128 == 0 && lda % 8 == 0 && ldb % 8 == 0 && N <= (1 << 20) && K <= (1 << 20)))
      return refuse("gemm_tn: 16-bit operands with N and K multiples of 128 only");
    if (!tn_plan_pitch_ok(lda, ldb)) return refuse("gemm_tn: lda and ldb must be below 2^25 elements (the register-staged kernel's 32-bit row offsets)");
    const int64_t whole = (dbg & 8) ? 0 : M / TN_PLAN_STEP;       // (dbg 8: the register-staged kernel for everything)
    if (whole >= 8 && 64 * lda * 2 < (1ll << 31) && 64 * ldb * 2 < (1ll << 31)) {
      p.dma_rows = whole * TN_PLAN_STEP;
      tn_plan_split(whole, (N / 128) * (K / 128), dbg, &p.dma_slices, &p.dma_steps);
    }
    p.reg_rows = M - p.dma_rows;
  }
  if (p.reg_rows > 0) {
    int64_t per;
    tn_plan_split((p.reg_rows + TN_PLAN_STEP - 1) / TN_PLAN_STEP, (N / 128) * (K / 128), dbg, &p.reg_slices, &per);
    p.reg_per = per * TN_PLAN_STEP;
  }
  return p;
}

// workgroups of a 256 x 256 launch over `total` tiles: eight runs (one per XCD) of `chunk` tiles
static inline int64_t tn_plan_chunk(int64_t total) { return (total + 7) / 8; }
