// om_gemm_nt's kernel choice: gemm_plan() maps (dtypes, shape, leading dimensions, addresses, epilogue, switches) to a GemmPlan and
// does nothing else -- no launch, no HIP call, no global written, no pointer dereferenced (addresses are tested for alignment and for
// null only).  omk_gemm (gemm.hip) launches what it returns; om_debug_gemm_plan returns the family alone, so the table is testable on
// a machine without a GPU.  DESIGN.md lists the rules in the order they are tested here.
#pragma once
#include "kernels.h"

// the instantiation tables and shape predicates of the families, each beside the switch it describes
bool omk_gemm_wide7_has(int act, bool resid, int lnf);                                                             // gemm_wide7.hip
bool omk_gemm_wide7_f16_has(int act, bool resid, int lnf);                                                         // gemm_wide7_f16.hip
bool omk_gemm_wide7_train_ok(int64_t M, int64_t N, int64_t K, int64_t ldc, const GemmEpilogue& ep);                // gemm_wide7.hip
bool omk_gemm_skinny_ok(int in_dtype, int out_dtype, int64_t M, int64_t N, int64_t K, const GemmEpilogue& ep, int max_m);   // gemm_skinny.hip

struct GemmSwitches {
  int variant;      // OM_OPT_GEMM_VARIANT: 1 | 2 | 6 pins a tile generation (A/B measurements; 0: automatic)
  int cont;         // OM_OPT_GEMM_CONT: the bit mask of the continuous-ring kernels
  int skinny_m;     // OM_OPT_GEMM_SKINNY_M: most rows of the few-rows kernel
  int debug_gen;    // om_debug_gemm_gen: 0 default; 6: never generation 7; 70: generation 7 with one tile per workgroup (A/B)
  int64_t plan_m;   // > 0: rule 5 prices the tile generations as for a contraction of this many rows (omk_gemm_as: a lane of the
                    //   encoder forward runs the kernels its whole batch would); 0: the call's own M
};

// every switch the planner reads, read once per call
static GemmSwitches gemm_switches(int debug_gen) {
  return GemmSwitches{om_option(OM_OPT_GEMM_VARIANT), om_option(OM_OPT_GEMM_CONT), om_option(OM_OPT_GEMM_SKINNY_M), debug_gen, 0};
}

// the continuous ring needs three K steps (its prefetch reaches at most one tile ahead)
static bool g7_ring_ok(int64_t K) { return K * 2 >= 3 * 128; }

// Shapes generation 7 takes from omk_gemm at these switches: what omk_gemm_ln_fusable promises the encoder, and the first half of
// g7_admits.  om_debug_gemm_gen(6) holds back bfloat16 only: float16 has no generation 6 to fall back to.
static bool g7_shape_ok(int dtype, int64_t M, int64_t N, int64_t K, const GemmSwitches& sw) {
  return M >= 512 && gemm_whole_tiles(M, N, K) && sw.variant == 0 && (dtype == OM_F16 || (dtype == OM_BF16 && sw.debug_gen != 6));
}

// Generation 7's admission, one predicate for both 16-bit formats (p holds act / resid / train / lnf; `wide`: rule 4 of gemm_plan).
// The one clause that differs: float16 refuses a multiplied residual next to a fused LayerNorm; bfloat16 has that kernel (T5's gated
// tanh-GELU, LNF 1).  A multiplied "residual" that is null is refused for float16 here and ignored by bfloat16, as before.
static bool g7_admits(int dtype, bool wide, int64_t M, int64_t N, int64_t K, const GemmEpilogue& ep, const GemmPlan& p, const GemmSwitches& sw) {
  const bool f16 = dtype == OM_F16;
  if (!wide || !g7_shape_ok(dtype, M, N, K, sw) || p.train || ((uintptr_t)ep.bias & 15)) return false;
  if (ep.ln_stats && (ep.rln_stats || ep.stats_out)) return false;      // fused LayerNorm: either the A side or the output side
  if (p.lnf >= 2 && !ep.stats_out) return false;                          // the output-side variants write row statistics
  if (p.resid && (ep.ldr * 2) % 128 != 0) return false;                   // residual rows are read in 128-byte units
  if (f16 && (ep.act & OM_ACT_MUL_RESID) && (p.lnf != 0 || !p.resid)) return false;
  return f16 ? omk_gemm_wide7_f16_has(p.act, p.resid, p.lnf) : omk_gemm_wide7_has(p.act, p.resid, p.lnf);
}

// Which generation-7 kernel serves an admitted call: 7c16 / 7r16 (continuous ring) where the ring fits and the format's bit of
// OM_OPT_GEMM_CONT is set, else the restart-per-tile kernel 7; 0: the eight-bit plane exists on the ring only and K is too short.
static int g7_kernel(int dtype, int64_t K, const GemmPlan& p, const GemmSwitches& sw) {
  if (sw.debug_gen == 70 && dtype == OM_BF16 && p.lnf == 0 && !p.resid && (p.act == OM_ACT_NONE || p.act == OM_ACT_GELU_ERF))
    return OM_GEMM_FAMILY_G7_ONE_TILE;                                    // A/B of the cross-tile prefetch: two variants only
  const bool ring = g7_ring_ok(K);
  if (!p.resid && p.lnf <= 1 && ring && (sw.cont & 1)) return OM_GEMM_FAMILY_G7C16;                      // bit 0: no residual
  if (p.resid && (p.lnf == 0 || p.lnf == 2) && ring && (sw.cont & 2)) return OM_GEMM_FAMILY_G7R16;      // bit 1: one-plane residual
  if (p.lnf == 4) return ring ? OM_GEMM_FAMILY_G7R16 : 0;
  // two-plane residual: bit 8 float16, bit 9 bfloat16 (off by default: the continuous kernel is 1.3 % faster end to end, but its 16 x 16 x 32
  // summation order moves the config-1 fixture's tie-broken MRR@10 from 0.0025 to 0.0037 against the reference's own 0.0035 -- one swapped pair)
  if (p.resid && p.lnf == 3 && ring && (sw.cont & (dtype == OM_BF16 ? 512 : 256))) return OM_GEMM_FAMILY_G7R16;
  return OM_GEMM_FAMILY_G7;
}

static GemmPlan gemm_plan(int in_dtype, uintptr_t A, int64_t lda, uintptr_t B, int64_t ldb, int out_dtype, uintptr_t C, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, const GemmEpilogue ep, const GemmSwitches sw) {
  const bool f16 = in_dtype == OM_F16, b16 = f16 || in_dtype == OM_BF16;
  GemmPlan p = {0, nullptr, ep.act & 0xff, ep.resid != nullptr, ep.pre_act != nullptr || ep.drop_p > 0.f, gemm_lnf(ep, f16)};
  auto run = [&](int family) { p.family = family; return p; };
  auto refuse = [&](const char* why) { p.error = why; return p; };
  // 1. arguments
  if (M <= 0 || N <= 0) return p;
  if (K <= 0) return refuse("K must be positive");
  const int64_t es = in_dtype == OM_F32 ? 4 : 2;
  if ((K * es) % 128 != 0) return refuse("K*sizeof(elem) must be a multiple of 128 bytes");
  if ((lda * es) % 16 != 0 || (ldb * es) % 16 != 0) return refuse("lda/ldb must keep rows 16-byte aligned");
  if ((A & 15) || (B & 15)) return refuse("A/B must be 16-byte aligned");
  if (p.act == OM_ACT_GELU_ERF_GRAD && !p.resid) return refuse("gelu-grad epilogue needs resid");
  // 2. few rows (a query, a handful of sequences): the weight-streaming kernel, N / 16 workgroups instead of N / 128
  if (sw.variant == 0 && sw.debug_gen == 0 && omk_gemm_skinny_ok(in_dtype, out_dtype, M, N, K, ep, sw.skinny_m)) return run(OM_GEMM_FAMILY_SKINNY);
  // 3. the f32-stream and pending-LayerNorm epilogues exist there only
  if (ep.resid32 || ep.out32 || ep.a_ln32 || ep.rln32) return refuse("f32 residual / f32 sum / pending-LayerNorm epilogue: the few-rows kernel only (gemm_skinny.hip)");
  // a second plane exists in generation 7's output-side LayerNorm kernels only: every other family would drop it without a word
  if ((ep.out_lo || ep.resid_lo) && p.lnf < 3) return refuse("two-plane residual stream: only with the output-side LayerNorm epilogue");
  // 4. the 256-row kernels write whole 16-byte output segments; small or ragged problems use v1
  const int64_t vec = out_dtype == OM_F32 ? 4 : 8;
  const bool wide = sw.variant != 1 && M >= 512 && N % vec == 0 && ldc % vec == 0 && (C & 15) == 0 &&
                    (!p.resid || (ep.ldr % vec == 0 && ((uintptr_t)ep.resid & 15) == 0));
  // 5. Pick the tile generation that finishes first: whole rounds of (256 CUs x resident workgroups)
  // times the tile's work over its measured relative efficiency (profiles/r01_selftest_gemm_v4.log).
  int gen = 1;
  if (wide) {
    // cost = rounds x (work a CU has in flight per round) / efficiency; v1 keeps 2 workgroups per CU
    const int64_t Mt = sw.plan_m > 0 ? sw.plan_m : M;
    auto rounds = [&](int64_t bm, int64_t bn, int64_t slots) {
      const int64_t tiles = ((Mt + bm - 1) / bm) * ((N + bn - 1) / bn);
      return (double)((tiles + slots - 1) / slots);
    };
    const double c4 = N >= 256 ? rounds(256, 256, 256) * (256.0 * 256.0) / 1.00 : 1e30;
    const double c2 = rounds(256, 128, 256) * (256.0 * 128.0) / 0.92;
    const double c1 = rounds(128, 128, 512) * (2 * 128.0 * 128.0) / 0.70;
    gen = c4 <= c2 && c4 <= c1 ? 6 : (c2 <= c1 ? 2 : 1);     // 6 falls back to 2 where it has no variant
    if (sw.variant == 2) gen = 2;
    if (sw.variant == 6) gen = N >= 256 ? 6 : 2;
    // A/B (OM_OPT_GEMM_CONT bit 4): plain 16-bit shapes of whole 256 x 256 tiles go to the continuous-ring kernels even when
    // those leave CUs idle (training: N = 768 at 9 216 token rows is 108 tiles -- the cost model above prefers 216 tiles of
    // 256 x 128 on generation 2; the idle CUs are not idle in a training step, the weight-gradient lane runs beside).
    // Bit 7 (round 5): float16 follows the same rules.
    const bool plain16 = (in_dtype == OM_BF16 || (f16 && (sw.cont & 128))) && out_dtype == in_dtype && !ep.pre_act && ep.drop_p == 0.f &&
                         gemm_whole_tiles(M, N, K) && g7_ring_ok(K);
    if ((sw.cont & 16) && plain16) gen = 6;
    // Round 5 (bit 6, default on): the model above prices generation 2 at 0.92 of a 256 x 256 tile's rate; measured in the training
    // step (profiles/r05_train_timeline_v0.txt) its K step takes ~2 650 cycles for 1 024 cycles of MFMA against 2 425 for 2 048 on
    // the continuous ring -- 0.55.  With that figure the QKV projection of the training forward (9 216 x 2 304: 324 whole tiles, two
    // rounds) moves to the continuous kernel (51 -> ~40 us); the N = 768 shapes (108 tiles on 256 CUs) stay where they are.
    if ((sw.cont & 64) && plain16 && gen == 2 && sw.variant == 0) {
      const double c7 = rounds(256, 256, 256) * (256.0 * 256.0), c2r = rounds(256, 128, 256) * (256.0 * 128.0) / 0.55;
      if (c7 < c2r) gen = 6;
    }
  }
  // 6. the training forward's FFN1 (gelu + gelu' to the tape, bit 5): the continuous 256 x 256 kernel with its two-output epilogue
  if (wide && b16 && out_dtype == in_dtype && sw.variant == 0 && sw.debug_gen != 6 && (sw.cont & 32) && omk_gemm_wide7_train_ok(M, N, K, ldc, ep))
    return run(OM_GEMM_FAMILY_G7C16);
  if (f16 && out_dtype == OM_F16) {
    // 7. float16 -> float16: generation 7 where it admits the call, else the generic 128 / 256-row tiles (which also take the training
    // epilogues of float16 training).  Round 5 (bit 7, default on): a PLAIN float16 contraction goes there only where the tile-choice
    // model above says so, as bfloat16 does.  Before, every whole-tile float16 shape went there: the N = 768 data gradients of a
    // training step (108 tiles on 256 CUs) took 66 / 51 us where generation 2 takes 62 / 47, and 60 / 48 against 50 / 40 at the 5 120
    // rows of a packed batch (profiles/r05_gemm_variant_probe.json).  The fused-LayerNorm variants exist in generation 7 only.
    if (g7_admits(in_dtype, wide, M, N, K, ep, p, sw) && (p.lnf != 0 || gen == 6 || !(sw.cont & 128))) {
      const int k7 = g7_kernel(in_dtype, K, p, sw);
      return k7 ? run(k7) : refuse("two-plane residual epilogue with the eight-bit plane: K >= 192");
    }
    if (p.lnf) return refuse("float16: the fused LayerNorm epilogues need whole 256 x 256 tiles");
    return run(wide && gen != 1 ? OM_GEMM_FAMILY_V2 : OM_GEMM_FAMILY_V1);
  }
  // 8. a fused LayerNorm is generation 7's, whatever the cost model says
  if (p.lnf && !(wide && in_dtype == OM_BF16 && out_dtype == OM_BF16 && N >= 256)) return refuse("fused LayerNorm epilogue needs the 256x256 bf16 kernel");
  if (p.lnf) gen = 6;
  if (gen == 6) {
    // v6 reads the bias as float4 and writes pre-activation pairs
    const bool aligned = (((uintptr_t)ep.bias & 15) == 0) && (ep.ldp % 2 == 0) && (((uintptr_t)ep.pre_act & 3) == 0);
    if (!aligned && p.lnf) return refuse("fused LayerNorm epilogue needs 16-byte aligned bias");
    if (!aligned) gen = 2;
    // 9. bfloat16 -> bfloat16 of whole tiles: generation 7
    else if (in_dtype == OM_BF16 && out_dtype == OM_BF16 && g7_admits(in_dtype, wide, M, N, K, ep, p, sw)) return run(g7_kernel(in_dtype, K, p, sw));
    else if (p.lnf) return refuse("fused LayerNorm epilogue: whole 256 x 256 tiles of bf16, inference only (generation 7)");
    // 10. generation 6 where it has the variant, else generation 2
    else if (omk_gemm_wide6_b16_has(in_dtype, out_dtype, p.act, p.train, p.resid) || omk_gemm_wide6_f32_has(in_dtype, out_dtype, p.act, p.train, p.resid))
      return run(OM_GEMM_FAMILY_V6);
    else gen = 2;
  }
  // 11. the generic tiles
  if (in_dtype == OM_F32 && out_dtype == OM_BF16) return run(OM_GEMM_FAMILY_V1);      // generation 1 only
  if (!(out_dtype == OM_F32 ? (in_dtype == OM_F32 || b16) : (in_dtype == OM_BF16 && out_dtype == OM_BF16))) return refuse("unsupported dtype combination");
  return run(gen == 2 ? OM_GEMM_FAMILY_V2 : OM_GEMM_FAMILY_V1);
}
