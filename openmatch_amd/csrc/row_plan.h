// Which row kernel a normalisation runs: row_fwd_plan() maps (entry, format, shape, row pitches, alignment, second plane) to the forward
// body of elementwise.hip, row_bwd_plan() maps (format, mode, shape, which f32 tensors and partial sums are given, the switch word) to the
// ln_bwd_kernel instantiation of train_kernels.hip with its grid and LDS bytes -- or to a refusal with its reason, or to "nothing to do".
// They do nothing else: no launch, no HIP call, no global written, no pointer read.  The four omk_layernorm* entries and the three
// backward entries call them; om_debug_row_fwd_plan / om_debug_row_bwd_plan return their words, so the rules are testable on a machine
// without a GPU.  DESIGN.md 4e lists the rules in the order tested here, and the oddities that are kept.
#pragma once
#include <stdint.h>

#include "train_kernels.h"

// the width every row kernel of the two units takes: four-element vectors, at most eight of them per lane of a 64-lane wave
static inline const char* row_width_error(int H) { return (H % 4 != 0 || H > 2048) ? "hidden size must be a multiple of 4 and <= 2048" : nullptr; }
// four-element vectors per lane of the one-wave-per-row kernels (the template argument MAX_VEC / NV)
static inline int row_max_vec(int H) { return H <= 1024 ? 4 : 8; }

// ---- forward ----
enum RowFwdEntry { ROW_FWD_LAYERNORM = 0, ROW_FWD_F32OUT = 1, ROW_FWD_FROM_F32 = 2, ROW_FWD_DUAL = 3 };      // omk_layernorm, _f32out, _from_f32, _dual

struct RowFwdPlan {
  const char* error;      // non-null: the call is refused, nothing is launched
  bool empty;             // M <= 0: nothing to do
  int body;               // OM_ROW_FWD_GENERIC (layernorm_kernel) | OM_ROW_FWD_X8 (layernorm_bf16x8_kernel)
  int nv;                 // generic: MAX_VEC 4 | 8; x8: NV 1..4
  int tin, tout;          // OM_F32 | OM_BF16 | OM_F16 of the rows read and written
  bool plane, lo8;        // x8: a second plane is read; that plane is the eight-bit one
};

// data_aligned: x, y and the second plane (where given) are 16-byte aligned; param_aligned: g and b (where given) are
static inline RowFwdPlan row_fwd_plan(int entry, int dtype, int64_t M, int H, int64_t ldx, int64_t ldy, bool data_aligned, bool param_aligned,
                                      bool plane, bool lo8) {
  const bool b16 = dtype == OM_BF16 || dtype == OM_F16;
  const int fmt = b16 ? dtype : OM_F32;                                           // (any other dtype value runs the f32 kernels)
  const bool f32_in = entry == ROW_FWD_FROM_F32 || entry == ROW_FWD_DUAL;         // these two take no second plane and never the x8 body
  RowFwdPlan p = {nullptr, false, OM_ROW_FWD_GENERIC, row_max_vec(H), f32_in ? OM_F32 : fmt, entry == ROW_FWD_F32OUT ? OM_F32 : fmt, false, false};
  auto refuse = [&](const char* why) { p.error = why; return p; };
  if (!f32_in && lo8 && !(plane && dtype == OM_F16 && H % 256 == 0 && ldx % H == 0))
    return refuse("eight-bit second plane: float16 rows of a whole-tile [M, H] tensor");
  if (const char* why = row_width_error(H)) return refuse(why);
  if (M <= 0) { p.empty = true; return p; }
  if (entry == ROW_FWD_DUAL && !b16) return refuse("a 16-bit output format");
  if (f32_in) return p;
  // the x8 body: 16-bit rows of whole 16-byte vectors -- both row pitches in their own format -- up to 1024 columns, everything aligned;
  // bfloat16 always takes it then, float16 only with a second plane.  A second plane has no other kernel.
  const int out_vec = p.tout == OM_F32 ? 4 : 8;
  const bool x8 = b16 && (dtype == OM_BF16 || plane) && H % 8 == 0 && H <= 1024 && ldx % 8 == 0 && ldy % out_vec == 0 && data_aligned && param_aligned;
  if (plane && !x8) return refuse("two-plane LayerNorm input: 16-bit rows of whole 16-byte vectors only");
  if (x8) {
    const int nv = (H / 8 + 31) / 32;
    p.body = OM_ROW_FWD_X8;
    p.nv = nv <= 1 ? 1 : nv;
    p.plane = plane;
    p.lo8 = plane && lo8;
  }
  return p;
}

// the OM_ROW_* word of include/openmatch_hip.h: composed here and nowhere else
static inline int row_fwd_word(const RowFwdPlan& p) {
  return p.body | p.nv << 4 | p.tin << 8 | p.tout << 12 | (p.plane ? 1 << 16 : 0) | (p.lo8 ? 1 << 17 : 0);
}

// ---- backward (ln_bwd_kernel<T, NV, MODE, PF>; MODE 0: x from memory, MODE 1: the embedding backward) ----
struct RowSwitches {
  int wgrad_stream;      // OM_OPT_TRAIN_WGRAD_STREAM: bit 3 takes the prefetching body out (A/B)
};
static inline RowSwitches row_switches() { return RowSwitches{om_option(OM_OPT_TRAIN_WGRAD_STREAM)}; }

struct RowBwdPlan {
  const char* error;      // non-null: the call is refused, nothing is launched
  bool empty;             // M <= 0: nothing to do (partial_blocks is 0)
  int mode, nv, waves;    // NV 3 | 4 | 8; waves per block 8 | 4
  bool prefetch;          // the body that loads the next row's x32 / dy while this row is reduced
  bool partial;           // MODE 0: the blocks' column sums go to `partial`, not into dg / db
  int64_t grid;
  int partial_blocks;     // what *partial_blocks receives: the MODE 0 grid, in MODE 1 as well
  int64_t lds;            // dynamic LDS bytes: [2][waves][H] f32, <= 64 KiB for both shapes
};

static inline RowBwdPlan row_bwd_plan(int dtype, int mode, int64_t M, int H, int L, bool has_x32, bool has_dy32, bool has_partial, RowSwitches sw) {
  RowBwdPlan p = {nullptr, false, mode, 0, 0, false, false, 0, 0, 0};
  auto refuse = [&](const char* why) { p.error = why; return p; };
  if (M <= 0) { p.empty = true; return p; }
  if (const char* why = row_width_error(H)) return refuse(why);
  if (mode == 1 && (L < 1 || M % L)) return refuse("embedding backward: M must be B * L");
  // eight waves per block; four where the wider per-lane state needs the 256-register budget (above 1024 columns, and MODE 1)
  p.waves = (H <= 1024 && mode == 0) ? 8 : 4;
  p.nv = (H <= 768 && mode == 0) ? 3 : row_max_vec(H);
  // the prefetching body: 16-bit rows with x32 and without dy32; wider rows spill with it
  p.prefetch = mode == 0 && (dtype == OM_BF16 || dtype == OM_F16) && has_x32 && !has_dy32 && H <= 768 && (sw.wgrad_stream & 8) == 0;
  p.partial = mode == 0 && has_partial;
  // two blocks per CU: ~12 MB of loads in flight (one row per wave at a time), what ~5 TB/s x ~2 us of latency needs;
  // more blocks only add same-address atomics on d_gamma / d_beta (1024 blocks: 41 us, 256: 30 us per call)
  const int64_t want = (M + p.waves - 1) / p.waves;
  p.grid = p.partial_blocks = (int)(want > OM_LNB_MAX_BLOCKS ? OM_LNB_MAX_BLOCKS : want);
  if (mode == 1) p.grid = (int64_t)L * (256 / L > 0 ? 256 / L : 1);      // one position per block, 256 / L blocks per position (kernel comment)
  p.lds = (int64_t)2 * p.waves * H * (int64_t)sizeof(float);
  return p;
}

static inline int row_bwd_word(const RowBwdPlan& p) {
  return OM_ROW_LN_BWD | p.nv << 4 | p.mode << 8 | p.waves << 12 | (p.prefetch ? 1 << 16 : 0) | (p.partial ? 1 << 17 : 0);
}
