// Which kernel an attention call runs: attn_plan_fwd(), attn_plan_bwd() and attn_plan_gqa() map (dtype, shape, which optional arguments
// are present, switches) to a plan and do nothing else -- no launch, no HIP call, no global written, no pointer dereferenced.
// omk_attention (attention.hip), omk_attention_bwd (train_kernels.hip) and omk_attention_gqa (attention_causal.hip) launch what they
// return; om_debug_attention_plan, om_debug_attention_bwd_plan and om_debug_attention_gqa_plan return the plan alone, so the three
// tables are testable on a machine without a GPU.  DESIGN.md 4c lists the rules in the order they are tested here.
#pragma once
#include "kernels.h"

struct AttnSwitches {
  int fast;         // OM_OPT_ATTENTION_FAST: bit 0 the 16-bit kernels for bfloat16 (float16 has no others); bit 1 (tests) the tile-at-a-time
                    // kernels at every length; bit 2 (A/B) the first online-softmax forward kernel instead of the chunked 16-bit one
};

// every switch the planners read, read once per call
static AttnSwitches attn_switches() { return AttnSwitches{om_option(OM_OPT_ATTENTION_FAST)}; }

// 32-key tiles a workgroup holds for a sequence of L keys (the template argument KT of the whole-row kernels): the one place the rule is written
static int attn_kt(int L) { return L <= 32 ? 1 : L <= 64 ? 2 : L <= 128 ? 4 : L <= 192 ? 6 : 8; }

static bool attn_is16(int dtype) { return dtype == OM_BF16 || dtype == OM_F16; }

// What a planner decided: the kernel family (OM_ATTN_FAMILY_* forward, OM_ATTN_BWD_FAMILY_* backward; 0: launch nothing -- an empty
// batch, or a refusal with its reason in `error`), the key tiles (4 for the kernels that walk 128-key chunks) and the two template flags.
struct AttnPlan { int family; int kt; bool bias, drop; const char* error; };

// w: half window of banded attention (key k visible from query q iff |q - k| <= w), <= 0 none
static AttnPlan attn_plan_fwd(int dtype, int64_t B, int L, int H, int heads, bool has_bias, float drop_p, bool has_kmax, bool has_cu, int w,
                              const AttnSwitches sw) {
  AttnPlan p = {0, 0, has_bias, drop_p > 0.f, nullptr};
  auto run = [&](int family, int kt) { p.family = family; p.kt = kt; return p; };
  auto refuse = [&](const char* why) { p.error = why; return p; };
  const bool d32 = H == heads * 32;
  // 1. arguments
  if (dtype != OM_F32 && !attn_is16(dtype)) return refuse("attention: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (B <= 0) return p;
  // 2. a window that reaches every key is full attention
  const bool band = w > 0 && w < L - 1;
  if (band && H != heads * 64) return refuse("banded attention: head_dim must be 64");
  if (band && (has_bias || p.drop || has_cu)) return refuse("banded attention: no position bias, dropout, packed rows or reverse walk");
  if (!band && !d32 && H != heads * 64) return refuse("head_dim must be 32 or 64");
  // (packed rows need a 16-bit kernel: 64-wide bfloat16 has one under bit 0 only)
  if (has_cu && !(dtype == OM_F16 || (dtype == OM_BF16 && (d32 || sw.fast)))) return refuse("packed rows: the 16-bit attention kernels");
  if (L < 1 || L > 1024) return refuse("sequence length must be in [1,1024]");
  if (L > 256 && p.drop && (L > 512 || dtype == OM_F32)) return refuse("attention with dropout: up to 512 tokens in the 16-bit formats (float32: 256)");
  if (B * heads > 0x7fffffffLL) return refuse("batch too large for one launch");
  // 3. 32-wide heads: one kernel for every format, length and switch value (beyond 256 tokens it walks 256-key chunks)
  if (d32) return run(OM_ATTN_FAMILY_D32, attn_kt(L));
  // 4. band
  if (band) return run(dtype == OM_F32 ? OM_ATTN_FAMILY_BAND32 : OM_ATTN_FAMILY_BAND16, 4);
  // 5. beyond 256 tokens, or at every length under bit 1 (tests; 16-bit formats: their masks and results must agree with the others'):
  // the online-softmax kernels -- the chunked 16-bit one, or the first one (float32; bfloat16 without bit 0; bit 2, A/B)
  const bool fast16 = dtype == OM_F16 || (dtype == OM_BF16 && sw.fast);       // float16 has the 16-bit kernels only
  if (L > 256 || ((sw.fast & 2) && dtype != OM_F32)) return run(fast16 && !(sw.fast & 4) ? OM_ATTN_FAMILY_FWD16C : OM_ATTN_FAMILY_LONG, 4);
  // 6. the low-instruction-count 16-bit kernel (inference, and training with dropout); its KT = 4 body without bias and dropout skips
  // the key tiles past kmax[b] (or past a packed sequence's end)
  if (fast16) return run(attn_kt(L) == 4 && !has_bias && !p.drop && (has_kmax || has_cu) ? OM_ATTN_FAMILY_FWD16_KMAX4 : OM_ATTN_FAMILY_FWD16, attn_kt(L));
  // 7. the generic kernel: float32, and bfloat16 without bit 0
  return run(OM_ATTN_FAMILY_GENERIC, attn_kt(L));
}

// packed: the training step runs over packed rows (then has_cu as well); has_bias / has_drel: the T5 / MPNet position bias and its gradient buffer
static AttnPlan attn_plan_bwd(int dtype, int64_t B, int L, int H, int heads, bool has_bias, bool has_drel, bool has_cu, bool packed,
                              const AttnSwitches sw) {
  AttnPlan p = {0, 0, has_bias, false, nullptr};
  auto run = [&](int family, int kt) { p.family = family; p.kt = kt; return p; };
  auto refuse = [&](const char* why) { p.error = why; return p; };
  const bool b16 = attn_is16(dtype);
  // 1. arguments
  if (B <= 0) return p;
  if (H != heads * 32 && H != heads * 64) return refuse("head_dim must be 32 or 64");
  // 2. 32-wide heads: one kernel up to 256 tokens in every format (it recomputes the row statistics)
  if (H == heads * 32) {
    if (L < 1 || L > 256) return refuse("training with head_dim 32 supports sequence lengths up to 256");
    if (has_cu && !b16) return refuse("packed rows: attention backward for 16-bit formats");
    if (B * heads > 0x7fffffffLL) return refuse("batch too large for one launch");
    if (has_bias != has_drel) return refuse("attention backward: a position bias needs its gradient buffer (and the reverse)");
    if (!b16 && dtype != OM_F32) return refuse("attention backward: dtype must be OM_F32, OM_BF16 or OM_F16");
    return run(OM_ATTN_BWD_FAMILY_D32, attn_kt(L));
  }
  // 3. the two-pass kernels with one score tile in registers at a time (16-bit formats, up to 512 tokens): beyond 256 tokens -- and from
  // 193 on: the generic kernel keeps a whole score row in registers, which is fine up to six key tiles (it wins by 4-7 % of a step at
  // 144 ... 192 tokens) and 20 % of a step slower with eight (profiles/r06_train_long_sequences.txt); at every length under bit 1
  // (tests).  They do not read cu: packed training is not offered beyond 256 tokens (om_encoder_train_packed_supported).
  if (L > 256 || (!packed && dtype != OM_F32 && ((sw.fast & 2) || ((sw.fast & 1) && L > 192)))) {
    if (L < 1 || L > 512) return refuse("attention backward (tile-at-a-time form): up to 512 tokens");
    if (!b16) return refuse("attention backward beyond 256 tokens: 16-bit formats");
    if (has_cu) return refuse("attention backward (tile-at-a-time form): no packed rows");
    return run(OM_ATTN_BWD_FAMILY_LONG, 4);
  }
  if (has_cu && !b16) return refuse("packed rows: attention backward for 16-bit formats");
  // 4. the transposing-read kernel: 16-bit formats up to 128 tokens under bit 0 (a bias without its gradient buffer: the generic kernel)
  if (b16 && L >= 1 && L <= 128 && sw.fast && has_bias == has_drel) return run(OM_ATTN_BWD_FAMILY_BWD16, attn_kt(L));
  // 5. the generic kernel: its three transposed [64][L + 4] images must fit the 160 KiB of LDS -- 256 keys in 16 bits, 192 in float32
  if (L < 1 || L > 256)
    return refuse(has_cu && !has_bias && !has_drel ? "packed rows: attention backward up to 256 tokens, head_dim 64" : "training supports sequence lengths up to 256");
  if (dtype == OM_F32 && L > 192) return refuse("float32 training supports sequence lengths up to 192 (16-bit formats: 256)");
  return run(OM_ATTN_BWD_FAMILY_GENERIC, attn_kt(L));
}

// ---- grouped-query attention over the projection [M, (heads + 2 kv_heads) * head_dim]: the causal kernels of the decoder-only stacks
// (head_dim 64: attention_causal.hip; 128: attention_causal128.hip) and Gemma3's bidirectional ones (256: attention_d256.hip) ----
// The dynamic LDS of a (head_dim, body) pair; each unit's launcher ties its kernels' own figure to this one with a static_assert.
constexpr int attn_gqa_lds(int head_dim, bool f32) {
  return head_dim == 64 ? (f32 ? 67584 : 33280) : head_dim == 128 ? (f32 ? 136192 : 66048) : (f32 ? 136960 : 65792);
}

// What attn_plan_gqa decided: the family (OM_ATTN_GQA_FAMILY_*; 0: launch nothing -- an empty batch, or a refusal with its reason in
// `error`), the body (float32, or the 16-bit one of the call's format), the grid and the dynamic LDS bytes.
struct AttnGqaPlan { int family; bool f32; unsigned grid_x, grid_y; int lds; const char* error; };

// causal: key k visible from query q iff k <= q (else w: the half window, <= 0 none); packed: rows packed by sequence, and then
// has_ext says whether the offsets cu are given (padded rows: the key extents kmax, which may be absent).  L is the padded length in
// both forms: a packed launch gets the grid and the body the padded launch of the same batch gets.
static AttnGqaPlan attn_plan_gqa(int dtype, int64_t B, int L, int heads, int kv_heads, int head_dim, bool causal, int w, bool packed, bool has_ext) {
  AttnGqaPlan p = {0, dtype == OM_F32, 0, 0, 0, nullptr};
  auto refuse = [&](const char* why) { p.error = why; return p; };
  // 1. arguments
  if (dtype != OM_F32 && !attn_is16(dtype)) return refuse("grouped-query attention: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (B <= 0) return p;
  // 2. the kernels that exist: causal at 64 and 128 columns without a window, bidirectional at 256
  if (causal && head_dim != 64 && head_dim != 128) return refuse("grouped heads: head_dim must be 64 or 128");
  if (causal && w > 0) return refuse("causal attention: no window");
  if (!causal && head_dim != 256) return refuse("bidirectional grouped-query attention: head_dim must be 256");
  if (L < 1 || L > 1024) return refuse(causal ? "causal attention: sequence length must be in [1,1024]" : "attention (head_dim 256): sequence length must be in [1,1024]");
  if (heads < 1 || kv_heads < 1 || heads % kv_heads) return refuse("grouped heads: n_kv_heads must be at least 1 and divide n_heads");
  if (packed && !has_ext)
    return refuse(causal ? "causal attention over packed rows: the sequence offsets cu" : "attention (head_dim 256) over packed rows: the sequence offsets cu");
  if (B * heads > 0x7fffffffLL) return refuse(causal ? "causal attention: batch too large for one launch" : "attention (head_dim 256): batch too large for one launch");
  // (the LDS-DMA addresses a sequence's K / V rows with a 32-bit byte offset from its first row)
  if (head_dim == 256 && (int64_t)L * ((int64_t)heads + 2 * (int64_t)kv_heads) * 512 > 0x7fffffffLL)
    return refuse("attention (head_dim 256): too many heads for one sequence's 32-bit row offsets");
  // 3. the family: a window that reaches every key is full attention
  p.family = head_dim == 64 ? OM_ATTN_GQA_FAMILY_CAUSAL64 : head_dim == 128 ? OM_ATTN_GQA_FAMILY_CAUSAL128
           : w > 0 && w < L - 1 ? OM_ATTN_GQA_FAMILY_BAND256 : OM_ATTN_GQA_FAMILY_FULL256;
  p.grid_x = (unsigned)(heads * B);
  p.grid_y = (unsigned)((L + 127) / 128);
  p.lds = attn_gqa_lds(head_dim, p.f32);
  return p;
}
