// Which layer loop an encoder forward runs: encoder_plan() maps (configuration, batch shape, what the caller wants back, which optional
// weights are present, switches) to an EncPlan and does nothing else -- no launch, no HIP call, no global written, no pointer
// dereferenced but the configuration's.  encoder_forward_impl (encoder.hip) carves its workspace by the plan and runs the loop it names;
// om_encoder_packed_supported asks it; om_debug_encoder_plan returns it alone, so the table is testable on a machine without a GPU.
// DESIGN.md 4d lists the rules in the order they are tested here.
#pragma once
#include <algorithm>

#include "kernels.h"

bool omk_gemm_skinny_ok(int in_dtype, int out_dtype, int64_t M, int64_t N, int64_t K, const GemmEpilogue& ep, int max_m);      // gemm_skinny.hip

struct EncSwitches {
  int fused_ln;       // OM_OPT_ENCODER_FUSED_LN: 0 = one normalisation kernel per site (A/B)
  int two_plane;      // OM_OPT_ENCODER_TWO_PLANE: bit 0 bfloat16, bit 1 float16: the second plane of the residual stream; bit 2: float16's in eight bits
  int pingpong;       // OM_OPT_ENCODER_PINGPONG: the fused path's kernels alternate their walk over the token rows
  int skinny_m;       // OM_OPT_GEMM_SKINNY_M: most rows of the few-rows paths
  int few_ln_fuse;    // OM_OPT_FEW_ROWS_LN_FUSE: most rows of the pending-LayerNorm path
  int attention_fast; // OM_OPT_ATTENTION_FAST: read by om_encoder_packed_supported only (attn_plan.h decides the attention kernel itself)
  int skip_pad;       // OM_OPT_ENCODER_SKIP_PAD: read by encoder_skip_pad only (the plan itself does not change with it)
  int cls_tail;       // OM_OPT_ENCODER_CLS_TAIL: read by encoder_cls_tail only (likewise)
  int lanes;          // OM_OPT_ENCODER_LANES: read by encoder_lanes only (likewise): the least padded token rows per lane, 0: off
};

// every switch the planner reads, read once per call (omk_gemm_ln_fusable reads OM_OPT_GEMM_VARIANT and om_debug_gemm_gen itself)
static EncSwitches encoder_switches() {
  return EncSwitches{om_option(OM_OPT_ENCODER_FUSED_LN), om_option(OM_OPT_ENCODER_TWO_PLANE), om_option(OM_OPT_ENCODER_PINGPONG),
                     om_option(OM_OPT_GEMM_SKINNY_M), om_option(OM_OPT_FEW_ROWS_LN_FUSE), om_option(OM_OPT_ATTENTION_FAST),
                     om_option(OM_OPT_ENCODER_SKIP_PAD), om_option(OM_OPT_ENCODER_CLS_TAIL), om_option(OM_OPT_ENCODER_LANES)};
}

struct EncPlanIn {
  const OmEncoderConfig* c;
  int64_t B, L, packed_rows;      // packed_rows > 0: om_encoder_forward_packed
  bool want_hidden;               // out_hidden is given
  bool gated_ffn, has_rel_bias, has_type_emb;      // layers_host[0].ffn1g_w, rel_bias, type_emb are given
};

// What the planner decided.  path: OM_ENC_PATH_*; 0: run nothing -- an empty batch, or a refusal with its reason in `error` (the one
// refusal that knows its path, "packed rows need the fused 16-bit path", keeps it for the OM_OPT_ENCODER_DEBUG line).
struct EncPlan {
  int path;
  const char* error;
  int64_t M;          // token rows: packed_rows, or B * L
  int64_t Mp;         // M in whole 256-row tiles for 16-bit batches of >= 512 rows (the buffers are that tall)
  int64_t Mg;         // rows of the contractions: M on the few-rows kernels, else Mp
  bool few_rows;      // the contractions run on the weight-streaming kernel (gemm_skinny.hip)
  bool two;           // fused BERT path: the residual stream has its second plane
  int lo8;            //   ... in eight bits (float16)
  bool pingpong;      // fused BERT path: alternate walk directions
  bool rel_bias;      // a relative-position bias is expanded and handed to every attention launch
  bool alloc_few32;   // carve's condition for r32a / r32b / y32: WIDER than path == BERT_FEW32 | BERT_PENDING_LN (follow-up)
};

// rule 1: the configuration alone (the texts of the former check_cfg)
static const char* encoder_cfg_error(const OmEncoderConfig* c) {
  if (c->dtype != OM_F32 && c->dtype != OM_BF16 && c->dtype != OM_F16) return "dtype must be OM_F32, OM_BF16 or OM_F16";
  // float16 (the reference's --fp16 = torch.cuda.amp float16, retriever/dense_retriever.py:76): BERT-family erf-GELU encoders, and
  // (round 5) T5 encoder stacks with ReLU / tanh-GELU feed-forwards.  As under the reference's autocast, nothing clamps: a checkpoint
  // whose feed-forward activations leave the float16 range overflows here as it does there (the caller picks OM_BF16 for those).
  if (c->dtype == OM_F16 && c->arch == OM_ARCH_BERT && c->act != OM_ACT_GELU_ERF) return "float16 mode: erf-GELU BERT-family encoders only";
  if (c->dtype == OM_F16 && c->arch == OM_ARCH_T5 && c->act != OM_ACT_RELU && c->act != OM_ACT_GELU_TANH)
    return "float16 mode: T5 feed-forwards with ReLU or tanh-GELU only";
  if (c->arch != OM_ARCH_BERT && c->arch != OM_ARCH_T5 && c->arch != OM_ARCH_MODERNBERT && c->arch != OM_ARCH_NOMICBERT) return "unknown arch";
  // NomicBERT (inference): 64-wide rotated heads, SwiGLU over one [gate; up] contraction (omk_swiglu_rows: whole 64-column groups), no
  // relative bias; all three formats -- float16 as for BERT: nothing clamps
  if (c->arch == OM_ARCH_NOMICBERT) {
    if (c->head_dim != 64 || c->n_heads * 64 != c->hidden) return "NomicBERT: only head_dim 64 with n_heads*64 == hidden is supported";
    if (c->act != OM_ACT_SILU) return "NomicBERT: hidden_act must be \"silu\"";
    if (!(c->rope_theta_global > 0.f)) return "NomicBERT: a positive rope theta";
    if (c->rel_buckets != 0) return "NomicBERT: no relative position bias (rel_buckets must be 0)";
    if (c->hidden % 64 || c->ffn % 64 || c->ffn < 64) return "NomicBERT: hidden and ffn must be multiples of 64";
  }
  // ModernBERT (inference): 64-wide heads, the gated erf-GELU feed-forward (float16 included), at most 64 layers (sliding_layers bits)
  if (c->arch == OM_ARCH_MODERNBERT) {
    if (c->head_dim != 64 || c->n_heads * 64 != c->hidden) return "ModernBERT: only head_dim 64 with n_heads*64 == hidden is supported";
    if (c->act != OM_ACT_GELU_ERF) return "ModernBERT: hidden_activation must be \"gelu\" (erf)";
    if (c->n_layers > 64) return "ModernBERT: at most 64 layers";
    if (!(c->rope_theta_global > 0.f) || !(c->rope_theta_local > 0.f) || c->half_window < 0)
      return "ModernBERT: positive rope thetas and a non-negative half window";
  }
  // BERT family: 32-wide heads (MiniLM-shaped encoders, attention_d32.hip) or 64-wide; T5 (and the monoT5 decoder): d_kv 64
  if (c->arch == OM_ARCH_T5 && (c->head_dim != 64 || c->n_heads * 64 != c->hidden))
    return "T5 encoders: only d_kv 64 with n_heads*64 == d_model is supported";
  if ((c->head_dim != 32 && c->head_dim != 64) || c->n_heads * c->head_dim != c->hidden)
    return "head_dim must be 32 or 64 with n_heads*head_dim == hidden";
  if (c->arch == OM_ARCH_BERT && c->rel_buckets != 0 && (c->rel_buckets < 4 || c->rel_buckets % 2 || c->rel_max_dist <= c->rel_buckets / 4))
    return "relative position bias: an even number of buckets >= 4 and a maximum distance beyond the exact buckets";
  const int es = c->dtype == OM_F32 ? 4 : 2;
  if ((c->hidden * es) % 128 || (c->ffn * es) % 128) return "hidden/ffn rows must be multiples of 128 bytes";
  if (c->head_in > 0 && ((c->head_in * 4) % 128 || c->head_in != c->hidden)) return "head_in must equal hidden";
  return nullptr;
}

// the BERT-family post-LayerNorm stacks: the four BERT loops serve both
static inline bool enc_bert_family(const OmEncoderConfig* c) { return c->arch == OM_ARCH_BERT || c->arch == OM_ARCH_NOMICBERT; }
// columns FFN1 writes: F, or NomicBERT's [gate; up] pair (2F; omk_swiglu_rows then leaves the F columns FFN2 contracts over)
static inline int enc_ffn1_cols(const OmEncoderConfig* c) { return c->arch == OM_ARCH_NOMICBERT ? 2 * c->ffn : c->ffn; }

// whether the four contractions of a layer run [rows, *] on the kernel that implements the fused-norm epilogues (F1: enc_ffn1_cols)
static bool enc_ln_fusable(int dt, int64_t rows, int H, int F, int F1) {
  return omk_gemm_ln_fusable(dt, rows, H, H) && omk_gemm_ln_fusable(dt, rows, F1, H) && omk_gemm_ln_fusable(dt, rows, 3 * H, H) &&
         omk_gemm_ln_fusable(dt, rows, H, F);
}

// whether the four contractions of a BERT layer take their pending-LayerNorm forms on the few-rows kernel at this shape (the
// epilogues' addresses are tested for null only)
static bool enc_pending_ln_ok(int dt, int64_t M, int H, int F, int F1, int act, int max_m) {
  static const float one = 1.f;
  GemmEpilogue a = {}, r = {};
  a.a_ln32 = &one; a.a_ln_g = &one; a.a_ln_b = &one;
  r.rln32 = &one; r.rln32_stats = &one; r.rln_g = &one; r.rln_b = &one; r.out32 = const_cast<float*>(&one);
  GemmEpilogue f = a;
  f.act = act;
  return omk_gemm_skinny_ok(dt, dt, M, 3 * (int64_t)H, H, a, max_m) && omk_gemm_skinny_ok(dt, dt, M, F1, H, f, max_m) &&
         omk_gemm_skinny_ok(dt, dt, M, H, H, r, max_m) && omk_gemm_skinny_ok(dt, dt, M, H, F, r, max_m);
}

// rules 2 ... 7, for a configuration that passed rule 1 -- or whose caller leaves that rule to the forward (om_encoder_packed_supported)
static EncPlan encoder_plan_checked(const EncPlanIn& in, const EncSwitches sw) {
  const OmEncoderConfig* c = in.c;
  EncPlan p = {};
  auto run = [&](int path) { p.path = path; return p; };
  auto refuse = [&](const char* why) { p.error = why; return p; };
  const int dt = c->dtype, H = c->hidden, F = c->ffn, F1 = enc_ffn1_cols(c);
  const bool half = dt == OM_BF16 || dt == OM_F16, packed = in.packed_rows > 0, bert = enc_bert_family(c), nomic = c->arch == OM_ARCH_NOMICBERT;
  // 2. rows -- filled whatever is refused below: the workspace size of a call does not depend on whether the call would be taken.
  // 16-bit batches of >= 512 tokens are padded to whole 256-row tiles: the persistent GEMM generation (gemm_wide7.h) takes whole
  // tiles only.  Rows are independent in every contraction, so whatever the pad rows hold stays in the pad rows; every other kernel
  // (embedding, attention, normalisation, pooling) sees M rows.
  p.M = packed ? in.packed_rows : in.B * in.L;
  p.Mp = half && p.M >= 512 ? (p.M + 255) / 256 * 256 : p.M;
  // (what carve has always tested for the f32-stream buffers: rule 4 without its bfloat16 exception, rule 7b without its two-plane bit)
  p.alloc_few32 = half && bert && !packed && p.M <= (int64_t)std::max(0, sw.skinny_m);
  // 3. arguments
  if (in.B <= 0) return p;
  if (in.L < 1 || in.L > 1024) return refuse("sequence length must be in [1,1024]");
  if (packed) {
    if (dt == OM_F32 || in.want_hidden || c->pooling == OM_POOL_NONE || c->n_layers < 1)
      return refuse("packed rows: 16-bit inference that returns representations only");
    if (in.packed_rows % 256 || in.packed_rows < 512 || in.packed_rows > in.B * in.L + 255)
      return refuse("packed_rows: a multiple of 256 in [512, B * L + 255]");
  }
  // 4. few rows (a served query, a handful of sequences; round 5): up to OM_OPT_GEMM_SKINNY_M rows the contractions run on the
  // weight-streaming kernel (gemm_skinny.hip) with the normalisations as kernels -- the persistent 256 x 256 tiles of the fused path
  // put 6 ... 24 workgroups on 256 CUs there and take ~150 us per layer whatever the batch (profiles/r05_small_forward_*.txt).
  // (bfloat16 BERT from 512 rows on stays on the fused path: its two-plane residual stream is what holds bfloat16 inside the
  // reference's own autocast deviation, and the unfused path keeps one plane)
  p.few_rows = !packed && half && p.M <= (int64_t)sw.skinny_m && !(dt == OM_BF16 && bert && p.M >= 512 && (sw.two_plane & 1) != 0);
  p.Mg = p.few_rows ? p.M : p.Mp;
  const bool fusable = sw.fused_ln != 0 && !p.few_rows && c->n_layers > 0 && H % 8 == 0 && enc_ln_fusable(dt, p.Mg, H, F, F1);
  // 5. ModernBERT: one loop, norms as kernels
  if (c->arch == OM_ARCH_MODERNBERT) {
    if (packed) return refuse("packed rows: not for ModernBERT (om_encoder_packed_supported is 0)");
    return run(OM_ENC_PATH_MODERNBERT);
  }
  // 6. T5: RMSNorm fused across the contractions (16-bit, >= 512 rows, widths of 256), else per site
  // (gated feed-forward layers keep the kernels: two folded GEMMs per norm measured 1 % slower, tools/gtr_bench.py)
  if (!bert) {
    if (!in.has_rel_bias) return refuse("T5 needs rel_bias and final_ln_g");
    p.rel_bias = true;
    p.path = fusable && !in.gated_ffn ? OM_ENC_PATH_T5_FUSED : OM_ENC_PATH_T5_PLAIN;
    if (packed && p.path != OM_ENC_PATH_T5_FUSED) return refuse("packed rows need the fused 16-bit path (T5: widths of 256, no gated feed-forward)");
    return p;
  }
  // 7. BERT family
  if (in.L > c->max_pos) return refuse(nomic ? "NomicBERT: sequence longer than max_pos (max_position_embeddings)" : "sequence longer than the position table");
  // (a table without a bucket count, or the reverse, is an error, never a forward without the bias)
  if (in.has_rel_bias != (c->rel_buckets > 0)) return refuse("relative position bias: rel_bias and rel_buckets must be set together");
  if (in.has_type_emb && c->type_vocab <= 0) return refuse("token types: a type_emb table needs type_vocab > 0");      // (type_emb == NULL: word + position only)
  p.rel_bias = in.has_rel_bias;
  const bool plane = (sw.two_plane & (dt == OM_BF16 ? 1 : 2)) != 0;      // this format's bit of the two-plane switch
  // 7a. LayerNorm fused across the contractions (16-bit, >= 512 rows, widths of 256, erf-GELU; NomicBERT: its SiLU is no epilogue --
  // FFN1 runs with OM_ACT_NONE over the 2F columns, which is the shape tested)
  if (fusable && (c->act == OM_ACT_GELU_ERF || nomic)) {
    p.two = plane;
    p.lo8 = plane && dt == OM_F16 && (sw.two_plane & 4) ? 1 : 0;
    p.pingpong = sw.pingpong != 0;
    return run(OM_ENC_PATH_BERT_FUSED);
  }
  // 7b. few rows with the residual stream in f32 (round 6; needs the format's two-plane bit), its LayerNorms pending up to
  // OM_OPT_FEW_ROWS_LN_FUSE rows where the few-rows kernel has the four epilogues; 7c. one normalisation kernel per site
  const bool few32 = p.few_rows && c->n_layers > 0 && plane;
  p.path = !few32 ? OM_ENC_PATH_BERT_PLAIN
           : p.M <= (int64_t)sw.few_ln_fuse && enc_pending_ln_ok(dt, p.Mg, H, F, F1, nomic ? OM_ACT_NONE : c->act, sw.skinny_m) ? OM_ENC_PATH_BERT_PENDING_LN
                                                                                                       : OM_ENC_PATH_BERT_FEW32;
  if (packed) return refuse("packed rows need the fused 16-bit path (hidden, ffn multiples of 256; erf-GELU)");
  return p;
}

static EncPlan encoder_plan(const EncPlanIn& in, const EncSwitches sw) {
  if (const char* why = encoder_cfg_error(in.c)) {
    EncPlan p = {};
    p.error = why;
    return p;
  }
  return encoder_plan_checked(in, sw);
}

// om_encoder_packed_supported at given switches: whether om_encoder_forward_packed would take (c, B, L, packed_rows) -- the plan of
// that call names a path and no refusal.  Three clauses are STRICTER than the plan: (a), (b), (c).
static bool encoder_packed_ok(const OmEncoderConfig* c, bool gated_ffn, int64_t B, int64_t L, int64_t packed_rows, const EncSwitches sw) {
  if (!c || B <= 0 || packed_rows <= 0) return false;
  if ((c->dtype != OM_BF16 && c->dtype != OM_F16) || (!enc_bert_family(c) && c->arch != OM_ARCH_T5)) return false;      // (what it keeps of rule 1)
  // (a) few rows: the padded entry's contractions take the weight-streaming kernel -- decided there on ITS row count B * L, so only a
  // batch whose PADDED form is that small is sent back (B = 64, L = 128 with 1 024 real tokens would otherwise run the tile kernels
  // over all 8 192 padded rows: ADVICE r5)
  if (B * L <= (int64_t)sw.skinny_m) return false;
  // (b) 64-wide bfloat16 heads without the 16-bit attention kernels: the forward would fail in its first attention launch
  // (restates attn_plan.h; kept as it was written, 32-wide heads included, which attn_plan_fwd would take)
  if (c->dtype == OM_BF16 && !sw.attention_fast) return false;
  // (c) float16 T5: ReLU only (the forward takes tanh-GELU as well)
  if (c->arch == OM_ARCH_T5 && c->dtype == OM_F16 && c->act != OM_ACT_RELU) return false;
  // the call it plans: the fields the host may leave unset (it asks with widths, format and rows) are set so that they refuse nothing
  OmEncoderConfig q = *c;
  q.pooling = OM_POOL_FIRST;
  q.max_pos = 1024;
  const bool rel = c->arch == OM_ARCH_T5 || c->rel_buckets > 0;
  const EncPlan p = encoder_plan_checked(EncPlanIn{&q, B, L, packed_rows, false, gated_ffn, rel, false}, sw);
  return p.path && !p.error;
}

// Whether a PADDED call (in.packed_rows == 0) whose plan is p skips its pad rows on the device ("pad rows"): it then
// runs the packed layer loops with the loose bound roundup256(B * L) -- a bound that always holds, so the host need not know the
// token count -- and its contractions read the count from device memory (GemmEpilogue::rows_dev).  The rule, stated once: the switch
// is on, the caller wants representations only, and the call plans a fused path that om_encoder_forward_packed would take at that
// bound.  Everything else -- float32, ModernBERT, few rows, widths off 256, gated T5, hidden states, an A/B switch that unfuses --
// runs as before.
static bool encoder_skip_pad(const EncPlanIn& in, const EncPlan& p, const EncSwitches sw) {
  if (!sw.skip_pad || in.packed_rows != 0 || in.want_hidden || in.c->pooling == OM_POOL_NONE) return false;
  if (p.error || (p.path != OM_ENC_PATH_BERT_FUSED && p.path != OM_ENC_PATH_T5_FUSED)) return false;
  return encoder_packed_ok(in.c, in.gated_ffn, in.B, in.L, p.Mp, sw);      // (p.Mp = roundup256(B * L) on a fused path)
}

// Whether a call whose plan is p runs the per-row tail of its LAST layer -- out-proj, FFN1, FFN2 and the two statistics reductions,
// everything after the last attention -- over the B [CLS] rows alone ("[CLS] rows of the last layer").  Pooling "first"
// reads nothing else of that layer, and after attention no row sees another.  The rule, stated once: the switch is on, the call plans
// the fused BERT path with 16-bit second planes (the eight-bit plane is stored tile by tile: not worth a gather), pooling is "first",
// no hidden states are wanted, there are at least two layers, B >= 512 (below that the compact launches would be mostly pad rows and
// the forward is launch-bound anyway), and the compact height Mc = roundup256(B) is at most a quarter of the buffers' (else the gain
// is not worth three launches; it is also what lets the compact buffers alias the dead qkv area, encoder.hip).  All three entry
// forms -- padded with or without pad-skip, packed -- plan alike: Mp covers each.  *Mc: the compact height where the rule holds.
static bool encoder_cls_tail(const EncPlanIn& in, const EncPlan& p, const EncSwitches sw, int64_t* Mc = nullptr) {
  if (!sw.cls_tail || p.error || p.path != OM_ENC_PATH_BERT_FUSED || p.lo8) return false;
  if (in.c->pooling != OM_POOL_FIRST || in.want_hidden || in.c->n_layers < 2 || in.B < 512) return false;
  const int64_t mc = (in.B + 255) / 256 * 256;
  if (4 * mc > p.Mp) return false;
  if (Mc) *Mc = mc;
  return true;
}

// Whether a PADDED call whose plan is p runs as two half-batches -- "lanes" -- on two streams ("two lanes"): sequences
// [0, B0) on the caller's stream, [B0, B) on a stream the library owns, each the whole chain of a call of its own over its rows of the
// one workspace.  Since the pad rows are skipped, a launch's last round of tiles leaves most of the chip empty; the other lane's
// workgroups take those CUs.  The rule, stated once: the switch is on (its value is the least PADDED token rows a lane must have); it is
// the padded entry; a pooling is set and no hidden states are wanted; the call plans the fused BERT path without a relative-position
// bias; B0 -- the largest count <= B / 2 with B0 * L in whole 256-row tiles, so that lane 1's buffers start on a tile -- and B - B0
// both have that many rows; and each lane, planned as the call (B0, L) / (B - B0, L) it is, gets the whole's path, planes and walk,
// the whole's pad-skip decision and the whole's [CLS]-tail decision: a lane runs the kernels the whole call would, over fewer rows,
// and every kernel of the chain keeps a row's bits whatever rides along.  A lane of ENC_LANE_ROWS_END padded rows or more does not
// fork either: the tail a lane can fill is one round of a launch however tall the launch is, while two chains that share the caches
// slow each other in proportion to their size -- 2 048 x 128 (lanes of 131 072 rows) measured 2.4 % SLOWER forked, 1 024 x 128 4.3 %
// faster, the batches between them 0.5-1.7 % faster.  What the forward adds at fork time (no capture, no timing
// mode, folded weights given, the same GEMM family per contraction): encoder.hip encoder_fork.  *B0: lane 0's sequences.
static const int64_t ENC_LANE_ROWS_END = 131072;
static bool encoder_lanes(const EncPlanIn& in, const EncPlan& p, const EncSwitches sw, int64_t* B0 = nullptr) {
  if (sw.lanes <= 0 || in.packed_rows != 0 || in.want_hidden || in.has_rel_bias || in.c->pooling == OM_POOL_NONE) return false;
  if (p.error || p.path != OM_ENC_PATH_BERT_FUSED || p.rel_bias || in.B < 2 || in.L < 1) return false;
  int64_t step = 256;      // sequences per whole number of tiles: 256 / gcd(L, 256)
  for (int64_t l = in.L; step > 1 && l % 2 == 0; l /= 2) step /= 2;
  const int64_t b0 = in.B / 2 / step * step;
  if (b0 <= 0 || b0 * in.L < (int64_t)sw.lanes || (in.B - b0) * in.L < (int64_t)sw.lanes) return false;
  if ((in.B - b0) * in.L >= ENC_LANE_ROWS_END) return false;
  const bool skip = encoder_skip_pad(in, p, sw), tail = encoder_cls_tail(in, p, sw);
  for (const int64_t bh : {b0, in.B - b0}) {
    EncPlanIn li = in;
    li.B = bh;
    const EncPlan lp = encoder_plan_checked(li, sw);
    if (lp.error || lp.path != p.path || lp.two != p.two || lp.lo8 != p.lo8 || lp.pingpong != p.pingpong) return false;
    if (encoder_skip_pad(li, lp, sw) != skip || encoder_cls_tail(li, lp, sw) != tail) return false;
  }
  if (B0) *B0 = b0;
  return true;
}
