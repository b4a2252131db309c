// om_encoder_forward: the whole eval-mode encoder (BERT post-LN -- NomicBERT on the same loops --, T5 pre-RMSNorm or ModernBERT pre-LN stack)
// + pooling + LinearHead + normalise, as a fixed sequence of launches on ONE stream -- or, for a large padded fused-BERT batch, as
// two such sequences over two halves of the batch on two streams, forked and joined on the caller's (encoder_fork).
// Stands in for DRModel.encode (modeling/dense_retrieval_model.py:133-155) and the HF model
// it calls (HF:models/bert/modeling_bert.py:623-684 / HF:models/t5/modeling_t5.py T5Stack).
//
// Activation buffers live in the caller's workspace ([M = B*L tokens] x width, compute dtype):
//   x   [M,H]   hidden state entering a layer (LN output; T5: residual stream)
//   y   [M,H]   pre-LayerNorm sum (BERT) / normed input (T5)
//   x1  [M,H]   post-attention hidden (BERT)
//   qkv [M,3H]  fused projection      ctx [M,H] attention output
//   ff  [M,F]   FFN inner activation  ff2 [M,F] gate (T5 v1.1, ModernBERT)
//   NomicBERT: ff [M,2F] holds (gate | up) of the one FFN1 contraction, ff2 [M,F] silu(gate) * up (omk_swiglu_rows), FFN2's operand
#include <math.h>

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "encoder_plan.h"

// Folded LayerNorm weights (W * gamma, its row sums, the folded bias) depend on the weights alone.  A caller that
// keeps weights across forwards folds them ONCE into a buffer it owns (om_encoder_fold_bytes / om_encoder_fold_weights,
// OmEncoderWeights::folded) -- 23 launches of ln_fold_kernel per forward gone; without one they are folded per forward
// into workspace scratch.  (Round 2 kept a library-owned cache keyed by weight pointers, which allocated inside a forward
// and could serve stale folds after an in-place weight update: gone.)
//
// Blob layout, per layer l: [qkv: W' (3H x H, 16-bit) | column sums (3H f32) | folded bias (3H f32)]
//                           [ffn1: W' (F x H)         | column sums (F f32)  | folded bias (F f32)], every part 256-byte aligned.
// BERT: qkv of layer l is folded with LN2 of layer l-1 (layer 0's slot is unused), ffn1 with LN1 of layer l.
// T5 (not gated): qkv with the layer's first RMSNorm weight (l >= 1), ffn1 with its second.
// NomicBERT: as BERT, the ffn1 slot 2F rows tall ([gate; up] is one weight, one fold); no biases, so the folded bias is the beta term alone.
namespace {
struct FoldSlot { size_t w, cs, bf; };
struct FoldLayout { size_t per_layer, total; FoldSlot qkv, ffn1; };
FoldLayout fold_layout(const OmEncoderConfig* c) {
  const size_t H = c->hidden, F = enc_ffn1_cols(c);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  FoldLayout L;
  L.qkv.w = take(3 * H * H * 2); L.qkv.cs = take(3 * H * 4); L.qkv.bf = take(3 * H * 4);
  L.ffn1.w = take(F * H * 2); L.ffn1.cs = take(F * 4); L.ffn1.bf = take(F * 4);
  L.per_layer = off;
  L.total = off * (size_t)c->n_layers;
  return L;
}
bool fold_applies(const OmEncoderConfig* c) {      // (ModernBERT runs no fused normalisation: nothing to fold)
  return c->arch != OM_ARCH_MODERNBERT && (c->dtype == OM_BF16 || c->dtype == OM_F16) && c->n_layers > 0 && c->hidden % 256 == 0 && c->ffn % 256 == 0;
}
}  // namespace

extern "C" size_t om_encoder_fold_bytes(const OmEncoderConfig* cfg) {
  if (!cfg || !fold_applies(cfg)) return 0;
  return fold_layout(cfg).total;
}

extern "C" int om_encoder_fold_weights(const OmEncoderConfig* c, const OmEncoderWeights* w, void* blob, size_t bytes, void* stream) {
  if (!c || !w || !blob) OM_FAIL("null argument");
  if (!fold_applies(c)) OM_FAIL("nothing to fold for this configuration (om_encoder_fold_bytes is 0)");
  const FoldLayout L = fold_layout(c);
  if (bytes < L.total || ((uintptr_t)blob & 255)) OM_FAIL("fold buffer too small or not 256-byte aligned");
  const OmLayerWeights* Ls = w->layers_host;
  if (!Ls) OM_FAIL("layers_host is null");
  hipStream_t s = (hipStream_t)stream;
  const int H = c->hidden, F = enc_ffn1_cols(c);
  const bool bert = enc_bert_family(c);
  for (int l = 0; l < c->n_layers; ++l) {
    char* base = (char*)blob + (size_t)l * L.per_layer;
    const OmLayerWeights& lw = Ls[l];
    if (l > 0) {
      const float* g = bert ? Ls[l - 1].ln2_g : lw.ln1_g;
      const float* beta = bert ? Ls[l - 1].ln2_b : nullptr;
      if (omk_ln_fold(c->dtype, lw.qkv_w, g, beta, bert ? lw.qkv_b : nullptr, base + L.qkv.w, (float*)(base + L.qkv.cs),
                      (float*)(base + L.qkv.bf), 3 * H, H, s)) return 1;
    }
    if (!lw.ffn1g_w) {
      const float* g = bert ? lw.ln1_g : lw.ln2_g;
      const float* beta = bert ? lw.ln1_b : nullptr;
      if (omk_ln_fold(c->dtype, lw.ffn1_w, g, beta, bert ? lw.ffn1_b : nullptr, base + L.ffn1.w, (float*)(base + L.ffn1.cs),
                      (float*)(base + L.ffn1.bf), F, H, s)) return 1;
    }
  }
  return 0;
}

// Wf / colsum / bf of one site: from the caller's fold buffer, or computed into workspace scratch
static int folded_weights(const OmEncoderConfig* c, const OmEncoderWeights* w, int layer, bool ffn1, const void* W, const float* g,
                          const float* beta, const float* b, int N, int K, void* scratch_w, float* scratch_cs, float* scratch_bf,
                          hipStream_t s, const void** Wf, const float** cs, const float** bf) {
  if (w->folded) {
    const FoldLayout L = fold_layout(c);
    const char* base = (const char*)w->folded + (size_t)layer * L.per_layer;
    const FoldSlot& sl = ffn1 ? L.ffn1 : L.qkv;
    *Wf = base + sl.w; *cs = (const float*)(base + sl.cs); *bf = (const float*)(base + sl.bf);
    return 0;
  }
  if (omk_ln_fold(c->dtype, W, g, beta, b, scratch_w, scratch_cs, scratch_bf, N, K, s)) return 1;
  *Wf = scratch_w; *cs = scratch_cs; *bf = scratch_bf;
  return 0;
}

struct EncWs {
  char *x, *y, *x1, *qkv, *ctx, *ff, *ff2;
  float *pooled, *headout, *posbias;
  float* final32;   // 16-bit runs: the last normalisation's output in f32 for the pooling tail (CLS rows, or all rows for mean pooling)
  int* lut;
  int* kmax;        // per batch row: 1 + its last unmasked key (omk_mask_extent), read by every layer's attention launch
  int *cu, *cls_rows, *row_map;   // packed rows (om_encoder_forward_packed): sequence offsets [B + 2], [CLS] row of each sequence [B], token of each row
  // fused-LayerNorm path (16-bit): folded weight, its column sums and bias, two statistics buffers per layer, the slot
  // partials one GEMM leaves (kernels.h: GemmEpilogue::stats_out), and the second plane of the two residual tensors
  char* wfold;
  float *colsum, *bfold, *stats1, *stats2, *slots;
  char *y_lo, *x1_lo;
  float *r32a, *r32b, *y32;   // few-rows 16-bit BERT (round 6): the f32 residual stream -- LayerNorm outputs and pre-LayerNorm sums as autocast keeps them
  size_t total;
};

// p: the call's plan, for its row counts (M; Mp, the height of the buffers the contractions run on) and alloc_few32
static EncWs carve(const OmEncoderConfig* c, const EncPlan& p, int64_t B, int64_t L, int64_t packed_rows, char* base) {
  const bool half = c->dtype == OM_BF16 || c->dtype == OM_F16;
  const size_t es = half ? 2 : 4;
  const size_t Mreal = (size_t)p.M, M = (size_t)p.Mp, H = c->hidden, F = c->ffn, F1 = enc_ffn1_cols(c);
  const bool bertf = enc_bert_family(c);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  EncWs w;
  w.x = take(M * H * es);
  w.y = take(M * H * es);
  w.x1 = take(M * H * es);
  w.qkv = take(M * 3 * H * es);
  w.ctx = take(M * H * es);
  w.ff = take(M * F1 * es);
  w.ff2 = take(c->arch == OM_ARCH_T5 || c->arch == OM_ARCH_MODERNBERT || c->arch == OM_ARCH_NOMICBERT ? M * F * es : 0);
  w.pooled = (float*)take((size_t)B * H * 4);
  w.headout = (float*)take((size_t)B * (c->head_out > 0 ? c->head_out : 1) * 4);
  // relative-position bias [heads, L, L]: T5, and a BERT-family stack configured with a bucket table (MPNet: rel_buckets > 0)
  const bool rel = c->arch == OM_ARCH_T5 || (c->arch == OM_ARCH_BERT && c->rel_buckets > 0);
  w.posbias = (float*)take(rel ? (size_t)c->n_heads * L * L * 4 : 0);
  w.lut = (int*)take(rel ? (size_t)(2 * L) * 4 : 0);
  w.kmax = (int*)take((size_t)B * 4);
  w.cu = (int*)take(packed_rows > 0 ? (size_t)(B + 2) * 4 : 0);
  w.cls_rows = (int*)take(packed_rows > 0 ? (size_t)B * 4 : 0);
  w.row_map = (int*)take(packed_rows > 0 ? (size_t)packed_rows * 4 : 0);
  w.final32 = (float*)take(half && c->pooling != OM_POOL_NONE ? (c->pooling == OM_POOL_FIRST ? (size_t)B : Mreal) * H * 4 : 0);
  const bool fuse = half && c->arch != OM_ARCH_MODERNBERT;   // fused-norm path (BERT LayerNorm / T5 RMSNorm; ModernBERT has none)
  const size_t wide = std::max((size_t)3 * H, F1);
  w.wfold = take(fuse ? wide * H * es : 0);
  w.colsum = (float*)take(fuse ? wide * 4 : 0);
  w.bfold = (float*)take(fuse ? wide * 4 : 0);
  // one (sum, sum of squares) buffer per LayerNorm site (written whole by omk_ln_stats_reduce: nothing to zero)
  w.stats1 = (float*)take(fuse ? (size_t)2 * c->n_layers * M * 8 : 0);
  w.stats2 = w.stats1 ? w.stats1 + (size_t)c->n_layers * M * 2 : nullptr;
  w.slots = (float*)take(fuse ? (size_t)2 * ((H + 255) / 256) * M * 8 : 0);
  const bool two = fuse && bertf;      // both 16-bit formats (round 6): the planes exist whether or not the switch uses them
  w.y_lo = take(two ? M * H * es : 0);
  w.x1_lo = take(two ? M * H * es : 0);
  w.r32a = (float*)take(p.alloc_few32 ? Mreal * H * 4 : 0);
  w.r32b = (float*)take(p.alloc_few32 ? Mreal * H * 4 : 0);
  w.y32 = (float*)take(p.alloc_few32 ? Mreal * H * 4 : 0);
  w.total = off;
  return w;
}

// the bytes of a call do not depend on whether it would be taken: the plan's row counts are filled before any of its refusals
static size_t workspace_bytes(const OmEncoderConfig* c, int64_t B, int64_t L, int64_t packed_rows) {
  const EncPlan p = encoder_plan_checked(EncPlanIn{c, B, L, packed_rows, false, false, false, false}, encoder_switches());
  return carve(c, p, B, L, packed_rows, nullptr).total;
}

extern "C" size_t om_encoder_workspace_bytes(const OmEncoderConfig* cfg, int64_t B, int64_t L) {
  if (!cfg || B <= 0 || L <= 0) return 0;
  return workspace_bytes(cfg, B, L, 0);
}

extern "C" size_t om_encoder_workspace_bytes_packed(const OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0) return 0;
  return workspace_bytes(cfg, B, L, packed_rows);
}

// Whether om_encoder_forward_packed would take (cfg, B, L, packed_rows) under the CURRENT run-time switches: the plan of that call names
// a path and no refusal.  The host layer asks before it chooses the packed entry, so that an A/B switch (OM_GEMM_VARIANT,
// OM_ENCODER_FUSED_LN = 0, OM_ATTENTION_FAST = 0, om_debug_gemm_gen) degrades a compact batch to the padded entry instead of failing
// the call.  It asks with widths, format, activation and rows (no head counts, no pooling, no position table): rule 1 of
// the plan is left to the forward but for format and arch, and the caller states its pooling and hidden-state wishes itself
// (encoder.py packed_rows_apply).  The clauses, three of them STRICTER than the plan: encoder_plan.h encoder_packed_ok.
extern "C" int om_encoder_packed_supported(const OmEncoderConfig* c, int gated_ffn, int64_t B, int64_t L, int64_t packed_rows) {
  return encoder_packed_ok(c, gated_ffn != 0, B, L, packed_rows, encoder_switches()) ? 1 : 0;
}

// host only: the plan of a forward at the current switches (include/openmatch_hip.h)
extern "C" int om_debug_encoder_plan(const OmEncoderConfig* c, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                                     int want_hidden) {
  if (!c) {
    om_set_error("om_debug_encoder_plan: null argument");
    return -1;
  }
  const EncPlan p = encoder_plan(EncPlanIn{c, B, L, packed_rows, want_hidden != 0, gated_ffn != 0, has_rel_bias != 0, c->type_vocab > 0},
                                 encoder_switches());
  if (p.error) {
    om_set_error(std::string("om_debug_encoder_plan: ") + p.error);
    return -1;
  }
  return p.path | (int)p.few_rows << 8 | (int)p.two << 9 | p.lo8 << 10;
}

// host only: whether a padded forward would skip its pad rows on the device (include/openmatch_hip.h)
extern "C" int om_debug_encoder_skip_pad(const OmEncoderConfig* c, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int want_hidden) {
  if (!c) {
    om_set_error("om_debug_encoder_skip_pad: null argument");
    return -1;
  }
  const EncPlanIn in = {c, B, L, 0, want_hidden != 0, gated_ffn != 0, has_rel_bias != 0, c->type_vocab > 0};
  const EncSwitches sw = encoder_switches();
  return encoder_skip_pad(in, encoder_plan(in, sw), sw) ? 1 : 0;
}

// host only: whether a forward would run its last layer's per-row tail over the [CLS] rows alone (include/openmatch_hip.h)
extern "C" int om_debug_encoder_cls_tail(const OmEncoderConfig* c, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                                         int want_hidden) {
  if (!c) {
    om_set_error("om_debug_encoder_cls_tail: null argument");
    return -1;
  }
  const EncPlanIn in = {c, B, L, packed_rows, want_hidden != 0, gated_ffn != 0, has_rel_bias != 0, c->type_vocab > 0};
  const EncSwitches sw = encoder_switches();
  return encoder_cls_tail(in, encoder_plan(in, sw), sw) ? 1 : 0;
}

extern "C" int om_t5_relative_bucket(int relative_position, int num_buckets, int max_distance) {
  // bidirectional: half the buckets for each sign; exact below max_exact, log-spaced above
  int nb = num_buckets / 2;
  int bucket = relative_position > 0 ? nb : 0;
  const int n = relative_position < 0 ? -relative_position : relative_position;
  const int max_exact = nb / 2;
  if (n < max_exact) return bucket + n;
  const double v = log((double)n / max_exact) / log((double)max_distance / max_exact) * (nb - max_exact);
  int large = max_exact + (int)v;
  if (large > nb - 1) large = nb - 1;
  return bucket + large;
}

static int check_cfg(const OmEncoderConfig* c) {
  if (const char* why = encoder_cfg_error(c)) OM_FAIL(why);
  return 0;
}

// One forward, as every layer loop below reads it.  packed rows (cu != NULL): the token axis holds only the rows up to each sequence's
// last unmasked token, back to back; every per-token kernel and contraction then runs over packed_rows rows instead of B * L.
struct EncCall {
  const OmEncoderConfig* c;
  const OmEncoderWeights* w;
  const int64_t* mask;
  int64_t B, L;
  const EncPlan& p;
  const EncWs& ws;
  const float* posbias;   // the expanded relative-position bias (plan.rel_bias), else NULL
  const int* cu;          // packed rows: ws.cu, else NULL
  const int* row_map;     // packed rows: ws.row_map (the token of each row: NomicBERT's rotary positions), else NULL
  void* out_hidden;
  hipStream_t s;
  const int* rows_dev;    // a padded call that skips its pad rows: &cu[B], the token count on the device, for every contraction of the
                          //   fused loops (GemmEpilogue::rows_dev); else NULL
  int64_t cls_mc;         // > 0 (encoder_cls_tail): bert_fused runs its last layer's per-row tail over this many compact rows, the [CLS] rows
  std::vector<int>* families;   // not NULL (bert_fused, asked by encoder_fork): launch nothing; append the GEMM family each contraction plans
  int64_t whole_mg, whole_mc;   // a lane (bert_fused): the whole call's Mg and compact height -- its contractions choose their tile
                                //   generation as for those (omk_gemm's plan_m), so a lane runs the kernels the whole would; else 0
};

// Where a layer loop left the stream that the last normalisation reads (final_norm below).
struct EncStream {
  const void* x;          // the pre-norm tensor [M, H] in the compute type; NULL: nothing is left to normalise, see `hidden`
  const void* x_lo;       //   its second plane (fused BERT path), in eight bits under lo8
  int lo8;
  const float *g, *b;     //   the normalisation's weights; rms: a T5 RMSNorm
  int rms;
  void* spare;            //   where the normalised rows go in the compute type when the caller gave no out_hidden
  char* hidden;           // x == NULL: the rows in the compute type as they are (a BERT stack of no layers), or already normalised
  const float* rows32;    //   ... in both forms (the two omk_layernorm_dual paths): their f32 copy, all M rows
  bool cls_compact;       // x / x_lo hold the B [CLS] rows alone, row b = sequence b, pitch H (bert_fused under encoder_cls_tail)
};

#define GEMM(A_, lda_, W_, ldw_, C_, ldc_, N_, K_, bias_, res_, ldr_, act_)                        \
  do {                                                                                             \
    if (om_gemm_nt(dt, A_, lda_, W_, ldw_, dt, C_, ldc_, Mg, N_, K_, bias_, res_, ldr_, act_, s)) \
      return 1;                                                                                    \
  } while (0)
#define RUN(expr) do { if (expr) return 1; } while (0)
// what every layer loop reads of its call (all of it, but for M in bert_fused)
#define ENC_LOCALS                                                                                                   \
  const OmEncoderConfig* c = k.c; const EncWs& ws = k.ws; const OmLayerWeights* Ls = k.w->layers_host; hipStream_t s = k.s;     \
  const int dt = c->dtype, H = c->hidden, F = c->ffn, nh = c->n_heads;                                              \
  const int64_t B = k.B, L = k.L, M = k.p.M, Mg = k.p.Mg
// NomicBERT on the four BERT loops: Q / K rotated in place after the QKV contraction; FFN1 is ONE contraction over (gate | up) -- F1 = 2F
// columns, no activation -- and omk_swiglu_rows turns them into FFN2's operand ffa (all Mg rows: FFN2 contracts over every row it is
// given); no biases (the weights' *_b are NULL).  BERT: F1 = F, act1 = the activation, ffa = ws.ff, and neither launch.
#define NOMIC_LOCALS                                                                                                 \
  const bool nomic = c->arch == OM_ARCH_NOMICBERT;                                                                   \
  const int F1 = enc_ffn1_cols(c), act1 = nomic ? OM_ACT_NONE : c->act;                                             \
  const void* const ffa = nomic ? ws.ff2 : ws.ff
#define NOMIC_ROPE() do { if (nomic) RUN(omk_rope(dt, ws.qkv, M, (int)L, H, c->rope_theta_global, s, k.row_map)); } while (0)
#define NOMIC_SWIGLU(rows_) do { if (nomic) RUN(omk_swiglu_rows(dt, ws.ff, ws.ff2, rows_, F, s)); } while (0)

// LayerNorm fused across the GEMMs (16-bit, large batches): the LayerNorm outputs are never
// written.  The GEMM that produces a pre-LayerNorm sum y also accumulates its row statistics; the
// GEMM that consumes LN(y) reads y itself against the folded weight W*gamma and rescales its
// rows in the epilogue; the GEMM that adds LN(y) as a residual normalises it on the fly
// (kernels.h: GemmEpilogue::ln_*, rln_*, stats_out).  23 of the 25 LayerNorm passes over
// [M,H] disappear (the embedding LayerNorm and the last one stay).
// (attention under every path: head_dim 32 -> attention_d32.hip; L > 256 -> the key-chunked / online-softmax kernels)
static int bert_fused(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  NOMIC_LOCALS;
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  const float inv_h = 1.0f / (float)H;
  // Two-plane residual stream (bfloat16): y1 = ws.y + ws.y_lo, y2 = ws.x1 + ws.x1_lo; the GEMMs that consume LN(y)
  // as their A operand read the first plane, the residual adds and the final LayerNorm read both.
  // (OM_OPT_ENCODER_TWO_PLANE: bit 0 bfloat16 (round 3), bit 1 float16 (round 6) -- the headline format, whose single plane was
  // what kept it outside the reference's own float16 autocast on small-weight models: DESIGN.md section 2)
  // bit 2 (float16, opt-in): the second plane in eight bits -- + 2.6 % passages/s, the same cosine / dot ratios, one more swapped tie on
  // the config-1 fixture's MRR@10 (gemm_wide7.h kernel 7r16, LNF == 4)
  const bool two = k.p.two;
  const int lo8 = k.p.lo8;
  const int nslots = 2 * (H / 256);
  // y1 lives in ws.y, y2 in ws.x1; ws.x is the embedding output (layer 0's input)
  // Ping-pong walk: every kernel of the chain starts on the rows its producer wrote last (reverse = 1 on every second
  // launch), so the head of each activation tensor (200-800 MB, far beyond the 32 MB of L2) is found in the 256 MB
  // memory-side cache instead of HBM.  OM_OPT_ENCODER_PINGPONG = 0 walks every kernel first row to last.
  const bool pingpong = k.p.pingpong;
  int walk = 1;               // the embedding kernel wrote first row to last
  // [CLS] rows of the last layer (encoder_plan.h encoder_cls_tail): after that layer's attention every launch is per-row work and
  // pooling "first" reads B rows, so the rows are gathered -- Mc = roundup256(B) of them, the pad replicating sequence B - 1 -- and the
  // three contractions run one or a few tiles each, with the epilogue fields of the full-row launches: a row's bits do not depend on
  // the tile it sits in.  The compact buffers live in ws.qkv, dead once attention has read it (seven planes [Mc, H] and two statistics
  // arrays against [Mp, 3H]: the rule's 4 Mc <= Mp); FFN1's compact output takes the head of ws.ff, dead as well.
  // k.families: the loop as a question -- which family does each contraction plan, with the pointers and epilogues it would launch with
  const bool probe = k.families != nullptr;
  auto gemm = [&](const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t rows, int64_t N, int64_t K,
                  const GemmEpilogue& ep) {
    const int64_t as = rows == Mg ? k.whole_mg : k.whole_mc;
    if (!probe) return omk_gemm(dt, A, lda, W, ldw, dt, C, ldc, rows, N, K, ep, s, as);
    k.families->push_back(omk_gemm_family(dt, A, lda, W, ldw, dt, C, ldc, rows, N, K, ep, as));
    return 0;
  };
#define LAUNCH(expr) do { if (!probe) RUN(expr); } while (0)
  const int64_t Mc = k.cls_mc;
  const size_t cplane = (size_t)Mc * H * 2;
  char* const cbase = ws.qkv;
  float* const cst2p = (float*)(cbase + 7 * cplane);
  float* const cst1 = cst2p + 2 * Mc;
  if (Mc > 0 && ((char*)(cst1 + 2 * Mc) > ws.qkv + (size_t)Mg * 3 * H * 2 || Mc > Mg || c->n_layers < 2 || lo8))
    OM_FAIL("[CLS] tail: the compact buffers do not fit the qkv area");
#define OM_WALK() (pingpong ? (walk ^= 1, walk ^ 1) : 0)
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    const bool last = l == c->n_layers - 1, tail = last && Mc > 0;
    float* st1 = tail ? cst1 : ws.stats1 + (size_t)l * Mg * 2;      // LN1 of this layer
    float* st2 = ws.stats2 + (size_t)l * Mg * 2;                     // LN2 of this layer
    const float* st2p = l ? ws.stats2 + (size_t)(l - 1) * Mg * 2 : nullptr;   // LN2 of the previous one
    // what the three per-row contractions read and write: the full-height buffers, or under `tail` their compact counterparts
    const int64_t Mr = tail ? Mc : Mg;
    const int* const rdev = tail ? nullptr : k.rows_dev;
    const char *ctx = ws.ctx, *xin = ws.x1, *xin_lo = ws.x1_lo;
    char *y = ws.y, *y_lo = ws.y_lo, *xout = ws.x1, *xout_lo = ws.x1_lo;
    GemmEpilogue e = {};
    // ---- QKV: x0 for the first layer, LN2_{l-1}(y2) folded afterwards
    if (l == 0) {
      e.bias = lw.qkv_b; e.reverse = OM_WALK(); e.rows_dev = k.rows_dev;
      RUN(gemm(ws.x, H, lw.qkv_w, H, ws.qkv, 3 * H, Mg, 3 * H, H, e));
    } else {
      const OmLayerWeights& pw = Ls[l - 1];
      const void* wf; const float *cs, *bfp;
      RUN(folded_weights(c, k.w, l, false, lw.qkv_w, pw.ln2_g, pw.ln2_b, lw.qkv_b, 3 * H, H, ws.wfold, ws.colsum, ws.bfold, s, &wf, &cs, &bfp));
      e.bias = bfp; e.ln_stats = st2p; e.ln_colsum = cs; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps; e.reverse = OM_WALK(); e.rows_dev = k.rows_dev;
      RUN(gemm(ws.x1, H, wf, H, ws.qkv, 3 * H, Mg, 3 * H, H, e));
    }
    if (!probe) NOMIC_ROPE();
    const int attn_walk = OM_WALK();
    LAUNCH(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, scale, 0.f, 0, s, attn_walk, ws.kmax, k.cu));
    if (tail) {
      const GatherPlane planes[3] = {{ws.ctx, cbase}, {ws.x1, cbase + cplane}, {two ? ws.x1_lo : nullptr, cbase + 2 * cplane}};
      LAUNCH(omk_gather_rows(planes, st2p, cst2p, k.cu ? ws.cls_rows : nullptr, B, L, Mc, H, s));
      ctx = cbase; xin = cbase + cplane; xin_lo = cbase + 2 * cplane; st2p = cst2p;
      y = cbase + 3 * cplane; y_lo = cbase + 4 * cplane; xout = cbase + 5 * cplane; xout_lo = cbase + 6 * cplane;
    }
    // ---- attention output + residual -> y1, statistics of LN1
    e = GemmEpilogue{};
    e.bias = lw.o_b; e.ldr = H; e.stats_out = ws.slots; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps;
    if (two) { e.out_lo = y_lo; e.lo8 = lo8; }
    if (l == 0) {
      e.resid = ws.x;                    // the embedding output: one plane
    } else {
      const OmLayerWeights& pw = Ls[l - 1];
      e.resid = xin; e.rln_stats = st2p; e.rln_g = pw.ln2_g; e.rln_b = pw.ln2_b;
      if (two) e.resid_lo = xin_lo;
    }
    e.reverse = OM_WALK(); e.rows_dev = rdev;
    RUN(gemm(ctx, H, lw.o_w, H, y, H, Mr, H, H, e));
    LAUNCH(omk_ln_stats_reduce(ws.slots, nslots, Mr, st1, s));
    // ---- FFN1 on LN1(y1), folded
    const void* wf1; const float *cs1, *bf1;
    RUN(folded_weights(c, k.w, l, true, lw.ffn1_w, lw.ln1_g, lw.ln1_b, lw.ffn1_b, F1, H, ws.wfold, ws.colsum, ws.bfold, s, &wf1, &cs1, &bf1));
    e = GemmEpilogue{};
    e.bias = bf1; e.act = act1; e.ln_stats = st1; e.ln_colsum = cs1; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps;
    e.reverse = OM_WALK(); e.rows_dev = rdev;
    RUN(gemm(y, H, wf1, H, ws.ff, F1, Mr, F1, H, e));
    if (!probe) NOMIC_SWIGLU(Mr);
    // ---- FFN2 + LN1(y1) as the residual -> y2, statistics of LN2
    e = GemmEpilogue{};
    e.bias = lw.ffn2_b; e.resid = y; e.ldr = H; e.rln_stats = st1; e.rln_g = lw.ln1_g; e.rln_b = lw.ln1_b;
    e.stats_out = ws.slots; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps;
    if (two) { e.resid_lo = y_lo; e.out_lo = xout_lo; e.lo8 = lo8; }
    e.reverse = OM_WALK(); e.rows_dev = rdev;
    RUN(gemm(ffa, F, lw.ffn2_w, F, xout, H, Mr, H, F, e));
    // (the last layer's LN2 is final_norm's, which computes its own statistics: the slots the kernel had to write are not reduced)
    if (!last) LAUNCH(omk_ln_stats_reduce(ws.slots, nslots, Mg, st2, s));
  }
#undef LAUNCH
#undef OM_WALK
  const OmLayerWeights& lastw = Ls[c->n_layers - 1];
  *out = EncStream{ws.x1, two ? ws.x1_lo : nullptr, lo8, lastw.ln2_g, lastw.ln2_b, 0, ws.x};
  if (Mc > 0) { out->x = cbase + 5 * cplane; out->x_lo = two ? cbase + 6 * cplane : nullptr; out->cls_compact = true; }
  return 0;
}

// A handful of rows (<= 64: a served query), 16-bit (round 6): the f32 residual stream of bert_few32 with its LayerNorms PENDING --
// no normalisation launches between the embedding and the last layer (86 -> 63 dependent launches for bert-base; a launch costs
// 5.3 us here whatever it does, profiles/r06_few_rows_graph_probe.json).  y_a / y_b hold the pre-LayerNorm sums in f32; the
// contraction that consumes LN(y) normalises its operand rows itself and leaves (mean, rstd) per row, the one that adds LN(y)
// re-derives the element from them (gemm_skinny.hip: a_ln32 / rln32; ln_row.h is the one definition of the arithmetic, so
// the bits are those of bert_few32 -- test_few_rows_forward_*).
static int bert_pending_ln(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  NOMIC_LOCALS;
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  float* const y_a = ws.y32;      // attention block's sum: ctx Wo^T + b + x
  float* const y_b = ws.r32b;     // feed-forward block's sum: ff W2^T + b + x1
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    float* const st1 = ws.stats1 + (size_t)l * M * 2;                          // (mean, rstd) of LN1 of this layer
    float* const st2p = l ? ws.stats2 + (size_t)(l - 1) * M * 2 : nullptr;     // ... of LN2 of the previous one
    GemmEpilogue e = {};
    e.bias = lw.qkv_b; e.ln_eps = c->ln_eps;
    if (l) { e.a_ln32 = y_b; e.a_ln_g = Ls[l - 1].ln2_g; e.a_ln_b = Ls[l - 1].ln2_b; e.a_ln_stats_out = st2p; }
    RUN(omk_gemm(dt, ws.x, H, lw.qkv_w, H, dt, ws.qkv, 3 * H, Mg, 3 * H, H, e, s));
    NOMIC_ROPE();
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, scale, 0.f, 0, s, 0, ws.kmax));
    e = GemmEpilogue{};
    e.bias = lw.o_b; e.ldr = H; e.out32 = y_a; e.ln_eps = c->ln_eps;
    if (l) { e.rln32 = y_b; e.rln32_stats = st2p; e.rln_g = Ls[l - 1].ln2_g; e.rln_b = Ls[l - 1].ln2_b; }
    else e.resid32 = ws.r32a;
    RUN(omk_gemm(dt, ws.ctx, H, lw.o_w, H, dt, ws.y, H, Mg, H, H, e, s));
    e = GemmEpilogue{};
    e.bias = lw.ffn1_b; e.act = act1; e.ln_eps = c->ln_eps;
    e.a_ln32 = y_a; e.a_ln_g = lw.ln1_g; e.a_ln_b = lw.ln1_b; e.a_ln_stats_out = st1;
    RUN(omk_gemm(dt, ws.x1, H, lw.ffn1_w, H, dt, ws.ff, F1, Mg, F1, H, e, s));
    NOMIC_SWIGLU(Mg);
    e = GemmEpilogue{};
    e.bias = lw.ffn2_b; e.ldr = H; e.out32 = y_b; e.ln_eps = c->ln_eps;
    e.rln32 = y_a; e.rln32_stats = st1; e.rln_g = lw.ln1_g; e.rln_b = lw.ln1_b;
    RUN(omk_gemm(dt, ffa, F, lw.ffn2_w, F, dt, ws.y, H, Mg, H, F, e, s));
  }
  const OmLayerWeights& last = Ls[c->n_layers - 1];
  void* dst = k.out_hidden ? k.out_hidden : (void*)ws.x;
  RUN(omk_layernorm_dual(dt, y_b, H, dst, ws.r32a, H, last.ln2_g, last.ln2_b, M, H, c->ln_eps, s));
  *out = EncStream{};
  out->hidden = (char*)dst; out->rows32 = ws.r32a;
  return 0;
}

// Few rows (a served query, a handful of sequences), 16-bit (round 6): the residual stream in f32, as the reference's autocast keeps
// it (layer_norm runs and returns fp32; a 16-bit dense output + an fp32 LayerNorm output is an fp32 sum: HF:models/bert/modeling_bert.py
// :289-293,347-351 under retriever/dense_retriever.py:76) -- what the two-plane stream is to the fused path.  Every LayerNorm writes
// its output twice (16-bit: the next contraction's operand; f32: what the next residual add reads), the residual contractions add
// the f32 copy and leave their sum in f32 (gemm_skinny.hip: resid32 / out32).  Rounds 4-5 kept one 16-bit plane here.
static int bert_few32(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  NOMIC_LOCALS;
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  void* dst = ws.x;
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    GEMM(ws.x, H, lw.qkv_w, H, ws.qkv, 3 * H, 3 * H, H, lw.qkv_b, nullptr, 0, OM_ACT_NONE);
    NOMIC_ROPE();
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, scale, 0.f, 0, s, 0, ws.kmax));
    GemmEpilogue e = {};
    e.bias = lw.o_b; e.resid32 = ws.r32a; e.ldr = H; e.out32 = ws.y32;
    RUN(omk_gemm(dt, ws.ctx, H, lw.o_w, H, dt, ws.y, H, Mg, H, H, e, s));                  // y32 = ctx Wo^T + b + x (f32)
    RUN(omk_layernorm_dual(dt, ws.y32, H, ws.x1, ws.r32b, H, lw.ln1_g, lw.ln1_b, M, H, c->ln_eps, s));
    GEMM(ws.x1, H, lw.ffn1_w, H, ws.ff, F1, F1, H, lw.ffn1_b, nullptr, 0, act1);
    NOMIC_SWIGLU(Mg);
    e = GemmEpilogue{};
    e.bias = lw.ffn2_b; e.resid32 = ws.r32b; e.ldr = H; e.out32 = ws.y32;
    RUN(omk_gemm(dt, ffa, F, lw.ffn2_w, F, dt, ws.y, H, Mg, H, F, e, s));                   // y32 = ff W2^T + b + x1 (f32)
    if (l == c->n_layers - 1 && k.out_hidden) dst = k.out_hidden;
    RUN(omk_layernorm_dual(dt, ws.y32, H, dst, ws.r32a, H, lw.ln2_g, lw.ln2_b, M, H, c->ln_eps, s));
  }
  // (the pooled rows come from the f32 copy of the last normalisation: the reference's autocast returns fp32)
  *out = EncStream{};
  out->hidden = (char*)dst; out->rows32 = ws.r32a;
  return 0;
}

// one normalisation kernel per site: float32, and the 16-bit shapes no other path takes.  The last layer's second LayerNorm is
// final_norm's; a stack of no layers leaves the embedding output as it is.
static int bert_plain(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  NOMIC_LOCALS;
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    if (l) RUN(omk_layernorm(dt, ws.y, H, ws.x, H, Ls[l - 1].ln2_g, Ls[l - 1].ln2_b, M, H, c->ln_eps, 0, s));
    GEMM(ws.x, H, lw.qkv_w, H, ws.qkv, 3 * H, 3 * H, H, lw.qkv_b, nullptr, 0, OM_ACT_NONE);
    NOMIC_ROPE();
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, scale, 0.f, 0, s, 0, ws.kmax));
    GEMM(ws.ctx, H, lw.o_w, H, ws.y, H, H, H, lw.o_b, ws.x, H, OM_ACT_NONE);
    RUN(omk_layernorm(dt, ws.y, H, ws.x1, H, lw.ln1_g, lw.ln1_b, M, H, c->ln_eps, 0, s));
    GEMM(ws.x1, H, lw.ffn1_w, H, ws.ff, F1, F1, H, lw.ffn1_b, nullptr, 0, act1);
    NOMIC_SWIGLU(Mg);
    GEMM(ffa, F, lw.ffn2_w, F, ws.y, H, H, F, lw.ffn2_b, ws.x1, H, OM_ACT_NONE);
  }
  *out = EncStream{};
  if (c->n_layers > 0) *out = EncStream{ws.y, nullptr, 0, Ls[c->n_layers - 1].ln2_g, Ls[c->n_layers - 1].ln2_b, 0, ws.x};
  else out->hidden = ws.x;
  return 0;
}

// ModernBERT (HF:models/modernbert/modeling_modernbert.py ModernBertModel.forward): the unfused pre-norm loop of t5_plain with
// LayerNorms (optional biases), no norm before layer 0's attention, rotary Q / K, a sliding window on the layers flagged in
// sliding_layers, and the GeGLU feed-forward gelu_erf(Wi[:F] x) * Wi[F:] x as two contractions over the one packed Wi.
static int modernbert(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    if (!lw.ffn1g_w) OM_FAIL("ModernBERT layers need the gate half of Wi (ffn1g_w)");
    const void* a_in = ws.x;
    if (lw.ln1_g) {                                                        // attn_norm (nn.Identity in layer 0)
      RUN(omk_layernorm(dt, ws.x, H, ws.y, H, lw.ln1_g, lw.ln1_b, M, H, c->ln_eps, 0, s));
      a_in = ws.y;
    }
    GEMM(a_in, H, lw.qkv_w, H, ws.qkv, 3 * H, 3 * H, H, lw.qkv_b, nullptr, 0, OM_ACT_NONE);
    const bool sliding = ((c->sliding_layers >> l) & 1) != 0;
    RUN(omk_rope(dt, ws.qkv, M, (int)L, H, sliding ? c->rope_theta_local : c->rope_theta_global, s));
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, nullptr, B, (int)L, H, nh, scale, 0.f, 0, s, 0, ws.kmax, nullptr, sliding ? c->half_window : 0));
    GEMM(ws.ctx, H, lw.o_w, H, ws.x, H, H, H, lw.o_b, ws.x, H, OM_ACT_NONE);        // x += Wo(ctx)
    RUN(omk_layernorm(dt, ws.x, H, ws.y, H, lw.ln2_g, lw.ln2_b, M, H, c->ln_eps, 0, s));
    GEMM(ws.y, H, lw.ffn1g_w, H, ws.ff2, F, F, H, nullptr, nullptr, 0, OM_ACT_NONE);
    GEMM(ws.y, H, lw.ffn1_w, H, ws.ff, F, F, H, lw.ffn1_b, ws.ff2, F, c->act | OM_ACT_MUL_RESID);
    GEMM(ws.ff, F, lw.ffn2_w, F, ws.x, H, H, F, lw.ffn2_b, ws.x, H, OM_ACT_NONE);    // x += Wo(mlp)
  }
  *out = EncStream{ws.x, nullptr, 0, k.w->final_ln_g, k.w->final_ln_b, 0, ws.y};      // final_norm
  return 0;
}

// RMSNorm fused across the GEMMs (16-bit, >= 512 tokens), the pre-norm counterpart of bert_fused: the GEMM that updates the
// residual stream x accumulates sum(x^2) per row; the GEMMs that consume rms(x) * g read x itself against the folded weight
// W * g and scale their rows by rsqrt(mean(x^2) + eps) in the epilogue.  Only the first and the final norm run as kernels.
static int t5_fused(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  const float inv_h = 1.0f / (float)H;
  const int nslots = 2 * (H / 256);
  auto folded = [&](int layer_, bool ffn1_, const void* A_, const void* W_, const float* g_, const float* stats_, void* C_, int N_, int act_,
                    const void* res_, int64_t ldr_) -> int {
    const void* wf; const float *cs, *bfp;
    // (the gated feed-forward's two weights are not in the caller's fold buffer -- and gated layers are not fused at all)
    if (folded_weights(c, k.w, layer_, ffn1_, W_, g_, nullptr, nullptr, N_, H, ws.wfold, ws.colsum, ws.bfold, s, &wf, &cs, &bfp)) return 1;
    (void)cs; (void)bfp;            // RMSNorm: no mean, no shift -- only the folded weight is used
    GemmEpilogue e = {};
    e.act = act_; e.resid = res_; e.ldr = ldr_;
    e.ln_stats = stats_; e.ln_rms = 1; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps; e.rows_dev = k.rows_dev;
    return omk_gemm(dt, A_, H, wf, H, dt, C_, N_, Mg, N_, H, e, s);
  };
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    float* st1 = ws.stats1 + (size_t)l * Mg * 2;                     // sum(x1^2): input of the FFN norm
    float* st2 = ws.stats2 + (size_t)l * Mg * 2;                     // sum(x'^2): input of the next layer's first norm
    if (l == 0) {
      RUN(omk_layernorm(dt, ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));
      GemmEpilogue e0 = {};            // (om_gemm_nt's plain epilogue, with the row count)
      e0.rows_dev = k.rows_dev;
      RUN(omk_gemm(dt, ws.y, H, lw.qkv_w, H, dt, ws.qkv, 3 * H, Mg, 3 * H, H, e0, s));
    } else {
      RUN(folded(l, false, ws.x, lw.qkv_w, lw.ln1_g, ws.stats2 + (size_t)(l - 1) * Mg * 2, ws.qkv, 3 * H, OM_ACT_NONE, nullptr, 0));
    }
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, 1.0f, 0.f, 0, s, 0, ws.kmax, k.cu));
    GemmEpilogue e = {};
    e.resid = ws.x; e.ldr = H; e.stats_out = ws.slots; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps; e.rows_dev = k.rows_dev;
    RUN(omk_gemm(dt, ws.ctx, H, lw.o_w, H, dt, ws.x, H, Mg, H, H, e, s));           // x += o(ctx), sum(x^2)
    RUN(omk_ln_stats_reduce(ws.slots, nslots, Mg, st1, s));
    RUN(folded(l, true, ws.x, lw.ffn1_w, lw.ln2_g, st1, ws.ff, F, c->act, nullptr, 0));      // (the plan excludes gated layers)
    e = GemmEpilogue{};
    e.resid = ws.x; e.ldr = H; e.stats_out = ws.slots; e.ln_inv_h = inv_h; e.ln_eps = c->ln_eps; e.rows_dev = k.rows_dev;
    RUN(omk_gemm(dt, ws.ff, F, lw.ffn2_w, F, dt, ws.x, H, Mg, H, F, e, s));         // x += wo(ff), sum(x^2)
    RUN(omk_ln_stats_reduce(ws.slots, nslots, Mg, st2, s));
  }
  *out = EncStream{ws.x, nullptr, 0, k.w->final_ln_g, nullptr, 1, ws.y};
  return 0;
}

static int t5_plain(const EncCall& k, EncStream* out) {
  ENC_LOCALS;
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    RUN(omk_layernorm(dt, ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));
    GEMM(ws.y, H, lw.qkv_w, H, ws.qkv, 3 * H, 3 * H, H, nullptr, nullptr, 0, OM_ACT_NONE);
    RUN(omk_attention(dt, ws.qkv, ws.ctx, k.mask, k.posbias, B, (int)L, H, nh, 1.0f, 0.f, 0, s, 0, ws.kmax));
    GEMM(ws.ctx, H, lw.o_w, H, ws.x, H, H, H, nullptr, ws.x, H, OM_ACT_NONE);  // x += o(ctx)
    RUN(omk_layernorm(dt, ws.x, H, ws.y, H, lw.ln2_g, nullptr, M, H, c->ln_eps, 1, s));
    if (lw.ffn1g_w) {
      GEMM(ws.y, H, lw.ffn1g_w, H, ws.ff2, F, F, H, nullptr, nullptr, 0, OM_ACT_NONE);
      GEMM(ws.y, H, lw.ffn1_w, H, ws.ff, F, F, H, nullptr, ws.ff2, F, c->act | OM_ACT_MUL_RESID);
    } else {
      GEMM(ws.y, H, lw.ffn1_w, H, ws.ff, F, F, H, nullptr, nullptr, 0, c->act);
    }
    GEMM(ws.ff, F, lw.ffn2_w, F, ws.x, H, H, F, nullptr, ws.x, H, OM_ACT_NONE);  // x += wo(ff)
  }
  *out = EncStream{ws.x, nullptr, 0, k.w->final_ln_g, nullptr, 1, ws.y};
  return 0;
}

// The last normalisation of every stack, stated once.  A 16-bit run normalises the rows pooling reads into f32 (the reference's
// autocast runs layer_norm in fp32 and returns fp32), into ws.final32: the B [CLS] rows for pooling "first" (already the pooled
// vectors; packed: the [CLS] row of sequence b is packed row cls_rows[b]), else all M rows.  The rows in the compute type are written
// only where someone reads them: the caller's out_hidden, a float32 run's pooling, or no pooling at all.  Hidden states AND
// representations: both normalisations run, so that encode() and forward() give the same representations.
// Leaves *hidden / *rows32 / *n32 (how many f32 rows: B, M, or 0 for none) for the pooling that follows.
static int final_norm(const EncCall& k, const EncStream& n, char** hidden, const float** rows32, int64_t* n32) {
  const OmEncoderConfig* c = k.c; const EncWs& ws = k.ws; hipStream_t s = k.s;
  const int dt = c->dtype, H = c->hidden;
  const int64_t B = k.B, L = k.L, M = k.p.M;
  const bool pooled32 = dt != OM_F32 && c->pooling != OM_POOL_NONE;
  *hidden = n.hidden; *rows32 = ws.final32; *n32 = 0;
  if (!n.x) {
    if (n.rows32 && c->pooling != OM_POOL_NONE) { *rows32 = n.rows32; *n32 = M; }
    return 0;
  }
  if (k.out_hidden || !pooled32) {
    void* dst = k.out_hidden ? k.out_hidden : n.spare;
    RUN(omk_layernorm(dt, n.x, H, dst, H, n.g, n.b, M, H, c->ln_eps, n.rms, s, n.x_lo, n.lo8));
    *hidden = (char*)dst;
  }
  if (pooled32 && c->pooling == OM_POOL_FIRST) {
    const int* rows = k.cu && !n.cls_compact ? ws.cls_rows : nullptr;
    RUN(omk_layernorm_f32out(dt, n.x, rows || n.cls_compact ? H : L * H, ws.final32, H, n.g, n.b, B, H, c->ln_eps, n.rms, s, n.x_lo, rows, n.lo8));
    *n32 = B;
  } else if (pooled32) {
    RUN(omk_layernorm_f32out(dt, n.x, H, ws.final32, H, n.g, n.b, M, H, c->ln_eps, n.rms, s, n.x_lo, nullptr, n.lo8));
    *n32 = M;
  }
  return 0;
}

// pooled rows [B, H] f32 -> out_reps: the optional head contraction, l2norm, and for packed rows (cu != NULL) the overflow poison
// (a bound below the token count: NaN, never a truncated batch).  Without a head, `pooled` is out_reps itself.
int omk_pooled_tail(const OmEncoderConfig* c, const OmEncoderWeights* w, const float* pooled, float* out_reps, int64_t B, const int* cu,
                    int64_t packed_rows, hipStream_t s) {
  int D = c->hidden;
  if (c->head_in > 0 && w->head_w) {
    D = c->head_out;
    RUN(om_gemm_nt(OM_F32, pooled, c->hidden, w->head_w, c->head_in, OM_F32, out_reps, D, B, D, c->head_in, nullptr, nullptr, 0, OM_ACT_NONE, s));
  }
  if (c->normalize) RUN(omk_l2norm(out_reps, out_reps, B, D, s));
  if (cu) RUN(omk_pack_overflow_poison(cu, B, packed_rows, out_reps, B * (int64_t)D, s));
  return 0;
}

// Pad rows skipped on the device (encoder_plan.h encoder_skip_pad): cu [B + 2] | cls_rows [B] | row_map [rows] of such a call.  They cannot
// come from the caller's workspace -- om_encoder_workspace_bytes of a padded call is what it was -- so the library keeps one buffer
// per (device, stream): calls on a stream are stream-ordered, so reusing it is safe; two streams get two buffers.  Grow-only and kept
// for the life of the process, like the library's other device caches (om_t5_lut_device); growing waits for the device before it
// frees.  A buffer that a capturing stream was handed is never freed (a captured graph replays its address): it is retired.
// *out stays NULL -- the call then runs over all its rows -- when the buffer would have to be created or grown while `s` is capturing.
// Limits (include/openmatch_hip.h states them for the caller): entries are never pruned, so a process keeps one buffer per distinct
// stream handle it ever encoded on; growing synchronises the device and allocates, which invalidates a capture another thread has
// open in global mode on another stream; a retired or captured buffer is shared by the graph's replays and later eager calls on that
// stream, which is stream-ordered only if the graph is replayed on the stream it was captured on.
static int skip_pad_buffer(hipStream_t s, size_t ints, int** out) {
  struct Buf { int* p = nullptr; size_t n = 0; bool captured = false; };
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, Buf> bufs;
  *out = nullptr;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {      // (cannot tell: as if capturing with nothing to hand out)
    (void)hipGetLastError();
    return 0;
  }
  const bool capturing = st != hipStreamCaptureStatusNone;
  std::lock_guard<std::mutex> lk(mu);
  Buf& b = bufs[std::make_pair(dev, s)];
  if (b.n < ints) {
    if (capturing) return 0;
    if (b.p && !b.captured) { OM_HIP(hipDeviceSynchronize()); OM_HIP(hipFree(b.p)); }
    b = Buf{};
    OM_HIP(hipMalloc(&b.p, ints * sizeof(int)));
    b.n = ints;
  }
  b.captured |= capturing;
  *out = b.p;
  return 0;
}

// One chain of launches on one stream: the whole call, or one lane of it (encoder_fork below).  `in` / `plan` are the CHAIN's own -- a
// lane is planned as the call (B_h, L) it is -- and `ws` is its view of the workspace.
struct EncChain {
  const OmEncoderConfig* c;
  const OmEncoderWeights* w;
  const int64_t *input_ids, *attention_mask, *token_type_ids;
  void* out_hidden;
  float* out_reps;
  EncPlanIn in;
  EncPlan plan;
  EncSwitches sw;
  EncWs ws;
  hipStream_t s;
  int* side;      // encoder_skip_pad holds and skip_pad_buffer(s) had a buffer: cu | cls_rows | row_map of the chain; else NULL
  int64_t whole_mg, whole_mc;      // a lane: EncCall's fields of these names; the whole call: 0
};

// Two views of one workspace (encoder_plan.h encoder_lanes): lane 0 takes token rows [0, B0 * L) and sequences [0, B0) of every buffer
// of the whole call's carve, lane 1 the rest -- B0 * L is in whole tiles, so lane 1's height Mp - B0 * L is roundup256((B - B0) * L),
// what a call of its own would carve.  The statistics and slot arrays are indexed with the chain's own Mg as pitch (bert_fused), so
// each is split into two contiguous blocks sized by the lanes' heights.  Nothing is carved twice: om_encoder_workspace_bytes is what it
// was.  What a lane never touches is NULL in its view: the fold scratch (w->folded is given), the bias table, the f32 stream, and the
// three packed-row arrays (a lane that skips its pad rows has them in the side buffer of its own stream).
static EncWs lane_view(const OmEncoderConfig* c, const EncWs& w, const EncPlan& lane, int h, int64_t B0, int64_t L) {
  const size_t H = c->hidden, F = c->ffn, F1 = enc_ffn1_cols(c), es = 2;
  const size_t row0 = h ? (size_t)(B0 * L) : 0, seq0 = h ? (size_t)B0 : 0;
  EncWs v = {};
  v.x = w.x + row0 * H * es; v.y = w.y + row0 * H * es; v.x1 = w.x1 + row0 * H * es;
  v.qkv = w.qkv + row0 * 3 * H * es;
  v.ctx = w.ctx + row0 * H * es;
  v.ff = w.ff + row0 * F1 * es;
  v.ff2 = c->arch == OM_ARCH_NOMICBERT ? w.ff2 + row0 * F * es : w.ff2;
  v.y_lo = w.y_lo + row0 * H * es; v.x1_lo = w.x1_lo + row0 * H * es;
  v.pooled = w.pooled + seq0 * H;
  v.headout = w.headout + seq0 * (size_t)(c->head_out > 0 ? c->head_out : 1);
  v.kmax = w.kmax + seq0;
  v.final32 = w.final32 + (c->pooling == OM_POOL_FIRST ? seq0 : row0) * H;
  v.stats1 = w.stats1 + 4 * (size_t)c->n_layers * row0;
  v.stats2 = v.stats1 + (size_t)c->n_layers * (size_t)lane.Mg * 2;
  v.slots = w.slots + 4 * ((H + 255) / 256) * row0;
  v.total = w.total;
  return v;
}

// (offset, bytes) of every field of a lane's view, in the order include/openmatch_hip.h documents (om_debug_encoder_lane_ranges)
static void lane_ranges(const OmEncoderConfig* c, const EncWs& v, const EncPlan& lane, int64_t Bh, const char* base, int64_t* out) {
  const size_t H = c->hidden, F = c->ffn, F1 = enc_ffn1_cols(c), es = 2, M = (size_t)lane.Mp, B = (size_t)Bh;
  const bool nomic = c->arch == OM_ARCH_NOMICBERT;
  const std::pair<const void*, size_t> f[OM_ENCODER_LANE_RANGES] = {
      {v.x, M * H * es}, {v.y, M * H * es}, {v.x1, M * H * es}, {v.qkv, M * 3 * H * es}, {v.ctx, M * H * es}, {v.ff, M * F1 * es},
      {v.ff2, nomic ? M * F * es : 0}, {v.pooled, B * H * 4}, {v.headout, B * (size_t)(c->head_out > 0 ? c->head_out : 1) * 4}, {v.kmax, B * 4},
      {v.final32, (c->pooling == OM_POOL_FIRST ? B : (size_t)lane.M) * H * 4}, {v.stats1, (size_t)2 * c->n_layers * M * 8},
      {v.slots, (size_t)2 * ((H + 255) / 256) * M * 8}, {v.y_lo, M * H * es}, {v.x1_lo, M * H * es}};
  for (int i = 0; i < OM_ENCODER_LANE_RANGES; ++i) {
    out[2 * i] = (int64_t)((const char*)f[i].first - base);
    out[2 * i + 1] = (int64_t)f[i].second;
  }
}

// host only: the lanes rule at the current switches (include/openmatch_hip.h)
extern "C" int om_debug_encoder_lanes(const OmEncoderConfig* c, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                                      int want_hidden, int64_t* B0) {
  if (!c) {
    om_set_error("om_debug_encoder_lanes: null argument");
    return -1;
  }
  const EncPlanIn in = {c, B, L, packed_rows, want_hidden != 0, gated_ffn != 0, has_rel_bias != 0, c->type_vocab > 0};
  const EncSwitches sw = encoder_switches();
  return encoder_lanes(in, encoder_plan(in, sw), sw, B0) ? 1 : 0;
}

// host only: where lane `lane` of the call (B, L) lives in the call's workspace (include/openmatch_hip.h)
extern "C" int om_debug_encoder_lane_ranges(const OmEncoderConfig* c, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int lane,
                                            int64_t* out, int cap) {
  if (!c || !out || cap < 2 * OM_ENCODER_LANE_RANGES || (lane != 0 && lane != 1)) {
    om_set_error("om_debug_encoder_lane_ranges: null argument, a lane other than 0 | 1, or room for fewer than 15 pairs");
    return -1;
  }
  EncPlanIn in = {c, B, L, 0, false, gated_ffn != 0, has_rel_bias != 0, c->type_vocab > 0};
  const EncSwitches sw = encoder_switches();
  const EncPlan whole = encoder_plan(in, sw);
  int64_t B0 = 0;
  if (!encoder_lanes(in, whole, sw, &B0)) {
    om_set_error("om_debug_encoder_lane_ranges: this call does not fork (om_debug_encoder_lanes)");
    return -1;
  }
  static char origin[1];      // (offsets are differences of addresses: any base will do)
  const EncWs ws = carve(c, whole, B, L, 0, origin);
  in.B = lane ? B - B0 : B0;
  const EncPlan lp = encoder_plan_checked(in, sw);
  lane_ranges(c, lane_view(c, ws, lp, lane, B0, L), lp, in.B, origin, out);
  return OM_ENCODER_LANE_RANGES;
}

static std::atomic<int64_t> g_lane_forks{0};
extern "C" int64_t om_debug_encoder_lane_forks(void) { return g_lane_forks.load(); }

// The stream lane 1 runs on and the two events of the fork and the join: one per (device, caller stream), created on first use, kept
// for the life of the process like skip_pad_buffer's entries (train.hip's WgradLane is the precedent).  Non-blocking: torch's default
// stream is the null stream, and a blocking stream would serialise against it.
struct LaneStream { hipStream_t side = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
static int lane_stream(hipStream_t s, LaneStream* out) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, LaneStream> lanes;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  LaneStream& l = lanes[std::make_pair(dev, s)];
  if (!l.side) {
    LaneStream n;
    OM_HIP(hipStreamCreateWithFlags(&n.side, hipStreamNonBlocking));
    OM_HIP(hipEventCreateWithFlags(&n.fork, hipEventDisableTiming));
    OM_HIP(hipEventCreateWithFlags(&n.join, hipEventDisableTiming));
    l = n;
  }
  *out = l;
  return 0;
}

static int encoder_chain(const EncChain& q, std::vector<int>* families);

// A padded call as two lanes (encoder_plan.h encoder_lanes).  *forked = 0 and nothing enqueued: the caller runs the one
// chain it always ran -- a no is never an error.  Beyond the rule, decided here with host checks alone:
//   - w->folded: without it every lane would fold into the one workspace scratch;
//   - the stream is not capturing: a captured graph stays one linear chain;
//   - not in timing mode: hipEvents around co-running kernels price nothing, so the roofline pass keeps measuring one stream;
//   - every contraction of the layer loop (and the head's) plans the same GEMM family at each lane's height as at the whole's, asked
//     with the pointers and epilogues the launches carry (bert_fused under EncCall::families).  Within a family a row's bits do not
//     depend on the rows beside it; across families they may.  The one place where the family moves with M is the tile-choice model
//     of gemm_plan.h rule 5 (the first layer's plain QKV at small shapes), so a lane's contractions are priced at the WHOLE's height
//     (EncCall::whole_mg / whole_mc -> omk_gemm's plan_m): the lanes then run the kernels the whole call would, and this check is what
//     proves it call by call instead of assuming it.
// After the fork the join is made whatever the lanes return, so the caller's stream is never left unordered against the side stream.
static int encoder_fork(const EncChain& whole, int* forked) {
  *forked = 0;
  const OmEncoderConfig* c = whole.c;
  const int64_t B = whole.in.B, L = whole.in.L;
  int64_t B0 = 0;
  if (!whole.w->folded || om_timing_on() || !encoder_lanes(whole.in, whole.plan, whole.sw, &B0)) return 0;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(whole.s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (st != hipStreamCaptureStatusNone) return 0;
  LaneStream ls;
  RUN(lane_stream(whole.s, &ls));
  const bool skip = encoder_skip_pad(whole.in, whole.plan, whole.sw);
  int64_t whole_mc = 0;
  if (!encoder_cls_tail(whole.in, whole.plan, whole.sw, &whole_mc)) whole_mc = 0;
  const int64_t D =c->head_in > 0 && whole.w->head_w ? c->head_out : c->hidden;
  EncChain lane[2] = {whole, whole};
  for (int h = 0; h < 2; ++h) {
    EncChain& q = lane[h];
    const int64_t seq0 = h ? B0 : 0;
    q.in.B = h ? B - B0 : B0;
    q.plan = encoder_plan_checked(q.in, q.sw);
    q.ws = lane_view(c, whole.ws, q.plan, h, B0, L);
    q.input_ids += seq0 * L; q.attention_mask += seq0 * L;
    if (q.token_type_ids) q.token_type_ids += seq0 * L;
    q.out_reps += seq0 * D;
    if (h) q.s = ls.side;
    q.whole_mg = whole.plan.Mg; q.whole_mc = whole_mc;
    q.side = nullptr;
    if (skip) {
      RUN(skip_pad_buffer(q.s, (size_t)(q.plan.Mp + 2 * q.in.B + 2), &q.side));
      if (!q.side) return 0;
    }
  }
  if (lane[0].plan.Mp != B0 * L || lane[0].plan.Mp + lane[1].plan.Mp != whole.plan.Mp) return 0;      // (the rule's B0: cannot happen)
  EncChain ask = whole;
  ask.side = lane[0].side;      // any address: the planner tests it for null only
  std::vector<int> fam_whole, fam_lane[2];
  if (encoder_chain(ask, &fam_whole) || encoder_chain(lane[0], &fam_lane[0]) || encoder_chain(lane[1], &fam_lane[1])) return 0;
  if (fam_lane[0] != fam_whole || fam_lane[1] != fam_whole || std::find_if(fam_whole.begin(), fam_whole.end(), [](int f) { return f <= 0; }) != fam_whole.end())
    return 0;

  OM_HIP(hipEventRecord(ls.fork, whole.s));
  OM_HIP(hipStreamWaitEvent(ls.side, ls.fork, 0));
  *forked = 1;
  g_lane_forks.fetch_add(1);
  // lane 0 first: the head start its host enqueue order gives keeps the two chains out of phase
  int rc = encoder_chain(lane[0], nullptr);
  if (!rc) rc = encoder_chain(lane[1], nullptr);
  hipError_t e = hipEventRecord(ls.join, ls.side);
  if (e == hipSuccess) e = hipStreamWaitEvent(whole.s, ls.join, 0);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ls.side);      // no event to wait on: order the caller's stream by waiting here
    if (!rc) OM_FAIL(std::string("encoder lanes: join failed: ") + hipGetErrorString(e));
  }
  return rc;
}

// plan, carve, then the call's chain -- or its two lanes
static int encoder_forward_impl(const OmEncoderConfig* c, const OmEncoderWeights* w,
                                const int64_t* input_ids, const int64_t* attention_mask,
                                const int64_t* token_type_ids, int64_t B, int64_t L,
                                void* out_hidden, float* out_reps, void* workspace,
                                size_t workspace_bytes, void* stream, int64_t packed_rows) {
  if (!c || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(c)) return 1;
  if (B <= 0) return 0;
  const OmLayerWeights* Ls = w->layers_host;
  if (!Ls) OM_FAIL("layers_host is null");
  const EncPlanIn plan_in = {c, B, L, packed_rows, out_hidden != nullptr, c->n_layers > 0 && Ls[0].ffn1g_w != nullptr, w->rel_bias != nullptr,
                             w->type_emb != nullptr};
  const EncSwitches sw = encoder_switches();
  const EncPlan plan = encoder_plan_checked(plan_in, sw);
  if (om_option(OM_OPT_ENCODER_DEBUG) && plan.path && enc_bert_family(c))
    fprintf(stderr, "om_encoder_forward: M=%ld fused_ln=%d packed=%d few_rows=%d pending_ln=%d L=%ld head_dim=%d rel_bias=%d\n", (long)plan.M,
            (int)(plan.path == OM_ENC_PATH_BERT_FUSED), (int)(packed_rows > 0), (int)plan.few_rows, (int)(plan.path == OM_ENC_PATH_BERT_PENDING_LN), (long)L,
            c->head_dim, (int)plan.rel_bias);
  if (om_option(OM_OPT_ENCODER_DEBUG) && plan.path && c->arch == OM_ARCH_T5)
    fprintf(stderr, "om_encoder_forward (t5): M=%ld fused_norm=%d packed=%d\n", (long)plan.M, (int)(plan.path == OM_ENC_PATH_T5_FUSED), (int)(packed_rows > 0));
  if (plan.error) OM_FAIL(plan.error);
  if (c->arch == OM_ARCH_T5 && !w->final_ln_g) OM_FAIL("T5 needs rel_bias and final_ln_g");
  if (c->arch == OM_ARCH_MODERNBERT && (!w->emb_ln_g || !w->final_ln_g)) OM_FAIL("ModernBERT needs emb_ln_g and final_ln_g");
  if (c->arch == OM_ARCH_NOMICBERT && (!w->type_emb || w->pos_emb || w->rel_bias)) OM_FAIL("NomicBERT needs type_emb and takes no pos_emb or rel_bias");
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  EncChain whole = {c, w, input_ids, attention_mask, token_type_ids, out_hidden, out_reps, plan_in, plan, sw,
                    carve(c, plan, B, L, packed_rows, (char*)workspace), (hipStream_t)stream, nullptr, 0, 0};
  if (whole.ws.total > workspace_bytes) OM_FAIL("workspace too small");
  if (c->pooling != OM_POOL_NONE && !out_reps) OM_FAIL("out_reps required when pooling is set");
  int forked = 0;
  RUN(encoder_fork(whole, &forked));
  if (forked) return 0;
  if (encoder_skip_pad(plan_in, plan, sw)) RUN(skip_pad_buffer(whole.s, (size_t)(plan.Mp + 2 * B + 2), &whole.side));
  return encoder_chain(whole, nullptr);
}

// the chain's layer loop, the last normalisation, pooling.  families: launch nothing, answer which GEMM family each contraction of the
// fused BERT loop and the head would plan (encoder_fork)
static int encoder_chain(const EncChain& q, std::vector<int>* families) {
  const OmEncoderConfig* c = q.c; const OmEncoderWeights* w = q.w;
  const int64_t *input_ids = q.input_ids, *attention_mask = q.attention_mask, *token_type_ids = q.token_type_ids;
  void* const out_hidden = q.out_hidden; float* const out_reps = q.out_reps;
  const EncPlanIn& plan_in = q.in; const EncPlan& plan = q.plan; const EncSwitches sw = q.sw;
  const int64_t B = q.in.B, L = q.in.L, packed_rows = q.in.packed_rows;
  const bool bert = enc_bert_family(c);
  EncWs ws = q.ws;
  hipStream_t s = q.s;
  const int dt = c->dtype, H = c->hidden;
  const int64_t M = plan.M;
  // A padded call that skips its pad rows (encoder_skip_pad) IS the packed call with the bound roundup256(B * L) from here on -- the
  // same plan but for its row counts, which stay the padded call's (M = B * L <= the bound: every token has a row below M, so the
  // per-row kernels need no more; Mp = Mg = the bound, the height of the workspace's buffers) -- with its three arrays in the
  // library's side buffer, and the contractions stop at the token count the packing launch leaves in cu[B].
  int64_t pack_bound = packed_rows;
  const bool skip = q.side != nullptr;
  if (skip) {
    pack_bound = plan.Mp;
    ws.cu = q.side; ws.cls_rows = q.side + (B + 2); ws.row_map = ws.cls_rows + B;
  }
  const bool packed = pack_bound > 0;      // the token axis holds packed rows
  int64_t cls_mc = 0;                      // the last layer's per-row tail over the [CLS] rows alone (encoder_plan.h encoder_cls_tail)
  if (!encoder_cls_tail(plan_in, plan, sw, &cls_mc)) cls_mc = 0;
  const int* const row_map = packed ? ws.row_map : nullptr;
  if (families) {
    if (plan.path != OM_ENC_PATH_BERT_FUSED) OM_FAIL("encoder lanes: the fused BERT path only");
    const EncCall k = {c, w, attention_mask, B, L, plan, ws, nullptr, packed ? ws.cu : nullptr, row_map, out_hidden, s, skip ? ws.cu + B : nullptr,
                       cls_mc, families, q.whole_mg, q.whole_mc};
    EncStream unused = {};
    RUN(bert_fused(k, &unused));
    if (c->head_in > 0 && w->head_w)      // omk_pooled_tail's contraction
      families->push_back(omk_gemm_family(OM_F32, ws.pooled, c->hidden, w->head_w, c->head_in, OM_F32, out_reps, c->head_out, B, c->head_out,
                                          c->head_in, GemmEpilogue{}));
    return 0;
  }

  RUN(omk_mask_extent(attention_mask, B, (int)L, ws.kmax, s));
  if (packed) RUN(omk_pack_rows(ws.kmax, B, (int)L, pack_bound, ws.cu, ws.cls_rows, ws.row_map, s));
  // Relative-position bias (T5; MPNet): one bucket table for all layers, expanded once per forward to [heads, L, L] and handed to EVERY
  // attention launch (BERT family: next to the BERT scale, the kernels scale q.k only)
  if (plan.rel_bias) {
    const int* lut = nullptr;                    // device-resident, cached per (L, buckets, max distance): no copy, no sync
    RUN(om_t5_lut_device((int)L, c->rel_buckets, c->rel_max_dist, &lut));
    RUN(omk_t5_bias(w->rel_bias, lut, ws.posbias, (int)L, c->n_heads, s));
  }
  // (the two f32-stream paths: the embedding leaves its LayerNorm output in both forms)
  const bool few32 = plan.path == OM_ENC_PATH_BERT_FEW32 || plan.path == OM_ENC_PATH_BERT_PENDING_LN;
  if (bert)
    RUN(omk_embed(dt, input_ids, token_type_ids, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_g, w->emb_ln_b, ws.x, M, (int)L, H,
                  c->vocab, c->type_vocab, c->ln_eps, 1, s, row_map, few32 ? ws.r32a : nullptr));
  else if (c->arch == OM_ARCH_MODERNBERT)
    RUN(omk_embed(dt, input_ids, nullptr, w->word_emb, nullptr, nullptr, w->emb_ln_g, w->emb_ln_b, ws.x, M, (int)L, H, c->vocab, 1, c->ln_eps, 1, s));
  else
    RUN(omk_embed(dt, input_ids, nullptr, w->word_emb, nullptr, nullptr, nullptr, nullptr, ws.x, M, (int)L, H, c->vocab, 1, c->ln_eps, 0, s, row_map));

  const EncCall k = {c, w, attention_mask, B, L, plan, ws, plan.rel_bias ? ws.posbias : nullptr, packed ? ws.cu : nullptr, row_map, out_hidden, s,
                     skip ? ws.cu + B : nullptr, cls_mc, nullptr, q.whole_mg, q.whole_mc};
  EncStream stream_out = {};
  switch (plan.path) {
    case OM_ENC_PATH_BERT_FUSED: RUN(bert_fused(k, &stream_out)); break;
    case OM_ENC_PATH_BERT_PENDING_LN: RUN(bert_pending_ln(k, &stream_out)); break;
    case OM_ENC_PATH_BERT_FEW32: RUN(bert_few32(k, &stream_out)); break;
    case OM_ENC_PATH_BERT_PLAIN: RUN(bert_plain(k, &stream_out)); break;
    case OM_ENC_PATH_MODERNBERT: RUN(modernbert(k, &stream_out)); break;
    case OM_ENC_PATH_T5_FUSED: RUN(t5_fused(k, &stream_out)); break;
    case OM_ENC_PATH_T5_PLAIN: RUN(t5_plain(k, &stream_out)); break;
    default: OM_FAIL("no path planned");
  }
  char* final_hidden;
  const float* f32_rows;       // the f32 rows of the last normalisation (the few-rows paths leave them in their f32 residual buffer)
  int64_t final32_rows;
  RUN(final_norm(k, stream_out, &final_hidden, &f32_rows, &final32_rows));

  if (c->pooling != OM_POOL_NONE) {
    float* pooled = c->head_in > 0 && w->head_w ? ws.pooled : out_reps;
    if (final32_rows == B && c->pooling == OM_POOL_FIRST && (f32_rows == ws.final32 || L == 1))
      OM_HIP(hipMemcpyAsync(pooled, f32_rows, (size_t)B * H * 4, hipMemcpyDeviceToDevice, s));
    else if (final32_rows == M)
      RUN(omk_pool(OM_F32, f32_rows, attention_mask, pooled, B, (int)L, H, c->pooling, s, k.cu));
    else
      RUN(omk_pool(dt, final_hidden, attention_mask, pooled, B, (int)L, H, c->pooling, s));
    RUN(omk_pooled_tail(c, w, pooled, out_reps, B, k.cu, pack_bound, s));
  }
  return 0;
}
#undef NOMIC_SWIGLU
#undef NOMIC_ROPE
#undef NOMIC_LOCALS
#undef ENC_LOCALS
#undef GEMM
#undef RUN

extern "C" int om_encoder_forward(const OmEncoderConfig* c, const OmEncoderWeights* w,
                                  const int64_t* input_ids, const int64_t* attention_mask,
                                  const int64_t* token_type_ids, int64_t B, int64_t L,
                                  void* out_hidden, float* out_reps, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return encoder_forward_impl(c, w, input_ids, attention_mask, token_type_ids, B, L, out_hidden, out_reps, workspace, workspace_bytes, stream, 0);
}

extern "C" int om_encoder_forward_packed(const OmEncoderConfig* c, const OmEncoderWeights* w,
                                         const int64_t* input_ids, const int64_t* attention_mask,
                                         const int64_t* token_type_ids, int64_t B, int64_t L, int64_t packed_rows,
                                         float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  return encoder_forward_impl(c, w, input_ids, attention_mask, token_type_ids, B, L, nullptr, out_reps, workspace, workspace_bytes, stream, packed_rows);
}
