// What a training step runs: train_plan() maps (configuration, batch shape, forward or backward, what the caller wants back, whether a
// bias table is given, the flags the tape was written with, switches) to a TrainPlan and does nothing else -- no launch, no HIP call,
// no global read or written, no pointer dereferenced but the configuration's.  train_forward_impl / train_backward_impl (train.hip)
// carve the tape and the workspace by the plan and launch what it names; the four *_bytes entries and
// om_encoder_train_packed_supported ask it; om_debug_train_plan returns it alone, so the table is testable on a machine without a GPU.
// DESIGN.md 4g lists the rules in the order they are tested here.
//
// Kept as they were when the rules were collected here (each is pinned by tests/test_train_plan.py; none is fixed here):
//   - the weight-gradient lane turns on for ANY non-zero OM_OPT_TRAIN_WGRAD_STREAM word, not for bit 0 alone (2, 4 and 8 turn it on too);
//   - x32a / x32b are reserved for every bert16 shape, whatever OM_OPT_TRAIN_RES32 says;
//   - the keep slices are reserved whatever OM_OPT_TRAIN_WGRAD_BATCH says;
//   - the tape-flag map is written by the BERT forward only: a T5 backward takes whatever flags its tape address last had, and flags
//     given to a backward are taken as they are (res32 without bert16 is possible; nothing of a T5 step reads either flag);
//   - the forward's and the backward's packed-rows refusals have different texts;
//   - train_packed_ok is deliberately stricter than attn_plan.h (float16 packs with OM_OPT_ATTENTION_FAST on only; nothing beyond 256 tokens);
//   - the forward takes the f32 tail for pooling "first" in every 16-bit run with layers, the backward for bert16 alone;
//   - a backward may reuse the forward's transposes under bit 1 of the lane word alone: the forward's other conditions (16 bits, layers)
//     are in what the lane remembers of that forward (train.hip WgradLane::wt_*).
// Bit 3 of OM_OPT_TRAIN_WGRAD_STREAM is not read here: the LayerNorm-backward row kernel's own plan reads it (row_plan.h: row_switches).
#pragma once
#include <algorithm>

#include "gemm_tn_plan.h"

struct TrainSwitches {
  int res32;           // OM_OPT_TRAIN_RES32: a 16-bit BERT forward keeps its residual stream in f32
  int tape_grad;       // OM_OPT_TRAIN_TAPE_GRAD: a 16-bit forward keeps gelu'(f) on the tape in place of f
  int wgrad_stream;    // OM_OPT_TRAIN_WGRAD_STREAM, the whole word: non-zero: the lane; bit 1: early transposes; bit 2: LayerNorm atomics
  int wgrad_batch;     // OM_OPT_TRAIN_WGRAD_BATCH: layers per deferred weight-gradient launch
  int attention_fast;  // OM_OPT_ATTENTION_FAST: read by train_packed_ok only (attn_plan.h decides the attention kernels itself)
};

// every switch the training chain consults, read once per call
static TrainSwitches train_switches() {
  return TrainSwitches{om_option(OM_OPT_TRAIN_RES32), om_option(OM_OPT_TRAIN_TAPE_GRAD), om_option(OM_OPT_TRAIN_WGRAD_STREAM),
                       om_option(OM_OPT_TRAIN_WGRAD_BATCH), om_option(OM_OPT_ATTENTION_FAST)};
}

struct TrainPlanIn {
  const OmEncoderConfig* c;
  int64_t B, L, packed_rows;      // packed_rows > 0: the _packed entries
  bool want_hidden;               // out_hidden / d_hidden is given
  bool has_rel_bias;              // OmEncoderWeights::rel_bias is given
  bool backward;
  int tape_flags;                 // -1: from the switches (a forward; a backward whose tape is not in the map); >= 0: as the tape was written
};

// what a 16-bit BERT tape holds (fixed by the FORWARD, remembered per tape: train.hip tape_flags_set)
constexpr int TAPE_RES32 = 1, TAPE_PRE_GRAD = 2;
// TrainPlan::tail: how the pooled rows are made (forward) / where their gradient goes (backward)
constexpr int TRAIN_TAIL_NONE = 0;        // the hidden states are handed out / their gradient handed in
constexpr int TRAIN_TAIL_PLAIN = 1;       // pooling over the final hidden state in the compute format
constexpr int TRAIN_TAIL_F32_CLS = 2;     // an f32 evaluation of the last LayerNorm over the [CLS] rows
constexpr int TRAIN_TAIL_F32_MEAN = 3;    // ... over every row, pooled in f32

struct TrainPlan {
  const char* error;      // the first failing rule's text; nothing is launched
  int rule;               // ... and its number below: the impl functions keep their pointer checks between rule 4's refusal and the later ones
  bool empty;             // B <= 0: nothing runs, nothing is refused
  int64_t M, Mp, B, L;    // token rows (packed_rows, or B * L), M in whole 64-row steps
  int H, F, nl, nh, D;
  size_t es;              // bytes per element of the compute format
  bool t5, gated;
  bool rel;               // a BERT-family stack with a relative-position bias table (MPNet: OmEncoderConfig::rel_buckets > 0)
  bool packed;            // M = the caller's row bound; sequence b lives in rows cu[b] .. cu[b + 1] - 1 of every [M, .] tensor
  bool bert16;            // 16-bit BERT with ffn >= 2 * hidden: the configurations res32 applies to
  bool res32;             // the pre-LayerNorm sums y1 / y2 are f32 on the tape
  bool pre_grad;          // the tape holds gelu'(f) in place of f
  int tail;               // TRAIN_TAIL_*
  bool keep;              // the workspace reserves a keep slice per layer (deferred weight gradients)
  bool early_wt;          // forward: transpose the weights on the side stream; backward: such transposes may be reused
  bool lane;              // backward: the weight gradients run on the side stream
  int wbatch;             // backward: layers per deferred, batched weight-gradient launch (0: one launch per site)
  bool ln_atomics;        // backward: the LayerNorm parameter sums by atomics (A/B)
};

inline int train_tape_flags(const TrainPlan& p) { return (p.res32 ? TAPE_RES32 : 0) | (p.pre_grad ? TAPE_PRE_GRAD : 0); }

// rule 1: the configuration and the sequence length alone
static const char* train_cfg_error(const OmEncoderConfig* c, int64_t L) {
  if (c->arch != OM_ARCH_BERT && c->arch != OM_ARCH_T5) return "unknown arch";
  if (c->dtype != OM_F32 && c->dtype != OM_BF16 && c->dtype != OM_F16) return "dtype must be OM_F32, OM_BF16 or OM_F16";
  // float16 training (the reference's --fp16 = torch.cuda.amp float16 + GradScaler for every backbone): BERT-family since round 5, T5 stacks
  // since round 6 (ReLU / gated tanh-GELU feed-forwards; as under the reference's autocast nothing clamps -- a checkpoint whose feed-forward
  // activations leave the float16 range overflows there and here alike, the loss scaler skips such steps)
  if (c->arch == OM_ARCH_T5 && (c->head_dim != 64 || c->n_heads * 64 != c->hidden)) return "T5 training: only d_kv 64 with n_heads*64 == d_model";
  if ((c->head_dim != 32 && c->head_dim != 64) || c->n_heads * c->head_dim != c->hidden) return "head_dim must be 32 or 64 with n_heads*head_dim == hidden";
  if (L < 1 || L > 512) return "training supports sequence lengths up to 512";      // (257 .. 512: round 6, the tile-at-a-time attention kernels)
  // 32-wide heads (attention_d32.hip): one backward kernel with a whole score row in registers, every format
  if (c->head_dim == 32 && L > 256) return "training with head_dim 32 supports sequence lengths up to 256";
  if (c->dtype == OM_F32 && L > 192 && c->head_dim != 32) return "float32 training supports sequence lengths up to 192 (16-bit formats: 512)";
  if (c->arch == OM_ARCH_BERT && c->act != OM_ACT_GELU_ERF) return "BERT training supports the erf-GELU FFN";
  if (c->arch == OM_ARCH_T5 && (c->act & 0xff) != OM_ACT_RELU && (c->act & 0xff) != OM_ACT_GELU_TANH)
    return "T5 training supports relu and gated gelu_new feed-forward layers";
  const int es = c->dtype == OM_F32 ? 4 : 2;
  if ((c->hidden * es) % 128 || (c->ffn * es) % 128) return "hidden/ffn rows must be multiples of 128 bytes";
  if (c->pooling != OM_POOL_FIRST && c->pooling != OM_POOL_MEAN) return "pooling must be first or mean";
  return nullptr;
}

// om_encoder_train_packed_supported at given switches.  Packed rows in training (round 5): the contractions, normalisations and the
// tape run over `packed_rows` rows -- the tokens up to each sequence's last unmasked one, back to back -- instead of B * L (the
// reference pads every sequence of a batch to one length, dataset/data_collator.py:13-24, and computes over the padding).  16-bit
// BERT-family and (round 6) T5 configurations with widths of 256, L <= 256, packed_rows a multiple of 256 that is >= the token count
// (a bound that is too small turns the representations into NaN).
static bool train_packed_ok(const OmEncoderConfig* c, int64_t B, int64_t L, int64_t packed_rows, const TrainSwitches sw) {
  if (!c || B <= 0 || L <= 0 || packed_rows <= 0) return false;
  if ((c->arch != OM_ARCH_BERT && c->arch != OM_ARCH_T5) || (c->dtype != OM_BF16 && c->dtype != OM_F16) || c->n_layers <= 0) return false;      // (T5: round 6)
  if (packed_rows % 256 || packed_rows < 512 || packed_rows > B * L + 255 || packed_rows >= B * L) return false;
  if (c->hidden % 256 || c->ffn % 256 || (c->n_heads * 64 != c->hidden && c->n_heads * 32 != c->hidden)) return false;
  if (c->pooling != OM_POOL_FIRST && c->pooling != OM_POOL_MEAN) return false;
  if (!sw.attention_fast || L > 256) return false;      // (deliberately stricter than attn_plan.h: float16 packs with the switch on only, and no packed rows beyond 256 tokens)
  if (c->arch == OM_ARCH_BERT && (size_t)c->ffn < (size_t)2 * c->hidden) return false;      // (the f32 pooled tail borrows the [M, F] scratch)
  return true;
}

// whether the four weight-gradient contractions of a BERT layer -- dW2 [H,F], dW1 [F,H], dWo [H,H], dWqkv [3H,H] over M tokens -- all
// take the direct kernel (batch: the 256 x 256 kernel of the deferred launch); what omk_gemm_tn_ok / omk_gemm_tn_batch_ok answer
static bool train_wgrads_direct(int dt, int64_t M, int H, int F, bool batch) {
  auto ok = [&](int64_t N, int64_t K) { return !tn_plan(dt, M, N, K, N, K, 0, batch).error; };
  return ok(H, F) && ok(F, H) && ok(H, H) && ok(3 * H, H);
}

// rules 2 ... 7, for a configuration that passed rule 1 -- or whose caller does not ask that rule (the *_bytes entries)
static TrainPlan train_plan_checked(const TrainPlanIn& in, const TrainSwitches sw) {
  const OmEncoderConfig* c = in.c;
  TrainPlan p = {};
  auto refuse = [&](int rule, const char* why) { p.rule = rule; p.error = why; return p; };
  // 2. shape, tape format and the keep slices -- filled whatever is refused below: the bytes of a call do not depend on whether the
  // call would be taken
  p.packed = in.packed_rows > 0;
  p.B = in.B; p.L = in.L; p.M = p.packed ? in.packed_rows : in.B * in.L; p.Mp = (p.M + 63) / 64 * 64;
  p.H = c->hidden; p.F = c->ffn; p.nl = c->n_layers; p.nh = c->n_heads;
  p.D = c->head_in > 0 ? c->head_out : c->hidden;
  p.es = (c->dtype == OM_BF16 || c->dtype == OM_F16) ? 2 : 4;
  p.t5 = c->arch == OM_ARCH_T5;
  p.rel = c->arch == OM_ARCH_BERT && c->rel_buckets > 0;
  p.gated = p.t5 && (c->act & 0xff) == OM_ACT_GELU_TANH;      // T5 v1.1: gated gelu_new (wi_0, wi_1)
  p.bert16 = !p.t5 && p.es == 2 && (size_t)p.F * p.es >= (size_t)p.H * 4;
  if (in.tape_flags >= 0) {      // the tape as its forward wrote it, not as the switches say now
    p.res32 = (in.tape_flags & TAPE_RES32) != 0;
    p.pre_grad = (in.tape_flags & TAPE_PRE_GRAD) != 0;
  } else {
    p.res32 = p.bert16 && sw.res32 != 0;
    p.pre_grad = p.es == 2 && sw.tape_grad != 0;
  }
  p.keep = !p.t5 && p.es == 2 && p.H % 256 == 0 && p.F % 256 == 0 && p.M >= 32;
  // 3. an empty batch
  if (in.B <= 0) {
    p.empty = true;
    return p;
  }
  // 4. packed rows
  if (p.packed && (in.want_hidden || !train_packed_ok(c, in.B, in.L, in.packed_rows, sw)))
    return refuse(4, in.backward ? "packed rows in training: not for this configuration (om_encoder_train_packed_supported)"
                              : "packed rows in training: 16-bit BERT-family or T5 encoder, widths of 256, L <= 256, rows a multiple of 256 in [512, B * L) "
                                "(om_encoder_train_packed_supported)");
  // 5. BERT family: a table without a bucket count, or the reverse, is an error, never a step without the bias
  if (!p.t5 && in.has_rel_bias != p.rel) return refuse(5, "relative position bias: rel_bias and rel_buckets must be set together");
  // 6. the pooled tail.  16-bit BERT: the pooled rows come from an f32 evaluation of the LAST LayerNorm, and their gradient enters its
  // backward in f32 (train.hip train_tail_forward); the [M, H] f32 rows of the mean borrow the [M, F] 16-bit scratch (bert16: F >= 2 H)
  const int f32_tail = c->pooling == OM_POOL_FIRST ? TRAIN_TAIL_F32_CLS : TRAIN_TAIL_F32_MEAN;
  if (in.want_hidden) p.tail = TRAIN_TAIL_NONE;
  else if (p.t5) p.tail = TRAIN_TAIL_PLAIN;
  else if (in.backward) p.tail = p.bert16 ? f32_tail : TRAIN_TAIL_PLAIN;
  else p.tail = p.es == 2 && p.nl > 0 && (c->pooling == OM_POOL_FIRST || p.bert16) ? f32_tail : TRAIN_TAIL_PLAIN;
  if (p.packed && !p.t5 && p.tail == TRAIN_TAIL_PLAIN) return refuse(6, "packed rows in training: the 16-bit pooled tail only");
  // 7. the BERT stack's streams.  Forward: the early weight transposes (bit 1 of the lane word, 16 bits).  Backward: the lane when every
  // weight gradient takes the direct kernel (16-bit, widths of 128); deferred, batched weight gradients -- 0 .. 12 layers per launch --
  // where the keep slices exist and the 256 x 256 kernel takes all four sites; the LayerNorm sums' A/B
  if (p.t5) return p;
  p.early_wt = (sw.wgrad_stream & 2) != 0 && (in.backward || (p.es == 2 && p.nl > 0));
  if (!in.backward) return p;
  p.lane = sw.wgrad_stream != 0 && train_wgrads_direct(c->dtype, p.M, p.H, p.F, false);
  p.wbatch = p.keep && train_wgrads_direct(c->dtype, p.M, p.H, p.F, true) ? std::min(std::max(sw.wgrad_batch, 0), 12) : 0;
  p.ln_atomics = (sw.wgrad_stream & 4) != 0;
  return p;
}

static TrainPlan train_plan(const TrainPlanIn& in, const TrainSwitches sw) {
  if (const char* why = train_cfg_error(in.c, in.L)) {
    TrainPlan p = {};
    p.rule = 1;
    p.error = why;
    return p;
  }
  return train_plan_checked(in, sw);
}
