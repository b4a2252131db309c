// om_gemma3_encoder_forward: EmbeddingGemma's backbone -- HF Gemma3TextModel with use_bidirectional_attention
// (HF:models/gemma3/modeling_gemma3.py Gemma3TextModel.forward, eval mode, no cache) + pooling + LinearHead + normalise, as a fixed
// sequence of launches on ONE stream.  The f32-residual pre-norm loop of causal_forward_impl (encoder_causal.hip) with what Gemma3
// changes:
//
//   x = embed(ids)                                   (the host has scaled the table by float32(sqrt(hidden)) in f32)
//   per layer:  qkv = Wqkv rms(x, ln1_g)             input_layernorm; no biases
//               q, k = rope(rms_head(q, q_norm_g)), rope(rms_head(k, k_norm_g))      the layer TYPE's frequencies (sliding / full)
//               h = Wo attn(q, k, v)                 heads of 256 columns, grouped K / V, scale = query_pre_attn_scalar ** -0.5,
//                                                    bidirectional; sliding layers: |q - k| <= half_window
//               x += rms(h, post_attention_norm_g)   the norm acts on the sublayer OUTPUT (omk_rmsnorm_add)
//               h = Wdown (gelu_tanh(Wgate y) * Wup y),  y = rms(x, ln2_g)           pre_feedforward_layernorm
//               x += rms(h, post_feedforward_norm_g)
//   hidden = rms(x, final_ln_g)
//
// Every norm weight arrives as g = 1 + w (Gemma3RMSNorm multiplies by 1 + weight; the host adds in f32, bit-identical to HF's
// 1.0 + weight.float()), so the row kernels of the other stacks serve unchanged.  The gated feed-forward is T5 v1.1's: the up
// projection first, then the gate contraction with the tanh-GELU epilogue multiplied by it (OM_ACT_GELU_TANH | OM_ACT_MUL_RESID).
// The residual stream x stays in f32 in every compute format, as the reference's autocast keeps it; o_proj and down_proj write the
// compute format (their outputs are normalised before they are added).
//
// om_gemma3_encoder_forward_packed is the SAME launch sequence (gemma3_forward_impl below, one layer loop for both entries, as
// causal_forward_impl of encoder_causal.hip) with M = packed_rows: each sequence's rows up to its last unmasked token, back to back
// (omk_pack_rows).  The embedding gathers through row_map, the q / k norm + rotation reads its position from it, attention walks cu,
// pooling reads cu / cls_rows.  Rows past the token count are embedded as zeros and stay finite (a zero row normalises to zero; its ctx
// rows are cleared once, since no attention workgroup writes them); nothing pools from them.  Representations only.
// Not built: the on-device pad skip of the padded entry (it rests on GemmEpilogue::rows_dev, which only the generation-7 whole-tile
// kernels read; EmbeddingGemma's feed-forward width 1152 is no multiple of 256, so its contractions run on the generic tiles), and
// training.
#include <math.h>

#include <cmath>

#include "kernels.h"

namespace {

struct Gemma3Ws {
  char *x, *y, *qkv, *ctx, *ff, *ff2;
  float *pooled, *headout, *final32;
  int* kmax;
  int *cu, *cls_rows, *row_map;   // packed rows: sequence offsets [B + 2], first row of each sequence [B], token of each row [packed_rows]
  int64_t Mp;       // row count the contractions run on: M rounded up to whole 256-row tiles for large 16-bit batches (as encoder_causal.hip)
  size_t total;
};

Gemma3Ws carve(const OmGemma3Config* gc, int64_t B, int64_t L, char* base, int64_t packed_rows = 0) {
  const OmEncoderConfig* c = &gc->base.base;
  const bool half = c->dtype == OM_BF16 || c->dtype == OM_F16;
  const size_t es = half ? 2 : 4;
  const size_t Mreal = packed_rows > 0 ? (size_t)packed_rows : (size_t)B * L, H = c->hidden, F = c->ffn;
  const size_t A = (size_t)c->n_heads * 256, P = (size_t)(c->n_heads + 2 * gc->base.n_kv_heads) * 256;
  const size_t M = (half && Mreal >= 512) ? (Mreal + 255) / 256 * 256 : Mreal;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  Gemma3Ws w;
  w.x = take(M * H * 4);
  w.y = take(M * H * es);
  w.qkv = take(M * P * es);
  w.ctx = take(M * A * es);
  w.ff = take(M * F * es);
  w.ff2 = take(M * F * es);
  w.pooled = (float*)take((size_t)B * H * 4);
  w.headout = (float*)take((size_t)B * (c->head_out > 0 ? c->head_out : 1) * 4);
  w.kmax = (int*)take((size_t)B * 4);
  w.final32 = (float*)take(c->pooling == OM_POOL_MEAN ? Mreal * H * 4 : 0);      // mean pooling reads every row of the f32 final norm
  w.cu = (int*)take(packed_rows > 0 ? (size_t)(B + 2) * 4 : 0);
  w.cls_rows = (int*)take(packed_rows > 0 ? (size_t)B * 4 : 0);
  w.row_map = (int*)take(packed_rows > 0 ? (size_t)packed_rows * 4 : 0);
  w.Mp = (int64_t)M;
  w.total = off;
  return w;
}

int check_cfg(const OmGemma3Config* gc) {
  const OmCausalConfig* cc = &gc->base;
  const OmEncoderConfig* c = &cc->base;
  if (c->dtype != OM_F32 && c->dtype != OM_BF16 && c->dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  if (c->arch != OM_ARCH_GEMMA3) OM_FAIL("base.base.arch must be OM_ARCH_GEMMA3");
  if (c->head_dim != 256 || c->n_heads < 1) OM_FAIL("Gemma3: only head_dim 256 is supported, with at least one head");
  if (cc->n_kv_heads < 1 || c->n_heads % cc->n_kv_heads) OM_FAIL("Gemma3: n_kv_heads must be at least 1 and divide n_heads");
  if (c->act != OM_ACT_GELU_TANH) OM_FAIL("Gemma3: hidden_activation must be \"gelu_pytorch_tanh\" (OM_ACT_GELU_TANH)");
  if (c->hidden < 64 || c->hidden % 64 || c->ffn < 64 || c->ffn % 64 || c->hidden > 2048)
    OM_FAIL("Gemma3: hidden and ffn widths are multiples of 64, hidden at most 2048");
  if (c->n_layers < 0 || c->n_layers > 64 || c->vocab < 1) OM_FAIL("Gemma3: 0 to 64 layers and a vocabulary");
  if (c->pooling == OM_POOL_LAST) OM_FAIL("Gemma3: pooling 'last' is not served for the bidirectional encoder (OM_POOL_NONE, OM_POOL_FIRST or OM_POOL_MEAN)");
  if (c->pooling != OM_POOL_NONE && c->pooling != OM_POOL_FIRST && c->pooling != OM_POOL_MEAN)
    OM_FAIL("pooling must be OM_POOL_NONE, OM_POOL_FIRST or OM_POOL_MEAN");
  if (c->head_in > 0 && c->head_in != c->hidden) OM_FAIL("head_in must equal hidden");
  if (gc->bidirectional != 1) OM_FAIL("Gemma3: use_bidirectional_attention must be True (the causal Gemma3 is not served)");
  if (gc->attn_logit_softcapping != 0.f) OM_FAIL("Gemma3: attn_logit_softcapping must be None (0)");
  if (!(gc->attn_scale > 0.f) || !std::isfinite(gc->attn_scale)) OM_FAIL("Gemma3: a positive attn_scale (query_pre_attn_scalar ** -0.5)");
  if (gc->half_window < 0) OM_FAIL("Gemma3: half_window (sliding_window - 1) must not be negative");
  if (gc->sliding_layers && gc->half_window < 1) OM_FAIL("Gemma3: sliding layers need a half_window of at least 1");
  if (c->n_layers < 64 && (gc->sliding_layers >> c->n_layers)) OM_FAIL("Gemma3: sliding_layers names a layer past n_layers");
  if (!(gc->full_scaling > 0.f) || !(gc->sliding_scaling > 0.f)) OM_FAIL("Gemma3: positive rotary attention scalings");
  for (int i = 0; i < 128; ++i)
    if (!(gc->full_inv_freq[i] >= 0.f) || !std::isfinite(gc->full_inv_freq[i]) || !(gc->sliding_inv_freq[i] >= 0.f) || !std::isfinite(gc->sliding_inv_freq[i]))
      OM_FAIL("Gemma3: full_inv_freq and sliding_inv_freq hold 128 finite, non-negative frequencies each");
  return 0;
}

// The causal rule (encoder_causal.hip packed_rows_rule) and one clause more: packed_rows itself must lie above OM_OPT_GEMM_SKINNY_M.  All
// five contractions here are format-in / format-out, so a 16-bit call of at most that many rows plans the few-rows kernel where the padded
// call plans a wide tile, and the two entries would part in bits and in speed.
bool packed_rows_rule(int64_t B, int64_t L, int64_t packed_rows) {
  if (B <= 0 || L <= 0 || L > 1024 || packed_rows <= 0) return false;
  if (packed_rows % 256 || packed_rows > B * L + 255) return false;
  const int64_t skinny = (int64_t)om_option(OM_OPT_GEMM_SKINNY_M);
  return B * L > skinny && packed_rows > skinny;
}

}  // namespace

extern "C" size_t om_gemma3_encoder_workspace_bytes(const OmGemma3Config* cfg, int64_t B, int64_t L) {
  if (!cfg || B <= 0 || L <= 0 || check_cfg(cfg)) return 0;
  return carve(cfg, B, L, nullptr).total;
}

// Whether om_gemma3_encoder_forward_packed takes (cfg, B, L, packed_rows): every compute format.  No region is excluded on grounds of
// speed (DESIGN.md section 8 holds what has been measured).
extern "C" int om_gemma3_encoder_packed_supported(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || !packed_rows_rule(B, L, packed_rows)) return 0;
  return check_cfg(cfg) ? 0 : 1;
}

extern "C" size_t om_gemma3_encoder_workspace_bytes_packed(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || check_cfg(cfg)) return 0;
  return carve(cfg, B, L, nullptr, packed_rows).total;
}

// both forward entries (arguments and config are checked by the caller): packed_rows == 0 is the padded layout [B * L rows], > 0 the
// packed one
static int gemma3_forward_impl(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host, const int64_t* input_ids,
                               const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t packed_rows) {
  const OmEncoderConfig* c = &gc->base.base;
  if (B <= 0) return 0;
  if (L < 1 || L > 1024) OM_FAIL("Gemma3: sequence length must be in [1,1024]");
  const bool packed = packed_rows > 0;
  if (packed) {
    if (c->pooling == OM_POOL_NONE || out_hidden) OM_FAIL("Gemma3 packed rows: representations only (a pooling, no out_hidden)");
    if (packed_rows % 256 || packed_rows > B * L + 255) OM_FAIL("Gemma3 packed_rows: a multiple of 256, at most B * L + 255");
  }
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  Gemma3Ws ws = carve(gc, B, L, (char*)workspace, packed_rows);
  if (ws.total > workspace_bytes) OM_FAIL("workspace too small");
  if (c->pooling != OM_POOL_NONE && !out_reps) OM_FAIL("out_reps required when pooling is set");
  const OmLayerWeights* Ls = w->layers_host;
  if (c->n_layers > 0 && (!Ls || !norms_host)) OM_FAIL("Gemma3: layers_host or the per-layer norm weights are null");
  if (!w->word_emb || !w->final_ln_g) OM_FAIL("Gemma3 needs word_emb (scaled by sqrt(hidden)) and final_ln_g (1 + norm.weight)");
  hipStream_t s = (hipStream_t)stream;
  const int dt = c->dtype, H = c->hidden, F = c->ffn, nh = c->n_heads, nkv = gc->base.n_kv_heads;
  const int A = nh * 256, P = (nh + 2 * nkv) * 256;
  const int64_t M = packed ? packed_rows : B * L, Mg = ws.Mp;
  const int* const row_map = packed ? ws.row_map : nullptr;

#define GEMM(A_, lda_, W_, ldw_, C_, ldc_, N_, K_, res_, ldr_, act_)                                      \
  do {                                                                                                     \
    if (om_gemm_nt(dt, A_, lda_, W_, ldw_, dt, C_, ldc_, Mg, N_, K_, nullptr, res_, ldr_, act_, s))       \
      return 1;                                                                                            \
  } while (0)
#define RUN(expr) do { if (expr) return 1; } while (0)

  // every layer's pointers are checked before the first launch: a refused call leaves nothing on the stream
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    const OmGemma3Norms& nw = norms_host[l];
    if (!lw.qkv_w || !lw.o_w || !lw.ln1_g || !lw.ln2_g || !lw.ffn1_w || !lw.ffn1g_w || !lw.ffn2_w)
      OM_FAIL("Gemma3 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)");
    if (!nw.q_norm_g || !nw.k_norm_g || !nw.post_attention_norm_g || !nw.post_feedforward_norm_g)
      OM_FAIL("Gemma3 layers need q_norm_g, k_norm_g, post_attention_norm_g and post_feedforward_norm_g");
    if (lw.qkv_b || lw.o_b || lw.ffn1_b || lw.ffn2_b) OM_FAIL("Gemma3: attention_bias must be False (no projection has a bias)");
  }
  RUN(omk_mask_extent(attention_mask, B, (int)L, ws.kmax, s));
  if (packed) {
    RUN(omk_pack_rows(ws.kmax, B, (int)L, packed_rows, ws.cu, ws.cls_rows, ws.row_map, s));
    OM_HIP(hipMemsetAsync(ws.ctx, 0, (size_t)M * A * (dt == OM_F32 ? 4 : 2), s));      // the tail rows: no attention workgroup writes them
  }
  RUN(omk_embed(OM_F32, input_ids, nullptr, w->word_emb, nullptr, nullptr, nullptr, nullptr, ws.x, M, (int)L, H, c->vocab, 1, c->ln_eps, 0, s, row_map));
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    const OmGemma3Norms& nw = norms_host[l];
    const bool sliding = (gc->sliding_layers >> l) & 1;
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));   // input_layernorm
    GEMM(ws.y, H, lw.qkv_w, H, ws.qkv, P, P, H, nullptr, 0, OM_ACT_NONE);
    RUN(omk_qknorm_rope(dt, ws.qkv, M, (int)L, nh, nkv, 256, nw.q_norm_g, nw.k_norm_g, c->ln_eps, sliding ? gc->sliding_inv_freq : gc->full_inv_freq,
                        sliding ? gc->sliding_scaling : gc->full_scaling, s, row_map, 1));
    if (packed) RUN(omk_attention_gqa_d256_packed(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, gc->attn_scale, sliding ? gc->half_window : 0, ws.cu, s));
    else RUN(omk_attention_gqa_d256(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, gc->attn_scale, sliding ? gc->half_window : 0, ws.kmax, s));
    GEMM(ws.ctx, A, lw.o_w, A, ws.y, H, H, A, nullptr, 0, OM_ACT_NONE);                                    // h = o_proj(ctx)
    RUN(omk_rmsnorm_add(dt, ws.y, H, (float*)ws.x, H, nw.post_attention_norm_g, M, H, c->ln_eps, s));       // x += post_attention_layernorm(h)
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln2_g, nullptr, M, H, c->ln_eps, 1, s));   // pre_feedforward_layernorm
    GEMM(ws.y, H, lw.ffn1g_w, H, ws.ff2, F, F, H, nullptr, 0, OM_ACT_NONE);                                // up_proj
    GEMM(ws.y, H, lw.ffn1_w, H, ws.ff, F, F, H, ws.ff2, F, OM_ACT_GELU_TANH | OM_ACT_MUL_RESID);           // ff = gelu_tanh(gate_proj) * up
    GEMM(ws.ff, F, lw.ffn2_w, F, ws.y, H, H, F, nullptr, 0, OM_ACT_NONE);                                  // h = down_proj(ff)
    RUN(omk_rmsnorm_add(dt, ws.y, H, (float*)ws.x, H, nw.post_feedforward_norm_g, M, H, c->ln_eps, s));     // x += post_feedforward_layernorm(h)
  }
  // norm: the hidden states in the compute dtype when asked for; the pooled rows ALWAYS as f32 rows of the normalisation of just the
  // rows pooling reads, as the other stacks do
  const float* fg = w->final_ln_g;
  const float* xf = (const float*)ws.x;
  if (out_hidden) RUN(omk_layernorm_from_f32(dt, xf, H, out_hidden, H, fg, nullptr, M, H, c->ln_eps, 1, s));
  if (c->pooling != OM_POOL_NONE) {
    float* pooled = c->head_in > 0 && w->head_w ? ws.pooled : out_reps;
    if (c->pooling == OM_POOL_FIRST) {
      if (packed) RUN(omk_layernorm_f32out(OM_F32, xf, H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s, nullptr, ws.cls_rows));
      else RUN(omk_layernorm_f32out(OM_F32, xf, L * H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s));
    } else {
      RUN(omk_layernorm_f32out(OM_F32, xf, H, ws.final32, H, fg, nullptr, M, H, c->ln_eps, 1, s));
      RUN(omk_pool(OM_F32, ws.final32, attention_mask, pooled, B, (int)L, H, OM_POOL_MEAN, s, packed ? ws.cu : nullptr));
    }
    RUN(omk_pooled_tail(c, w, pooled, out_reps, B, packed ? ws.cu : nullptr, packed_rows, s));      // a bound below the token count poisons the representations
  }
#undef GEMM
#undef RUN
  return 0;
}

extern "C" int om_gemma3_encoder_forward(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host, const int64_t* input_ids,
                                         const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  if (!gc || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(gc)) return 1;
  return gemma3_forward_impl(gc, w, norms_host, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace, workspace_bytes, stream, 0);
}

extern "C" int om_gemma3_encoder_forward_packed(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host,
                                                const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows,
                                                float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  if (!gc || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(gc)) return 1;
  return gemma3_forward_impl(gc, w, norms_host, input_ids, attention_mask, B, L, nullptr, out_reps, workspace, workspace_bytes, stream, packed_rows);
}
