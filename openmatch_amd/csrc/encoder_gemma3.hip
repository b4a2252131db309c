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
// What this stack shares with the Llama / Qwen3 one lives in prenorm_stack.h: the workspace and its carving, the argument checks, the
// launches in front of the layer loop (mask extents, packed rows, embedding) and behind it (final norm, pooling, head), and the
// packed-rows rule.  Here: check_cfg, the per-layer pointer checks and the layer loop.
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

#include "prenorm_stack.h"

namespace {

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


const PrenormFamily kGemma3{"Gemma3", 0, false, "Gemma3: layers_host or the per-layer norm weights are null",
                            "Gemma3 needs word_emb (scaled by sqrt(hidden)) and final_ln_g (1 + norm.weight)"};

}  // namespace

extern "C" size_t om_gemma3_encoder_workspace_bytes(const OmGemma3Config* cfg, int64_t B, int64_t L) {
  if (!cfg || B <= 0 || L <= 0 || check_cfg(cfg)) return 0;
  return prenorm_carve(&cfg->base.base, cfg->base.n_kv_heads, 256, false, B, L, nullptr).total;
}

// Whether om_gemma3_encoder_forward_packed takes (cfg, B, L, packed_rows): every compute format.  No region is excluded on grounds of
// speed (DESIGN.md section 8 holds what has been measured).  The causal entries' rule with another lower bound: packed_rows itself must
// lie above OM_OPT_GEMM_SKINNY_M.  All five contractions here are format-in / format-out, so a 16-bit call of at most that many rows
// plans the few-rows kernel where the padded call plans a wide tile, and the two entries would part in bits and in speed.
extern "C" int om_gemma3_encoder_packed_supported(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || !prenorm_packed_rows_rule(B, L, packed_rows, (int64_t)om_option(OM_OPT_GEMM_SKINNY_M) + 1)) return 0;
  return check_cfg(cfg) ? 0 : 1;
}

extern "C" size_t om_gemma3_encoder_workspace_bytes_packed(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || check_cfg(cfg)) return 0;
  return prenorm_carve(&cfg->base.base, cfg->base.n_kv_heads, 256, false, B, L, nullptr, packed_rows).total;
}

// both forward entries: packed_rows == 0 is the padded layout [B * L rows], > 0 the packed one
static int gemma3_forward_impl(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host, const int64_t* input_ids,
                               const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t packed_rows) {
  if (!gc || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(gc)) return 1;
  const OmEncoderConfig* c = &gc->base.base;
  if (B <= 0) return 0;
  PrenormWs ws;
  RUN(prenorm_check(kGemma3, c, gc->base.n_kv_heads, 256, w, w->layers_host && norms_host, B, L, out_hidden, out_reps, workspace, workspace_bytes,
                    packed_rows, &ws));
  // every layer's pointers are checked before the first launch: a refused call leaves nothing on the stream
  const OmLayerWeights* Ls = w->layers_host;
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    const OmGemma3Norms& nw = norms_host[l];
    if (!lw.qkv_w || !lw.o_w || !lw.ln1_g || !lw.ln2_g || !lw.ffn1_w || !lw.ffn1g_w || !lw.ffn2_w)
      OM_FAIL("Gemma3 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)");
    if (!nw.q_norm_g || !nw.k_norm_g || !nw.post_attention_norm_g || !nw.post_feedforward_norm_g)
      OM_FAIL("Gemma3 layers need q_norm_g, k_norm_g, post_attention_norm_g and post_feedforward_norm_g");
    if (lw.qkv_b || lw.o_b || lw.ffn1_b || lw.ffn2_b) OM_FAIL("Gemma3: attention_bias must be False (no projection has a bias)");
  }
  hipStream_t s = (hipStream_t)stream;
  const bool packed = packed_rows > 0;
  const int dt = c->dtype, H = c->hidden, F = c->ffn, nh = c->n_heads, nkv = gc->base.n_kv_heads, A = ws.A, P = ws.P;
  const int64_t M = ws.M;
  const int* const row_map = packed ? ws.row_map : nullptr;
  const PrenormGemm gemm{dt, ws.Mp, s};

  RUN(prenorm_begin(c, w, ws, input_ids, attention_mask, B, L, packed_rows, s));
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    const OmGemma3Norms& nw = norms_host[l];
    const bool sliding = (gc->sliding_layers >> l) & 1;
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));   // input_layernorm
    RUN(gemm(ws.y, H, lw.qkv_w, H, dt, ws.qkv, P, P, H));
    RUN(omk_qknorm_rope(dt, ws.qkv, M, (int)L, nh, nkv, 256, nw.q_norm_g, nw.k_norm_g, c->ln_eps, sliding ? gc->sliding_inv_freq : gc->full_inv_freq,
                        sliding ? gc->sliding_scaling : gc->full_scaling, s, row_map, 1));
    RUN(omk_attention_gqa(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, 256, false, gc->attn_scale, sliding ? gc->half_window : 0, packed,
                          packed ? ws.cu : ws.kmax, s));
    RUN(gemm(ws.ctx, A, lw.o_w, A, dt, ws.y, H, H, A));                                                    // h = o_proj(ctx)
    RUN(omk_rmsnorm_add(dt, ws.y, H, (float*)ws.x, H, nw.post_attention_norm_g, M, H, c->ln_eps, s));       // x += post_attention_layernorm(h)
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln2_g, nullptr, M, H, c->ln_eps, 1, s));   // pre_feedforward_layernorm
    RUN(gemm(ws.y, H, lw.ffn1g_w, H, dt, ws.ff2, F, F, H));                                                // up_proj
    RUN(gemm(ws.y, H, lw.ffn1_w, H, dt, ws.ff, F, F, H, nullptr, ws.ff2, F, OM_ACT_GELU_TANH | OM_ACT_MUL_RESID));   // ff = gelu_tanh(gate_proj) * up
    RUN(gemm(ws.ff, F, lw.ffn2_w, F, dt, ws.y, H, H, F));                                                  // h = down_proj(ff)
    RUN(omk_rmsnorm_add(dt, ws.y, H, (float*)ws.x, H, nw.post_feedforward_norm_g, M, H, c->ln_eps, s));     // x += post_feedforward_layernorm(h)
  }
  return prenorm_tail(c, w, ws, attention_mask, B, L, out_hidden, out_reps, packed_rows, s);
}

extern "C" int om_gemma3_encoder_forward(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host, const int64_t* input_ids,
                                         const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return gemma3_forward_impl(gc, w, norms_host, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace, workspace_bytes, stream, 0);
}

extern "C" int om_gemma3_encoder_forward_packed(const OmGemma3Config* gc, const OmEncoderWeights* w, const OmGemma3Norms* norms_host,
                                                const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows,
                                                float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  return gemma3_forward_impl(gc, w, norms_host, input_ids, attention_mask, B, L, nullptr, out_reps, workspace, workspace_bytes, stream, packed_rows);
}
