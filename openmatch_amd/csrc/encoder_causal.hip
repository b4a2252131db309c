// om_causal_encoder_forward: a decoder-only backbone used as an encoder (HF:models/llama/modeling_llama.py LlamaModel.forward,
// HF:models/qwen2/modeling_qwen2.py Qwen2Model.forward; eval mode, no KV cache) + pooling + LinearHead + normalise, as a fixed
// sequence of launches on ONE stream.  The unfused pre-norm loop of the ModernBERT branch of om_encoder_forward (encoder.hip) with
// RMSNorms, grouped K / V heads, rotary q / k from a host-supplied frequency table, CAUSAL attention and the SwiGLU feed-forward:
//
//   x = embed(ids)
//   per layer:  qkv = Wqkv rms(x, ln1_g) + b ; rope(q, k) ; x += Wo causal_attn(q, k, v) (+ b_o)
//               x += Wdown (silu(Wgate rms(x, ln2_g)) * Wup rms(x, ln2_g))
//   hidden = rms(x, final_ln_g)
//
// SwiGLU is two plain contractions and one elementwise kernel (silu_mul_kernel below), not a GEMM epilogue: the epilogues are
// instantiated per activation in every tile generation and om_gemm_nt's planner (gemm_plan.h) switches on the activation code, so
// a new code there is a change to every existing contraction's planning surface; the elementwise pass costs one read of two
// [M, F] tensors and one write.
//
// The residual stream x is kept in F32 in every compute format, as the reference's autocast keeps it (the embedding output and every
// residual sum are fp32 there; only the linear layers' outputs are 16-bit): o_proj and down_proj read 16-bit operands and add into
// f32 (om_gemm_nt with an f32 output), the RMSNorms read f32 and write the compute format.  A 16-bit stream was measured first: on
// a peaked-attention model (q / k weights x 6, llama3 rope, 512 tokens) bfloat16 sat at 1 - cos 2.65e-3 against HF's own autocast
// at 1.77e-3.
//
// What this stack shares with Gemma3's (encoder_gemma3.hip) lives in prenorm_stack.h: the workspace (PrenormWs: x [M, H] f32 residual
// stream; in the compute dtype y, qkv, ctx, ff / ff2) and its carving, the argument checks, the launches in front of the layer loop
// (mask extents, packed rows, embedding) and behind it (final norm, pooling first / last / mean, head), and the packed-rows rule.  Here:
// check_cfg / check_cfg2, the per-layer pointer checks, the layer loop and the SwiGLU kernel.
//
// om_causal2_encoder_forward / _packed (Qwen3Model, HF:models/qwen3/modeling_qwen3.py) are the same loop with three things read from
// their config instead of assumed: head_dim 64 or 128, an attention width A that need not equal H (o_proj contracts over A), and the
// RMSNorm of each q and k head, applied with the rotation in one pass (omk_qknorm_rope) where the older entries call omk_rope_gqa.
//
// om_causal_encoder_forward_packed is the SAME launch sequence (causal_forward_impl below, one layer loop for both entries) with
// M = packed_rows: each sequence's rows up to its last unmasked token, back to back (omk_pack_rows).  The embedding gathers through
// row_map, the rotary pass reads its position from it, attention walks cu, pooling reads cu / cls_rows / the last-token rows.  Rows
// past the token count are embedded as zeros and stay finite (a zero row normalises to zero; its ctx rows are cleared once, since no
// attention workgroup writes them); nothing pools from them.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "prenorm_stack.h"

namespace {

template <typename T> struct Io8;          // eight consecutive elements <-> floats
template <> struct Io8<float> {
  static constexpr int N = 4;
  __device__ static inline void load(const float* p, float (&v)[4]) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  __device__ static inline void store(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <typename T> struct Io8Half {
  static constexpr int N = 8;
  __device__ static inline void load(const T* p, float (&v)[8]) {
    const uint4 t = *(const uint4*)p;
    v[0] = Half16<T>::lo(t.x); v[1] = Half16<T>::hi(t.x); v[2] = Half16<T>::lo(t.y); v[3] = Half16<T>::hi(t.y);
    v[4] = Half16<T>::lo(t.z); v[5] = Half16<T>::hi(t.z); v[6] = Half16<T>::lo(t.w); v[7] = Half16<T>::hi(t.w);
  }
  __device__ static inline void store(T* p, const float (&v)[8]) {
    *(uint4*)p = make_uint4(Half16<T>::pack2(v[0], v[1]), Half16<T>::pack2(v[2], v[3]), Half16<T>::pack2(v[4], v[5]), Half16<T>::pack2(v[6], v[7]));
  }
};
template <> struct Io8<bf16_t> : Io8Half<bf16_t> {};
template <> struct Io8<f16_t> : Io8Half<f16_t> {};

// up[i] = silu(gate[i]) * up[i] over n elements (n a multiple of the 16-byte vector: the widths are multiples of 64), in f32,
// rounded once.  silu(g) = g / (1 + exp(-g)) (torch.nn.functional.silu).
template <typename T>
__global__ __launch_bounds__(256) void silu_mul_kernel(const T* __restrict__ gate, T* __restrict__ up, int64_t nvec) {
  constexpr int N = Io8<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float g[N], u[N];
    Io8<T>::load(gate + i * N, g);
    Io8<T>::load(up + i * N, u);
#pragma unroll
    for (int e = 0; e < N; ++e) u[e] = g[e] / (1.0f + expf(-g[e])) * u[e];
    Io8<T>::store(up + i * N, u);
  }
}

int omk_silu_mul(int dtype, const void* gate, void* up, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  const int N = dtype == OM_F32 ? 4 : 8;
  if (n % N) OM_FAIL("silu-mul: whole 16-byte vectors only");
  const int64_t nvec = n / N;
  const unsigned grid = (unsigned)std::min<int64_t>((nvec + 255) / 256, 256 * 16);
  if (dtype == OM_BF16) hipLaunchKernelGGL(silu_mul_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)gate, (bf16_t*)up, nvec);
  else if (dtype == OM_F16) hipLaunchKernelGGL(silu_mul_kernel<f16_t>, dim3(grid), dim3(256), 0, s, (const f16_t*)gate, (f16_t*)up, nvec);
  else hipLaunchKernelGGL(silu_mul_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)gate, (float*)up, nvec);
  OM_LAUNCH_CHECK();
  return 0;
}

int check_cfg(const OmCausalConfig* cc) {
  const OmEncoderConfig* c = &cc->base;
  if (c->dtype != OM_F32 && c->dtype != OM_BF16 && c->dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  if (c->arch != OM_ARCH_CAUSAL) OM_FAIL("base.arch must be OM_ARCH_CAUSAL");
  if (c->head_dim != 64 || c->n_heads < 1 || c->n_heads * 64 != c->hidden) OM_FAIL("Llama / Qwen2: only head_dim 64 with n_heads*64 == hidden is supported");
  if (cc->n_kv_heads < 1 || c->n_heads % cc->n_kv_heads) OM_FAIL("Llama / Qwen2: n_kv_heads must be at least 1 and divide n_heads");
  if (c->act != OM_ACT_SILU) OM_FAIL("Llama / Qwen2: hidden_act must be \"silu\" (OM_ACT_SILU)");
  if (c->ffn < 64 || c->ffn % 64 || c->hidden > 2048) OM_FAIL("Llama / Qwen2: hidden and ffn widths are multiples of 64, hidden at most 2048");
  if (c->n_layers < 0 || c->vocab < 1) OM_FAIL("Llama / Qwen2: n_layers >= 0 and a vocabulary");
  if (c->pooling != OM_POOL_NONE && c->pooling != OM_POOL_FIRST && c->pooling != OM_POOL_MEAN && c->pooling != OM_POOL_LAST)
    OM_FAIL("pooling must be OM_POOL_NONE, OM_POOL_FIRST, OM_POOL_MEAN or OM_POOL_LAST");
  if (c->head_in > 0 && c->head_in != c->hidden) OM_FAIL("head_in must equal hidden");
  if (!(cc->rope_attention_scaling > 0.f)) OM_FAIL("Llama / Qwen2: a positive rope_attention_scaling");
  for (int i = 0; i < 32; ++i)
    if (!(cc->inv_freq[i] >= 0.f) || !std::isfinite(cc->inv_freq[i])) OM_FAIL("Llama / Qwen2: inv_freq holds 32 finite, non-negative frequencies");
  return 0;
}

// the om_causal2_* entries (Qwen3): head_dim 64 or 128, an attention width of its own, optional q / k norm
int check_cfg2(const OmCausalConfig2* c2) {
  const OmCausalConfig* cc = &c2->base;
  const OmEncoderConfig* c = &cc->base;
  if (c->dtype != OM_F32 && c->dtype != OM_BF16 && c->dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  if (c->arch != OM_ARCH_CAUSAL) OM_FAIL("base.arch must be OM_ARCH_CAUSAL");
  if ((c->head_dim != 64 && c->head_dim != 128) || c->n_heads < 1) OM_FAIL("Qwen3: head_dim must be 64 or 128, with at least one head");
  if (cc->n_kv_heads < 1 || c->n_heads % cc->n_kv_heads) OM_FAIL("Qwen3: n_kv_heads must be at least 1 and divide n_heads");
  if (c->act != OM_ACT_SILU) OM_FAIL("Qwen3: hidden_act must be \"silu\" (OM_ACT_SILU)");
  if (c->hidden < 64 || c->hidden % 64 || c->ffn < 64 || c->ffn % 64 || c->hidden > 2048)
    OM_FAIL("Qwen3: hidden and ffn widths are multiples of 64, hidden at most 2048");
  if (c->n_layers < 0 || c->vocab < 1) OM_FAIL("Qwen3: n_layers >= 0 and a vocabulary");
  if (c->pooling != OM_POOL_NONE && c->pooling != OM_POOL_FIRST && c->pooling != OM_POOL_MEAN && c->pooling != OM_POOL_LAST)
    OM_FAIL("pooling must be OM_POOL_NONE, OM_POOL_FIRST, OM_POOL_MEAN or OM_POOL_LAST");
  if (c->head_in > 0 && c->head_in != c->hidden) OM_FAIL("head_in must equal hidden");
  if (!(cc->rope_attention_scaling > 0.f)) OM_FAIL("Qwen3: a positive rope_attention_scaling");
  if (c2->qk_norm != 0 && c2->qk_norm != 1) OM_FAIL("Qwen3: qk_norm is 0 or 1");
  const float* f = c->head_dim == 128 ? c2->inv_freq : cc->inv_freq;
  for (int i = 0; i < c->head_dim / 2; ++i)
    if (!(f[i] >= 0.f) || !std::isfinite(f[i])) OM_FAIL("Qwen3: inv_freq holds head_dim / 2 finite, non-negative frequencies");
  return 0;
}

// how the shared refusals read (prenorm_stack.h); both serve OM_POOL_LAST and take packed_rows from 512
const PrenormFamily kCausal{"", 512, true, "layers_host is null", "Llama / Qwen2 need word_emb and final_ln_g (norm.weight)"};
const PrenormFamily kQwen3{"", 512, true, "layers_host is null", "Qwen3 needs word_emb and final_ln_g (norm.weight)"};

// What the one layer loop reads beyond OmCausalConfig: the Llama / Qwen2 entries fill it with head_dim 64, their 32 frequencies and no
// norm; `v2` selects the names in messages and the q / k norm + rotation pass (the older entries keep omk_rope_gqa)
struct CausalExtra {
  bool v2;
  int head_dim;
  const float* inv_freq;
  const OmCausalQkNorm* qk_norm;      // [n_layers] on the host, or NULL: no q / k norm
};

}  // namespace

extern "C" size_t om_causal_encoder_workspace_bytes(const OmCausalConfig* cfg, int64_t B, int64_t L) {
  if (!cfg || B <= 0 || L <= 0 || cfg->n_kv_heads < 1 || cfg->base.n_heads < 1) return 0;
  return prenorm_carve(&cfg->base, cfg->n_kv_heads, 64, true, B, L, nullptr).total;
}

// Whether om_causal_encoder_forward_packed takes (cfg, B, L, packed_rows): the stack is unfused, so every compute format and none of
// the fused-LayerNorm switches enter.  No region is excluded on grounds of speed: the packed entry's throughput has not been measured
// yet (DESIGN.md section 8 says what is to be done when it is).
extern "C" int om_causal_encoder_packed_supported(const OmCausalConfig* cc, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cc || !prenorm_packed_rows_rule(B, L, packed_rows, kCausal.packed_floor)) return 0;
  return check_cfg(cc) ? 0 : 1;
}

extern "C" size_t om_causal_encoder_workspace_bytes_packed(const OmCausalConfig* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || cfg->n_kv_heads < 1 || cfg->base.n_heads < 1) return 0;
  return prenorm_carve(&cfg->base, cfg->n_kv_heads, 64, true, B, L, nullptr, packed_rows).total;
}

// all four forward entries (the config is checked by the caller): packed_rows == 0 is the padded layout [B * L rows], > 0 the packed one
static int causal_forward_impl(const OmCausalConfig* cc, const CausalExtra& ex, const OmEncoderWeights* w, const int64_t* input_ids,
                               const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t packed_rows) {
  const OmEncoderConfig* c = &cc->base;
  if (B <= 0) return 0;
  PrenormWs ws;
  RUN(prenorm_check(ex.v2 ? kQwen3 : kCausal, c, cc->n_kv_heads, ex.head_dim, w, w->layers_host != nullptr, B, L, out_hidden, out_reps, workspace,
                    workspace_bytes, packed_rows, &ws));
  // every layer's pointers are checked before the first launch: a refused call leaves nothing on the stream
  const OmLayerWeights* Ls = w->layers_host;
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    if (!lw.qkv_w || !lw.o_w || !lw.ln1_g || !lw.ln2_g || !lw.ffn1_w || !lw.ffn1g_w || !lw.ffn2_w)
      OM_FAIL(ex.v2 ? "Qwen3 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)"
                    : "Llama / Qwen2 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)");
    if (ex.qk_norm && (!ex.qk_norm[l].q_norm_g || !ex.qk_norm[l].k_norm_g)) OM_FAIL("Qwen3 layers with qk_norm need q_norm_g and k_norm_g");
  }
  hipStream_t s = (hipStream_t)stream;
  const bool packed = packed_rows > 0;
  const int dt = c->dtype, H = c->hidden, F = c->ffn, nh = c->n_heads, nkv = cc->n_kv_heads, hd = ex.head_dim, A = ws.A, P = ws.P;
  const int64_t M = ws.M;
  const int* const row_map = packed ? ws.row_map : nullptr;
  const PrenormGemm gemm{dt, ws.Mp, s};

  RUN(prenorm_begin(c, w, ws, input_ids, attention_mask, B, L, packed_rows, s));
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));   // input_layernorm
    RUN(gemm(ws.y, H, lw.qkv_w, H, dt, ws.qkv, P, P, H, lw.qkv_b));
    if (ex.v2) {                                                                                           // q_norm, k_norm, rotary positions
      const OmCausalQkNorm* qn = ex.qk_norm ? &ex.qk_norm[l] : nullptr;
      RUN(omk_qknorm_rope(dt, ws.qkv, M, (int)L, nh, nkv, hd, qn ? qn->q_norm_g : nullptr, qn ? qn->k_norm_g : nullptr, c->ln_eps, ex.inv_freq,
                          cc->rope_attention_scaling, s, row_map));
    } else {
      RUN(omk_rope_gqa(dt, ws.qkv, M, (int)L, nh, nkv, cc->inv_freq, cc->rope_attention_scaling, s, row_map));
    }
    RUN(omk_attention_gqa(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, hd, true, scale, 0, packed, packed ? ws.cu : ws.kmax, s));
    // the residual sums: operands in the compute dtype, f32 output and residual (x += A W^T + bias)
    RUN(gemm(ws.ctx, A, lw.o_w, A, OM_F32, ws.x, H, H, A, lw.o_b, ws.x, H));                               // x += o_proj(ctx)
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln2_g, nullptr, M, H, c->ln_eps, 1, s));   // post_attention_layernorm
    RUN(gemm(ws.y, H, lw.ffn1_w, H, dt, ws.ff2, F, F, H));                                                 // gate_proj
    RUN(gemm(ws.y, H, lw.ffn1g_w, H, dt, ws.ff, F, F, H));                                                 // up_proj
    RUN(omk_silu_mul(dt, ws.ff2, ws.ff, M * F, s));                                                        // ff = silu(gate) * up
    RUN(gemm(ws.ff, F, lw.ffn2_w, F, OM_F32, ws.x, H, H, F, nullptr, ws.x, H));                            // x += down_proj(ff)
  }
  return prenorm_tail(c, w, ws, attention_mask, B, L, out_hidden, out_reps, packed_rows, s);
}

extern "C" int om_causal_encoder_forward(const OmCausalConfig* cc, const OmEncoderWeights* w, const int64_t* input_ids,
                                         const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!cc || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(cc)) return 1;
  return causal_forward_impl(cc, CausalExtra{false, 64, cc->inv_freq, nullptr}, w, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace,
                             workspace_bytes, stream, 0);
}

extern "C" int om_causal_encoder_forward_packed(const OmCausalConfig* cc, const OmEncoderWeights* w, const int64_t* input_ids,
                                                const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows, float* out_reps,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  if (!cc || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg(cc)) return 1;
  return causal_forward_impl(cc, CausalExtra{false, 64, cc->inv_freq, nullptr}, w, input_ids, attention_mask, B, L, nullptr, out_reps, workspace,
                             workspace_bytes, stream, packed_rows);
}

// ---- Qwen3: the same loop behind a config that adds the head width, the q / k norm and 64 frequencies ----
static CausalExtra extra_of(const OmCausalConfig2* c2, const OmCausalQkNorm* qk_norm_host) {
  const int hd = c2->base.base.head_dim;
  return CausalExtra{true, hd, hd == 128 ? c2->inv_freq : c2->base.inv_freq, c2->qk_norm ? qk_norm_host : nullptr};
}

extern "C" size_t om_causal2_encoder_workspace_bytes(const OmCausalConfig2* cfg, int64_t B, int64_t L) {
  if (!cfg || B <= 0 || L <= 0 || check_cfg2(cfg)) return 0;
  return prenorm_carve(&cfg->base.base, cfg->base.n_kv_heads, cfg->base.base.head_dim, true, B, L, nullptr).total;
}

extern "C" int om_causal2_encoder_packed_supported(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || !prenorm_packed_rows_rule(B, L, packed_rows, kQwen3.packed_floor)) return 0;
  return check_cfg2(cfg) ? 0 : 1;
}

extern "C" size_t om_causal2_encoder_workspace_bytes_packed(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || check_cfg2(cfg)) return 0;
  return prenorm_carve(&cfg->base.base, cfg->base.n_kv_heads, cfg->base.base.head_dim, true, B, L, nullptr, packed_rows).total;
}

// the two Qwen3 forward entries: packed_rows == 0 is the padded one
static int causal2_forward(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host, const int64_t* input_ids,
                           const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                           size_t workspace_bytes, void* stream, int64_t packed_rows) {
  if (!cfg || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg2(cfg)) return 1;
  if (cfg->qk_norm && cfg->base.base.n_layers > 0 && !qk_norm_host) OM_FAIL("Qwen3: qk_norm is set but the q / k norm weights are null");
  return causal_forward_impl(&cfg->base, extra_of(cfg, qk_norm_host), w, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace,
                             workspace_bytes, stream, packed_rows);
}

extern "C" int om_causal2_encoder_forward(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                                          const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden,
                                          float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  return causal2_forward(cfg, w, qk_norm_host, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace, workspace_bytes, stream, 0);
}

extern "C" int om_causal2_encoder_forward_packed(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                                                 const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L,
                                                 int64_t packed_rows, float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  return causal2_forward(cfg, w, qk_norm_host, input_ids, attention_mask, B, L, nullptr, out_reps, workspace, workspace_bytes, stream, packed_rows);
}
