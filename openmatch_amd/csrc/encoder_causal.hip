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
// Activation buffers ([M = B*L tokens] x width): x [M, H] f32 residual stream; in the compute dtype y normed input,
// qkv [M, (heads + 2 kv) * head_dim], ctx [M, A = heads * head_dim], ff / ff2 [M, F].
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

#include "kernels.h"

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

// rows[b] = the token row of sequence b's LAST unmasked token (kmax[b] = 1 + its index; L for a row without one: the last column)
__global__ void last_rows_kernel(const int* __restrict__ kmax, int64_t B, int L, int* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rows[b] = (int)(b * L + kmax[b] - 1);
}

// packed rows: the row of sequence b's last unmasked token is cu[b] + kmax[b] - 1, clamped into the buffer as cls_rows is (a bound that
// was too small: the representations are poisoned afterwards)
__global__ void last_rows_packed_kernel(const int* __restrict__ kmax, const int* __restrict__ cu, int64_t B, int rows_cap, int* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rows[b] = min(cu[b] + kmax[b] - 1, rows_cap - 1);
}

struct CausalWs {
  char *x, *y, *qkv, *ctx, *ff, *ff2;
  float *pooled, *headout, *final32;
  int *kmax, *last_rows;
  int *cu, *cls_rows, *row_map;   // packed rows: sequence offsets [B + 2], first row of each sequence [B], token of each row [packed_rows]
  int64_t Mp;       // row count the contractions run on: M rounded up to whole 256-row tiles for large 16-bit batches (as encoder.hip)
  size_t total;
};

// head_dim: 64 for the Llama / Qwen2 entries; the config's own for the om_causal2_* entries, whose attention width A = n_heads * head_dim
// need not equal the hidden size
CausalWs carve(const OmCausalConfig* cc, int head_dim, int64_t B, int64_t L, char* base, int64_t packed_rows = 0) {
  const OmEncoderConfig* c = &cc->base;
  const bool half = c->dtype == OM_BF16 || c->dtype == OM_F16;
  const size_t es = half ? 2 : 4;
  const size_t Mreal = packed_rows > 0 ? (size_t)packed_rows : (size_t)B * L, H = c->hidden, F = c->ffn;
  const size_t A = (size_t)c->n_heads * head_dim, P = (size_t)(c->n_heads + 2 * cc->n_kv_heads) * head_dim;
  const size_t M = (half && Mreal >= 512) ? (Mreal + 255) / 256 * 256 : Mreal;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  CausalWs w;
  w.x = take(M * H * 4);
  w.y = take(M * H * es);
  w.qkv = take(M * P * es);
  w.ctx = take(M * A * es);
  w.ff = take(M * F * es);
  w.ff2 = take(M * F * es);
  w.pooled = (float*)take((size_t)B * H * 4);
  w.headout = (float*)take((size_t)B * (c->head_out > 0 ? c->head_out : 1) * 4);
  w.kmax = (int*)take((size_t)B * 4);
  w.last_rows = (int*)take((size_t)B * 4);
  w.final32 = (float*)take(c->pooling == OM_POOL_MEAN ? Mreal * H * 4 : 0);      // mean pooling reads every row of the f32 final norm
  w.cu = (int*)take(packed_rows > 0 ? (size_t)(B + 2) * 4 : 0);
  w.cls_rows = (int*)take(packed_rows > 0 ? (size_t)B * 4 : 0);
  w.row_map = (int*)take(packed_rows > 0 ? (size_t)packed_rows * 4 : 0);
  w.Mp = (int64_t)M;
  w.total = off;
  return w;
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

bool packed_rows_rule(int64_t B, int64_t L, int64_t packed_rows) {
  if (B <= 0 || L <= 0 || L > 1024 || packed_rows <= 0) return false;
  if (packed_rows % 256 || packed_rows < 512 || packed_rows > B * L + 255) return false;
  // few rows: the padded entry's contractions take the weight-streaming kernel -- decided there on ITS row count B * L, so a batch
  // whose PADDED form is that small is sent back (as om_encoder_packed_supported)
  return B * L > (int64_t)om_option(OM_OPT_GEMM_SKINNY_M);
}

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
  return carve(cfg, 64, B, L, nullptr).total;
}

// Whether om_causal_encoder_forward_packed takes (cfg, B, L, packed_rows): the stack is unfused, so every compute format and none of
// the fused-LayerNorm switches enter.  No region is excluded on grounds of speed: the packed entry's throughput has not been measured
// yet (DESIGN.md section 8 says what is to be done when it is).
extern "C" int om_causal_encoder_packed_supported(const OmCausalConfig* cc, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cc || !packed_rows_rule(B, L, packed_rows)) return 0;
  return check_cfg(cc) ? 0 : 1;
}

extern "C" size_t om_causal_encoder_workspace_bytes_packed(const OmCausalConfig* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || cfg->n_kv_heads < 1 || cfg->base.n_heads < 1) return 0;
  return carve(cfg, 64, B, L, nullptr, packed_rows).total;
}

// all four forward entries (the config is checked by the caller): packed_rows == 0 is the padded layout [B * L rows], > 0 the packed one
static int causal_forward_impl(const OmCausalConfig* cc, const CausalExtra& ex, const OmEncoderWeights* w, const int64_t* input_ids,
                               const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t packed_rows) {
  const OmEncoderConfig* c = &cc->base;
  if (B <= 0) return 0;
  if (L < 1 || L > 1024) OM_FAIL("sequence length must be in [1,1024]");
  const bool packed = packed_rows > 0;
  if (packed) {
    if (c->pooling == OM_POOL_NONE || out_hidden) OM_FAIL("packed rows: representations only (a pooling, no out_hidden)");
    if (packed_rows % 256 || packed_rows < 512 || packed_rows > B * L + 255) OM_FAIL("packed_rows: a multiple of 256 in [512, B * L + 255]");
  }
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  CausalWs ws = carve(cc, ex.head_dim, B, L, (char*)workspace, packed_rows);
  if (ws.total > workspace_bytes) OM_FAIL("workspace too small");
  if (c->pooling != OM_POOL_NONE && !out_reps) OM_FAIL("out_reps required when pooling is set");
  const OmLayerWeights* Ls = w->layers_host;
  if (c->n_layers > 0 && !Ls) OM_FAIL("layers_host is null");
  if (!w->word_emb || !w->final_ln_g) OM_FAIL(ex.v2 ? "Qwen3 needs word_emb and final_ln_g (norm.weight)" : "Llama / Qwen2 need word_emb and final_ln_g (norm.weight)");
  hipStream_t s = (hipStream_t)stream;
  const int dt = c->dtype, H = c->hidden, F = c->ffn, nh = c->n_heads, nkv = cc->n_kv_heads;
  const int hd = ex.head_dim, A = nh * hd, P = (nh + 2 * nkv) * hd;      // A: the attention width (ctx rows, o_proj's contraction)
  const int64_t M = packed ? packed_rows : B * L, Mg = ws.Mp;
  const int* const row_map = packed ? ws.row_map : nullptr;

#define GEMM(A_, lda_, W_, ldw_, C_, ldc_, N_, K_, bias_, res_, ldr_)                                      \
  do {                                                                                                     \
    if (om_gemm_nt(dt, A_, lda_, W_, ldw_, dt, C_, ldc_, Mg, N_, K_, bias_, res_, ldr_, OM_ACT_NONE, s)) \
      return 1;                                                                                            \
  } while (0)
  // x (f32) += A W^T (+ bias): operands in the compute dtype, f32 output and residual
#define GEMM_ACC(A_, lda_, W_, ldw_, N_, K_, bias_)                                                              \
  do {                                                                                                           \
    if (om_gemm_nt(dt, A_, lda_, W_, ldw_, OM_F32, ws.x, N_, Mg, N_, K_, bias_, ws.x, N_, OM_ACT_NONE, s)) \
      return 1;                                                                                                  \
  } while (0)
#define RUN(expr) do { if (expr) return 1; } while (0)

  RUN(omk_mask_extent(attention_mask, B, (int)L, ws.kmax, s));
  if (packed) {
    RUN(omk_pack_rows(ws.kmax, B, (int)L, packed_rows, ws.cu, ws.cls_rows, ws.row_map, s));
    OM_HIP(hipMemsetAsync(ws.ctx, 0, (size_t)M * A * (dt == OM_F32 ? 4 : 2), s));      // the tail rows: no attention workgroup writes them
  }
  RUN(omk_embed(OM_F32, input_ids, nullptr, w->word_emb, nullptr, nullptr, nullptr, nullptr, ws.x, M, (int)L, H, c->vocab, 1, c->ln_eps, 0, s, row_map));
  const float scale = 1.0f / sqrtf((float)c->head_dim);
  for (int l = 0; l < c->n_layers; ++l) {
    const OmLayerWeights& lw = Ls[l];
    if (!lw.qkv_w || !lw.o_w || !lw.ln1_g || !lw.ln2_g || !lw.ffn1_w || !lw.ffn1g_w || !lw.ffn2_w)
      OM_FAIL(ex.v2 ? "Qwen3 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)"
                    : "Llama / Qwen2 layers need qkv_w, o_w, ln1_g, ln2_g, ffn1_w (gate_proj), ffn1g_w (up_proj) and ffn2_w (down_proj)");
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln1_g, nullptr, M, H, c->ln_eps, 1, s));   // input_layernorm
    GEMM(ws.y, H, lw.qkv_w, H, ws.qkv, P, P, H, lw.qkv_b, nullptr, 0);
    if (ex.v2) {                                                                                           // q_norm, k_norm, rotary positions
      const OmCausalQkNorm* qn = ex.qk_norm ? &ex.qk_norm[l] : nullptr;
      if (qn && (!qn->q_norm_g || !qn->k_norm_g)) OM_FAIL("Qwen3 layers with qk_norm need q_norm_g and k_norm_g");
      RUN(omk_qknorm_rope(dt, ws.qkv, M, (int)L, nh, nkv, hd, qn ? qn->q_norm_g : nullptr, qn ? qn->k_norm_g : nullptr, c->ln_eps, ex.inv_freq,
                          cc->rope_attention_scaling, s, row_map));
    } else {
      RUN(omk_rope_gqa(dt, ws.qkv, M, (int)L, nh, nkv, cc->inv_freq, cc->rope_attention_scaling, s, row_map));
    }
    if (hd == 128) {
      if (packed) RUN(omk_attention_causal_d128_packed(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, scale, ws.cu, s));
      else RUN(omk_attention_causal_d128(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, scale, ws.kmax, s));
    } else {
      if (packed) RUN(omk_attention_causal_packed(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, scale, ws.cu, s));
      else RUN(omk_attention_causal(dt, ws.qkv, ws.ctx, attention_mask, B, (int)L, nh, nkv, scale, ws.kmax, s));
    }
    GEMM_ACC(ws.ctx, A, lw.o_w, A, H, A, lw.o_b);                                                          // x += o_proj(ctx)
    RUN(omk_layernorm_from_f32(dt, (const float*)ws.x, H, ws.y, H, lw.ln2_g, nullptr, M, H, c->ln_eps, 1, s));   // post_attention_layernorm
    GEMM(ws.y, H, lw.ffn1_w, H, ws.ff2, F, F, H, nullptr, nullptr, 0);                                     // gate_proj
    GEMM(ws.y, H, lw.ffn1g_w, H, ws.ff, F, F, H, nullptr, nullptr, 0);                                     // up_proj
    RUN(omk_silu_mul(dt, ws.ff2, ws.ff, M * F, s));                                                        // ff = silu(gate) * up
    GEMM_ACC(ws.ff, F, lw.ffn2_w, F, H, F, nullptr);                                                       // x += down_proj(ff)
  }
  // norm: the hidden states in the compute dtype when asked for; the pooled rows ALWAYS as f32 rows of the normalisation of just the
  // rows pooling reads (the reference's autocast leaves the norm's arithmetic in fp32), as the other stacks do
  const float* fg = w->final_ln_g;
  const float* xf = (const float*)ws.x;
  if (out_hidden) RUN(omk_layernorm_from_f32(dt, xf, H, out_hidden, H, fg, nullptr, M, H, c->ln_eps, 1, s));
  if (c->pooling != OM_POOL_NONE) {
    float* pooled = c->head_in > 0 && w->head_w ? ws.pooled : out_reps;
    if (c->pooling == OM_POOL_FIRST) {
      if (packed) RUN(omk_layernorm_f32out(OM_F32, xf, H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s, nullptr, ws.cls_rows));
      else RUN(omk_layernorm_f32out(OM_F32, xf, L * H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s));
    } else if (c->pooling == OM_POOL_LAST) {
      const dim3 grid((unsigned)((B + 255) / 256));
      if (packed) hipLaunchKernelGGL(last_rows_packed_kernel, grid, dim3(256), 0, s, ws.kmax, ws.cu, B, (int)packed_rows, ws.last_rows);
      else hipLaunchKernelGGL(last_rows_kernel, grid, dim3(256), 0, s, ws.kmax, B, (int)L, ws.last_rows);
      OM_LAUNCH_CHECK();
      RUN(omk_layernorm_f32out(OM_F32, xf, H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s, nullptr, ws.last_rows));
    } else {
      RUN(omk_layernorm_f32out(OM_F32, xf, H, ws.final32, H, fg, nullptr, M, H, c->ln_eps, 1, s));
      RUN(omk_pool(OM_F32, ws.final32, attention_mask, pooled, B, (int)L, H, OM_POOL_MEAN, s, packed ? ws.cu : nullptr));
    }
    RUN(omk_pooled_tail(c, w, pooled, out_reps, B, packed ? ws.cu : nullptr, packed_rows, s));
  }
#undef GEMM_ACC
#undef GEMM
#undef RUN
  return 0;
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
  return carve(&cfg->base, cfg->base.base.head_dim, B, L, nullptr).total;
}

extern "C" int om_causal2_encoder_packed_supported(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || !packed_rows_rule(B, L, packed_rows)) return 0;
  return check_cfg2(cfg) ? 0 : 1;
}

extern "C" size_t om_causal2_encoder_workspace_bytes_packed(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows) {
  if (!cfg || B <= 0 || L <= 0 || packed_rows <= 0 || check_cfg2(cfg)) return 0;
  return carve(&cfg->base, cfg->base.base.head_dim, B, L, nullptr, packed_rows).total;
}

extern "C" int om_causal2_encoder_forward(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                                          const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden,
                                          float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (!cfg || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg2(cfg)) return 1;
  if (cfg->qk_norm && cfg->base.base.n_layers > 0 && !qk_norm_host) OM_FAIL("Qwen3: qk_norm is set but the q / k norm weights are null");
  return causal_forward_impl(&cfg->base, extra_of(cfg, qk_norm_host), w, input_ids, attention_mask, B, L, out_hidden, out_reps, workspace,
                             workspace_bytes, stream, 0);
}

extern "C" int om_causal2_encoder_forward_packed(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                                                 const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L,
                                                 int64_t packed_rows, float* out_reps, void* workspace, size_t workspace_bytes, void* stream) {
  if (packed_rows <= 0) OM_FAIL("packed_rows must be positive");
  if (!cfg || !w || !input_ids || !attention_mask) OM_FAIL("null argument");
  if (check_cfg2(cfg)) return 1;
  if (cfg->qk_norm && cfg->base.base.n_layers > 0 && !qk_norm_host) OM_FAIL("Qwen3: qk_norm is set but the q / k norm weights are null");
  return causal_forward_impl(&cfg->base, extra_of(cfg, qk_norm_host), w, input_ids, attention_mask, B, L, nullptr, out_reps, workspace,
                             workspace_bytes, stream, packed_rows);
}
