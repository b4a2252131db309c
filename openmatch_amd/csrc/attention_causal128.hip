// What a Qwen3 embedder (HF:models/qwen3/modeling_qwen3.py) adds to the decoder-only stack of attention_causal.hip (gfx950, inference):
//
//   * omk_attention_causal128, the launcher of omk_attention_gqa's CAUSAL128 family (attention_causal.hip; launch only): causal
//     grouped-query attention over heads of 128 columns.  The projection rows are
//     [M, (heads + 2 kv_heads) * 128] (q heads | k heads | v heads), ctx rows [M, heads * 128].  Grid, policy (AttnCausal), key
//     extents and the packed form are those of the 64-wide kernels: one workgroup of 256 threads per (sequence, query head,
//     128-query block) walking 128-key chunks up to the diagonal chunk, clipped to kmax[b] or the packed extent.  The bodies are
//     attn_chunked_wide.h at D = 128.
//
//   * omk_qknorm_rope: the per-head RMSNorm of q and k (Qwen3Attention.forward: q_norm(q_proj(x).view(.., head_dim)), k_norm alike)
//     and the rotary positions in ONE pass over the q and k columns, for head_dim 64 or 128, norm or no norm (a NULL weight vector:
//     that side is rotated only).  The v heads are never touched.  D / 8 lanes own one head of one row: lane j holds the four pairs
//     (4j .. 4j + 3, D/2 + 4j .. D/2 + 4j + 3), so each rotation stays inside a lane and the sum of squares is a shuffle reduction
//     inside the group (16 lanes at D = 128).  In f32: ss = sum x^2; r = 1 / sqrt(ss / D + eps); n = x * r; y = n * g; then
//     y' = y cos + rotate_half(y) sin with products and sum kept apart as rope_rotate4 does, rounded once on store.
//     Rounding points of HF in the 16-bit formats (the reference's autocast: q_proj's output is 16-bit, the norm weight and the
//     cos / sin tables are f32): Qwen3RMSNorm casts x * rsqrt(..) back to the input dtype BEFORE the weight multiply -- reproduced
//     by one convert of n to the storage format and back; the weight multiply and the rotation then run in f32 as they do there (an
//     f32 weight times a 16-bit tensor promotes), and the stored value is rounded once, where HF rounds when the attention
//     contraction casts its operands.  Not reproduced: a model held in 16-bit outright (weights cast by .to(dtype)), where the weight
//     multiply and each product of the rotation round to 16 bits as well.
//     cos / sin come from omk_rope_table's device table of D / 2 columns per position.
//     Gemma3 (gemma = 1, head_dim 256, 32 lanes per head): Gemma3RMSNorm multiplies the f32 normalised value by (1 + weight) and
//     casts once at the end, so that mode has no rounding between the two multiplies and takes g = 1 + w from the host.
#include "attn_chunked_wide.h"
#include "attn_plan.h"

namespace {

// The wrappers: what they do is written once in attn_chunked_wide.h (attn_grouped_padded / attn_grouped_packed).
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_causal16_d128_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  attn_grouped_padded<128>(qkv, ctx, mask, L, heads, kv_heads, scale, AttnCausal{}, kmax);
}

__global__ __launch_bounds__(256) void attention_causal32_d128_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  attn_grouped_padded<128>(qkv, ctx, mask, L, heads, kv_heads, scale, AttnCausal{}, kmax);
}

// Packed rows: a query block at or past its sequence's end leaves before it touches LDS or memory.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_causal16_d128_packed_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale,
    const int* __restrict__ cu) {
  attn_grouped_packed<128>(qkv, ctx, mask, Lp, heads, kv_heads, scale, AttnCausal{}, cu);
}

__global__ __launch_bounds__(256) void attention_causal32_d128_packed_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale,
    const int* __restrict__ cu) {
  attn_grouped_packed<128>(qkv, ctx, mask, Lp, heads, kv_heads, scale, AttnCausal{}, cu);
}

// ---- q / k RMSNorm + rotary positions ---------------------------------------------------------------------------------------
// one thread: the pairs (i0 .. i0 + 3, D/2 + i0 .. D/2 + i0 + 3) of one q or k head of one row; D / 8 consecutive lanes: the head.
// row_map != NULL (packed rows): the position of row t is row_map[t] % L, rows with row_map[t] < 0 are left as they are.  A group is
// wholly inside or wholly outside the launch and the row test is the same for all of its lanes, so the shuffles below meet live lanes.
// RAW (Gemma3RMSNorm: (x.float() * rsqrt(..)) * (1.0 + weight.float()), cast once at the end): the normalised value is NOT rounded to
// the storage format before the weight multiply, and g is the host's 1 + w.  D = 256 (32 lanes per head) exists in this mode only.
template <typename T, int D, bool RAW = false>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(T* __restrict__ qkv, const float2* __restrict__ tab, int64_t M, int L, int heads,
                                                          int rot_heads, int pitch, const float* __restrict__ qg, const float* __restrict__ kg,
                                                          float eps, const int* __restrict__ row_map) {
  constexpr int G = D / 8;                                  // lanes per head
  const int per_row = rot_heads * G;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t row = idx / per_row;
  const int j = (int)(idx % per_row);
  const int seg = j / G, i0 = (j % G) * 4;                  // seg: head (q heads, then k heads); i0: first of four pairs
  int pos = (int)(row % L);
  if (row_map) {
    const int tok = row_map[row];
    if (tok < 0) return;
    pos = tok % L;
  }
  T* const p = qkv + row * (int64_t)pitch + (int64_t)seg * D + i0;
  float a[4], b[4];
  Vec4IO<T>::load4(p, a);
  Vec4IO<T>::load4(p + D / 2, b);
  const float* const g = seg < heads ? qg : kg;
  if (g) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += a[e] * a[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += b[e] * b[e];
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) ss += __shfl_xor(ss, m, G);
    const float r = 1.0f / sqrtf(ss * (1.0f / D) + eps);    // rsqrt(mean + eps)
    const float4 ga = *(const float4*)(g + i0), gb = *(const float4*)(g + D / 2 + i0);
    const float wa[4] = {ga.x, ga.y, ga.z, ga.w}, wb[4] = {gb.x, gb.y, gb.z, gb.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (RAW) {
        a[e] = __fmul_rn(__fmul_rn(a[e], r), wa[e]);
        b[e] = __fmul_rn(__fmul_rn(b[e], r), wb[e]);
      } else {
        a[e] = __fmul_rn(Vec4IO<T>::round(__fmul_rn(a[e], r)), wa[e]);
        b[e] = __fmul_rn(Vec4IO<T>::round(__fmul_rn(b[e], r)), wb[e]);
      }
    }
  }
  const float2* const t = tab + (size_t)pos * (D / 2) + i0;
  float ra[4], rb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float2 cs = t[e];
    ra[e] = __fadd_rn(__fmul_rn(a[e], cs.x), __fmul_rn(-b[e], cs.y));
    rb[e] = __fadd_rn(__fmul_rn(b[e], cs.x), __fmul_rn(a[e], cs.y));
  }
  Vec4IO<T>::store4(p, ra);
  Vec4IO<T>::store4(p + D / 2, rb);
}

template <typename T>
void qknorm_rope_launch_as(T* qkv, const float2* tab, int64_t M, int L, int heads, int kv_heads, int D, const float* qg, const float* kg, float eps,
                           const int* row_map, hipStream_t s) {
  const int rot = heads + kv_heads, pitch = (heads + 2 * kv_heads) * D;
  const unsigned grid = (unsigned)((M * rot * (D / 8) + 255) / 256);
  if (D == 256) hipLaunchKernelGGL((qknorm_rope_kernel<T, 256, true>), dim3(grid), dim3(256), 0, s, qkv, tab, M, L, heads, rot, pitch, qg, kg, eps, row_map);
  else if (D == 128) hipLaunchKernelGGL((qknorm_rope_kernel<T, 128>), dim3(grid), dim3(256), 0, s, qkv, tab, M, L, heads, rot, pitch, qg, kg, eps, row_map);
  else hipLaunchKernelGGL((qknorm_rope_kernel<T, 64>), dim3(grid), dim3(256), 0, s, qkv, tab, M, L, heads, rot, pitch, qg, kg, eps, row_map);
}

int check_gqa_d(int heads, int kv_heads, int head_dim) {
  if (heads < 1 || kv_heads < 1 || heads % kv_heads) OM_FAIL("grouped heads: n_kv_heads must be at least 1 and divide n_heads");
  if (head_dim != 64 && head_dim != 128) OM_FAIL("grouped heads: head_dim must be 64 or 128");
  return 0;
}

}  // namespace

int omk_qknorm_rope(int dtype, void* qkv, int64_t M, int L, int heads, int kv_heads, int head_dim, const float* q_norm_g, const float* k_norm_g,
                    float eps, const float* inv_freq_host, float scaling, hipStream_t s, const int* row_map, int gemma) {
  if (M <= 0) return 0;
  if (L < 1 || L > 1024) OM_FAIL("rotary positions: sequence length must be in [1,1024]");
  // head_dim 256 is Gemma3's: its norm is not rounded before the weight multiply, and that instantiation alone exists at 256
  if (gemma ? (head_dim != 256 || !q_norm_g || !k_norm_g) : head_dim == 256)
    OM_FAIL("q / k norm and rotary positions: head_dim 256 with both norm weights is the Gemma3 form, and the Gemma3 form is head_dim 256 only");
  if (check_gqa_d(heads, kv_heads, gemma ? 128 : head_dim)) return 1;
  if (!inv_freq_host) OM_FAIL("rotary positions: a frequency table of head_dim / 2 values");
  if (M * (heads + kv_heads) * (head_dim / 8) > 0x7fffffffLL * 256) OM_FAIL("q / k norm and rotary positions: too many rows for one launch");
  const float2* tab = nullptr;
  if (omk_rope_table(inv_freq_host, head_dim / 2, scaling, &tab)) return 1;
  if (dtype == OM_BF16) qknorm_rope_launch_as((bf16_t*)qkv, tab, M, L, heads, kv_heads, head_dim, q_norm_g, k_norm_g, eps, row_map, s);
  else if (dtype == OM_F16) qknorm_rope_launch_as((f16_t*)qkv, tab, M, L, heads, kv_heads, head_dim, q_norm_g, k_norm_g, eps, row_map, s);
  else qknorm_rope_launch_as((float*)qkv, tab, M, L, heads, kv_heads, head_dim, q_norm_g, k_norm_g, eps, row_map, s);
  OM_LAUNCH_CHECK();
  return 0;
}

// launch only: attn_plan_gqa (attn_plan.h) has checked the arguments and chosen the body, the grid and the LDS bytes; ext: kmax [B]
// (padded rows) or cu [B + 1] (packed rows)
int omk_attention_causal128(const AttnGqaPlan& p, int dtype, bool packed, const void* qkv, void* ctx, const int64_t* mask, int L, int heads,
                            int kv_heads, float scale, const int* ext, hipStream_t s) {
  static_assert(attn_gqa_lds(128, true) == AttnWide<128>::LDS32 && attn_gqa_lds(128, false) == AttnWide<128>::LDS16, "the plan's LDS bytes are these kernels'");
  const dim3 grid(p.grid_x, p.grid_y);
  if (p.f32)
    return attn_launch_form<attention_causal32_d128_kernel, attention_causal32_d128_packed_kernel, float>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads,
                                                                                                            scale, ext);
  return attn_with_type16(dtype, [&](auto t) {
    typedef decltype(t) T;
    return attn_launch_form<attention_causal16_d128_kernel<T>, attention_causal16_d128_packed_kernel<T>, T>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads,
                                                                                                              scale, ext);
  });
}

// Test hooks (tests/test_qwen3_kernels.py, tests/test_gemma3_kernels.py, tools/causal_lm_bench.py): the norm-and-rotation pass alone.
extern "C" int om_debug_qknorm_rope(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, int head_dim, const float* q_norm_g,
                                    const float* k_norm_g, float eps, const float* inv_freq, float scaling, void* stream) {
  if (!qkv || !inv_freq) OM_FAIL("null argument");
  if (debug_dtype(dtype)) return 1;
  return omk_qknorm_rope(dtype, qkv, M, L, n_heads, n_kv_heads, head_dim, q_norm_g, k_norm_g, eps, inv_freq, scaling, (hipStream_t)stream, nullptr);
}

extern "C" int om_debug_qknorm_rope_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, int head_dim, const float* q_norm_g,
                                         const float* k_norm_g, float eps, const float* inv_freq, float scaling, const int* row_map, void* stream) {
  if (!qkv || !inv_freq || !row_map) OM_FAIL("null argument");
  if (debug_dtype(dtype)) return 1;
  return omk_qknorm_rope(dtype, qkv, rows, L, n_heads, n_kv_heads, head_dim, q_norm_g, k_norm_g, eps, inv_freq, scaling, (hipStream_t)stream, row_map);
}

// Gemma3's form alone (tests/test_gemma3_kernels.py): head_dim 256, g = 1 + w from the caller, no rounding before the weight multiply
extern "C" int om_debug_qknorm_rope_d256(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, const float* q_norm_g,
                                         const float* k_norm_g, float eps, const float* inv_freq, float scaling, void* stream) {
  if (!qkv || !inv_freq || !q_norm_g || !k_norm_g) OM_FAIL("null argument");
  if (debug_dtype(dtype)) return 1;
  return omk_qknorm_rope(dtype, qkv, M, L, n_heads, n_kv_heads, 256, q_norm_g, k_norm_g, eps, inv_freq, scaling, (hipStream_t)stream, nullptr, 1);
}

// the same over packed rows (tests/test_gemma3_packed_kernels.py): the position of row t is row_map[t] % L, rows with row_map[t] < 0 are
// left as they are
extern "C" int om_debug_qknorm_rope_d256_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, const float* q_norm_g,
                                              const float* k_norm_g, float eps, const float* inv_freq, float scaling, const int* row_map,
                                              void* stream) {
  if (!qkv || !inv_freq || !q_norm_g || !k_norm_g || !row_map) OM_FAIL("null argument");
  if (debug_dtype(dtype)) return 1;
  return omk_qknorm_rope(dtype, qkv, rows, L, n_heads, n_kv_heads, 256, q_norm_g, k_norm_g, eps, inv_freq, scaling, (hipStream_t)stream, row_map, 1);
}
