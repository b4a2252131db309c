// Grouped-query attention over heads of 256 columns (gfx950, inference): what EmbeddingGemma's Gemma3TextModel with
// use_bidirectional_attention needs (HF:models/gemma3/modeling_gemma3.py) -- full layers where every unmasked key is visible and
// sliding layers where key k is visible from query q iff |q - k| <= w and k is unmasked.
//
// Launch only: omk_attention_gqa (attention_causal.hip) plans (attn_plan.h attn_plan_gqa) and sends its FULL256 and BAND256 families to
// omk_attention_d256 at the end of this file.
//
//   * Padded rows: softmax(Q K^T * scale + mask) V over the grouped projection [M, (heads + 2 kv_heads) * 256]
//     (q heads | k heads | v heads) into ctx [M, heads * 256]; query head h reads K / V head h / (heads / kv_heads) (HF repeat_kv).
//     The scale is the caller's (Gemma3: query_pre_attn_scalar ** -0.5, a config field of its own).  One workgroup of 256 threads per
//     (sequence, query head, 128-query block) walks 64-key chunks clipped to kmax[b] (keys at or past it are padding); with a band it
//     walks only the keys [qb - w, qb + 127 + w] its queries can reach.  0 < w < L - 1 is the band (AttnBand), anything else full
//     attention (AttnFull): a window that reaches every key never takes the band kernel, so the two give the same bits there.
//     The bodies are attn_chunked_wide.h at D = 256; 16-bit x {full, band} per format, float32 x {full, band}.
//     A wave of either body holds more than 256 registers (no __launch_bounds__ second argument): one workgroup per CU.
//
//   * The same over PACKED rows, under the contract of attention_causal16_d128_packed_kernel: sequence b
//     is rows cu[b] .. cu[b + 1] - 1 of qkv and ctx, the body's L and key extent are the sequence's own row count Lb, the mask row keeps
//     the padded pitch (mask + b * L: masked tokens inside an extent stay masked).  The grid is the padded launch's; a workgroup whose
//     query block starts at or past Lb returns before its first barrier, and row loads stay clamped to Lb - 1, so the last sequence
//     reads nothing past the buffer.  Band or full is decided on the PADDED L, as above: the packed launch runs the body the padded
//     launch of the same batch runs and agrees with it bit for bit on every row up to each extent.  Thin wrappers over the same two
//     bodies: six more kernels with the padded ones' register counts and no scratch.
#include "attn_chunked_wide.h"
#include "attn_plan.h"

namespace {

// The wrappers: what they do is written once in attn_chunked_wide.h (attn_grouped_padded / attn_grouped_packed).
template <typename T, typename Policy>
__global__ __launch_bounds__(256) void attention_d256_16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale, Policy pol,
    const int* __restrict__ kmax) {
  attn_grouped_padded<256>(qkv, ctx, mask, L, heads, kv_heads, scale, pol, kmax);
}

template <typename Policy>
__global__ __launch_bounds__(256) void attention_d256_32_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale, Policy pol,
    const int* __restrict__ kmax) {
  attn_grouped_padded<256>(qkv, ctx, mask, L, heads, kv_heads, scale, pol, kmax);
}

// Packed rows: a query block at or past its sequence's end leaves before it touches LDS or memory.
template <typename T, typename Policy>
__global__ __launch_bounds__(256) void attention_d256_16_packed_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale, Policy pol,
    const int* __restrict__ cu) {
  attn_grouped_packed<256>(qkv, ctx, mask, Lp, heads, kv_heads, scale, pol, cu);
}

template <typename Policy>
__global__ __launch_bounds__(256) void attention_d256_32_packed_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale, Policy pol,
    const int* __restrict__ cu) {
  attn_grouped_packed<256>(qkv, ctx, mask, Lp, heads, kv_heads, scale, pol, cu);
}

// one policy's kernels in the plan's body; ext: kmax [B] (padded rows) or cu [B + 1] (PACKED rows)
template <typename Policy>
int launch_policy(const AttnGqaPlan& p, int dtype, bool packed, const void* qkv, void* ctx, const int64_t* mask, int L, int heads, int kv_heads,
                  float scale, Policy pol, const int* ext, hipStream_t s) {
  static_assert(attn_gqa_lds(256, true) == AttnWide<256>::LDS32 && attn_gqa_lds(256, false) == AttnWide<256>::LDS16, "the plan's LDS bytes are these kernels'");
  const dim3 grid(p.grid_x, p.grid_y);
  if (p.f32)
    return attn_launch_form<attention_d256_32_kernel<Policy>, attention_d256_32_packed_kernel<Policy>, float>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads,
                                                                                                                scale, pol, ext);
  return attn_with_type16(dtype, [&](auto t) {
    typedef decltype(t) T;
    return attn_launch_form<attention_d256_16_kernel<T, Policy>, attention_d256_16_packed_kernel<T, Policy>, T>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads,
                                                                                                                  scale, pol, ext);
  });
}

}  // namespace

// launch only: attn_plan_gqa (attn_plan.h) has checked the arguments and chosen band or full, the body, the grid and the LDS bytes --
// all from the PADDED L, so a packed launch runs what the padded launch of the batch runs
int omk_attention_d256(const AttnGqaPlan& p, int dtype, bool packed, const void* qkv, void* ctx, const int64_t* mask, int L, int heads,
                       int kv_heads, float scale, int w, const int* ext, hipStream_t s) {
  if (p.family == OM_ATTN_GQA_FAMILY_BAND256) return launch_policy(p, dtype, packed, qkv, ctx, mask, L, heads, kv_heads, scale, AttnBand{w}, ext, s);
  return launch_policy(p, dtype, packed, qkv, ctx, mask, L, heads, kv_heads, scale, AttnFull{}, ext, s);
}
