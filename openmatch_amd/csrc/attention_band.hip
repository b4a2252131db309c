// ModernBERT's sliding-window attention (HF:models/modernbert/modeling_modernbert.py, gfx950), head_dim 64, inference: the two band
// kernels -- wrappers of the shared chunked bodies (attn_chunked.h) -- and their launch.
//
//   * omk_attention_band: softmax(Q K^T / 8 + mask) V where key k is visible from query q only if |q - k| <= w
//     (masking_utils.sliding_window_bidirectional_overlay: inclusive at both ends) AND k is unmasked.  A workgroup owns
//     128 queries of one (sequence, head) and walks only the keys [qb - w, qb + 127 + w] that its band can reach, clipped to
//     [0, kmax[b]) (keys at or past kmax are padding), in chunks of 128: at 1 024 tokens and w = 64 two chunks instead of eight.
//     Per score the band is a select, not an add (AttnBand, attn_chunked.h).  No bias, dropout or packed rows.
//     16-bit: attention_band16_kernel = attn_chunked16 with the band; float32: attention_band32_kernel = attn_chunked_qreg with it.
//     Launch only: omk_attention (attention.hip) sends a call here when its planner (attn_plan.h) finds 0 < w < L - 1; a window
//     that reaches every key is full attention and never arrives.
//
// ModernBERT's rotary positions (omk_rope) are in attention_causal.hip, next to omk_rope_gqa and the one rotary kernel they share.
#include "attn_chunked.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256, 2) void attention_band16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int H, int heads, float scale, int w,
    const int* __restrict__ kmax) {
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int kend = kmax ? __builtin_amdgcn_readfirstlane(kmax[b]) : L;
  attn_chunked16<T, AttnBand, false, false>(attn_rows_fused(qkv, ctx, b * L, H, h), AttnBand{w}, mask + b * L, L, kend, blockIdx.y * 128, scale, AttnFullArgs{});
}

__global__ __launch_bounds__(256) void attention_band32_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int H, int heads, float scale,
    int w, const int* __restrict__ kmax) {
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  attn_chunked_qreg<float, AttnBand>(attn_rows_fused(qkv, ctx, b * L, H, h), AttnBand{w}, mask + b * L, L, kmax ? kmax[b] : L, blockIdx.y * 128, scale, AttnFullArgs{});
}

}  // namespace

// launch only: attn_plan_fwd (attn_plan.h) has checked the arguments and found 0 < w < L - 1
int omk_attention_band(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int H, int heads, float scale,
                       int w, const int* kmax, hipStream_t s) {
  const dim3 grid((unsigned)(heads * B), (unsigned)((L + 127) / 128));
  if (dtype == OM_F32) {
    const int lds = 128 * AttnGeom<float>::ROWB + 64 * 132 * 4 + 128 * 4 + 128 * 4;
    if (attn_lds_once<attention_band32_kernel>(lds)) return 1;
    hipLaunchKernelGGL(attention_band32_kernel, grid, dim3(256), lds, s, (const float*)qkv, (float*)ctx, mask, L, H, heads, scale, w, kmax);
  } else {
    const int lds = 2 * 128 * 128 + 128 * 4;
    if (dtype == OM_F16)
      hipLaunchKernelGGL(attention_band16_kernel<f16_t>, grid, dim3(256), lds, s, (const f16_t*)qkv, (f16_t*)ctx, mask, L, H, heads, scale, w, kmax);
    else
      hipLaunchKernelGGL(attention_band16_kernel<bf16_t>, grid, dim3(256), lds, s, (const bf16_t*)qkv, (bf16_t*)ctx, mask, L, H, heads, scale, w, kmax);
  }
  OM_LAUNCH_CHECK();
  return 0;
}
