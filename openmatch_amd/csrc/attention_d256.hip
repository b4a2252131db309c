// Grouped-query attention over heads of 256 columns (gfx950, inference): what EmbeddingGemma's Gemma3TextModel with
// use_bidirectional_attention needs (HF:models/gemma3/modeling_gemma3.py) -- full layers where every unmasked key is visible and
// sliding layers where key k is visible from query q iff |q - k| <= w and k is unmasked.
//
//   * omk_attention_gqa_d256: softmax(Q K^T * scale + mask) V over the grouped projection [M, (heads + 2 kv_heads) * 256]
//     (q heads | k heads | v heads) into ctx [M, heads * 256]; query head h reads K / V head h / (heads / kv_heads) (HF repeat_kv).
//     The scale is the caller's (Gemma3: query_pre_attn_scalar ** -0.5, a config field of its own).  One workgroup of 256 threads per
//     (sequence, query head, 128-query block) walks 64-key chunks clipped to kmax[b] (keys at or past it are padding); with a band it
//     walks only the keys [qb - w, qb + 127 + w] its queries can reach.  0 < w < L - 1 is the band (AttnBand), anything else full
//     attention (AttnFull): a window that reaches every key never takes the band kernel, so the two give the same bits there.
//     The bodies are attn_chunked_wide.h at D = 256; 16-bit x {full, band} per format, float32 x {full, band}.
//     A wave of either body holds more than 256 registers (no __launch_bounds__ second argument): one workgroup per CU.
//
//   * omk_attention_gqa_d256_packed: the same over PACKED rows, under the contract of attention_causal16_d128_packed_kernel: sequence b
//     is rows cu[b] .. cu[b + 1] - 1 of qkv and ctx, the body's L and key extent are the sequence's own row count Lb, the mask row keeps
//     the padded pitch (mask + b * L: masked tokens inside an extent stay masked).  The grid is the padded launch's; a workgroup whose
//     query block starts at or past Lb returns before its first barrier, and row loads stay clamped to Lb - 1, so the last sequence
//     reads nothing past the buffer.  Band or full is decided on the PADDED L, as above: the packed launch runs the body the padded
//     launch of the same batch runs and agrees with it bit for bit on every row up to each extent.  Thin wrappers over the same two
//     bodies: six more kernels with the padded ones' register counts and no scratch.
#include "attn_chunked_wide.h"

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

// ext: kmax [B] (padded rows) or cu [B + 1] (PACKED rows); every dtype code but the two 16-bit ones counts as float32
template <typename Policy>
int launch_policy(int dtype, const void* qkv, void* ctx, const int64_t* mask, dim3 grid, int L, int heads, int kv_heads, float scale, Policy pol,
                  const int* ext, bool packed, hipStream_t s) {
  return attn_with_type(dtype, [&](auto t) {
    typedef decltype(t) T;
    if constexpr (std::is_same<T, float>::value)
      return attn_launch_form<attention_d256_32_kernel<Policy>, attention_d256_32_packed_kernel<Policy>, float>(packed, grid, AttnWide<256>::LDS32, s, qkv, ctx, mask, L,
                                                                                                                  heads, kv_heads, scale, pol, ext);
    else
      return attn_launch_form<attention_d256_16_kernel<T, Policy>, attention_d256_16_packed_kernel<T, Policy>, T>(packed, grid, AttnWide<256>::LDS16, s, qkv, ctx, mask, L,
                                                                                                                    heads, kv_heads, scale, pol, ext);
  });
}

int check_args(int64_t B, int L, int heads, int kv_heads) {
  if (L < 1 || L > 1024) OM_FAIL("attention (head_dim 256): sequence length must be in [1,1024]");
  if (heads < 1 || kv_heads < 1 || heads % kv_heads) OM_FAIL("grouped heads: n_kv_heads must be at least 1 and divide n_heads");
  if (B * heads > 0x7fffffffLL) OM_FAIL("attention (head_dim 256): batch too large for one launch");
  // the LDS-DMA addresses a sequence's K / V rows with a 32-bit byte offset from its first row
  if ((int64_t)L * (heads + 2 * kv_heads) * 512 > 0x7fffffffLL) OM_FAIL("attention (head_dim 256): too many heads for one sequence's 32-bit row offsets");
  return 0;
}

// both forms: the grid and the choice of body come from the PADDED L, so a packed launch runs what the padded launch of the batch runs
int attention_gqa_d256_launch(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int heads, int kv_heads, float scale,
                              int w, const int* ext, bool packed, hipStream_t s) {
  if (B <= 0) return 0;
  if (check_args(B, L, heads, kv_heads)) return 1;
  const dim3 grid((unsigned)(heads * B), (unsigned)((L + 127) / 128));
  int rc;
  if (w > 0 && w < L - 1) rc = launch_policy(dtype, qkv, ctx, mask, grid, L, heads, kv_heads, scale, AttnBand{w}, ext, packed, s);
  else rc = launch_policy(dtype, qkv, ctx, mask, grid, L, heads, kv_heads, scale, AttnFull{}, ext, packed, s);
  if (rc) return 1;
  OM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int omk_attention_gqa_d256(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int heads, int kv_heads, float scale, int w,
                           const int* kmax, hipStream_t s) {
  return attention_gqa_d256_launch(dtype, qkv, ctx, mask, B, L, heads, kv_heads, scale, w, kmax, false, s);
}

int omk_attention_gqa_d256_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int heads, int kv_heads, float scale,
                                  int w, const int* cu, hipStream_t s) {
  if (B > 0 && !cu) OM_FAIL("attention (head_dim 256) over packed rows: the sequence offsets cu");
  return attention_gqa_d256_launch(dtype, qkv, ctx, mask, B, L, heads, kv_heads, scale, w, cu, true, s);
}

// Test hook (tests/test_gemma3_kernels.py, tools/gemma3_bench.py): the kernels alone; the key extents go into the grow-only device
// buffer the causal hooks keep per device (omk_causal_debug_kmax)
extern "C" int om_debug_attention_gqa_d256(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads,
                                           int n_kv_heads, float scale, int w, void* stream) {
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  if (B <= 0) return 0;
  if (check_args(B, L, n_heads, n_kv_heads)) return 1;
  hipStream_t s = (hipStream_t)stream;
  int* kmax = nullptr;
  if (omk_causal_debug_kmax(B, &kmax)) return 1;
  if (omk_mask_extent(mask, B, L, kmax, s)) return 1;
  return omk_attention_gqa_d256(dtype, qkv, ctx, mask, B, L, n_heads, n_kv_heads, scale, w, kmax, s);
}

// the packed kernels alone (tests/test_gemma3_packed_kernels.py, tools/gemma3_bench.py): cu [B + 1] as om_debug_pack_rows writes it
extern "C" int om_debug_attention_gqa_d256_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L,
                                                  int n_heads, int n_kv_heads, float scale, int w, void* stream) {
  if (!qkv || !ctx || !mask || !cu) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  return omk_attention_gqa_d256_packed(dtype, qkv, ctx, mask, B, L, n_heads, n_kv_heads, scale, w, cu, (hipStream_t)stream);
}
