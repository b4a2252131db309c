// Causal grouped-query attention of the decoder-only backbones (HF:models/llama/modeling_llama.py, HF:models/qwen2/modeling_qwen2.py),
// and the rotary positions of every backbone that has them (gfx950), head_dim 64, inference.  Here: the two causal kernels -- wrappers of
// the shared chunked bodies (attn_chunked.h) -- and their launcher, the ONE rotary kernel with its table cache and both of its entries,
// omk_rope (ModernBERT and NomicBERT, fused [M, 3H]) and omk_rope_gqa (grouped projection), and, at the end, the one grouped-query
// attention entry of all three head widths, omk_attention_gqa -- plan (attn_plan.h attn_plan_gqa), switch on the family, launch -- with
// the test hooks of all three (the 128- and 256-wide kernels and their launchers: attention_causal128.hip, attention_d256.hip).
//
//   * Rotary positions applied IN PLACE to the q and k heads of a projection whose rows hold (q heads | k heads | v heads) of 64
//     columns (apply_rotary_pos_emb with rotate_half: pairs (i, i + 32) of each head, position = row % L as HF's arange(L) whatever
//     the padding); the kernel takes the number of rotated heads and the row pitch, so the fused projection is the grouped one with
//     2H / 64 rotated heads and pitch 3H.  cos / sin come from a device table per (device, 32 frequencies, scaling) of 1 024
//     positions, built once as LlamaRotaryEmbedding.forward does in f32 (inv_freq * pos, then cos * attention_scaling,
//     sin * attention_scaling); every L reads a prefix of it.  omk_rope_gqa takes the HOST's frequencies -- the module's own
//     rotary_emb.inv_freq buffer -- so `default`, `linear` and `llama3` rope need no rule restated here; omk_rope computes them from
//     theta as ModernBertRotaryEmbedding does in f32 (inv_freq = 1 / theta ** (2i / 64)) with scaling 1.
//     The rotation is one separate pass (read + write of the q and k columns per row) rather than folded into the attention kernels'
//     K / Q loads: K reaches LDS by DMA there, untouched by the vector unit, so a fused rotation would have to rewrite K in LDS once
//     per (query block, key chunk) -- see DESIGN.md for the measured cost of the pass.
//
//   * The causal kernels (omk_attention_causal64; launch only): softmax(Q K^T * scale + mask) V where key k is visible from query q iff k <= q and k is unmasked;
//     query head h reads K / V head h / (n_heads / n_kv) (HF repeat_kv).  One workgroup owns 128 queries of one (sequence, query
//     head) and walks the 128-key chunks from key 0 up to its own diagonal chunk (clipped to kmax[b]: keys at or past it are
//     padding): at 1 024 tokens 4.5 chunks per block on average instead of eight.  The triangle is a select per score in the
//     diagonal chunk only (AttnCausal, attn_chunked.h).  16-bit: attention_causal16_kernel = attn_chunked16 with the triangle;
//     float32: attention_causal32_kernel = attn_chunked_qreg with it.  Every query head fetches its group's K / V chunks itself
//     (one workgroup per (sequence, query head, query block)); a form that serves a whole K / V group from one fetch has not been
//     built or measured.
//
//   * Packed rows (om_causal_encoder_forward_packed): the packed kernels run the same two bodies with an AttnRows filled
//     from cu -- sequence b is rows cu[b] .. cu[b + 1] - 1, the body's L is that row count, the mask keeps its [B, L] pitch -- and
//     omk_rope_gqa with a row_map takes a row's position from row_map[t] % L (the column omk_pack_rows recorded) instead of row % L.
//     omk_rope takes the same row_map (NomicBERT under om_encoder_forward_packed).
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "attn_chunked_wide.h"
#include "attn_plan.h"

#define RUN(expr) do { if (expr) return 1; } while (0)

namespace {

constexpr int kRopeMaxPos = 1024;

}  // namespace

// [kRopeMaxPos][n] (cos, sin) * scaling for one frequency vector of n values (32: head_dim 64, 64: head_dim 128), resident on the
// device: built and uploaded ONCE per (device, frequencies, scaling) -- the vector's length is part of the key
int omk_rope_table(const float* inv_freq, int n, float scaling, const float2** out) {
  static std::mutex mu;
  static std::map<std::tuple<int, std::vector<float>, float>, float2*> cache;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto key = std::make_tuple(dev, std::vector<float>(inv_freq, inv_freq + n), scaling);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::vector<float2> tab((size_t)kRopeMaxPos * n);
    for (int i = 0; i < n; ++i)
      for (int pos = 0; pos < kRopeMaxPos; ++pos) {
        const float f = inv_freq[i] * (float)pos;                            // inv_freq @ position_ids, f32
        const float c = (float)cos((double)f), sn = (float)sin((double)f);  // emb.cos(), emb.sin(), f32
        tab[(size_t)pos * n + i] = make_float2(c * scaling, sn * scaling);   // * attention_scaling, f32
      }
    float2* d = nullptr;
    OM_HIP(hipMalloc(&d, tab.size() * sizeof(float2)));
    OM_HIP(hipMemcpy(d, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
    it = cache.emplace(key, d).first;
  }
  *out = it->second;
  return 0;
}

namespace {

// one thread: four consecutive pairs (i .. i + 3, i + 32 .. i + 35) of one q or k head of one row; the v heads are never touched.
// q' = q cos + rotate_half(q) sin in f32 (HF: q.float() * cos + rotate_half(q.float()) * sin), rounded once; products and sum kept apart
// (no fused multiply-add) as torch evaluates them.  p: this thread's first element; t: its position's first (cos, sin).
template <typename T>
__device__ __forceinline__ void rope_rotate4(T* p, const float2* t) {
  float a[4], b[4];
  Vec4IO<T>::load4(p, a);
  Vec4IO<T>::load4(p + 32, b);
  float ra[4], rb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float2 cs = t[e];
    ra[e] = __fadd_rn(__fmul_rn(a[e], cs.x), __fmul_rn(-b[e], cs.y));
    rb[e] = __fadd_rn(__fmul_rn(b[e], cs.x), __fmul_rn(a[e], cs.y));
  }
  Vec4IO<T>::store4(p, ra);
  Vec4IO<T>::store4(p + 32, rb);
}

template <typename T>
__global__ __launch_bounds__(256) void rope_gqa_kernel(T* __restrict__ qkv, const float2* __restrict__ tab, int64_t M, int L, int rot_heads,
                                                       int pitch) {
  const int per_row = rot_heads * 8;                       // 8 threads per rotated head
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t row = idx / per_row;
  const int j = (int)(idx % per_row);
  const int seg = j / 8, i0 = (j % 8) * 4;                 // seg: head (q heads, then k heads); i0: first of four pairs
  const int pos = (int)(row % L);
  rope_rotate4(qkv + row * (int64_t)pitch + (int64_t)seg * 64 + i0, tab + (size_t)pos * 32 + i0);
}

// packed rows: row t holds token row_map[t] = b * L + column, so its position is row_map[t] % L; row_map[t] < 0 is a tail row, left
// as it is
template <typename T>
__global__ __launch_bounds__(256) void rope_gqa_rows_kernel(T* __restrict__ qkv, const float2* __restrict__ tab, int64_t M, int L, int rot_heads,
                                                            int pitch, const int* __restrict__ row_map) {
  const int per_row = rot_heads * 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t row = idx / per_row;
  const int j = (int)(idx % per_row);
  const int seg = j / 8, i0 = (j % 8) * 4;
  const int tok = row_map[row];
  if (tok < 0) return;
  rope_rotate4(qkv + row * (int64_t)pitch + (int64_t)seg * 64 + i0, tab + (size_t)(tok % L) * 32 + i0);
}

// The wrappers: what they do is written once in attn_chunked_wide.h (attn_grouped_padded / attn_grouped_packed).
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_causal16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  attn_grouped_padded<64>(qkv, ctx, mask, L, heads, kv_heads, scale, AttnCausal{}, kmax);
}

__global__ __launch_bounds__(256) void attention_causal32_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  attn_grouped_padded<64>(qkv, ctx, mask, L, heads, kv_heads, scale, AttnCausal{}, kmax);
}

// Packed rows: a query block at or past its sequence's end leaves before it touches LDS or memory.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_causal16_packed_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale,
    const int* __restrict__ cu) {
  attn_grouped_packed<64>(qkv, ctx, mask, Lp, heads, kv_heads, scale, AttnCausal{}, cu);
}

__global__ __launch_bounds__(256) void attention_causal32_packed_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int Lp, int heads, int kv_heads, float scale,
    const int* __restrict__ cu) {
  attn_grouped_packed<64>(qkv, ctx, mask, Lp, heads, kv_heads, scale, AttnCausal{}, cu);
}

}  // namespace

// launch only: attn_plan_gqa (attn_plan.h) has checked the arguments and chosen the body, the grid and the LDS bytes; ext: kmax [B]
// (padded rows) or cu [B + 1] (packed rows)
int omk_attention_causal64(const AttnGqaPlan& p, int dtype, bool packed, const void* qkv, void* ctx, const int64_t* mask, int L, int heads,
                           int kv_heads, float scale, const int* ext, hipStream_t s) {
  static_assert(attn_gqa_lds(64, true) == 128 * AttnGeom<float>::ROWB + 64 * 132 * 4 + 128 * 4 + 128 * 4 && attn_gqa_lds(64, false) == 2 * 128 * 128 + 128 * 4,
                "the plan's LDS bytes are these kernels'");
  const dim3 grid(p.grid_x, p.grid_y);
  if (p.f32) return attn_launch_form<attention_causal32_kernel, attention_causal32_packed_kernel, float>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads, scale, ext);
  return attn_with_type16(dtype, [&](auto t) {
    typedef decltype(t) T;
    return attn_launch_form<attention_causal16_kernel<T>, attention_causal16_packed_kernel<T>, T>(packed, grid, p.lds, s, qkv, ctx, mask, L, heads, kv_heads, scale, ext);
  });
}

// rot_heads rotated heads at the start of each row of `pitch` elements
template <typename T>
static void rope_launch_as(T* qkv, const float2* tab, int64_t M, int L, int rot_heads, int pitch, const int* row_map, hipStream_t s) {
  const unsigned grid = (unsigned)((M * rot_heads * 8 + 255) / 256);
  if (row_map) hipLaunchKernelGGL(rope_gqa_rows_kernel<T>, dim3(grid), dim3(256), 0, s, qkv, tab, M, L, rot_heads, pitch, row_map);
  else hipLaunchKernelGGL(rope_gqa_kernel<T>, dim3(grid), dim3(256), 0, s, qkv, tab, M, L, rot_heads, pitch);
}

static int rope_launch(int dtype, void* qkv, int64_t M, int L, int rot_heads, int pitch, const float* inv_freq_host, float scaling, hipStream_t s,
                       const int* row_map = nullptr) {
  const float2* tab = nullptr;
  if (omk_rope_table(inv_freq_host, 32, scaling, &tab)) return 1;
  if (dtype == OM_BF16) rope_launch_as((bf16_t*)qkv, tab, M, L, rot_heads, pitch, row_map, s);
  else if (dtype == OM_F16) rope_launch_as((f16_t*)qkv, tab, M, L, rot_heads, pitch, row_map, s);
  else rope_launch_as((float*)qkv, tab, M, L, rot_heads, pitch, row_map, s);
  OM_LAUNCH_CHECK();
  return 0;
}

int omk_rope(int dtype, void* qkv, int64_t M, int L, int H, float theta, hipStream_t s, const int* row_map) {
  if (M <= 0) return 0;
  if (L < 1 || L > kRopeMaxPos) OM_FAIL("rotary positions: sequence length must be in [1,1024]");
  if (H % 64 || !(theta > 0.f)) OM_FAIL("rotary positions: head_dim 64 and a positive theta");
  float inv_freq[32];
  for (int i = 0; i < 32; ++i) {
    const float e = (float)(2 * i) / 64.0f;                                  // arange(0, d, 2) / d, f32 (exact)
    const float p = (float)pow((double)theta, (double)e);                   // theta ** e, rounded to f32
    inv_freq[i] = 1.0f / p;                                                  // 1.0 / (...), f32
  }
  return rope_launch(dtype, qkv, M, L, 2 * H / 64, 3 * H, inv_freq, 1.0f, s, row_map);
}

int omk_rope_gqa(int dtype, void* qkv, int64_t M, int L, int heads, int kv_heads, const float* inv_freq_host, float scaling, hipStream_t s,
                 const int* row_map) {
  if (M <= 0) return 0;
  if (L < 1 || L > kRopeMaxPos) OM_FAIL("rotary positions: sequence length must be in [1,1024]");
  if (heads < 1 || kv_heads < 1 || heads % kv_heads) OM_FAIL("grouped heads: n_kv_heads must be at least 1 and divide n_heads");
  if (!inv_freq_host) OM_FAIL("rotary positions: a frequency table of 32 values");
  return rope_launch(dtype, qkv, M, L, heads + kv_heads, (heads + 2 * kv_heads) * 64, inv_freq_host, scaling, s, row_map);
}

// the one grouped-query attention entry: plan (attn_plan.h), switch on the family, launch
int omk_attention_gqa(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int heads, int kv_heads, int head_dim,
                      bool causal, float scale, int w, bool packed, const int* ext, hipStream_t s) {
  const AttnGqaPlan p = attn_plan_gqa(dtype, B, L, heads, kv_heads, head_dim, causal, w, packed, ext != nullptr);
  if (p.error) OM_FAIL(p.error);
  switch (p.family) {
    case 0: return 0;                                   // an empty batch
    case OM_ATTN_GQA_FAMILY_CAUSAL64: RUN(omk_attention_causal64(p, dtype, packed, qkv, ctx, mask, L, heads, kv_heads, scale, ext, s)); break;
    case OM_ATTN_GQA_FAMILY_CAUSAL128: RUN(omk_attention_causal128(p, dtype, packed, qkv, ctx, mask, L, heads, kv_heads, scale, ext, s)); break;
    default: RUN(omk_attention_d256(p, dtype, packed, qkv, ctx, mask, L, heads, kv_heads, scale, w, ext, s));      // FULL256, BAND256
  }
  OM_LAUNCH_CHECK();
  return 0;
}

// host only: what omk_attention_gqa would launch for these arguments -- out = {family, body (1: float32, 0: 16-bit), grid x, grid y,
// dynamic LDS bytes}; 0 with every word zero when nothing would launch, -1 for a refusal (its reason in om_last_error)
extern "C" int om_debug_attention_gqa_plan(int dtype, int64_t B, int L, int n_heads, int n_kv_heads, int head_dim, int causal, int w, int packed,
                                           int has_ext, int64_t out[5]) {
  if (!out) OM_FAIL("null argument");
  const AttnGqaPlan p = attn_plan_gqa(dtype, B, L, n_heads, n_kv_heads, head_dim, causal != 0, w, packed != 0, has_ext != 0);
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (p.error) { om_set_error(std::string(__func__) + ": " + p.error); return -1; }
  if (p.family) { out[0] = p.family; out[1] = p.f32; out[2] = p.grid_x; out[3] = p.grid_y; out[4] = p.lds; }
  return 0;
}

// Test hooks (tests/test_attention_causal.py, test_qwen3_kernels.py, test_gemma3_kernels.py and their packed twins, tools/causal_lm_bench.py,
// tools/gemma3_bench.py): the kernels alone.  The key extents of the padded form go into a grow-only device buffer the hooks keep per
// device (a forward has them in its workspace): like omk_rope_table it allocates on first use only, and launches after that are
// stream-ordered with no synchronisation -- calls on one device are expected from one stream at a time.
static int debug_kmax(int64_t B, int** out) {
  static std::mutex mu;
  static std::map<int, std::pair<int*, int64_t>> bufs;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto& e = bufs[dev];
  if (e.second < B) {
    if (e.first) { OM_HIP(hipDeviceSynchronize()); OM_HIP(hipFree(e.first)); e.first = nullptr; e.second = 0; }
    OM_HIP(hipMalloc(&e.first, (size_t)B * sizeof(int)));
    e.second = B;
  }
  *out = e.first;
  return 0;
}

// all six hooks after their null and dtype checks.  cu != NULL: the packed kernels.  Padded: the plan first, so that a refused call
// leaves nothing on the stream, then the extents (one more small launch), then the entry.
static int debug_attention_gqa(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L, int heads,
                               int kv_heads, int head_dim, bool causal, float scale, int w, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (cu) return omk_attention_gqa(dtype, qkv, ctx, mask, B, L, heads, kv_heads, head_dim, causal, scale, w, true, cu, s);
  const AttnGqaPlan p = attn_plan_gqa(dtype, B, L, heads, kv_heads, head_dim, causal, w, false, true);
  if (p.error) OM_FAIL(p.error);
  if (!p.family) return 0;
  int* kmax = nullptr;
  RUN(debug_kmax(B, &kmax));
  RUN(omk_mask_extent(mask, B, L, kmax, s));
  return omk_attention_gqa(dtype, qkv, ctx, mask, B, L, heads, kv_heads, head_dim, causal, scale, w, false, kmax, s);
}

extern "C" int om_debug_attention_causal(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads,
                                         int n_kv_heads, float scale, void* stream) {
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  OM_DBG_DTYPE("causal attention");
  return debug_attention_gqa(dtype, qkv, ctx, mask, nullptr, B, L, n_heads, n_kv_heads, 64, true, scale, 0, stream);
}

// the packed kernels alone: cu [B + 1] as om_debug_pack_rows wrote it
extern "C" int om_debug_attention_causal_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L,
                                                int n_heads, int n_kv_heads, float scale, void* stream) {
  if (!qkv || !ctx || !mask || !cu) OM_FAIL("null argument");
  OM_DBG_DTYPE("causal attention");
  return debug_attention_gqa(dtype, qkv, ctx, mask, cu, B, L, n_heads, n_kv_heads, 64, true, scale, 0, stream);
}

// the same two with a head width: 64 runs the kernels above, 128 those of attention_causal128.hip
extern "C" int om_debug_attention_causal_hd(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads,
                                            int n_kv_heads, int head_dim, float scale, void* stream) {
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  RUN(debug_dtype(dtype));
  return debug_attention_gqa(dtype, qkv, ctx, mask, nullptr, B, L, n_heads, n_kv_heads, head_dim, true, scale, 0, stream);
}

extern "C" int om_debug_attention_causal_hd_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L,
                                                   int n_heads, int n_kv_heads, int head_dim, float scale, void* stream) {
  if (!qkv || !ctx || !mask || !cu) OM_FAIL("null argument");
  RUN(debug_dtype(dtype));
  return debug_attention_gqa(dtype, qkv, ctx, mask, cu, B, L, n_heads, n_kv_heads, head_dim, true, scale, 0, stream);
}

// Gemma3's bidirectional kernels (attention_d256.hip): 0 < w < L - 1 the band, anything else full attention
extern "C" int om_debug_attention_gqa_d256(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads,
                                           int n_kv_heads, float scale, int w, void* stream) {
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  RUN(debug_dtype(dtype));
  return debug_attention_gqa(dtype, qkv, ctx, mask, nullptr, B, L, n_heads, n_kv_heads, 256, false, scale, w, stream);
}

extern "C" int om_debug_attention_gqa_d256_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L,
                                                  int n_heads, int n_kv_heads, float scale, int w, void* stream) {
  if (!qkv || !ctx || !mask || !cu) OM_FAIL("null argument");
  RUN(debug_dtype(dtype));
  return debug_attention_gqa(dtype, qkv, ctx, mask, cu, B, L, n_heads, n_kv_heads, 256, false, scale, w, stream);
}

extern "C" int om_debug_rope_gqa(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, const float* inv_freq, float scaling,
                                 void* stream) {
  if (!qkv || !inv_freq) OM_FAIL("null argument");
  OM_DBG_DTYPE("rotary positions");
  return omk_rope_gqa(dtype, qkv, M, L, n_heads, n_kv_heads, inv_freq, scaling, (hipStream_t)stream);
}

// row_map [rows] as om_debug_pack_rows wrote it
extern "C" int om_debug_rope_gqa_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, const float* inv_freq, float scaling,
                                      const int* row_map, void* stream) {
  if (!qkv || !inv_freq || !row_map) OM_FAIL("null argument");
  OM_DBG_DTYPE("rotary positions");
  return omk_rope_gqa(dtype, qkv, rows, L, n_heads, n_kv_heads, inv_freq, scaling, (hipStream_t)stream, row_map);
}
