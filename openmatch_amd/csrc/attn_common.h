// Shared pieces of the attention forward / backward kernels (gfx950).
#pragma once
#include <type_traits>

#include "gemm_core.h"
#include "kernels.h"

// ---- host side: from a plan (attn_plan.h) to a template instantiation ----
// A run-time key-tile count as a compile-time one: f(std::integral_constant<int, KT>{}) for the KT among KTS... that equals kt.  Each
// call site names the tile counts it instantiates.
template <int... KTS, typename F>
static int attn_with_kt(int kt, F&& f) {
  int rc = 1;
  if (!((kt == KTS && ((rc = f(std::integral_constant<int, KTS>{})), true)) || ...)) OM_FAIL("attention: no kernel of this key-tile count");
  return rc;
}
// the storage type of a planned call: f(T{}) with T = f16_t, bf16_t or float (every other dtype code counts as float32) ...
template <typename F>
static int attn_with_type(int dtype, F&& f) { return dtype == OM_F16 ? f(f16_t{}) : dtype == OM_BF16 ? f(bf16_t{}) : f(float{}); }
// ... and of a family that exists in the 16-bit formats only
template <typename F>
static int attn_with_type16(int dtype, F&& f) { return dtype == OM_F16 ? f(f16_t{}) : f(bf16_t{}); }
// the twin of attn_with_kt for the (BIAS, DROP) pair: f(std::bool_constant<BIAS>{}, std::bool_constant<DROP>{})
template <typename F>
static int attn_with_flags(bool bias, bool drop, F&& f) {
  const std::true_type yes;
  const std::false_type no;
  return bias ? (drop ? f(yes, yes) : f(yes, no)) : (drop ? f(no, yes) : f(no, no));
}
// Raise the dynamic LDS limit of Kernel to `lds` bytes, once per process (a kernel is always launched with the same figure: it follows
// from the template arguments).
template <auto Kernel>
static int attn_lds_once(int lds) {
  static std::atomic<bool> done{false};
  if (!done) {
    OM_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    done = true;
  }
  return 0;
}
// Launch the Padded or the Packed kernel of one body (one signature: the projection, ctx, then `rest`, whose last argument is kmax
// for the one and cu for the other) on `grid` x 256 threads with `lds` bytes of dynamic LDS; the caller checks the launch.
template <auto Padded, auto Packed, typename T, typename... Rest>
static int attn_launch_form(bool packed, dim3 grid, int lds, hipStream_t s, const void* qkv, void* ctx, Rest... rest) {
  if (packed) {
    if (attn_lds_once<Packed>(lds)) return 1;
    hipLaunchKernelGGL(Packed, grid, dim3(256), lds, s, (const T*)qkv, (T*)ctx, rest...);
  } else {
    if (attn_lds_once<Padded>(lds)) return 1;
    hipLaunchKernelGGL(Padded, grid, dim3(256), lds, s, (const T*)qkv, (T*)ctx, rest...);
  }
  return 0;
}
// the dtype check of the grouped-query test hooks that name no family
static int debug_dtype(int dtype) {
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("dtype must be OM_F32, OM_BF16 or OM_F16");
  return 0;
}

// four consecutive elements <-> floats; one value rounded to the storage format and back (the rotary and q / k norm passes)
template <typename T> struct Vec4IO;
template <> struct Vec4IO<float> {
  __device__ static inline void load4(const float* p, float (&v)[4]) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  __device__ static inline void store4(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
  __device__ static inline float round(float v) { return v; }
};
template <typename T> struct Vec4IO16 {
  __device__ static inline void load4(const T* p, float (&v)[4]) {
    const uint2 t = *(const uint2*)p;
    v[0] = Half16<T>::lo(t.x); v[1] = Half16<T>::hi(t.x); v[2] = Half16<T>::lo(t.y); v[3] = Half16<T>::hi(t.y);
  }
  __device__ static inline void store4(T* p, const float (&v)[4]) { *(uint2*)p = make_uint2(Half16<T>::pack2(v[0], v[1]), Half16<T>::pack2(v[2], v[3])); }
  __device__ static inline float round(float v) { return Half16<T>::value(Half16<T>::bits(v)); }
};
template <> struct Vec4IO<bf16_t> : Vec4IO16<bf16_t> {};
template <> struct Vec4IO<f16_t> : Vec4IO16<f16_t> {};

template <typename T> struct AttnGeom;
template <> struct AttnGeom<bf16_t> {
  static constexpr int ROWB = 128, CPR = 8, EPC = 8, NKK = 4;
  __device__ static inline int key(int row) { return (row >> 1) & 7; }
  __device__ static inline float exp_(float x) { return __expf(x); }
};
template <> struct AttnGeom<f16_t> {              // IEEE half: the same geometry as bfloat16
  static constexpr int ROWB = 128, CPR = 8, EPC = 8, NKK = 4;
  __device__ static inline int key(int row) { return (row >> 1) & 7; }
  __device__ static inline float exp_(float x) { return __expf(x); }
};
template <> struct AttnGeom<float> {
  static constexpr int ROWB = 256, CPR = 16, EPC = 4, NKK = 8;
  __device__ static inline int key(int row) { return row & 15; }
  __device__ static inline float exp_(float x) { return expf(x); }
};

// HF's masked score in the natural-exp kernels: torch.finfo(float32).min
constexpr float kFinfoMin = -3.4028235e38f;

// ds_read_b64_tr_b16: a transposing LDS read of a row-major 16-bit image; two of them hand a lane eight k slots of one column, an
// MFMA operand as read (attention_fwd16_body in attention.hip, attn_chunked16 in attn_chunked.h)
typedef short v4s_a_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s_a_t vtrd(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s_a_t __attribute__((address_space(3)))*)(p));
}
template <typename F>
__device__ __forceinline__ F vfrag_of(v4s_a_t a, v4s_a_t b) { return __builtin_bit_cast(F, (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}); }

// One 32-wide slab of a contraction whose left operand sits in a 32x32 accumulator layout:
//   o[dt][i][j] += sum_c a[i][c] * Bt[dt*32 + j][c]      (i = lane&31 of the A operand)
// `a` holds, for lane (i, half), the 16 values c = (r&3) + 8(r>>2) + 4*half, r in [0,16);
// `bt` points at Bt[(lane&31)][slab*32 + 4*half] of a TRANSPOSED LDS image with row pitch LP,
// so each lane reads its k-slots as contiguous 8/16-byte pieces.
template <typename T> struct SlabMma;
template <> struct SlabMma<bf16_t> {
  // k-slot j of half h  <->  c = 16u + 8(j>>2) + (j&3) + 4h
  __device__ static inline void run(const f32x16_t& a, const bf16_t* bt, int LP, f32x16_t (&o)[2]) {
    bf16x8_t pa[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[u][j] = (short)f32_to_bf16(a[8 * u + j]);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16_t* p = bt + dt * 32 * LP + 16 * u;
        const bf16x4_t v0 = *(const bf16x4_t*)p;
        const bf16x4_t v1 = *(const bf16x4_t*)(p + 8);
        bf16x8_t vb;
        vb[0] = v0[0]; vb[1] = v0[1]; vb[2] = v0[2]; vb[3] = v0[3];
        vb[4] = v1[0]; vb[5] = v1[1]; vb[6] = v1[2]; vb[7] = v1[3];
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[u], vb, o[dt], 0, 0, 0);
      }
  }
};
template <> struct SlabMma<f16_t> {
  __device__ static inline void run(const f32x16_t& a, const f16_t* bt, int LP, f32x16_t (&o)[2]) {
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
    f16x8_t pa[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[u][j] = (f16_t)a[8 * u + j];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f16_t* p = bt + dt * 32 * LP + 16 * u;
        const f16x4_t v0 = *(const f16x4_t*)p;
        const f16x4_t v1 = *(const f16x4_t*)(p + 8);
        f16x8_t vb;
        vb[0] = v0[0]; vb[1] = v0[1]; vb[2] = v0[2]; vb[3] = v0[3];
        vb[4] = v1[0]; vb[5] = v1[1]; vb[6] = v1[2]; vb[7] = v1[3];
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa[u], vb, o[dt], 0, 0, 0);
      }
  }
};
template <> struct SlabMma<float> {
  // register r of half h  <->  c = (r&3) + 8(r>>2) + 4h  (one register per k = 2 MFMA)
  __device__ static inline void run(const f32x16_t& a, const float* bt, int LP, f32x16_t (&o)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4_t vb = *(const f32x4_t*)(bt + dt * 32 * LP + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g + e], vb[e], o[dt], 0, 0, 0);
      }
  }
};

// Dropout of the attention probabilities.  One 64-bit hash serves the FOUR probabilities (b, h, q, 4 kg .. 4 kg + 3): bits
// 16 e .. 16 e + 15 decide element e (kept iff >= p * 2^16).  Four consecutive keys are exactly what one lane holds per
// accumulator group in the lane-per-query orientation of the forward and of the backward's first phase, so those
// kernels pay ~10 instead of ~35 integer instructions per probability (the three 64-bit multiplies of the hash were the
// largest single cost of the attention backward).  p is resolved to 2^-16; keep_scale uses the same rounded value.
using AttnDrop = DropCfg;   // kernels.h: 16-bit fields of one 64-bit hash per four elements
__host__ __device__ inline uint64_t attn_drop_bits(uint64_t seed, int64_t b, int h, int heads, int L, int q, int kg) {
  return om_hash64(seed, (((uint64_t)b * heads + h) * (uint64_t)L + q) * (uint64_t)((L + 3) >> 2) + kg);
}
__host__ __device__ inline bool attn_drop_keep(uint64_t bits, int e, uint32_t thresh) { return dropout_field(bits, e, thresh); }
// one probability (the lane-per-key orientation): the group's hash, this element's field
__host__ __device__ inline bool attn_drop_keep1(uint64_t seed, int64_t b, int h, int heads, int L, int q, int key, uint32_t thresh) {
  return attn_drop_keep(attn_drop_bits(seed, b, h, heads, L, q, key >> 2), key & 3, thresh);
}
