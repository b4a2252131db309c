// Decoder-only backbones (HF:models/llama/modeling_llama.py, HF:models/qwen2/modeling_qwen2.py; gfx950), head_dim 64, inference:
//
//   * omk_rope_gqa: rotary positions applied IN PLACE to the q and k heads of the grouped projection
//     [M, (n_heads + 2 n_kv) * 64] (columns q heads | k heads | v heads; apply_rotary_pos_emb with rotate_half: pairs (i, i + 32)
//     of each head, position = row % L as HF's arange(L) whatever the padding).  The 32 frequencies are the HOST's -- the module's
//     own rotary_emb.inv_freq buffer -- so `default`, `linear` and `llama3` rope need no rule restated here; cos / sin come from a
//     device table per (device, frequency vector, scaling) of 1 024 positions, built once as LlamaRotaryEmbedding.forward does in
//     f32 (inv_freq * pos, then cos * attention_scaling, sin * attention_scaling).
//
//   * omk_attention_causal: softmax(Q K^T * scale + mask) V where key k is visible from query q iff k <= q and k is unmasked;
//     query head h reads K / V head h / (n_heads / n_kv) (HF repeat_kv).  One workgroup owns 128 queries of one (sequence, query
//     head) -- four waves of 32 -- and walks the 128-key chunks from key 0 up to its own diagonal chunk (clipped to kmax[b]: keys at
//     or past it are padding) with the online softmax: at 1 024 tokens 4.5 chunks per block on average instead of eight.  The
//     triangle is a select per score in the diagonal chunk only: a key past the query scores min(v, -1e30) -- finite, like a padded
//     key -- so a padded query with no visible key (the first rows of a left-padded sequence) averages the values it visited
//     instead of producing NaN.  A block of padded queries past kmax[b] visits the first chunk only: no output depends on its rows.
//     16-bit: the key-chunked body of attention.hip (attention_fwd16c_kernel / attention_band16_kernel: LDS-DMA, transposing V
//     reads, exp2); float32: the generic online-softmax layout (attention_band32_kernel).  Every query head fetches its group's
//     K / V chunks itself (one workgroup per (sequence, query head, query block)); a form that serves a whole K / V group from
//     one fetch has not been built or measured.
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "attn_common.h"
#include "gemm_core7.h"

namespace {

constexpr int kRopeMaxPos = 1024;
constexpr float kFinfoMin = -3.4028235e38f;

// [kRopeMaxPos][32] (cos, sin) * scaling for one frequency vector, resident on the device: built and uploaded ONCE per
// (device, frequencies, scaling)
int rope_gqa_table_device(const float* inv_freq, float scaling, const float2** out) {
  static std::mutex mu;
  static std::map<std::tuple<int, std::vector<float>, float>, float2*> cache;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto key = std::make_tuple(dev, std::vector<float>(inv_freq, inv_freq + 32), scaling);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::vector<float2> tab((size_t)kRopeMaxPos * 32);
    for (int i = 0; i < 32; ++i)
      for (int pos = 0; pos < kRopeMaxPos; ++pos) {
        const float f = inv_freq[i] * (float)pos;                            // inv_freq @ position_ids, f32
        const float c = (float)cos((double)f), sn = (float)sin((double)f);  // emb.cos(), emb.sin(), f32
        tab[(size_t)pos * 32 + i] = make_float2(c * scaling, sn * scaling);  // * attention_scaling, f32
      }
    float2* d = nullptr;
    OM_HIP(hipMalloc(&d, tab.size() * sizeof(float2)));
    OM_HIP(hipMemcpy(d, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
    it = cache.emplace(key, d).first;
  }
  *out = it->second;
  return 0;
}

template <typename T> struct RopeIO;
template <> struct RopeIO<float> {
  __device__ static inline void load4(const float* p, float (&v)[4]) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  __device__ static inline void store4(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <typename T> struct RopeIO16 {
  __device__ static inline void load4(const T* p, float (&v)[4]) {
    const uint2 t = *(const uint2*)p;
    v[0] = Half16<T>::lo(t.x); v[1] = Half16<T>::hi(t.x); v[2] = Half16<T>::lo(t.y); v[3] = Half16<T>::hi(t.y);
  }
  __device__ static inline void store4(T* p, const float (&v)[4]) { *(uint2*)p = make_uint2(Half16<T>::pack2(v[0], v[1]), Half16<T>::pack2(v[2], v[3])); }
};
template <> struct RopeIO<bf16_t> : RopeIO16<bf16_t> {};
template <> struct RopeIO<f16_t> : RopeIO16<f16_t> {};

// one thread: four consecutive pairs (i .. i + 3, i + 32 .. i + 35) of one q or k head of one row; the v heads are never touched.
// q' = q cos + rotate_half(q) sin in f32, rounded once; products and sum kept apart (no fused multiply-add) as torch evaluates them.
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
  T* p = qkv + row * (int64_t)pitch + (int64_t)seg * 64 + i0;
  float a[4], b[4];
  RopeIO<T>::load4(p, a);
  RopeIO<T>::load4(p + 32, b);
  const float2* t = tab + (size_t)pos * 32 + i0;
  float ra[4], rb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float2 cs = t[e];
    ra[e] = __fadd_rn(__fmul_rn(a[e], cs.x), __fmul_rn(-b[e], cs.y));
    rb[e] = __fadd_rn(__fmul_rn(b[e], cs.x), __fmul_rn(a[e], cs.y));
  }
  RopeIO<T>::store4(p, ra);
  RopeIO<T>::store4(p + 32, rb);
}

// keys [0, hi) a 128-query block starting at qb walks: up to its diagonal chunk, clipped to kend; a block of padded queries at or
// past kend visits the first chunk alone (its rows only have to stay finite)
__device__ __forceinline__ int causal_key_end(int qb, int kend) {
  if (qb >= kend) return 1;
  return qb + 128 < kend ? qb + 128 : kend;
}

typedef short v4s_c_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s_c_t causal_vtrd(const char* p) {      // ds_read_b64_tr_b16
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s_c_t __attribute__((address_space(3)))*)(p));
}
template <typename F>
__device__ __forceinline__ F causal_vfrag(v4s_c_t a, v4s_c_t b) { return __builtin_bit_cast(F, (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}); }

// 16-bit: attention_band16_kernel's body (attention_band.hip) with grouped K / V heads and the triangle instead of the band.
// pitch: elements per qkv row, (heads + 2 kv_heads) * 64; ctx rows hold heads * 64.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_causal16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + 128 * 128;
  float* const sM = (float*)(smem + 2 * 128 * 128);
  const int h = blockIdx.x % heads;
  const int kvh = h / (heads / kv_heads);
  const int64_t b = blockIdx.x / heads;
  const int64_t row0 = b * L;
  const int qb = blockIdx.y * 128;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pitch = (heads + 2 * kv_heads) * 64;
  const int64_t ld2 = 2 * (int64_t)pitch;                   // row pitch of qkv in bytes
  const char* const qbase = (const char*)(qkv + row0 * pitch + h * 64);
  const char* const kbase = (const char*)(qkv + row0 * pitch + (heads + kvh) * 64);
  const char* const vbase = kbase + kv_heads * 128;
  const float LOG2E = 1.4426950408889634f;
  const int q0 = qb + wave * 32;
  const bool active = q0 < L;
  const int qi = q0 + l31;                                  // this lane's query (the triangle uses the true index)
  const int qrow = qi < L ? qi : (L - 1);
  frag_t qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const frag_t*)(qbase + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  const float c2 = scale * LOG2E;
  const int key = (l31 >> 1) & 7;
  const int i16 = lane & 15;
  const char* const vt0 = sV + (4 * half + (i16 >> 2)) * 128 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  const int vsw = (i16 >> 3) & 1;
  const int khi = causal_key_end(qb, kmax ? __builtin_amdgcn_readfirstlane(kmax[b]) : L);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = 0; kc < khi; kc += 128) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (i * 4 + wave) * 8 + (lane >> 3);
      const int rr = (kc + r) < L ? (kc + r) : (L - 1);
      const uint32_t off = (uint32_t)(rr * ld2) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
      const uint32_t offv = (uint32_t)(rr * ld2) + (((lane & 7) ^ (((r >> 1) & 1) << 2)) << 4);
      const uint32_t dst = (uint32_t)((i * 4 + wave) * 1024);
      g7_dma(kbase, off, g7_lds_addr(sK) + dst);
      g7_dma(vbase, offv, g7_lds_addr(sV) + dst);
    }
    if (tid < 128) sM[tid] = (kc + tid) < L ? (mask[b * L + kc + tid] != 0 ? 0.f : -1e30f) : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the DMA above is not in hipcc's bookkeeping
    __syncthreads();
    if (!active) continue;

    f32x16_t s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const char* krow = sK + (t * 32 + l31) * 128;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const frag_t a = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(a, qf[kk], s[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // the diagonal chunk alone holds keys past a query of this block (kc <= qb always: every earlier chunk is wholly visible)
    const int dlim = kc + 127 > q0 ? qi - kc : 128;          // keys of this chunk with index > dlim are in the future of this lane's query
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = fmaf(s[t][4 * g + e], c2, mb[e]);
          v = (k0 + e > dlim) ? fminf(v, -1e30f) : v;
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds key 0 < L (unmasked, or -1e30: finite): mx is finite from here on
    const float alpha = __builtin_amdgcn_exp2f(m_run - mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[t][r] - mx);
        s[t][r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = mx;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint4 pa[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
        pa[u] = make_uint4(Half16<T>::pack2(s[t][8 * u + 0], s[t][8 * u + 1]), Half16<T>::pack2(s[t][8 * u + 2], s[t][8 * u + 3]),
                           Half16<T>::pack2(s[t][8 * u + 4], s[t][8 * u + 5]), Half16<T>::pack2(s[t][8 * u + 6], s[t][8 * u + 7]));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const char* p = vt0 + (t * 32 + 16 * u) * 128 + ((dt ^ vsw) << 6);
          const frag_t vf = causal_vfrag<frag_t>(causal_vtrd(p), causal_vtrd(p + 8 * 128));
          MmaOps<T>::mma(vf, __builtin_bit_cast(frag_t, pa[u]), o[dt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();
  if (!active) return;
  const float inv = 1.0f / l_run;
  char* const so = sK + (wave * 32) * 128;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      uint32_t a0 = Half16<T>::pack2(o[dt][8 * gp + 0] * inv, o[dt][8 * gp + 1] * inv), a1 = Half16<T>::pack2(o[dt][8 * gp + 2] * inv, o[dt][8 * gp + 3] * inv);
      uint32_t b0 = Half16<T>::pack2(o[dt][8 * gp + 4] * inv, o[dt][8 * gp + 5] * inv), b1 = Half16<T>::pack2(o[dt][8 * gp + 6] * inv, o[dt][8 * gp + 7] * inv);
      auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      *(uint4*)(so + l31 * 128 + (((4 * dt + 2 * gp + half) ^ (l31 & 7)) << 4)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
  const int Hq = heads * 64;
  char* const out = (char*)(ctx + (row0 + q0) * (int64_t)Hq + h * 64);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (lane >> 3), c = lane & 7;
    const uint4 v = *(const uint4*)(so + row * 128 + ((c ^ (row & 7)) << 4));
    if (q0 + row < L) *(uint4*)(out + (int64_t)row * Hq * 2 + c * 16) = v;
  }
}

// float32: attention_band32_kernel's layout (attention_band.hip) over the keys up to the diagonal -- K row-major swizzled, V
// transposed, queries in registers, the per-query rescale through a 32-float LDS table per wave; natural exp, the mask's finfo.min.
__global__ __launch_bounds__(256) void attention_causal32_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int heads, int kv_heads, float scale,
    const int* __restrict__ kmax) {
  typedef AttnGeom<float> G;
  typedef typename MmaOps<float>::frag_t frag_t;
  constexpr int LP = 128 + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  float* sVt = (float*)(smem + 128 * G::ROWB);
  float* sM = (float*)(smem + 128 * G::ROWB + 64 * LP * 4);
  float* sF = sM + 128;                                     // [4 waves][32] per-query factors

  const int h = blockIdx.x % heads;
  const int kvh = h / (heads / kv_heads);
  const int64_t b = blockIdx.x / heads;
  const int qb = blockIdx.y * 128;
  const int tid = threadIdx.x;
  const int64_t ld = (int64_t)(heads + 2 * kv_heads) * 64;
  const float* qbase = qkv + b * L * ld + h * 64;
  const float* kbase = qkv + b * L * ld + (heads + kvh) * 64;
  const float* vbase = kbase + kv_heads * 64;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = qb + wave * 32;
  const int qrow = (q0 + l31) < L ? (q0 + l31) : (L - 1);
  frag_t qf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) qf[kk] = *(const frag_t*)(qbase + (int64_t)qrow * ld + (kk * 2 + half) * G::EPC);
  const int khi = causal_key_end(qb, kmax ? kmax[b] : L);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = 0; kc < khi; kc += 128) {
    __syncthreads();
    for (int idx = tid; idx < 128 * G::CPR; idx += 256) {
      const int row = idx / G::CPR, c = idx % G::CPR;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (kc + row < L) {
        kv = *(const uint4*)(kbase + (int64_t)(kc + row) * ld + c * G::EPC);
        vv = *(const uint4*)(vbase + (int64_t)(kc + row) * ld + c * G::EPC);
      }
      *(uint4*)(sK + row * G::ROWB + ((c ^ G::key(row)) << 4)) = kv;
      const float* ve = (const float*)&vv;
#pragma unroll
      for (int e = 0; e < G::EPC; ++e) sVt[(c * G::EPC + e) * LP + row] = ve[e];
    }
    if (tid < 128) sM[tid] = (kc + tid) < L ? (mask[b * L + kc + tid] != 0 ? 0.f : kFinfoMin) : -INFINITY;
    __syncthreads();

    f32x16_t s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const int row = t * 32 + l31;
      const char* krow = sK + row * G::ROWB;
      const int key = G::key(row);
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) {
        const frag_t a = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<float>::mma(a, qf[kk], s[t]);
      }
    }
    const int dlim = kc + 127 > q0 ? (q0 + l31) - kc : 128;  // the diagonal chunk alone: keys with index > dlim lie past this lane's query
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = s[t][4 * g + e] * scale + mb[e];
          v = (k0 + e > dlim) ? fminf(v, kFinfoMin) : v;
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = G::exp_(m_run - mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = G::exp_(s[t][r] - mx);
        sum += e;
        s[t][r] = e;
      }
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = mx;
    if (half == 0) sF[wave * 32 + l31] = alpha;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4_t a4 = *(const f32x4_t*)(sF + wave * 32 + 8 * g + 4 * half);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[0][4 * g + e] *= a4[e]; o[1][4 * g + e] *= a4[e]; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) SlabMma<float>::run(s[t], sVt + l31 * LP + t * 32 + 4 * half, LP, o);
  }
  __syncthreads();
  if (half == 0) sF[wave * 32 + l31] = 1.0f / l_run;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float* so = (float*)(sK + (size_t)(wave * 32) * G::ROWB);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4_t i4 = *(const f32x4_t*)(sF + wave * 32 + 8 * g + 4 * half);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = 8 * g + 4 * half + e;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) so[q * 64 + dt * 32 + l31] = o[dt][4 * g + e] * i4[e];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (q0 < L) {
    const int Hq = heads * 64;
    float* out = ctx + (b * L + q0) * Hq + h * 64;
    constexpr int VPR = G::ROWB / 16;
#pragma unroll
    for (int it = 0; it < 32 * VPR / 64; ++it) {
      const int idx = it * 64 + lane, row = idx / VPR, c = idx % VPR;
      const uint4 v = *(const uint4*)((const char*)so + row * G::ROWB + c * 16);
      if (q0 + row < L) *(uint4*)((char*)(out + (int64_t)row * Hq) + c * 16) = v;
    }
  }
}

}  // namespace

static int check_gqa(int heads, int kv_heads) {
  if (heads < 1 || kv_heads < 1 || heads % kv_heads) OM_FAIL("grouped heads: n_kv_heads must be at least 1 and divide n_heads");
  return 0;
}

int omk_rope_gqa(int dtype, void* qkv, int64_t M, int L, int heads, int kv_heads, const float* inv_freq_host, float scaling, hipStream_t s) {
  if (M <= 0) return 0;
  if (L < 1 || L > kRopeMaxPos) OM_FAIL("rotary positions: sequence length must be in [1,1024]");
  if (check_gqa(heads, kv_heads)) return 1;
  if (!inv_freq_host) OM_FAIL("rotary positions: a frequency table of 32 values");
  const float2* tab = nullptr;
  if (rope_gqa_table_device(inv_freq_host, scaling, &tab)) return 1;
  const int rot = heads + kv_heads, pitch = (heads + 2 * kv_heads) * 64;
  const int64_t n = M * rot * 8;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (dtype == OM_BF16) hipLaunchKernelGGL(rope_gqa_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (bf16_t*)qkv, tab, M, L, rot, pitch);
  else if (dtype == OM_F16) hipLaunchKernelGGL(rope_gqa_kernel<f16_t>, dim3(grid), dim3(256), 0, s, (f16_t*)qkv, tab, M, L, rot, pitch);
  else hipLaunchKernelGGL(rope_gqa_kernel<float>, dim3(grid), dim3(256), 0, s, (float*)qkv, tab, M, L, rot, pitch);
  OM_LAUNCH_CHECK();
  return 0;
}

// its own launch: the planner of the bidirectional kernels (attn_plan.h) and omk_attention know nothing of it
int omk_attention_causal(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int heads, int kv_heads, float scale,
                         const int* kmax, hipStream_t s) {
  if (B <= 0) return 0;
  if (L < 1 || L > 1024) OM_FAIL("causal attention: sequence length must be in [1,1024]");
  if (check_gqa(heads, kv_heads)) return 1;
  if (B * heads > 0x7fffffffLL) OM_FAIL("causal attention: batch too large for one launch");
  const dim3 grid((unsigned)(heads * B), (unsigned)((L + 127) / 128));
  if (dtype == OM_F32) {
    const int lds = 128 * AttnGeom<float>::ROWB + 64 * 132 * 4 + 128 * 4 + 128 * 4;
    if (attn_lds_once<attention_causal32_kernel>(lds)) return 1;
    hipLaunchKernelGGL(attention_causal32_kernel, grid, dim3(256), lds, s, (const float*)qkv, (float*)ctx, mask, L, heads, kv_heads, scale, kmax);
  } else {
    const int lds = 2 * 128 * 128 + 128 * 4;
    if (dtype == OM_F16)
      hipLaunchKernelGGL(attention_causal16_kernel<f16_t>, grid, dim3(256), lds, s, (const f16_t*)qkv, (f16_t*)ctx, mask, L, heads, kv_heads, scale, kmax);
    else
      hipLaunchKernelGGL(attention_causal16_kernel<bf16_t>, grid, dim3(256), lds, s, (const bf16_t*)qkv, (bf16_t*)ctx, mask, L, heads, kv_heads, scale, kmax);
  }
  OM_LAUNCH_CHECK();
  return 0;
}

// Test hooks (tests/test_attention_causal.py, tools/causal_lm_bench.py).  The key extents go into a grow-only device buffer the hook
// keeps per device (a forward has them in its workspace): like rope_gqa_table_device it allocates on first use only, and launches
// after that are stream-ordered with no synchronisation -- calls on one device are expected from one stream at a time.
static int causal_debug_kmax(int64_t B, int** out) {
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

extern "C" int om_debug_attention_causal(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads,
                                         int n_kv_heads, float scale, void* stream) {
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("causal attention: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (B <= 0) return 0;
  if (L < 1 || L > 1024) OM_FAIL("causal attention: sequence length must be in [1,1024]");
  if (check_gqa(n_heads, n_kv_heads)) return 1;
  hipStream_t s = (hipStream_t)stream;
  int* kmax = nullptr;
  if (causal_debug_kmax(B, &kmax)) return 1;
  if (omk_mask_extent(mask, B, L, kmax, s)) return 1;
  return omk_attention_causal(dtype, qkv, ctx, mask, B, L, n_heads, n_kv_heads, scale, kmax, s);
}

extern "C" int om_debug_rope_gqa(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, const float* inv_freq, float scaling,
                                 void* stream) {
  if (!qkv || !inv_freq) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("rotary positions: dtype must be OM_F32, OM_BF16 or OM_F16");
  return omk_rope_gqa(dtype, qkv, M, L, n_heads, n_kv_heads, inv_freq, scaling, (hipStream_t)stream);
}
