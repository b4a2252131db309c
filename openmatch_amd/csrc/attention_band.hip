// ModernBERT attention pieces (HF:models/modernbert/modeling_modernbert.py, gfx950), head_dim 64, inference:
//
//   * omk_rope: rotary positions applied IN PLACE to the Q and K columns of the fused projection [M, 3H]
//     (apply_rotary_pos_emb with rotate_half: pairs (i, i + 32) of each head, position = row % L, as HF's arange(L)
//     whatever the padding).  cos / sin come from a device table per (device, theta) of 1 024 positions x 32
//     frequencies, built on the host once exactly as ModernBertRotaryEmbedding does in f32 (inv_freq =
//     1 / theta ** (2i / 64), freqs = inv_freq * pos, then cos / sin); every L reads a prefix of it.
//     The rotation is one separate pass (read + write of 2H of the 3H columns per row) rather than folded into the
//     attention kernels' K / Q loads: K reaches LDS by DMA there, untouched by the vector unit, so a fused rotation
//     would have to rewrite K in LDS once per (query block, key chunk) -- see DESIGN.md for the measured cost of the pass.
//
//   * omk_attention_band: softmax(Q K^T / 8 + mask) V where key k is visible from query q only if |q - k| <= w
//     (masking_utils.sliding_window_bidirectional_overlay: inclusive at both ends) AND k is unmasked.  A workgroup owns
//     128 queries of one (sequence, head) -- four waves of 32 -- and walks only the keys [qb - w, qb + 127 + w] that its
//     band can reach, clipped to [0, kmax[b]) (keys at or past kmax are padding), in chunks of 128 with the online
//     softmax: at 1 024 tokens and w = 64 two chunks instead of eight.  Per score the band is a select, not an add:
//     out-of-band keys score min(v, -1e30) -- finite, like a padded key -- so a (padded) query whose band holds no
//     unmasked key averages the values it visited instead of producing NaN, and keys past L stay -inf.
//     16-bit: the key-chunked kernel of attention.hip (attention_fwd16c_kernel: LDS-DMA, transposing V reads, exp2);
//     float32: the generic online-softmax kernel (attention_long_kernel's layout, queries in registers).
//     Launch only: omk_attention (attention.hip) sends a call here when its planner (attn_plan.h) finds 0 < w < L - 1; a window
//     that reaches every key is full attention and never arrives.
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "attn_common.h"
#include "gemm_core7.h"

namespace {

constexpr int kRopeMaxPos = 1024;
constexpr float kFinfoMin = -3.4028235e38f;

// [kRopeMaxPos][32] (cos, sin) for one theta, resident on the device: built and uploaded ONCE per (device, theta)
int rope_table_device(float theta, const float2** out) {
  static std::mutex mu;
  static std::map<std::tuple<int, float>, float2*> cache;
  int dev = 0;
  OM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto key = std::make_tuple(dev, theta);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::vector<float2> tab((size_t)kRopeMaxPos * 32);
    for (int i = 0; i < 32; ++i) {
      const float e = (float)(2 * i) / 64.0f;                                // arange(0, d, 2) / d, f32 (exact)
      const float p = (float)pow((double)theta, (double)e);                 // theta ** e, rounded to f32
      const float inv = 1.0f / p;                                            // 1.0 / (...), f32
      for (int pos = 0; pos < kRopeMaxPos; ++pos) {
        const float f = inv * (float)pos;                                    // inv_freq @ position_ids, f32
        tab[(size_t)pos * 32 + i] = make_float2((float)cos((double)f), (float)sin((double)f));
      }
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

// one thread: four consecutive pairs (i .. i + 3, i + 32 .. i + 35) of one head of Q or K of one row.
// q' = q cos + rotate_half(q) sin in f32 (HF: q.float() * cos + rotate_half(q.float()) * sin), rounded once; the products and the
// sum are kept apart (no fused multiply-add) as torch evaluates them.
template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(T* __restrict__ qkv, const float2* __restrict__ tab, int64_t M, int L, int H) {
  const int per_row = H / 4;                               // (2 H columns rotated, 8 of them per thread -> H / 4 threads per row)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t row = idx / per_row;
  const int j = (int)(idx % per_row);
  const int seg = j / 8, i0 = (j % 8) * 4;                 // seg: head (Q heads, then K heads); i0: first of four pairs
  const int pos = (int)(row % L);
  T* p = qkv + row * 3 * (int64_t)H + (int64_t)seg * 64 + i0;
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

// keys [lo, hi) a 128-query block starting at qb walks: its band, clipped to [0, kend); at least one key (a block of padded
// queries beyond the band of every unmasked key still visits the last keys, all scored as masked, so its rows stay finite)
__device__ __forceinline__ void band_keys(int qb, int w, int kend, int& lo, int& hi) {
  lo = qb - w > 0 ? qb - w : 0;
  hi = qb + 128 + w < kend ? qb + 128 + w : kend;
  if (hi <= lo) { hi = kend; lo = kend - 1; }
}

typedef short v4s_b_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s_b_t band_vtrd(const char* p) {      // ds_read_b64_tr_b16
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s_b_t __attribute__((address_space(3)))*)(p));
}
template <typename F>
__device__ __forceinline__ F band_vfrag(v4s_b_t a, v4s_b_t b) { return __builtin_bit_cast(F, (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}); }

// 16-bit: attention_fwd16c_kernel (attention.hip) restricted to the band -- chunks start at the band's first key (any row: the
// DMA addresses rows one by one), the score of an out-of-band key is clamped to the masked value.  No bias, dropout or packed rows.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention_band16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int H, int heads, float scale, int w,
    const int* __restrict__ kmax) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + 128 * 128;
  float* const sM = (float*)(smem + 2 * 128 * 128);
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int64_t row0 = b * L;
  const int qb = blockIdx.y * 128;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld2 = 6 * (int64_t)H;                       // row pitch of qkv in bytes
  const char* const base = (const char*)(qkv + row0 * 3 * (int64_t)H + h * 64);
  const float LOG2E = 1.4426950408889634f;
  const int q0 = qb + wave * 32;
  const bool active = q0 < L;
  const int qi = q0 + l31;                                  // this lane's query (its band test uses the true index)
  const int qrow = qi < L ? qi : (L - 1);
  frag_t qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const frag_t*)(base + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  const float c2 = scale * LOG2E;
  const int key = (l31 >> 1) & 7;
  const int i16 = lane & 15;
  const char* const vt0 = sV + (4 * half + (i16 >> 2)) * 128 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  const int vsw = (i16 >> 3) & 1;
  int klo, khi;
  band_keys(qb, w, kmax ? __builtin_amdgcn_readfirstlane(kmax[b]) : L, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 128) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (i * 4 + wave) * 8 + (lane >> 3);
      const int rr = (kc + r) < L ? (kc + r) : (L - 1);
      const uint32_t off = (uint32_t)(rr * ld2) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
      const uint32_t offv = (uint32_t)(rr * ld2) + (((lane & 7) ^ (((r >> 1) & 1) << 2)) << 4);
      const uint32_t dst = (uint32_t)((i * 4 + wave) * 1024);
      g7_dma(base + 2 * H, off, g7_lds_addr(sK) + dst);
      g7_dma(base + 4 * H, offv, g7_lds_addr(sV) + dst);
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
    const int d0 = kc - qi;                                  // key - query of key kc
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = d0 + k0 + e;
          float v = fmaf(s[t][4 * g + e], c2, mb[e]);
          v = (d > w || d < -w) ? fminf(v, -1e30f) : v;
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds key klo < L (unmasked, or -1e30: finite): mx is finite from here on
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
          const frag_t vf = band_vfrag<frag_t>(band_vtrd(p), band_vtrd(p + 8 * 128));
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
  char* const out = (char*)(ctx + (row0 + q0) * (int64_t)H + h * 64);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (lane >> 3), c = lane & 7;
    const uint4 v = *(const uint4*)(so + row * 128 + ((c ^ (row & 7)) << 4));
    if (q0 + row < L) *(uint4*)(out + (int64_t)row * H * 2 + c * 16) = v;
  }
}

// float32: attention_long_kernel's layout (attention.hip) over the band's keys -- K row-major swizzled, V transposed, queries in
// registers, the per-query rescale through a 32-float LDS table per wave; natural exp, the mask's finfo.min.
__global__ __launch_bounds__(256) void attention_band32_kernel(
    const float* __restrict__ qkv, float* __restrict__ ctx, const int64_t* __restrict__ mask, int L, int H, int heads, float scale,
    int w, const int* __restrict__ kmax) {
  typedef AttnGeom<float> G;
  typedef typename MmaOps<float>::frag_t frag_t;
  constexpr int LP = 128 + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  float* sVt = (float*)(smem + 128 * G::ROWB);
  float* sM = (float*)(smem + 128 * G::ROWB + 64 * LP * 4);
  float* sF = sM + 128;                                     // [4 waves][32] per-query factors

  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int qb = blockIdx.y * 128;
  const int tid = threadIdx.x;
  const int64_t ld = 3 * (int64_t)H;
  const float* base = qkv + b * L * ld + h * 64;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = qb + wave * 32;
  const int qrow = (q0 + l31) < L ? (q0 + l31) : (L - 1);
  frag_t qf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) qf[kk] = *(const frag_t*)(base + (int64_t)qrow * ld + (kk * 2 + half) * G::EPC);
  int klo, khi;
  band_keys(qb, w, kmax ? kmax[b] : L, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 128) {
    __syncthreads();
    for (int idx = tid; idx < 128 * G::CPR; idx += 256) {
      const int row = idx / G::CPR, c = idx % G::CPR;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (kc + row < L) {
        kv = *(const uint4*)(base + (int64_t)(kc + row) * ld + H + c * G::EPC);
        vv = *(const uint4*)(base + (int64_t)(kc + row) * ld + 2 * H + c * G::EPC);
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
    const int d0 = kc - (q0 + l31);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = d0 + k0 + e;
          float v = s[t][4 * g + e] * scale + mb[e];
          v = (d > w || d < -w) ? fminf(v, kFinfoMin) : v;
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
    float* out = ctx + (b * L + q0) * H + h * 64;
    constexpr int VPR = G::ROWB / 16;
#pragma unroll
    for (int it = 0; it < 32 * VPR / 64; ++it) {
      const int idx = it * 64 + lane, row = idx / VPR, c = idx % VPR;
      const uint4 v = *(const uint4*)((const char*)so + row * G::ROWB + c * 16);
      if (q0 + row < L) *(uint4*)((char*)(out + (int64_t)row * H) + c * 16) = v;
    }
  }
}

}  // namespace

int omk_rope(int dtype, void* qkv, int64_t M, int L, int H, float theta, hipStream_t s) {
  if (M <= 0) return 0;
  if (L < 1 || L > kRopeMaxPos) OM_FAIL("rotary positions: sequence length must be in [1,1024]");
  if (H % 64 || !(theta > 0.f)) OM_FAIL("rotary positions: head_dim 64 and a positive theta");
  const float2* tab = nullptr;
  if (rope_table_device(theta, &tab)) return 1;
  const int64_t n = M * (H / 4);
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (dtype == OM_BF16) hipLaunchKernelGGL(rope_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (bf16_t*)qkv, tab, M, L, H);
  else if (dtype == OM_F16) hipLaunchKernelGGL(rope_kernel<f16_t>, dim3(grid), dim3(256), 0, s, (f16_t*)qkv, tab, M, L, H);
  else hipLaunchKernelGGL(rope_kernel<float>, dim3(grid), dim3(256), 0, s, (float*)qkv, tab, M, L, H);
  OM_LAUNCH_CHECK();
  return 0;
}

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
