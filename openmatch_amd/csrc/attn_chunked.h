// The two key-chunked online-softmax attention bodies (head_dim 64, gfx950), each written ONCE and shared by three kernels.
//
// A workgroup owns 128 queries of one (sequence, head) -- four waves of 32 -- and walks 128-key chunks with the online softmax:
// running maximum m and sum l per query, O rescaled by exp(m_old - m_new) per chunk.  Constant registers and LDS for any length.
//
//   attn_chunked16   (16-bit formats): K and V rows by LDS-DMA, transposing V reads, exp2 softmax, O^T with a query per lane
//                    -> attention_fwd16c_kernel (attention.hip), attention_band16_kernel (attention_band.hip),
//                       attention_causal16_kernel (attention_causal.hip)
//   attn_chunked_qreg (any format; float32 is its main use): K staged swizzled, V transposed, queries in registers (SlabMma), natural exp
//                    -> attention_long_kernel, attention_band32_kernel, attention_causal32_kernel
//
// Which keys a query sees is a compile-time POLICY (AttnFull, AttnBand, AttnCausal below).  A policy states two things: the key range
// [lo, hi) a query block walks, and the select applied to each score of a visited chunk.  Where the rows live is an AttnRows the
// __global__ wrapper fills -- fused [M, 3H], grouped (heads + 2 kv) * 64, or packed rows from cu -- so a body knows no layout.
// Everything a policy decides is an inline that is empty where a kernel lacks it: no branch, register or LDS enters the chunk loop of
// a kernel for a rule it does not have.  The wrappers keep the __launch_bounds__, the grid (heads * B, ceil(L / 128)), 256 threads
// and the LDS sizes; DESIGN.md section 4.
#pragma once
#include "attn_common.h"
#include "gemm_core7.h"

// Row 0 of this workgroup's sequence, at this head's 64 columns, in the projection (q, k, v) and in the context; pitches in elements.
template <typename T>
struct AttnRows {
  const T* q;
  const T* k;
  const T* v;
  int64_t ld;      // elements per q / k / v row
  T* ctx;
  int64_t ldc;     // elements per ctx row
};

// the fused projection [M, 3H] (q | k | v) and ctx [M, H]: head h of the sequence whose first row is row0
template <typename T>
__device__ __forceinline__ AttnRows<T> attn_rows_fused(const T* qkv, T* ctx, int64_t row0, int H, int h) {
  const T* const base = qkv + row0 * 3 * (int64_t)H + h * 64;
  return {base, base + H, base + 2 * H, 3 * (int64_t)H, ctx + row0 * (int64_t)H + h * 64, H};
}

// the grouped projection [M, (heads + 2 kv_heads) * D] (q heads | k heads | v heads) and ctx [M, heads * D] for the sequence whose
// first row is row0 (b * L padded, cu[b] packed), query head h: it reads K / V head h / (heads / kv_heads) (HF repeat_kv)
template <int D, typename T>
__device__ __forceinline__ AttnRows<T> attn_rows_grouped(const T* qkv, T* ctx, int64_t row0, int heads, int kv_heads, int h) {
  const int kvh = h / (heads / kv_heads);
  const int pitch = (heads + 2 * kv_heads) * D;
  const T* const row = qkv + row0 * pitch;
  const T* const k = row + (heads + kvh) * D;
  return {row + h * D, k, k + kv_heads * D, pitch, ctx + row0 * (int64_t)(heads * D) + h * D, heads * D};
}

// What the full-attention kernels alone take: the T5 bias table and dropout, both keyed with the padded pitch Lm (also for packed
// rows: the backward kernels and a packed step regenerate the same dropout mask).  Band and causal pass AttnFullArgs{}.
struct AttnFullArgs {
  const float* pos_bias = nullptr;
  float drop_p = 0.f;
  uint64_t seed = 0;
  int64_t b = 0;
  int h = 0, heads = 0, Lm = 0;
};

// ---- visibility policies --------------------------------------------------------------------------------------------------
// keys(qb, kend, lo, hi): keys [lo, hi) the 128-query block starting at qb walks, kend the key extent (L, or kmax[b]: keys at or past
//   it are padding).  Never empty: the first chunk holds a key < L, scored finite, so the running maximum is finite from there on.
// chunk(kc, q0, qi): one int per (chunk, lane) -- q0 the wave's first query, qi this lane's (true index, not clipped to L) ...
// select(v, c, k0, e, masked): ... from which the score v of key kc + k0 + e becomes min(v, masked) when the key is hidden: finite,
//   like a padded key, so a (padded) query with no visible key averages the values it visited instead of producing NaN.
struct AttnFull {
  __device__ __forceinline__ void keys(int, int kend, int& lo, int& hi) const { lo = 0; hi = kend; }
  __device__ __forceinline__ int chunk(int, int, int) const { return 0; }
  __device__ __forceinline__ float select(float v, int, int, int, float) const { return v; }
};
// |q - k| <= w, inclusive at both ends (HF masking_utils.sliding_window_bidirectional_overlay)
struct AttnBand {
  int w;
  // the band, clipped to [0, kend); a block of padded queries beyond the band of every unmasked key still visits the last key
  __device__ __forceinline__ void keys(int qb, int kend, int& lo, int& hi) const {
    lo = qb - w > 0 ? qb - w : 0;
    hi = qb + 128 + w < kend ? qb + 128 + w : kend;
    if (hi <= lo) { hi = kend; lo = kend - 1; }
  }
  __device__ __forceinline__ int chunk(int kc, int, int qi) const { return kc - qi; }        // key - query of key kc
  __device__ __forceinline__ float select(float v, int c, int k0, int e, float masked) const {
    const int d = c + k0 + e;
    return (d > w || d < -w) ? fminf(v, masked) : v;
  }
};
// k <= q
struct AttnCausal {
  // up to the diagonal chunk, clipped to kend; a block of padded queries at or past kend visits the first chunk alone
  __device__ __forceinline__ void keys(int qb, int kend, int& lo, int& hi) const {
    lo = 0;
    hi = qb >= kend ? 1 : (qb + 128 < kend ? qb + 128 : kend);
  }
  // the diagonal chunk alone holds keys past a query of this block (kc <= qb always: every earlier chunk is wholly visible); keys
  // of it with index > the result lie in the future of this lane's query
  __device__ __forceinline__ int chunk(int kc, int q0, int qi) const { return kc + 127 > q0 ? qi - kc : 128; }
  __device__ __forceinline__ float select(float v, int c, int k0, int e, float masked) const { return k0 + e > c ? fminf(v, masked) : v; }
};

// ---- the 16-bit body ------------------------------------------------------------------------------------------------------
// Per chunk: K and V rows by LDS-DMA (row-major, swizzled on the source address), S^T = K Q^T, exp2 softmax against the running
// maximum, V^T fragments by transposing LDS reads.  O^T keeps a query per LANE, so the rescaling by exp2(m_old - m_new) is one
// multiply per accumulator register with the lane's own factor.  Softmax in the log2 domain: v = fma(s, scale log2e, mask).  Masked
// and hidden keys carry -1e30 (finite: a fully masked row stays uniform, as with HF's finfo.min), keys past L -inf.
// LDS: K [128][128 B] | V [128][128 B] | mask [128] f32.  L: this sequence's rows; mask_row: its mask row; qb: the block's first query.
// BIAS, DROP: with AttnFull only.  Measured at 16 x 512 tokens, 12 heads: profiles/r06_train_long_sequences.txt.
template <typename T, typename Policy, bool BIAS, bool DROP>
__device__ __forceinline__ void attn_chunked16(const AttnRows<T>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                               int qb, float scale, const AttnFullArgs& x) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + 128 * 128;
  float* const sM = (float*)(smem + 2 * 128 * 128);
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld2 = 2 * a.ld;                             // row pitch of q / k / v in bytes
  const char* const qbase = (const char*)a.q;
  const char* const kbase = (const char*)a.k;
  const char* const vbase = (const char*)a.v;
  const float LOG2E = 1.4426950408889634f;
  const int q0 = qb + wave * 32;
  const bool active = q0 < L;                               // (wave-uniform; an inactive wave still fetches its share of every chunk)
  const int qi = q0 + l31;                                  // this lane's query (a policy's test uses the true index)
  const int qrow = qi < L ? qi : (L - 1);
  frag_t qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const frag_t*)(qbase + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  const float c2 = scale * LOG2E;
  const AttnDrop dr(x.drop_p);
  const int key = (l31 >> 1) & 7;
  const int i16 = lane & 15;
  const char* const vt0 = sV + (4 * half + (i16 >> 2)) * 128 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  const int vsw = (i16 >> 3) & 1;
  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 128) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    // K and V rows kc .. kc + 127 (any first row: the DMA addresses rows one by one): instruction i of wave w moves rows
    // (i * 4 + w) * 8 .. + 7, lane -> row (lane >> 3), physical 16-byte chunk (lane & 7) <- source chunk (lane & 7) ^ ((row >> 1) & 7)
    // for K, ^ 4 ((row >> 1) & 1) for V (attention_fwd16_body, attention.hip)
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
    if (tid < 128) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : -1e30f) : -INFINITY;
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
        const frag_t ka = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(ka, qf[kk], s[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
        f32x4_t pb = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BIAS) {
          const float* pr = x.pos_bias + ((int64_t)x.h * x.Lm + qrow) * x.Lm;      // (the table's pitch: the padded length, also for packed rows)
#pragma unroll
          for (int e = 0; e < 4; ++e) pb[e] = pr[(kc + k0 + e) < x.Lm ? (kc + k0 + e) : (x.Lm - 1)] * LOG2E;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = fmaf(s[t][4 * g + e], c2, mb[e]);
          // (attention_fwd16c_kernel has always added pb, zeros without BIAS -- an add the compiler must keep; band and causal never
          // did.  Kept as found: dropping it is a change of arithmetic, not of structure.)
          if constexpr (std::is_same<Policy, AttnFull>::value) v += pb[e];
          v = pol.select(v, pc, k0, e, -1e30f);
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds a key < L (unmasked, or -1e30: finite): mx is finite from here on
    const float alpha = __builtin_amdgcn_exp2f(m_run - mx);   // exp2(-inf) = 0 on the first chunk
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
    if constexpr (DROP) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint64_t bits = attn_drop_bits(x.seed, x.b, x.h, x.heads, x.Lm, qi, (kc + t * 32 + 8 * g + 4 * half) >> 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) s[t][4 * g + e] = attn_drop_keep(bits, e, dr.thresh) ? s[t][4 * g + e] : 0.f;
          __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;        // O^T: this lane's query in every register
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint4 pa[2];      // probabilities of this key tile as two k slabs (k slot e of half h <-> register 8u + e)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        pa[u] = make_uint4(Half16<T>::pack2(s[t][8 * u + 0], s[t][8 * u + 1]), Half16<T>::pack2(s[t][8 * u + 2], s[t][8 * u + 3]),
                           Half16<T>::pack2(s[t][8 * u + 4], s[t][8 * u + 5]), Half16<T>::pack2(s[t][8 * u + 6], s[t][8 * u + 7]));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const char* p = vt0 + (t * 32 + 16 * u) * 128 + ((dt ^ vsw) << 6);
          const frag_t vf = vfrag_of<frag_t>(vtrd(p), vtrd(p + 8 * 128));
          MmaOps<T>::mma(vf, __builtin_bit_cast(frag_t, pa[u]), o[dt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // O / l (x the keep scale): one v_permlane32_swap per dword pair makes 16 contiguous bytes, parked in the wave's own K rows and
  // written out as whole 128-byte rows
  __syncthreads();
  if (!active) return;
  const float inv = (DROP ? dr.keep_scale : 1.0f) / l_run;
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
  char* const out = (char*)(a.ctx + q0 * a.ldc);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (lane >> 3), c = lane & 7;
    const uint4 v = *(const uint4*)(so + row * 128 + ((c ^ (row & 7)) << 4));
    if (q0 + row < L) *(uint4*)(out + (int64_t)row * a.ldc * 2 + c * 16) = v;
  }
}

// ---- the queries-in-registers body ----------------------------------------------------------------------------------------
// K chunk row-major (swizzled), V chunk transposed, as in attention_kernel<T, 4>; the accumulators O[query][d] keep queries in
// REGISTERS and d in lanes (SlabMma), so the per-query factors travel through a 32-float LDS table per wave.  Natural exp; masked and
// hidden keys carry finfo.min, keys past L -inf.  K / V are re-read once per 128 queries (L2).
// LDS: K [128][ROWB] | V^T [64][132] T | mask [128] f32 | factors [4 waves][32] f32.
// x.pos_bias != NULL: the T5 table added to the scaled score.  x.drop_p > 0 (training beyond 256 tokens): the probabilities that meet V
// are masked with the (sequence, head, query, key) hash the backward regenerates (attn_common.h) and scaled one by one; the
// normaliser is the sum taken before the drop, as in the other kernels.  Both are run-time tests that fold away in band and causal.
template <typename T, typename Policy>
__device__ __forceinline__ void attn_chunked_qreg(const AttnRows<T>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                                  int qb, float scale, const AttnFullArgs& x) {
  typedef AttnGeom<T> G;
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int LP = 128 + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  T* sVt = (T*)(smem + 128 * G::ROWB);
  float* sM = (float*)(smem + 128 * G::ROWB + 64 * LP * (int)sizeof(T));
  float* sF = sM + 128;                                     // [4 waves][32] per-query factors

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = qb + wave * 32;
  const int qi = q0 + l31;
  const int qrow = qi < L ? qi : (L - 1);
  frag_t qf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) qf[kk] = *(const frag_t*)(a.q + (int64_t)qrow * a.ld + (kk * 2 + half) * G::EPC);

  const AttnDrop dr_(x.drop_p);
  const uint32_t thresh = dr_.thresh;
  const float keep_scale = dr_.keep_scale;
  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 128) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    for (int idx = tid; idx < 128 * G::CPR; idx += 256) {
      const int row = idx / G::CPR, c = idx % G::CPR;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (kc + row < L) {
        const int64_t off = (int64_t)(kc + row) * a.ld + c * G::EPC;
        kv = *(const uint4*)(a.k + off);
        vv = *(const uint4*)(a.v + off);
      }
      *(uint4*)(sK + row * G::ROWB + ((c ^ G::key(row)) << 4)) = kv;
      const T* ve = (const T*)&vv;
#pragma unroll
      for (int e = 0; e < G::EPC; ++e) sVt[(c * G::EPC + e) * LP + row] = ve[e];
    }
    if (tid < 128) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : kFinfoMin) : -INFINITY;
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
        const frag_t ka = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(ka, qf[kk], s[t]);
      }
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = s[t][4 * g + e] * scale;
          if (x.pos_bias) {
            const int kcol = (kc + k0 + e) < L ? (kc + k0 + e) : (L - 1);
            v += x.pos_bias[((int64_t)x.h * x.Lm + qrow) * x.Lm + kcol];
          }
          v += mb[e];
          v = pol.select(v, pc, k0, e, kFinfoMin);
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds a key < L (unmasked, or finfo.min: finite): mx is finite from here on
    const float alpha = G::exp_(m_run - mx);                 // exp(-inf) = 0 on the first chunk
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = G::exp_(s[t][r] - mx);
        sum += e;
        s[t][r] = (thresh && !attn_drop_keep1(x.seed, x.b, x.h, x.heads, x.Lm, qi, kc + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, thresh)) ? 0.f : (thresh ? e * keep_scale : e);
      }
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = mx;
    // rescale O: the factor of query q lives in lane q; O holds queries in registers -> through the wave's table
    if (half == 0) sF[wave * 32 + l31] = alpha;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (same wave: LDS operations execute in order)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4_t a4 = *(const f32x4_t*)(sF + wave * 32 + 8 * g + 4 * half);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[0][4 * g + e] *= a4[e]; o[1][4 * g + e] *= a4[e]; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) SlabMma<T>::run(s[t], sVt + l31 * LP + t * 32 + 4 * half, LP, o);
  }
  // O / l, parked in the wave's own K rows, stored as whole 16-byte vectors
  __syncthreads();
  if (half == 0) sF[wave * 32 + l31] = 1.0f / l_run;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  T* so = (T*)(sK + (size_t)(wave * 32) * G::ROWB);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4_t i4 = *(const f32x4_t*)(sF + wave * 32 + 8 * g + 4 * half);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = 8 * g + 4 * half + e;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) ElemOps<T>::store(so + q * 64 + dt * 32 + l31, o[dt][4 * g + e] * i4[e]);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (q0 < L) {
    T* out = a.ctx + q0 * a.ldc;
    constexpr int VPR = G::ROWB / 16;
#pragma unroll
    for (int it = 0; it < 32 * VPR / 64; ++it) {
      const int idx = it * 64 + lane, row = idx / VPR, c = idx % VPR;
      const uint4 v = *(const uint4*)((const char*)so + row * G::ROWB + c * 16);
      if (q0 + row < L) *(uint4*)((char*)(out + (int64_t)row * a.ldc) + c * 16) = v;
    }
  }
}
