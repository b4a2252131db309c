// The two key-chunked online-softmax attention bodies of attn_chunked.h at head_dim 256 (gfx950): the same walk -- a workgroup owns
// 128 queries of one (sequence, head), four waves of 32, with the running maximum m and sum l per query -- the same policies (AttnFull
// and AttnBand are the ones in use: Gemma3's bidirectional full and sliding layers) and the same AttnRows, with rows of 256 columns.
// What the row width changes: a query's fragments and the O^T accumulators alone are 64 + 128 registers in the 16-bit body (128 + 128
// in float32), so a wave takes more than 256 registers, a 256-thread workgroup runs ALONE on its CU whatever its LDS, and the key chunk
// is 64 keys, not 128: K and V of 64 keys at 512-byte rows are 64 KiB (128 keys would be 128 KiB of the CU's 160, with nothing left
// for the float32 body's padded rows), and a 64-key chunk halves the score registers.  AttnBand's key range is stated for a 128-query
// block and any chunk size; its select takes the key's offset in the chunk, so both policies serve these bodies unchanged.
//
//   attn_chunked16_d256   (16-bit formats): attn_chunked16 at four times the row width, 64-key chunks
//   attn_chunked32_d256   (float32, the parity mode): attn_chunked_qreg at four times the row width, 64-key chunks
//
// Masked and hidden keys keep the other bodies' finite values (-1e30 in the log2 domain / finfo.min), keys past L -inf, rows are
// clamped to L - 1 on load, so a fully masked query stays finite and nothing is read past the sequence.  DESIGN.md section 4.
#pragma once
#include "attn_chunked.h"

constexpr int kAttn16D256Lds = 2 * 64 * 512 + 64 * 4;                                   // K | V | mask
constexpr int kAttn32D256Lds = 64 * 260 * 4 + 256 * 68 * 4 + 64 * 4 + 128 * 4;          // K | V^T | mask | factors

// ---- the 16-bit body ------------------------------------------------------------------------------------------------------
// LDS: K [64][512 B] | V [64][512 B] | mask [64] f32 = 64.25 KiB.  A row is two 256-byte bank rows, 32 chunks of 16 bytes:
//   K: physical chunk = chunk ^ (row & 15) (the low four bits; the bank-row bit stays).  A K fragment read (ds_read_b128) takes ONE
//      chunk index of 16 rows that differ in row & 15 per 16-lane group -- sixteen distinct slots of one bank row.
//   V: physical chunk = chunk ^ ((row & 3) << 2): the 64-byte octants of a row permuted in fours by row & 3.  A transposing read
//      (ds_read_b64_tr_b16) takes, per 32-lane half, 64 bytes of the same columns from four consecutive rows -- rows 512 bytes apart
//      meet the same banks, the swizzle sends them to four distinct quarters of the bank row.
// Both are applied on the DMA's source address (the LDS image of an LDS-DMA instruction is lane-linear: 2 rows of 512 bytes) and again
// on the read.  Sixteen q fragments, eight O^T accumulators (a query per lane: the rescale is one multiply per register), the output
// parked in the wave's own 32 x 512 B of the K | V area.
template <typename T, typename Policy>
__device__ __forceinline__ void attn_chunked16_d256(const AttnRows<T>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                                    int qb, float scale) {
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + 64 * 512;
  float* const sM = (float*)(smem + 2 * 64 * 512);
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
  frag_t qf[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) qf[kk] = *(const frag_t*)(qbase + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  const float c2 = scale * LOG2E;
  const int key = l31 & 15;
  const int i16 = lane & 15;
  const int vq = i16 >> 2;                                  // row & 3 of the row this lane addresses in a transposing read
  const char* const vt0 = sV + (4 * half + vq) * 512 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 64) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    // K and V rows kc .. kc + 63: instruction i of wave w moves rows (i * 4 + w) * 2 and + 1, lane -> row (lane >> 5), physical chunk
    // (lane & 31) <- the source chunk the swizzle pairs with it
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = (i * 4 + wave) * 2 + (lane >> 5);
      const int rr = (kc + r) < L ? (kc + r) : (L - 1);
      const uint32_t rowoff = (uint32_t)(rr * ld2);
      const uint32_t swk = (uint32_t)(((lane & 31) ^ (r & 15)) << 4);
      const uint32_t swv = (uint32_t)(((lane & 31) ^ ((r & 3) << 2)) << 4);
      const uint32_t dst = (uint32_t)((i * 4 + wave) * 1024);
      g7_dma(kbase, rowoff + swk, g7_lds_addr(sK) + dst);
      g7_dma(vbase, rowoff + swv, g7_lds_addr(sV) + dst);
    }
    if (tid < 64) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : -1e30f) : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the DMA above is not in hipcc's bookkeeping
    __syncthreads();
    if (!active) continue;

    f32x16_t s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const char* krow = sK + (t * 32 + l31) * 512;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const frag_t ka = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(ka, qf[kk], s[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = fmaf(s[t][4 * g + e], c2, mb[e]);
          v = pol.select(v, pc, k0, e, -1e30f);
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds a key < L (unmasked, or -1e30: finite): mx is finite from here on
    const float alpha = __builtin_amdgcn_exp2f(m_run - mx);   // exp2(-inf) = 0 on the first chunk
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
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
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;        // O^T: this lane's query in every register
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint4 pa[2];      // probabilities of this key tile as two k slabs (k slot e of half h <-> register 8u + e)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        pa[u] = make_uint4(Half16<T>::pack2(s[t][8 * u + 0], s[t][8 * u + 1]), Half16<T>::pack2(s[t][8 * u + 2], s[t][8 * u + 3]),
                           Half16<T>::pack2(s[t][8 * u + 4], s[t][8 * u + 5]), Half16<T>::pack2(s[t][8 * u + 6], s[t][8 * u + 7]));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
          const char* p = vt0 + (t * 32 + 16 * u) * 512 + ((dt ^ vq) << 6);
          const frag_t vf = vfrag_of<frag_t>(vtrd(p), vtrd(p + 8 * 512));
          MmaOps<T>::mma(vf, __builtin_bit_cast(frag_t, pa[u]), o[dt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // O / l: one v_permlane32_swap per dword pair makes 16 contiguous bytes, parked in the wave's own 32 rows of the K | V area (chunk ^
  // (row & 15): the 16-byte stores and the row reads below both meet sixteen distinct slots) and written out as whole 512-byte rows
  __syncthreads();
  if (!active) return;
  const float inv = 1.0f / l_run;
  char* const so = smem + (wave * 32) * 512;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      uint32_t a0 = Half16<T>::pack2(o[dt][8 * gp + 0] * inv, o[dt][8 * gp + 1] * inv), a1 = Half16<T>::pack2(o[dt][8 * gp + 2] * inv, o[dt][8 * gp + 3] * inv);
      uint32_t b0 = Half16<T>::pack2(o[dt][8 * gp + 4] * inv, o[dt][8 * gp + 5] * inv), b1 = Half16<T>::pack2(o[dt][8 * gp + 6] * inv, o[dt][8 * gp + 7] * inv);
      auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      *(uint4*)(so + l31 * 512 + (((4 * dt + 2 * gp + half) ^ (l31 & 15)) << 4)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
  char* const out = (char*)(a.ctx + q0 * a.ldc);
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int row = it * 2 + (lane >> 5), c = lane & 31;
    const uint4 v = *(const uint4*)(so + row * 512 + ((c ^ (row & 15)) << 4));
    if (q0 + row < L) *(uint4*)(out + (int64_t)row * a.ldc * 2 + c * 16) = v;
  }
}

// ---- the float32 body -----------------------------------------------------------------------------------------------------
// attn_chunked32_d128 with 256 columns and 64-key chunks: the queries' thirty-two fragments and the eight accumulators O[query][d] in
// registers, d in lanes, the per-query factors through a 32-float LDS table per wave, natural exp.  LDS: K [64][1040 B] |
// V^T [256][68] | mask [64] | factors [4][32] = 133.75 KiB.  The K rows are 1024 bytes + 16 of padding instead of a swizzle:
// consecutive rows start one 16-byte slot apart in the bank row.  The parity mode: no speed target.
template <typename Policy>
__device__ __forceinline__ void attn_chunked32_d256(const AttnRows<float>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                                    int qb, float scale) {
  constexpr int LP = 256 + 4;                                // floats per K row (and per parked output row)
  constexpr int LV = 64 + 4;                                 // floats per V^T row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const sK = (float*)smem;
  float* const sVt = sK + 64 * LP;
  float* const sM = sVt + 256 * LV;
  float* const sF = sM + 64;                                 // [4 waves][32] per-query factors

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = qb + wave * 32;
  const int qi = q0 + l31;
  const int qrow = qi < L ? qi : (L - 1);
  f32x4_t qf[32];
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) qf[kk] = *(const f32x4_t*)(a.q + (int64_t)qrow * a.ld + (kk * 2 + half) * 4);

  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += 64) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      const int row = idx >> 6, c = idx & 63;
      f32x4_t kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (kc + row < L) {
        const int64_t off = (int64_t)(kc + row) * a.ld + c * 4;
        kv = *(const f32x4_t*)(a.k + off);
        vv = *(const f32x4_t*)(a.v + off);
      }
      *(f32x4_t*)(sK + row * LP + c * 4) = kv;
#pragma unroll
      for (int e = 0; e < 4; ++e) sVt[(c * 4 + e) * LV + row] = vv[e];
    }
    if (tid < 64) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : kFinfoMin) : -INFINITY;
    __syncthreads();

    f32x16_t s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const float* krow = sK + (t * 32 + l31) * LP;
#pragma unroll
      for (int kk = 0; kk < 32; ++kk) {
        const f32x4_t ka = *(const f32x4_t*)(krow + (kk * 2 + half) * 4);
        MmaOps<float>::mma(ka, qf[kk], s[t]);
      }
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = s[t][4 * g + e] * scale;
          v += mb[e];
          v = pol.select(v, pc, k0, e, kFinfoMin);
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds a key < L (unmasked, or finfo.min: finite): mx is finite from here on
    const float alpha = expf(m_run - mx);                    // exp(-inf) = 0 on the first chunk
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = expf(s[t][r] - mx);
        sum += e;
        s[t][r] = e;
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
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt][4 * g + e] *= a4[e];
    }
    // O[query][d] += P[query][key] V[key][d]: register r of half h <-> key (r & 3) + 8 (r >> 2) + 4 h of the tile (SlabMma<float>)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4_t vb = *(const f32x4_t*)(sVt + (dt * 32 + l31) * LV + t * 32 + 4 * half + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[t][4 * g + e], vb[e], o[dt], 0, 0, 0);
        }
  }
  // O / l, parked in the wave's own 32 rows of the K | V^T area (4 x 32 x 1040 B = 130 KiB of its 133), stored as whole 16-byte vectors
  __syncthreads();
  if (half == 0) sF[wave * 32 + l31] = 1.0f / l_run;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float* const so = sK + (wave * 32) * LP;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4_t i4 = *(const f32x4_t*)(sF + wave * 32 + 8 * g + 4 * half);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = 8 * g + 4 * half + e;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) so[q * LP + dt * 32 + l31] = o[dt][4 * g + e] * i4[e];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (q0 < L) {
    float* const out = a.ctx + q0 * a.ldc;
#pragma unroll
    for (int it = 0; it < 32; ++it) {
      const int idx = it * 64 + lane, row = idx >> 6, c = idx & 63;
      const f32x4_t v = *(const f32x4_t*)(so + row * LP + c * 4);
      if (q0 + row < L) *(f32x4_t*)(out + (int64_t)row * a.ldc + c * 4) = v;
    }
  }
}
