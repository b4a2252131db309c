// The two key-chunked online-softmax attention bodies of attn_chunked.h for heads wider than 64 columns (gfx950), each written ONCE
// for head_dim D = 128 and D = 256: the same walk -- a workgroup owns 128 queries of one (sequence, head), four waves of 32, and visits
// key chunks with the running maximum m and sum l per query -- the same policies and the same AttnRows.  Everything the row width
// decides is a member of AttnWide<D> below.
//
//   attn_chunked16_wide<D, T, Policy>   (16-bit formats): attn_chunked16 at D / 64 times the row width
//        -> attention_causal16_d128_kernel (attention_causal128.hip: AttnCausal), attention_d256_16_kernel (attention_d256.hip:
//           AttnFull and AttnBand, Gemma3's bidirectional full and sliding layers)
//   attn_chunked32_wide<D, Policy>      (float32, the parity mode): attn_chunked_qreg at D / 64 times the row width
//        -> attention_causal32_d128_kernel, attention_d256_32_kernel
//
// At the end of the file: attn_grouped_padded / attn_grouped_packed, what the __global__ wrappers over the grouped projection do at
// any head_dim (64 included: attention_causal.hip).
//
// Masked and hidden keys keep the 64-wide bodies' finite values (-1e30 in the log2 domain / finfo.min), keys past L -inf, rows are
// clamped to L - 1 on load, so a fully masked query stays finite and nothing is read past the sequence.  DESIGN.md section 4.
//
// NOT folded in: the 64-wide bodies of attn_chunked.h.  What differs there, for whoever takes that step (it needs its own assembly
// check, tools/isa_diff.py): their 128-byte rows are HALF a bank row, so the K swizzle is chunk ^ ((row >> 1) & 7) and the V swizzle
// chunk ^ (((row >> 1) & 1) << 2), and the transposing read picks its half with (i16 >> 3) & 1 where these bodies use row & 3;
// attn_chunked16 carries BIAS and DROP (the T5 table and dropout of the full-attention kernels); attn_chunked_qreg is generic over the
// storage type through AttnGeom / SlabMma, stages K swizzled instead of padded and serves 16-bit kernels too.
#pragma once
#include "attn_chunked.h"

// The geometry of both bodies at head_dim D.
// KC, the key chunk, is a CHOICE, not a formula.  128 keys at D = 128, as in the 64-wide bodies.  64 keys at D = 256: a query's
// fragments and the O^T accumulators alone are 64 + 128 registers in the 16-bit body (128 + 128 in float32), so a wave takes more
// than 256 registers and a 256-thread workgroup runs ALONE on its CU whatever its LDS; K and V of 64 keys at 512-byte rows are 64 KiB
// (128 keys would be 128 KiB of the CU's 160, with nothing left for the float32 body's padded rows), and a 64-key chunk halves the
// score registers.  AttnBand's key range is stated for a 128-query block and any chunk size and its select takes the key's offset in
// the chunk, so both policies in use at D = 256 (AttnFull, AttnBand) serve these bodies unchanged.
template <int D>
struct AttnWide {
  static_assert(D == 128 || D == 256, "head_dim 128 or 256");
  static constexpr int KC = D == 128 ? 128 : 64;             // keys per chunk
  static constexpr int NT = KC / 32;                         // score tiles (32 keys x 32 queries) per chunk
  static constexpr int NACC = D / 32;                        // output accumulators per wave
  // the 16-bit body
  static constexpr int ROWB = 2 * D;                         // bytes per K / V row: one (D = 128) or two (256) 256-byte bank rows
  static constexpr int CPR = ROWB / 16;                      // 16-byte chunks per row
  static constexpr int CSHIFT = D == 128 ? 4 : 5;            // lane >> CSHIFT: the lane's row in a lane-linear 1 KiB image ...
  static constexpr int CMASK = CPR - 1;                      // ... lane & CMASK: its chunk
  static constexpr int DMA_ROWS = 1024 / ROWB;               // rows one LDS-DMA instruction moves
  static constexpr int NDMA = KC / (4 * DMA_ROWS);           // instructions per wave, chunk and operand
  static constexpr int NQ16 = D / 16;                        // q fragments: each 32-lane half takes every other 16-byte chunk of the row
  static constexpr int LDS16 = 2 * KC * ROWB + KC * 4;       // K | V | mask
  // the float32 body
  static constexpr int VPR = D / 4;                          // 16-byte vectors per row
  static constexpr int VSHIFT = CSHIFT + 1;                  // idx >> VSHIFT, idx & (VPR - 1): row and vector of a linear index
  static constexpr int NQ32 = D / 8;                         // q fragments (every other 16-byte vector, as above)
  static constexpr int LPK = D + 4;                          // floats per K row (and per parked output row): 16 bytes of padding
  static constexpr int LPV = KC + 4;                         // floats per V^T row
  static constexpr int LDS32 = KC * LPK * 4 + D * LPV * 4 + KC * 4 + 128 * 4;      // K | V^T | mask | factors
  static_assert((1 << CSHIFT) == CPR && NDMA == 8, "the DMA's lane map");
};
static_assert(AttnWide<128>::LDS16 == 66048 && AttnWide<128>::LDS32 == 136192, "DESIGN.md section 4 documents these");
static_assert(AttnWide<256>::LDS16 == 65792 && AttnWide<256>::LDS32 == 136960, "DESIGN.md section 4 documents these");

// ---- the 16-bit body ------------------------------------------------------------------------------------------------------
// LDS: K [KC][ROWB] | V [KC][ROWB] | mask [KC] f32 = 64.5 KiB at D = 128 (two workgroups per CU), 64.25 KiB at 256.  A row is one or
// two whole 256-byte bank rows of 16 chunks of 16 bytes, so the swizzles differ from the 128-byte rows of attn_chunked16:
//   K: physical chunk = chunk ^ (row & 15) (the low four bits; at D = 256 the bank-row bit stays).  A K fragment read (ds_read_b128)
//      takes ONE chunk index of 16 rows that differ in row & 15 per 16-lane group -- sixteen distinct slots of one bank row.
//   V: physical chunk = chunk ^ ((row & 3) << 2): the 64-byte pieces of a row permuted in fours by row & 3.  A transposing read
//      (ds_read_b64_tr_b16) takes, per 32-lane half, 64 bytes of the same columns from four consecutive rows -- at D = 128 four
//      distinct quarters of the bank row, all 64 banks once; at D = 256 rows 512 bytes apart meet the same banks and the swizzle sends
//      them to four distinct quarters.  The two chunks of a 32-byte block never swap, as the read's addressing requires.
// Both are applied on the DMA's source address (the LDS image of an LDS-DMA instruction is lane-linear: DMA_ROWS rows of ROWB bytes)
// and again on the read.  NQ16 q fragments, NACC O^T accumulators (a query per lane: the rescale is one multiply per register), the
// output parked in the wave's own 32 x ROWB bytes at the start of LDS: its K rows at D = 128, K and V rows at D = 256.
//
// At D = 128 the kernel sits at its 256-register limit with two workgroups per CU, and three devices keep it out of scratch (each
// under `if constexpr (D == 128)`; at D = 256 the workgroup is alone on its CU with 512 registers and none of them is wanted).
template <int D, typename T, typename Policy>
__device__ __forceinline__ void attn_chunked16_wide(const AttnRows<T>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                                    int qb, float scale) {
  typedef AttnWide<D> W;
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + W::KC * W::ROWB;
  float* const sM = (float*)(smem + 2 * W::KC * W::ROWB);
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
  frag_t qf[W::NQ16];
#pragma unroll
  for (int kk = 0; kk < W::NQ16; ++kk) qf[kk] = *(const frag_t*)(qbase + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  const float c2 = scale * LOG2E;
  const int key = l31 & 15;
  const int i16 = lane & 15;
  const int vq = i16 >> 2;                                  // row & 3 of the row this lane addresses in a transposing read
  const char* const vt0 = sV + (4 * half + vq) * W::ROWB + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  // (D = 128, device 1) the DMA's source chunks, out of the chunk loop: row & 15 = wave * 4 + (lane >> 4) and row & 3 = lane >> 4 in
  // every one of a wave's instructions
  uint32_t swk128 = 0, swv128 = 0;
  if constexpr (D == 128) {
    swk128 = (uint32_t)(((lane & 15) ^ (wave * 4 + (lane >> 4))) << 4);
    swv128 = (uint32_t)(((lane & 15) ^ ((lane >> 4) << 2)) << 4);
  }
  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[W::NACC];
#pragma unroll
  for (int dt = 0; dt < W::NACC; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += W::KC) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    // K and V rows kc .. kc + KC - 1: instruction i of wave w moves rows (i * 4 + w) * DMA_ROWS .. + DMA_ROWS - 1, lane -> row
    // (lane >> CSHIFT), physical chunk (lane & CMASK) <- the source chunk the swizzle pairs with it
#pragma unroll
    for (int i = 0; i < W::NDMA; ++i) {
      const int r = (i * 4 + wave) * W::DMA_ROWS + (lane >> W::CSHIFT);
      const int rr = (kc + r) < L ? (kc + r) : (L - 1);
      const uint32_t rowoff = (uint32_t)(rr * ld2);
      const uint32_t swk = D == 128 ? swk128 : (uint32_t)(((lane & W::CMASK) ^ (r & 15)) << 4);
      const uint32_t swv = D == 128 ? swv128 : (uint32_t)(((lane & W::CMASK) ^ ((r & 3) << 2)) << 4);
      const uint32_t dst = (uint32_t)((i * 4 + wave) * 1024);
      g7_dma(kbase, rowoff + swk, g7_lds_addr(sK) + dst);
      g7_dma(vbase, rowoff + swv, g7_lds_addr(sV) + dst);
    }
    if (tid < W::KC) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : -1e30f) : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the DMA above is not in hipcc's bookkeeping
    __syncthreads();
    if (!active) continue;

    f32x16_t s[W::NT];
#pragma unroll
    for (int t = 0; t < W::NT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const char* krow = sK + (t * 32 + l31) * W::ROWB;
#pragma unroll
      for (int kk = 0; kk < W::NQ16; ++kk) {
        const frag_t ka = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(ka, qf[kk], s[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
    // (D = 128, device 2) the mask words of a key tile are read one tile ahead and no further (the fences): left alone the compiler
    // issues all sixteen reads at once, 64 registers next to s, o and q
    f32x4_t mbn[4];
    if constexpr (D == 128) {
#pragma unroll
      for (int g = 0; g < 4; ++g) mbn[g] = *(const f32x4_t*)(sM + 8 * g + 4 * half);
    }
#pragma unroll
    for (int t = 0; t < W::NT; ++t) {
      f32x4_t mbt[4];
      if constexpr (D == 128) {
#pragma unroll
        for (int g = 0; g < 4; ++g) mbt[g] = mbn[g];
        asm volatile("" ::: "memory");
        if (t < W::NT - 1) {
#pragma unroll
          for (int g = 0; g < 4; ++g) mbn[g] = *(const f32x4_t*)(sM + (t + 1) * 32 + 8 * g + 4 * half);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = t * 32 + 8 * g + 4 * half;
        f32x4_t mb;
        if constexpr (D == 128) mb = mbt[g];
        else mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = fmaf(s[t][4 * g + e], c2, mb[e]);
          v = pol.select(v, pc, k0, e, -1e30f);
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
        if constexpr (D == 128) __builtin_amdgcn_sched_barrier(0);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds a key < L (unmasked, or -1e30: finite): mx is finite from here on
    const float alpha = __builtin_amdgcn_exp2f(m_run - mx);   // exp2(-inf) = 0 on the first chunk
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < W::NT; ++t)
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
    for (int dt = 0; dt < W::NACC; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;        // O^T: this lane's query in every register
#pragma unroll
    for (int t = 0; t < W::NT; ++t) {
      uint4 pa[2];      // probabilities of this key tile as two k slabs (k slot e of half h <-> register 8u + e)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        pa[u] = make_uint4(Half16<T>::pack2(s[t][8 * u + 0], s[t][8 * u + 1]), Half16<T>::pack2(s[t][8 * u + 2], s[t][8 * u + 3]),
                           Half16<T>::pack2(s[t][8 * u + 4], s[t][8 * u + 5]), Half16<T>::pack2(s[t][8 * u + 6], s[t][8 * u + 7]));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int dt = 0; dt < W::NACC; ++dt) {
          const char* p = vt0 + (t * 32 + 16 * u) * W::ROWB + ((dt ^ vq) << 6);
          const frag_t vf = vfrag_of<frag_t>(vtrd(p), vtrd(p + 8 * W::ROWB));
          MmaOps<T>::mma(vf, __builtin_bit_cast(frag_t, pa[u]), o[dt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // O / l: one v_permlane32_swap per dword pair makes 16 contiguous bytes, parked in the wave's own 32 rows at the start of LDS (chunk
  // ^ (row & 15): the 16-byte stores and the row reads below both meet sixteen distinct slots) and written out as whole rows
  __syncthreads();
  if (!active) return;
  const float inv = 1.0f / l_run;
  char* const so = sK + (wave * 32) * W::ROWB;
  // (D = 128, device 3) the lane index anew, opaque to the compiler: it would otherwise compute this epilogue's addresses ahead of the
  // chunk loop and carry them through it -- in scratch, at two workgroups per CU
  int lane_e = lane;
  if constexpr (D == 128) {
    lane_e = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_e));
  }
  {
  const int lane = lane_e, half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int dt = 0; dt < W::NACC; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      uint32_t a0 = Half16<T>::pack2(o[dt][8 * gp + 0] * inv, o[dt][8 * gp + 1] * inv), a1 = Half16<T>::pack2(o[dt][8 * gp + 2] * inv, o[dt][8 * gp + 3] * inv);
      uint32_t b0 = Half16<T>::pack2(o[dt][8 * gp + 4] * inv, o[dt][8 * gp + 5] * inv), b1 = Half16<T>::pack2(o[dt][8 * gp + 6] * inv, o[dt][8 * gp + 7] * inv);
      auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      *(uint4*)(so + l31 * W::ROWB + (((4 * dt + 2 * gp + half) ^ (l31 & 15)) << 4)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
  char* const out = (char*)(a.ctx + q0 * a.ldc);
#pragma unroll
  for (int it = 0; it < 32 / W::DMA_ROWS; ++it) {
    const int row = it * W::DMA_ROWS + (lane >> W::CSHIFT), c = lane & W::CMASK;
    const uint4 v = *(const uint4*)(so + row * W::ROWB + ((c ^ (row & 15)) << 4));
    if (q0 + row < L) *(uint4*)(out + (int64_t)row * a.ldc * 2 + c * 16) = v;
  }
  }
}

// ---- the float32 body -----------------------------------------------------------------------------------------------------
// attn_chunked_qreg with D columns: the queries' NQ32 fragments and the NACC accumulators O[query][d] in registers, d in lanes, the
// per-query factors through a 32-float LDS table per wave, natural exp.  LDS: K [KC][LPK] | V^T [D][LPV] | mask [KC] |
// factors [4][32] = 133 KiB at D = 128, 133.75 KiB at 256, one workgroup per CU.  The K rows are 4 D bytes + 16 of padding instead of
// a swizzle: consecutive rows start one 16-byte slot apart in the bank row, so the sixteen rows of a fragment read's lane group meet
// sixteen distinct slots.  The parity mode: no speed target.
// (Linear indices are split into row and vector with a shift and a mask: `/` and `%` on int give other code at D = 256.)
template <int D, typename Policy>
__device__ __forceinline__ void attn_chunked32_wide(const AttnRows<float>& a, const Policy pol, const int64_t* __restrict__ mask_row, int L, int kend,
                                                    int qb, float scale) {
  typedef AttnWide<D> W;
  constexpr int LP = W::LPK, LV = W::LPV;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const sK = (float*)smem;
  float* const sVt = sK + W::KC * LP;
  float* const sM = sVt + D * LV;
  float* const sF = sM + W::KC;                              // [4 waves][32] per-query factors

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = qb + wave * 32;
  const int qi = q0 + l31;
  const int qrow = qi < L ? qi : (L - 1);
  f32x4_t qf[W::NQ32];
#pragma unroll
  for (int kk = 0; kk < W::NQ32; ++kk) qf[kk] = *(const f32x4_t*)(a.q + (int64_t)qrow * a.ld + (kk * 2 + half) * 4);

  int klo, khi;
  pol.keys(qb, kend, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o[W::NACC];
#pragma unroll
  for (int dt = 0; dt < W::NACC; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  for (int kc = klo; kc < khi; kc += W::KC) {
    __syncthreads();                                         // the previous chunk has been consumed by every wave
    for (int idx = tid; idx < W::KC * W::VPR; idx += 256) {
      const int row = idx >> W::VSHIFT, c = idx & (W::VPR - 1);
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
    if (tid < W::KC) sM[tid] = (kc + tid) < L ? (mask_row[kc + tid] != 0 ? 0.f : kFinfoMin) : -INFINITY;
    __syncthreads();

    f32x16_t s[W::NT];
#pragma unroll
    for (int t = 0; t < W::NT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const float* krow = sK + (t * 32 + l31) * LP;
#pragma unroll
      for (int kk = 0; kk < W::NQ32; ++kk) {
        const f32x4_t ka = *(const f32x4_t*)(krow + (kk * 2 + half) * 4);
        MmaOps<float>::mma(ka, qf[kk], s[t]);
      }
    }
    const int pc = pol.chunk(kc, q0, qi);
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < W::NT; ++t)
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
    for (int t = 0; t < W::NT; ++t)
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
        for (int dt = 0; dt < W::NACC; ++dt) o[dt][4 * g + e] *= a4[e];
    }
    // O[query][d] += P[query][key] V[key][d]: register r of half h <-> key (r & 3) + 8 (r >> 2) + 4 h of the tile (SlabMma<float>)
#pragma unroll
    for (int t = 0; t < W::NT; ++t)
#pragma unroll
      for (int dt = 0; dt < W::NACC; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4_t vb = *(const f32x4_t*)(sVt + (dt * 32 + l31) * LV + t * 32 + 4 * half + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[t][4 * g + e], vb[e], o[dt], 0, 0, 0);
        }
  }
  // O / l, parked in the wave's own 32 rows of LPK floats at the start of LDS (its K rows at D = 128; at D = 256 the four waves'
  // 4 x 32 x 1040 B = 130 KiB run through K into V^T, inside the 133 KiB), stored as whole 16-byte vectors
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
      for (int dt = 0; dt < W::NACC; ++dt) so[q * LP + dt * 32 + l31] = o[dt][4 * g + e] * i4[e];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (q0 < L) {
    float* const out = a.ctx + q0 * a.ldc;
#pragma unroll
    for (int it = 0; it < W::VPR / 2; ++it) {
      const int idx = it * 64 + lane, row = idx >> W::VSHIFT, c = idx & (W::VPR - 1);
      const f32x4_t v = *(const f32x4_t*)(so + row * LP + c * 4);
      if (q0 + row < L) *(f32x4_t*)(out + (int64_t)row * a.ldc + c * 4) = v;
    }
  }
}

// ---- the grouped-heads wrappers (any head_dim) ----------------------------------------------------------------------------
// What every __global__ wrapper over the grouped projection does on its grid (heads * B, ceil(L / 128)), once for padded rows and once
// for packed ones: find the head, the sequence and the 128-query block, fill the AttnRows (attn_rows_grouped) and run the body of its
// head_dim D and storage type T.  How they are written is pinned by the kernels' code, checked with tools/isa_diff.py:
//   * they CALL the body: a struct of (row0, L, kend, mask row, qb) handed back to the wrapper moves the scalar preamble of every kernel;
//   * the order of evaluation is the wrappers' as found -- the 16-bit ones read kmax[b] / cu[b] through readfirstlane and ahead of the
//     rows, the float32 ones plainly and, for kmax[b], after the mask row (F32 is a constant: one arm of each `?:` on it exists);
//   * the choice of body is spelled out in both: one more inlined call level between a wrapper and a float32 body swaps operands in
//     the causal kernels' write-out (their index arithmetic is reassociated together with the preamble's).
// Padded rows: sequence b is rows b * L .. + L - 1; keys at or past kmax[b] are padding (kmax NULL: none are).
template <int D, typename T, typename Policy>
__device__ __forceinline__ void attn_grouped_padded(const T* qkv, T* ctx, const int64_t* mask, int L, int heads, int kv_heads, float scale, const Policy pol,
                                                    const int* kmax) {
  constexpr bool F32 = std::is_same<T, float>::value;
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int kend16 = F32 ? 0 : (kmax ? __builtin_amdgcn_readfirstlane(kmax[b]) : L);
  const AttnRows<T> a = attn_rows_grouped<D>(qkv, ctx, b * L, heads, kv_heads, h);
  const int64_t* const mask_row = mask + b * L;
  const int kend = F32 ? (kmax ? kmax[b] : L) : kend16;
  const int qb = blockIdx.y * 128;
  if constexpr (D == 64 && F32) attn_chunked_qreg<float, Policy>(a, pol, mask_row, L, kend, qb, scale, AttnFullArgs{});
  else if constexpr (D == 64) attn_chunked16<T, Policy, false, false>(a, pol, mask_row, L, kend, qb, scale, AttnFullArgs{});
  else if constexpr (F32) attn_chunked32_wide<D, Policy>(a, pol, mask_row, L, kend, qb, scale);
  else attn_chunked16_wide<D, T, Policy>(a, pol, mask_row, L, kend, qb, scale);
}

// Packed rows: sequence b is rows cu[b] .. cu[b + 1] - 1 (omk_pack_rows), which is the body's L and its key extent; the mask row keeps
// the padded pitch Lp, so masked tokens inside the extent stay masked.  The grid is the padded launch's, (heads * B, ceil(Lp / 128)): a
// query block at or past the sequence's end -- every block of a sequence the row bound clamped to no rows -- leaves before it touches
// LDS or memory, so no row outside [cu[b], cu[b + 1]) is read or written.
template <int D, typename T, typename Policy>
__device__ __forceinline__ void attn_grouped_packed(const T* qkv, T* ctx, const int64_t* mask, int Lp, int heads, int kv_heads, float scale, const Policy pol,
                                                    const int* cu) {
  constexpr bool F32 = std::is_same<T, float>::value;
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int row0 = F32 ? cu[b] : __builtin_amdgcn_readfirstlane(cu[b]);
  const int Lb = (F32 ? cu[b + 1] : __builtin_amdgcn_readfirstlane(cu[b + 1])) - row0;
  const int qb = blockIdx.y * 128;
  if (qb >= Lb) return;
  const AttnRows<T> a = attn_rows_grouped<D>(qkv, ctx, (int64_t)row0, heads, kv_heads, h);
  const int64_t* const mask_row = mask + b * Lp;
  if constexpr (D == 64 && F32) attn_chunked_qreg<float, Policy>(a, pol, mask_row, Lb, Lb, qb, scale, AttnFullArgs{});
  else if constexpr (D == 64) attn_chunked16<T, Policy, false, false>(a, pol, mask_row, Lb, Lb, qb, scale, AttnFullArgs{});
  else if constexpr (F32) attn_chunked32_wide<D, Policy>(a, pol, mask_row, Lb, Lb, qb, scale);
  else attn_chunked16_wide<D, T, Policy>(a, pol, mask_row, Lb, Lb, qb, scale);
}
