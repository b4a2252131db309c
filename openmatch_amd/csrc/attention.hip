// Fused self-attention, head_dim 64, gfx950, and omk_attention, the one forward entry of every attention kernel.
// Replaces BertSelfAttention / T5Attention score+softmax+context
// (HF:models/bert/modeling_bert.py:111-136, HF:models/t5/modeling_t5.py:176-370; with dropout for training).
//
// omk_attention (at the end of this file) is: plan (attn_plan.h: argument checks, kernel family, key tiles, template flags), switch on
// the family, launch -- the kernels of this file (generic, 16-bit up to 256 tokens, 16-bit chunked, first online-softmax kernel) or the
// launchers of attention_d32.hip (32-wide heads) and attention_band.hip (a window).  No launcher here checks an argument or reads a switch.
//
// The generic kernel (attention_kernel, L <= 256):
// One workgroup per (batch, head); one wavefront per 32 query rows.  K is staged in LDS
// row-major (XOR-swizzled 16-byte slots), V is staged TRANSPOSED ([d][key], +4 pad) so both
// MFMA B-operands are contiguous LDS reads.  Scores are computed swapped (S^T = K Q^T): with
// the 32x32 accumulator map (col = lane&31, rows in registers) every lane then owns ONE query
// row and 16 keys per key tile, so the softmax is lane-local plus one exchange with lane^32,
// and the probabilities already sit in the A-operand layout of the P·V MFMA.
#include <type_traits>

#include "attn_chunked.h"
#include "attn_plan.h"

static thread_local int g_attn_last = 0;      // family | key tiles << 8 of this thread's last forward launch: omk_attention writes it from its plan
extern "C" int om_debug_attention_last(void) { return g_attn_last; }

template <typename T, int KT>
__global__ __launch_bounds__(64 * KT) void attention_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask,
    const float* __restrict__ pos_bias, int L, int H, int heads, float scale, float drop_p,
    uint64_t seed) {
  typedef AttnGeom<T> G;
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int LP = KT * 32 + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  T* sVt = (T*)(smem + KT * 32 * G::ROWB);
  float* sM = (float*)(smem + KT * 32 * G::ROWB + 64 * LP * (int)sizeof(T));

  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int64_t ld = 3 * (int64_t)H;
  const T* base = qkv + b * L * ld + h * 64;

  for (int idx = tid; idx < KT * 32 * G::CPR; idx += nthr) {
    const int row = idx / G::CPR, c = idx % G::CPR;
    uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
    if (row < L) {
      kv = *(const uint4*)(base + (int64_t)row * ld + H + c * G::EPC);
      vv = *(const uint4*)(base + (int64_t)row * ld + 2 * H + c * G::EPC);
    }
    *(uint4*)(sK + row * G::ROWB + ((c ^ G::key(row)) << 4)) = kv;
    const T* ve = (const T*)&vv;
#pragma unroll
    for (int e = 0; e < G::EPC; ++e) sVt[(c * G::EPC + e) * LP + row] = ve[e];
  }
  // additive key mask: padded keys get finfo.min (HF extended mask); keys past L do not exist
  for (int k = tid; k < KT * 32; k += nthr)
    sM[k] = k < L ? (mask[b * L + k] != 0 ? 0.f : kFinfoMin) : -INFINITY;
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q0 = wave * 32;
  if (q0 >= L) return;
  const int qrow = (q0 + l31) < L ? (q0 + l31) : (L - 1);

  frag_t qf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk)
    qf[kk] = *(const frag_t*)(base + (int64_t)qrow * ld + (kk * 2 + half) * G::EPC);

  // S^T = K Q^T : lane owns query l31, keys (r&3)+8(r>>2)+4*half of each 32-key tile
  f32x16_t s[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
    const int row = t * 32 + l31;
    const char* krow = sK + row * G::ROWB;
    const int key = G::key(row);
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
      const frag_t a = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
      MmaOps<T>::mma(a, qf[kk], s[t]);
    }
  }

  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k0 = t * 32 + 8 * g + 4 * half;
      const f32x4_t mb = *(const f32x4_t*)(sM + k0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = s[t][4 * g + e] * scale;
        if (pos_bias) {
          const int kc = (k0 + e) < L ? (k0 + e) : (L - 1);
          v += pos_bias[((int64_t)h * L + qrow) * L + kc];
        }
        v += mb[e];
        s[t][4 * g + e] = v;
        mx = fmaxf(mx, v);
      }
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = G::exp_(s[t][r] - mx);
      s[t][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[t][r] *= inv;
  if (drop_p > 0.f) {      // training: attention_probs dropout, mask regenerated in the backward (attn_common.h)
    const AttnDrop dr(drop_p);
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint64_t bits = attn_drop_bits(seed, b, h, heads, L, q0 + l31, (t * 32 + 8 * g + 4 * half) >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[t][4 * g + e] = attn_drop_keep(bits, e, dr.thresh) ? s[t][4 * g + e] * dr.keep_scale : 0.f;
      }
  }

  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int t = 0; t < KT; ++t) SlabMma<T>::run(s[t], sVt + l31 * LP + t * 32 + 4 * half, LP, o);

  // Context rows leave through LDS: the wave parks its [32 x 64] block in the K rows of its own
  // queries (every wave is past K and V^T after the barrier; waves without query rows have exited)
  // and writes whole 16-byte vectors, 8 (bf16) / 4 (f32) complete rows per instruction, instead of 32
  // two-byte stores per lane.
  __syncthreads();
  T* so = (T*)(sK + (size_t)q0 * G::ROWB);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (r & 3) + 8 * (r >> 2) + 4 * half;
      ElemOps<T>::store(so + q * 64 + dt * 32 + l31, o[dt][r]);
    }
  T* out = ctx + (b * L + q0) * H + h * 64;
  constexpr int VPR = G::ROWB / 16;                 // 16-byte vectors per row
#pragma unroll
  for (int it = 0; it < 32 * VPR / 64; ++it) {
    const int idx = it * 64 + lane, row = idx / VPR, c = idx % VPR;
    const uint4 v = *(const uint4*)((const char*)so + row * G::ROWB + c * 16);
    if (q0 + row < L) *(uint4*)((char*)(out + (int64_t)row * H) + c * 16) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16 inference kernel (no dropout): the same mathematics with ~2.5x fewer instructions per wave.  The kernel above
// is ISSUE-bound at the encoder's shape (L = 128: ~1400 instructions per wave, 4 waves per SIMD -- profiles/
// r01_bench_v8_kernel_stats.csv: 244 us per layer against a 146 us HBM floor): staging through VGPRs, V transposed
// with 256 two-byte LDS stores per lane, the context transposed back through LDS.  Here
//   * K and V go to LDS row-major by LDS-DMA (4 + 4 instructions per wave, swizzle on the source address);
//   * V^T fragments come from transposing LDS reads (ds_read_b64_tr_b16) of the row-major V image: two reads hand a
//     lane its d column's eight keys in exactly the k-slot order the probabilities' registers have, so they are the
//     A operand of  O^T = V^T P^T  as read (the first version transposed V on the matrix core: D = V_tile . I, two
//     MFMAs + eight cvt_pk per fragment pair -- a third of the kernel's MFMAs and ~15 % of its instructions);
//   * O^T puts a query row in each lane: one v_permlane32_swap per dword pair makes 16 contiguous bytes, parked in the
//     wave's own K rows and written out as whole 128-byte lines;
//   * softmax in the log2 domain: v = fma(s, scale log2e, mask), exp2(v - max) -- five instructions per score.
// Masked keys carry -1e30 (finite: a fully masked row stays uniform, as with HF's finfo.min), keys past L -inf.
// DBG (timing experiments, OM_OPT_ATTENTION_DEBUG): bit 0 no K / V fetch, bit 1 no arithmetic, bit 2 no stores
// T: bf16_t or f16_t (the float16 inference mode) -- same instruction stream, the other MFMA / conversion opcodes
// KTV: the key tiles this (batch, head) walks -- KT, or fewer when its trailing tiles hold no unmasked key (round 4).  Every key
// at or past kmax[b] is masked and its probability is exactly 0 (exp2(-1e30 - max) with the max over an unmasked key): its K / V
// rows need not be fetched, scored or multiplied.  One straight-line body per tile count (the kernel below switches once per
// workgroup): run-time guards around each tile's code cost the full-length case more than the short ones gained (161 vs 148 us,
// profiles/r04_probe12_*).
template <typename T, int KT, bool BIAS, bool DROP, int DBG, int KTV>
__device__ __forceinline__ void attention_fwd16_body(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask,
    const float* __restrict__ pos_bias, int L, int H, int heads, float scale, float drop_p, uint64_t seed, int rev,
    int64_t row0, int Lm) {      // row0: first row of this sequence in qkv / ctx (b * L, or its packed offset); L: ITS length; Lm: row pitch of `mask`
  typedef typename MmaOps<T>::frag_t frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + KT * 32 * 128;
  float* const sM = (float*)(smem + 2 * KT * 32 * 128);
  const int h = blockIdx.x % heads;
  // rev: batch rows last to first (workgroups start in blockIdx order) -- the rows the QKV projection wrote last are
  // still in the memory-side cache, and the output projection then starts on the context rows written last
  const int64_t b = rev ? (int64_t)(gridDim.x / heads) - 1 - blockIdx.x / heads : blockIdx.x / heads;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld2 = 6 * (int64_t)H;                       // row pitch of qkv in bytes
  const char* const base = (const char*)(qkv + row0 * 3 * (int64_t)H + h * 64);
  // K and V rows of this (batch, head): instruction i of wave w moves rows (i * KT + w) * 8 .. + 7, lane -> row
  // (lane >> 3), physical 16-byte chunk (lane & 7) <- source chunk (lane & 7) ^ ((row >> 1) & 7) for K (row-per-lane
  // 16-byte reads), ^ 4 ((row >> 1) & 1) for V: the four rows of a transposing read then sit in the four 64-byte
  // quarters of the bank cycle.  Rows past L repeat row L - 1 (their scores are masked to -inf).
  if (!(DBG & 1))
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (KTV < KT && i * KT + wave >= KTV * 4) continue;         // (wave-uniform) rows of a fully masked key tile
    const int r = (i * KT + wave) * 8 + (lane >> 3);
    const int rr = r < L ? r : L - 1;
    const uint32_t off = (uint32_t)(rr * ld2) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    const uint32_t offv = (uint32_t)(rr * ld2) + (((lane & 7) ^ (((r >> 1) & 1) << 2)) << 4);
    const uint32_t dst = (uint32_t)((i * KT + wave) * 1024);
    g7_dma(base + 2 * H, off, g7_lds_addr(sK) + dst);
    g7_dma(base + 4 * H, offv, g7_lds_addr(sV) + dst);
  }
  const float LOG2E = 1.4426950408889634f;
  for (int k = tid; k < KT * 32; k += 64 * KT)
    sM[k] = k < L ? (mask[b * Lm + k] != 0 ? 0.f : -1e30f) : -INFINITY;

  const int q0 = wave * 32;
  const int qrow = (q0 + l31) < L ? (q0 + l31) : (L - 1);
  frag_t qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const frag_t*)(base + (int64_t)qrow * ld2 + (kk * 2 + half) * 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the DMA above is not in hipcc's bookkeeping
  __syncthreads();
  if (q0 >= L) return;

  constexpr int KTC = (DBG & 2) ? 0 : KTV;         // key tiles the arithmetic walks
  // S^T = K Q^T : lane owns query l31, keys (r&3) + 8(r>>2) + 4 half of each 32-key tile
  const int key = (l31 >> 1) & 7;
  f32x16_t s[KTV];
#pragma unroll
  for (int t = 0; t < KTC; ++t) {
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
  const float c2 = scale * LOG2E;
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < KTC; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k0 = t * 32 + 8 * g + 4 * half;
      const f32x4_t mb = *(const f32x4_t*)(sM + k0);
      f32x4_t pb = {0.f, 0.f, 0.f, 0.f};
      if (BIAS) {              // T5: bias[h][q][k], four consecutive keys per load (L % 4 == 0 is not required: clamp)
        const float* pr = pos_bias + ((int64_t)h * Lm + qrow) * Lm;      // (the table's pitch: the padded length, also for packed rows)
#pragma unroll
        for (int e = 0; e < 4; ++e) pb[e] = pr[(k0 + e) < Lm ? (k0 + e) : (Lm - 1)] * LOG2E;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = fmaf(s[t][4 * g + e], c2, mb[e]) + pb[e];
        s[t][4 * g + e] = v;
        mx = fmaxf(mx, v);
      }
      __builtin_amdgcn_sched_barrier(0);      // keep the 16 mask vectors from being fetched all at once
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < KTC; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(s[t][r] - mx);
      s[t][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
  float inv = 1.0f / sum;
  if (DROP) {       // training forward: attention_probs dropout on the (still unnormalised) probabilities; the mask is
                    // regenerated by the backward from (seed, b, h, q, key group) -- attn_common.h
    const AttnDrop dr(drop_p);
#pragma unroll
    for (int t = 0; t < KTC; ++t)
  #pragma unroll
      for (int g = 0; g < 4; ++g) {
        // (keyed with the mask's row pitch Lm, not the sequence's own length: a packed and a padded step draw the same mask)
        const uint64_t bits = attn_drop_bits(seed, b, h, heads, Lm, q0 + l31, (t * 32 + 8 * g + 4 * half) >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[t][4 * g + e] = attn_drop_keep(bits, e, dr.thresh) ? s[t][4 * g + e] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
      }
    inv *= dr.keep_scale;
  }

  // V^T fragments by transposing LDS reads: lane (i = lane & 15, gg = lane bit 4, half) names 8-byte chunk i of the
  // [4 keys][16 d] block (keys 4 half .. + 3 of a 16-key step, d block 16 gg) and receives its d column's four keys --
  // two reads are the eight k slots of a fragment in the order the probabilities' registers have.
  const int i16 = lane & 15;
  const char* const vt0 = sV + (4 * half + (i16 >> 2)) * 128 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3);
  const int vsw = (i16 >> 3) & 1;               // the row's swizzle bit: (row >> 1) & 1 with row = 8 n + 4 half + (i16 >> 2)
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int t = 0; t < KTC; ++t) {
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
  if (DBG & 2) {                                    // keep the Q loads alive
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) o[0][kk] = (float)qf[kk][0];
  }
  // o[dt][r] = O[query l31][d = 32 dt + (r&3) + 8(r>>2) + 4 half]: scale by 1/sum, pack to bf16 -- 16 bytes per
  // (dt, register group of 8) after pairing the two halves' dwords.  Stored straight from this layout an instruction
  // writes 32 bytes to each of 32 rows; instead the block goes through the wave's own K rows (all waves are past K and
  // V after the barrier; waves without queries have exited and do not count) and leaves as whole 128-byte rows, 8 per
  // instruction.  16-byte chunk c of row r sits at chunk c ^ (r & 7): writes and reads are both conflict-free.
  // (Either way L2 writes exactly the context bytes -- WRITE_SIZE 201 MB per launch, profiles/r02_hbm_traffic.json -- and
  // the kernel runs at the memory system's pace: 805 MB per layer at ~5.2 TB/s, profiles/r02_attention_variants.log.)
  __syncthreads();
  char* const so = sK + q0 * 128;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      uint32_t a0 = Half16<T>::pack2(o[dt][8 * gp + 0] * inv, o[dt][8 * gp + 1] * inv), a1 = Half16<T>::pack2(o[dt][8 * gp + 2] * inv, o[dt][8 * gp + 3] * inv);
      uint32_t b0 = Half16<T>::pack2(o[dt][8 * gp + 4] * inv, o[dt][8 * gp + 5] * inv), b1 = Half16<T>::pack2(o[dt][8 * gp + 6] * inv, o[dt][8 * gp + 7] * inv);
      // (a: d group 2gp, b: d group 2gp + 1) -- lanes 32-63 of a swap with lanes 0-31 of b
      auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      // lanes 0-31: d = 32 dt + 16 gp + 0..7 ; lanes 32-63: d = 32 dt + 16 gp + 8..15   (chunk 4 dt + 2 gp + half)
      *(uint4*)(so + l31 * 128 + (((4 * dt + 2 * gp + half) ^ (l31 & 7)) << 4)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
  char* const out = (char*)(ctx + (row0 + q0) * (int64_t)H + h * 64);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (lane >> 3), c = lane & 7;
    const uint4 v = *(const uint4*)(so + row * 128 + ((c ^ (row & 7)) << 4));
    if (!(DBG & 4) || v.x == 0x12345u) { if (q0 + row < L) *(uint4*)(out + (int64_t)row * H * 2 + c * 16) = v; }
  }
}

template <typename T, int KT, bool BIAS, bool DROP, int DBG = 0>
__global__ __launch_bounds__(64 * KT, KT <= 4 ? ((BIAS || DROP) ? 3 : 4) : 2) void attention_fwd16_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask,
    const float* __restrict__ pos_bias, int L, int H, int heads, float scale, float drop_p, uint64_t seed, int rev,
    const int* __restrict__ kmax, const int* __restrict__ cu) {
#define OM_ATTN_BODY(V) attention_fwd16_body<T, KT, BIAS, DROP, DBG, V>(qkv, ctx, mask, pos_bias, Lb, H, heads, scale, drop_p, seed, rev, row0, L)
  const int64_t b = rev ? (int64_t)(gridDim.x / heads) - 1 - blockIdx.x / heads : blockIdx.x / heads;
  int64_t row0 = b * L;
  int Lb = L;
  if (cu) {                                          // packed rows (om_encoder_forward_packed): sequence b is rows cu[b] .. cu[b + 1] - 1
    const int c0 = __builtin_amdgcn_readfirstlane(cu[b]), c1 = __builtin_amdgcn_readfirstlane(cu[b + 1]);
    row0 = c0; Lb = c1 - c0;
    if (Lb <= 0) return;
  }
  if (KT == 4 && !BIAS && !DROP && (kmax || cu)) {   // (the encoder's inference shape; kmax[b] = L for a row without any unmasked key)
    const int kt = ((cu ? Lb : __builtin_amdgcn_readfirstlane(kmax[b])) + 31) >> 5;
    if (kt <= 1) { OM_ATTN_BODY(1); return; }
    if (kt == 2) { OM_ATTN_BODY(2); return; }
    if (kt == 3) { OM_ATTN_BODY(3); return; }
  }
  OM_ATTN_BODY(KT);
#undef OM_ATTN_BODY
}

template <typename T, int KT, bool BIAS, bool DROP>
static int launch_attn16(const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H,
                         int heads, float scale, float drop_p, uint64_t seed, hipStream_t s, int rev, const int* kmax, const int* cu) {
  const int lds = 2 * KT * 32 * 128 + KT * 32 * 4;
  if (attn_lds_once<attention_fwd16_kernel<T, KT, BIAS, DROP>>(lds)) return 1;
  // The timing variants (parts of the kernel compiled out: their results are WRONG) exist in probe builds only
  // (-DOM_PROBE_KERNELS: python -m openmatch_amd._build --probe); the product library ignores OM_OPT_ATTENTION_DEBUG.
#ifdef OM_PROBE_KERNELS
  const int dbg = (sizeof(T) == 2 && std::is_same<T, bf16_t>::value && KT == 4 && !BIAS && !DROP) ? om_option(OM_OPT_ATTENTION_DEBUG) : 0;
#else
  const int dbg = 0;
#endif
  if (dbg) {
#ifdef OM_PROBE_KERNELS
#define OM_ATTN_DBG(D)                                                                                                        \
  case D:                                                                                                                     \
    hipLaunchKernelGGL((attention_fwd16_kernel<bf16_t, 4, false, false, D>), dim3((unsigned)(heads * B)), dim3(256), lds, s,          \
                       (const bf16_t*)qkv, (bf16_t*)ctx, mask, pos_bias, L, H, heads, scale, drop_p, seed, rev, kmax, cu);    \
    break;
    switch (dbg) { OM_ATTN_DBG(1) OM_ATTN_DBG(2) OM_ATTN_DBG(3) OM_ATTN_DBG(4) OM_ATTN_DBG(5) OM_ATTN_DBG(6) OM_ATTN_DBG(7) default: break; }
#undef OM_ATTN_DBG
#endif
    OM_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL((attention_fwd16_kernel<T, KT, BIAS, DROP>), dim3((unsigned)(heads * B)), dim3(64 * KT), lds, s, (const T*)qkv,
                     (T*)ctx, mask, pos_bias, L, H, heads, scale, drop_p, seed, rev, kmax, cu);
  OM_LAUNCH_CHECK();
  return 0;
}
// ---------------------------------------------------------------------------------------------------------------
// Beyond 256 tokens in the 16-bit formats: attn_chunked16 (attn_chunked.h) over every key -- the body of the kernel above inside a loop
// over 128-key chunks with the online softmax.  Dropout, the T5 bias table and packed rows as in the kernel above: cu != NULL makes
// sequence b rows cu[b] .. cu[b + 1] - 1 of qkv / ctx and L its own row count, while the mask, the bias table and the dropout hash keep
// the padded pitch Lm.  No clipping to kmax.
template <typename T, bool BIAS, bool DROP>
__global__ __launch_bounds__(256, 2) void attention_fwd16c_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask,
    const float* __restrict__ pos_bias, int Lm, int H, int heads, float scale, float drop_p, uint64_t seed, const int* __restrict__ cu) {
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  int64_t row0 = b * Lm;
  int L = Lm;
  if (cu) {
    const int c0 = __builtin_amdgcn_readfirstlane(cu[b]), c1 = __builtin_amdgcn_readfirstlane(cu[b + 1]);
    row0 = c0; L = c1 - c0;
  }
  const int qb = blockIdx.y * 128;
  if (qb >= L) return;                                      // (whole workgroup)
  attn_chunked16<T, AttnFull, BIAS, DROP>(attn_rows_fused(qkv, ctx, row0, H, h), AttnFull{}, mask + b * Lm, L, L, qb, scale, AttnFullArgs{pos_bias, drop_p, seed, b, h, heads, Lm});
}

template <typename T, bool BIAS, bool DROP>
static int launch_attn16c(const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H,
                           int heads, float scale, float drop_p, uint64_t seed, hipStream_t s, const int* cu) {
  const int lds = 2 * 128 * 128 + 128 * 4;
  hipLaunchKernelGGL((attention_fwd16c_kernel<T, BIAS, DROP>), dim3((unsigned)(heads * B), (unsigned)((L + 127) / 128)), dim3(256), lds, s,
                     (const T*)qkv, (T*)ctx, mask, pos_bias, L, H, heads, scale, drop_p, seed, cu);
  OM_LAUNCH_CHECK();
  return 0;
}
// ---------------------------------------------------------------------------------------------------------------
// Long sequences (256 < L <= 1024) in any format: the kernels above keep a whole score row per lane (L / 2 registers) and all of
// K, V in LDS, which stops at 256 keys.  Document corpora are encoded at 512 tokens (the reference accepts anything up to
// max_position_embeddings).  attn_chunked_qreg (attn_chunked.h) over every key; bias, dropout and packed rows (cu) as in the kernel above.
template <typename T>
__global__ __launch_bounds__(256) void attention_long_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask,
    const float* __restrict__ pos_bias, int Lm, int H, int heads, float scale, float drop_p, uint64_t seed, const int* __restrict__ cu) {
  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  const int qb = blockIdx.y * 128;
  int64_t row0 = b * Lm;
  int L = Lm;
  if (cu) { row0 = cu[b]; L = cu[b + 1] - cu[b]; }
  if (qb >= L) return;                                       // (whole workgroup: a sequence shorter than this query block)
  attn_chunked_qreg<T, AttnFull>(attn_rows_fused(qkv, ctx, row0, H, h), AttnFull{}, mask + b * Lm, L, L, qb, scale, AttnFullArgs{pos_bias, drop_p, seed, b, h, heads, Lm});
}

template <typename T>
static int launch_attn_long(const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H,
                            int heads, float scale, float drop_p, uint64_t seed, hipStream_t s, const int* cu) {
  const int lds = 128 * AttnGeom<T>::ROWB + 64 * 132 * (int)sizeof(T) + 128 * 4 + 128 * 4;
  if (attn_lds_once<attention_long_kernel<T>>(lds)) return 1;
  hipLaunchKernelGGL((attention_long_kernel<T>), dim3((unsigned)(heads * B), (unsigned)((L + 127) / 128)), dim3(256), lds, s,
                     (const T*)qkv, (T*)ctx, mask, pos_bias, L, H, heads, scale, drop_p, seed, cu);
  OM_LAUNCH_CHECK();
  return 0;
}

template <typename T, int KT>
static int launch_attn(const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias,
                       int64_t B, int L, int H, int heads, float scale, float drop_p, uint64_t seed,
                       hipStream_t s) {
  constexpr int LP = KT * 32 + 4;
  const int lds = KT * 32 * AttnGeom<T>::ROWB + 64 * LP * (int)sizeof(T) + KT * 32 * 4;
  if (attn_lds_once<attention_kernel<T, KT>>(lds)) return 1;
  const int waves = (L + 31) / 32;
  hipLaunchKernelGGL((attention_kernel<T, KT>), dim3((unsigned)(heads * B)),
                     dim3(64 * waves), lds, s, (const T*)qkv, (T*)ctx, mask, pos_bias, L, H, heads,
                     scale, drop_p, seed);
  OM_LAUNCH_CHECK();
  return 0;
}

// kmax[b] = 1 + the last unmasked key of batch row b (L when the row has none): once per forward, read by every layer's
// attention launch (attention_fwd16_kernel: key tiles past it are skipped)
__global__ void mask_extent_kernel(const int64_t* __restrict__ mask, int64_t B, int L, int* __restrict__ kmax) {
  const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  int last = 0;
  for (int k = lane; k < L; k += 64) if (mask[b * L + k] != 0) last = k + 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) kmax[b] = last ? last : L;
}
// packed rows: cu[0..B] = exclusive scan of kmax clamped to `rows`; row_map[t] = b * L + pos of packed row t (-1 for the pad rows
// up to `rows`).  More tokens than `rows`: the sequences past the bound get the
// rows that are left (possibly none) so that no kernel leaves the buffers, cu[B + 1] keeps the true count, and the pooling
// tail turns every representation into NaN (omk_pack_overflow_poison) instead of returning a silently truncated batch.
// One launch, the row_map fill spread over the rows: EVERY workgroup repeats the scan (thread j sums its `per` consecutive sequences, an
// inclusive scan of the 1024 sums in LDS: B integers from L2), then fills its own 1024-row slices of row_map -- one row per thread,
// consecutive threads consecutive rows -- by searching the scanned sums for the row's chunk of sequences and walking that chunk.
// Workgroup 0 also writes cu and cls_rows as the single-workgroup kernel did.
__global__ __launch_bounds__(1024) void pack_rows_kernel(const int* __restrict__ kmax, int64_t B, int L, int64_t rows, int* __restrict__ cu,
                                                          int* __restrict__ cls_rows, int* __restrict__ row_map) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int64_t per = (B + 1023) / 1024, lo = tid * per, hi = lo + per < B ? lo + per : B;
  int sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += kmax[i];
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int total = part[1023];
  const int cap = (int)rows;
  if (blockIdx.x == 0) {
    int run = part[tid] - sum;                     // exclusive prefix of this thread's sequences
    for (int64_t i = lo; i < hi; ++i) {
      cu[i] = run < cap ? run : cap;
      cls_rows[i] = run < cap ? run : cap - 1;
      run += kmax[i];
    }
    if (tid == 1023) { cu[B] = total < cap ? total : cap; cu[B + 1] = total; }
  }
  for (int64_t t = (int64_t)blockIdx.x * 1024 + tid; t < rows; t += (int64_t)gridDim.x * 1024) {
    int v = -1;
    if (t < total) {
      // the first chunk j whose inclusive sum exceeds t holds row t (chunks of no tokens are passed over)
      int a = 0, b = 1023;
      while (a < b) { const int m = (a + b) >> 1; if (part[m] > (int)t) b = m; else a = m + 1; }
      int64_t i = a * per;
      int run = a ? part[a - 1] : 0;
      for (int n = kmax[i]; run + n <= (int)t; n = kmax[++i]) run += n;
      v = (int)(i * L + ((int)t - run));
    }
    row_map[t] = v;
  }
}
int omk_pack_rows(const int* kmax, int64_t B, int L, int64_t rows, int* cu, int* cls_rows, int* row_map, hipStream_t s) {
  if (B <= 0) return 0;
  if (rows > 0x7fffffff || B * (int64_t)L > 0x7fffffff) OM_FAIL("packed rows: token counts below 2^31");
  const int64_t slices = (rows + 1023) / 1024;
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)(slices < 1 ? 1 : slices > 1024 ? 1024 : slices)), dim3(1024), 0, s, kmax, B, L, rows, cu, cls_rows,
                     row_map);
  OM_LAUNCH_CHECK();
  return 0;
}

int omk_mask_extent(const int64_t* mask, int64_t B, int L, int* kmax, hipStream_t s) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(mask_extent_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, mask, B, L, kmax);
  OM_LAUNCH_CHECK();
  return 0;
}

// plan (attn_plan.h), switch on the family, launch
int omk_attention(int dtype, const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H, int heads,
                  float scale, float drop_p, uint64_t seed, hipStream_t s, int reverse, const int* kmax, const int* cu, int w) {
  g_attn_last = 0;
  const AttnPlan p = attn_plan_fwd(dtype, B, L, H, heads, pos_bias != nullptr, drop_p, kmax != nullptr, cu != nullptr, w, attn_switches());
  if (p.error) OM_FAIL(p.error);
  g_attn_last = p.family | (p.kt << 8);
  switch (p.family) {
    case 0: return 0;                                   // an empty batch
    case OM_ATTN_FAMILY_D32: return omk_attention_d32(p, dtype, qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s, reverse, kmax, cu);
    case OM_ATTN_FAMILY_BAND16: case OM_ATTN_FAMILY_BAND32: return omk_attention_band(dtype, qkv, ctx, mask, B, L, H, heads, scale, w, kmax, s);
    case OM_ATTN_FAMILY_FWD16: case OM_ATTN_FAMILY_FWD16_KMAX4:
      return attn_with_type16(dtype, [&](auto t) {
        return attn_with_kt<1, 2, 4, 6, 8>(p.kt, [&](auto kt) {
          return attn_with_flags(p.bias, p.drop, [&](auto bias, auto drop) {
            return launch_attn16<decltype(t), kt(), bias(), drop()>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s, reverse, kmax, cu);
          });
        });
      });
    case OM_ATTN_FAMILY_FWD16C:
      return attn_with_type16(dtype, [&](auto t) {
        return attn_with_flags(p.bias, p.drop, [&](auto bias, auto drop) {
          return launch_attn16c<decltype(t), bias(), drop()>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s, cu);
        });
      });
    case OM_ATTN_FAMILY_LONG:
      return attn_with_type(dtype, [&](auto t) { return launch_attn_long<decltype(t)>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s, cu); });
    default:                                            // OM_ATTN_FAMILY_GENERIC: float32 and bfloat16
      if (dtype == OM_BF16)
        return attn_with_kt<1, 2, 4, 6, 8>(p.kt, [&](auto kt) { return launch_attn<bf16_t, kt()>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s); });
      return attn_with_kt<1, 2, 4, 6, 8>(p.kt, [&](auto kt) { return launch_attn<float, kt()>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s); });
  }
}

// host only: what omk_attention would launch for these arguments at the current switches -- family | key tiles << 8, 0 when nothing
// would launch, -1 for a refusal (its reason in om_last_error); the last-launch word is not touched
extern "C" int om_debug_attention_plan(int dtype, int64_t B, int L, int H, int heads, int has_bias, float drop_p, int has_kmax, int has_cu, int w) {
  const AttnPlan p = attn_plan_fwd(dtype, B, L, H, heads, has_bias != 0, drop_p, has_kmax != 0, has_cu != 0, w, attn_switches());
  if (p.error) { om_set_error(std::string(__func__) + ": " + p.error); return -1; }
  return p.family | (p.kt << 8);
}

extern "C" int om_debug_attention_ex(int dtype, const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H,
                                     int heads, float scale, float drop_p, uint64_t seed, void* stream, int reverse, const int* kmax,
                                     const int* cu, int w) {
  g_attn_last = 0;
  if (!qkv || !ctx || !mask) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("attention: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (w > 0 && (pos_bias || drop_p > 0.f || cu || reverse)) OM_FAIL("banded attention: no position bias, dropout, packed rows or reverse walk");
  return omk_attention(dtype, qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, (hipStream_t)stream, reverse, kmax, cu, w);
}
extern "C" int om_debug_attention(const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int H, int heads, void* stream) {
  return om_debug_attention_ex(OM_BF16, qkv, ctx, mask, nullptr, B, L, H, heads, 0.125f, 0.f, 0, stream, 0, nullptr, nullptr, 0);
}
extern "C" int om_debug_rope(int dtype, void* qkv, int64_t M, int L, int H, float theta, void* stream) {
  if (!qkv) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("rotary positions: dtype must be OM_F32, OM_BF16 or OM_F16");
  return omk_rope(dtype, qkv, M, L, H, theta, (hipStream_t)stream);
}
extern "C" int om_debug_rope_rows(int dtype, void* qkv, int64_t rows, int L, int H, float theta, const int* row_map, void* stream) {
  if (!qkv || !row_map) OM_FAIL("null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("rotary positions: dtype must be OM_F32, OM_BF16 or OM_F16");
  return omk_rope(dtype, qkv, rows, L, H, theta, (hipStream_t)stream, row_map);
}
extern "C" int om_debug_mask_extent(const int64_t* mask, int64_t B, int L, int* kmax, void* stream) {
  if (!mask || !kmax) OM_FAIL("null argument");
  if (L < 1) OM_FAIL("mask extent: L must be at least 1");
  return omk_mask_extent(mask, B, L, kmax, (hipStream_t)stream);
}
extern "C" int om_debug_pack_rows(const int* kmax, int64_t B, int L, int64_t rows, int* cu, int* cls_rows, int* row_map, void* stream) {
  if (!kmax || !cu || !cls_rows || !row_map) OM_FAIL("null argument");
  if (rows < 1) OM_FAIL("packed rows: rows must be at least 1");
  return omk_pack_rows(kmax, B, L, rows, cu, cls_rows, row_map, (hipStream_t)stream);
}
// host only: the dropout decision of probability (b, h, q, key) exactly as the kernels take it (attn_common.h)
extern "C" int om_debug_attn_drop_keep(uint64_t seed, int64_t b, int h, int heads, int Lm, int q, int key, float p) {
  return attn_drop_keep1(seed, b, h, heads, Lm, q, key, AttnDrop(p).thresh) ? 1 : 0;
}
