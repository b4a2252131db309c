// Self-attention for 32-wide heads (MiniLM-L6, e5-small, bge-small, gte-small: hidden 384, 12 heads), gfx950.
// Forward up to 1 024 tokens in every format, backward up to 256 tokens.  The head-dim-64 kernels (attention.hip,
// attention_bwd16.hip, train_kernels.hip) are not touched.  Launch only: the planners (attn_plan.h) check the arguments and choose the tile
// count; omk_attention / omk_attention_bwd send their D32 family here.
//
// Forward (attention_d32_fwd_kernel): one workgroup per (sequence, head, 32 W queries), one wave per 32 queries.  The keys
// are walked in chunks of KT * 32 (one chunk for L <= 256) with the online softmax; per chunk K sits in LDS row-major
// (XOR-swizzled 16-byte slots) and V TRANSPOSED ([d][key], +4 pad).  Scores are computed swapped (S^T = K Q^T) as in the
// 64-wide kernels: each lane owns ONE query row and 16 keys per key tile, the softmax is lane-local plus one exchange with
// lane ^ 32.  The context is computed transposed as well (O^T = V^T P^T: the probabilities are the B operand exactly as
// they lie), so the running-max rescale, the 1 / sum and the store are per lane too: a wave's output is one 32 x 32
// accumulator, lane = query, registers = d.
// Masks as in the 64-wide kernels: a padded key adds finfo.min (HF's extended mask), keys past L do not exist, keys at or
// past kmax[b] are skipped; dropout from the (sequence, head, query, key) hash of attn_common.h on padded coordinates.
//
// Backward (attention_d32_bwd_kernel): the two-phase scheme of attention_bwd_kernel (train_kernels.hip) at D = 32 -- phase A
// query blocks (row statistics and dQ, one key tile in registers at a time), phase B key blocks (dK, dV) -- four waves, each
// over every fourth 32-row block, with the three transposed images K^T, Q^T, dO^T ([32][L + 4]) in LDS: 100 KiB at 256 tokens
// in float32, so float32 trains to 256 tokens as well.  No instantiation spills to scratch.
#include "attn_common.h"
#include "attn_plan.h"
#include "train_kernels.h"

namespace {

template <typename T> struct D32 {             // one head's slice of a row: 64 bytes (16-bit) / 128 bytes (f32)
  static constexpr int EPC = AttnGeom<T>::EPC;          // elements per 16-byte chunk
  static constexpr int CPR = 32 / EPC;                  // chunks per row
  static constexpr int ROWB = 32 * (int)sizeof(T);      // bytes per row
  static constexpr int NKK = AttnGeom<T>::NKK / 2;      // MmaOps fragments per row
  __device__ static inline int key(int row) { return (row >> (sizeof(T) == 2 ? 1 : 0)) & (CPR - 1); }
};

// o^T[d][i] += sum_c a[i][c] * Bt[d][c] over one 32-wide slab of c.  `a` is in the 32x32 accumulator layout (lane <-> i,
// register r of half h <-> c = (r&3) + 8(r>>2) + 4h); `bt` points at Bt[lane & 31][slab * 32 + 4 half] of a transposed
// LDS image with row pitch LP.  The result keeps i in the lane: register r of half h <-> d = (r&3) + 8(r>>2) + 4h.
template <typename T> struct ContractT;
template <typename T> struct ContractT16 {
  typedef typename MmaOps<T>::frag_t frag_t;
  typedef __attribute__((ext_vector_type(4))) short s4_t;
  __device__ static inline void run(const f32x16_t& a, const T* bt, int LP, f32x16_t& o) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {       // k-slot j of half h <-> c = 16u + 8(j>>2) + (j&3) + 4h
      const uint4 pa = make_uint4(Half16<T>::pack2(a[8 * u + 0], a[8 * u + 1]), Half16<T>::pack2(a[8 * u + 2], a[8 * u + 3]),
                                  Half16<T>::pack2(a[8 * u + 4], a[8 * u + 5]), Half16<T>::pack2(a[8 * u + 6], a[8 * u + 7]));
      const s4_t v0 = *(const s4_t*)(bt + 16 * u);
      const s4_t v1 = *(const s4_t*)(bt + 16 * u + 8);
      const frag_t vb = __builtin_bit_cast(frag_t, (bf16x8_t){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      MmaOps<T>::mma(vb, __builtin_bit_cast(frag_t, pa), o);
    }
  }
};
template <> struct ContractT<bf16_t> : ContractT16<bf16_t> {};
template <> struct ContractT<f16_t> : ContractT16<f16_t> {};
template <> struct ContractT<float> {
  __device__ static inline void run(const f32x16_t& a, const float* bt, int LP, f32x16_t& o) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4_t vb = *(const f32x4_t*)(bt + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[e], a[4 * g + e], o, 0, 0, 0);
    }
  }
};

// the lane's row of a transposed 32 x 32 result (register r of half h <-> d = (r&3) + 8(r>>2) + 4h), times `mul`:
// four pieces of four consecutive elements
template <typename T>
__device__ inline void store_row32(T* p, const f32x16_t& o, float mul, int half) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    T* q = p + 8 * g + 4 * half;
    if constexpr (sizeof(T) == 2) {
      *(uint2*)q = make_uint2(Half16<T>::pack2(o[4 * g] * mul, o[4 * g + 1] * mul), Half16<T>::pack2(o[4 * g + 2] * mul, o[4 * g + 3] * mul));
    } else {
      *(f32x4_t*)q = (f32x4_t){o[4 * g] * mul, o[4 * g + 1] * mul, o[4 * g + 2] * mul, o[4 * g + 3] * mul};
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward.  Grid (heads * B, ceil(Lm / (32 W))), W = blockDim.x / 64 waves.  KT: 32-key tiles per chunk.
// BIAS: pos_bias[h][q][k] (pitch Lm, the padded length, also for packed rows) is added to the SCALED score (MPNet's relative position bias).
template <typename T, int KT, bool DROP, bool BIAS>
__global__ __launch_bounds__(512) void attention_d32_fwd_kernel(
    const T* __restrict__ qkv, T* __restrict__ ctx, const int64_t* __restrict__ mask, const float* __restrict__ pos_bias, int Lm, int H,
    int heads, float scale, float drop_p, uint64_t seed, int rev, const int* __restrict__ kmax, const int* __restrict__ cu) {
  typedef D32<T> G;
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int KC = KT * 32, LP = KC + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;                                            // [KC][ROWB]
  T* const sVt = (T*)(smem + KC * G::ROWB);                         // [32][LP]
  float* const sM = (float*)(smem + KC * G::ROWB + 32 * LP * (int)sizeof(T));      // [KC]

  const int h = blockIdx.x % heads;
  const int64_t b = rev ? (int64_t)(gridDim.x / heads) - 1 - blockIdx.x / heads : blockIdx.x / heads;
  int64_t row0 = b * Lm;
  int Lq = Lm, Lk = Lm;                                             // queries of this sequence; keys walked
  if (cu) {                                                         // packed rows: sequence b is rows cu[b] .. cu[b + 1] - 1
    row0 = cu[b];
    Lq = Lk = cu[b + 1] - cu[b];
  } else if (kmax) {
    Lk = kmax[b];                                                   // keys past it are padding: probability exactly 0
  }
  const int qb = blockIdx.y * (int)blockDim.x / 2;                  // 32 queries per wave
  if (Lq <= 0 || qb >= Lq) return;                                  // (whole workgroup)

  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = tid >> 6;
  const int64_t ld = 3 * (int64_t)H;
  const T* const base = qkv + row0 * ld + h * 32;
  const int q0 = qb + wave * 32;
  const bool active = q0 < Lq;                                      // (wave-uniform; an inactive wave still stages its share)
  const int qrow = (q0 + l31) < Lq ? (q0 + l31) : (Lq - 1);
  frag_t qf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) qf[kk] = *(const frag_t*)(base + (int64_t)qrow * ld + (kk * 2 + half) * G::EPC);
  const AttnDrop dr(drop_p);
  const int key = G::key(l31);                                      // (t * 32 + l31 has the same swizzle key as l31)

  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;

  for (int kc = 0; kc < Lk; kc += KC) {
    __syncthreads();                                                // the previous chunk has been consumed
    for (int idx = tid; idx < KC * G::CPR; idx += nthr) {
      const int row = idx / G::CPR, c = idx % G::CPR;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
      if (kc + row < Lk) {
        kv = *(const uint4*)(base + (int64_t)(kc + row) * ld + H + c * G::EPC);
        vv = *(const uint4*)(base + (int64_t)(kc + row) * ld + 2 * H + c * G::EPC);
      }
      *(uint4*)(sK + row * G::ROWB + ((c ^ G::key(row)) << 4)) = kv;
      const T* ve = (const T*)&vv;
#pragma unroll
      for (int e = 0; e < G::EPC; ++e) sVt[(c * G::EPC + e) * LP + row] = ve[e];
    }
    for (int k = tid; k < KC; k += nthr)
      sM[k] = (kc + k) < Lk ? (mask[b * Lm + kc + k] != 0 ? 0.f : kFinfoMin) : -INFINITY;
    __syncthreads();
    if (!active) continue;
    const int nt = (Lk - kc + 31) >> 5;                             // key tiles of this chunk that exist (uniform)

    // S^T = K Q^T : lane owns query l31, keys (r&3) + 8(r>>2) + 4 half of each 32-key tile
    f32x16_t s[KT];
    float mx = m_run;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      if (t >= nt) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const char* krow = sK + (t * 32 + l31) * G::ROWB;
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) {
        const frag_t a = *(const frag_t*)(krow + (((kk * 2 + half) ^ key) << 4));
        MmaOps<T>::mma(a, qf[kk], s[t]);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4_t mb = *(const f32x4_t*)(sM + t * 32 + 8 * g + 4 * half);
        f32x4_t pb = {0.f, 0.f, 0.f, 0.f};
        if (BIAS) {              // four consecutive keys of this query's bias row (keys past the padded length: clamped, they are masked)
          const float* pr = pos_bias + ((int64_t)h * Lm + qrow) * Lm;
          const int k0 = kc + t * 32 + 8 * g + 4 * half;
#pragma unroll
          for (int e = 0; e < 4; ++e) pb[e] = pr[(k0 + e) < Lm ? (k0 + e) : (Lm - 1)];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = BIAS ? (s[t][4 * g + e] * scale + pb[e]) + mb[e] : s[t][4 * g + e] * scale + mb[e];
          s[t][4 * g + e] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the first chunk holds key 0 (unmasked, or finfo.min: finite), so mx is finite from here on
    const float alpha = AttnGeom<T>::exp_(m_run - mx);             // exp(-inf) = 0 on the first chunk
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      if (t >= nt) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = AttnGeom<T>::exp_(s[t][r] - mx);
        s[t][r] = e;
        sum += e;
      }
    }
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = mx;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= alpha;
    if (DROP) {     // attention_probs dropout on the unnormalised probabilities (keep_scale folds into the final 1 / sum)
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        if (t >= nt) break;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint64_t bits = attn_drop_bits(seed, b, h, heads, Lm, q0 + l31, (kc + t * 32 + 8 * g + 4 * half) >> 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) s[t][4 * g + e] = attn_drop_keep(bits, e, dr.thresh) ? s[t][4 * g + e] : 0.f;
        }
      }
    }
    // O^T += V^T P^T : lane keeps query l31
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      if (t >= nt) break;
      ContractT<T>::run(s[t], sVt + l31 * LP + t * 32 + 4 * half, LP, o);
    }
  }
  if (!active || q0 + l31 >= Lq) return;
  const float inv = (DROP ? dr.keep_scale : 1.f) / l_run;
  store_row32<T>(ctx + (row0 + q0 + l31) * (int64_t)H + h * 32, o, inv, half);
}

template <typename T, int KT, bool DROP, bool BIAS>
int launch_fwd(const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H, int heads, float scale, float drop_p,
               uint64_t seed, hipStream_t s, int rev, const int* kmax, const int* cu) {
  constexpr int KC = KT * 32;
  const int lds = KC * D32<T>::ROWB + 32 * (KC + 4) * (int)sizeof(T) + KC * 4;
  if (attn_lds_once<attention_d32_fwd_kernel<T, KT, DROP, BIAS>>(lds)) return 1;
  const int waves = L < 256 ? (L + 31) / 32 : 8;
  hipLaunchKernelGGL((attention_d32_fwd_kernel<T, KT, DROP, BIAS>), dim3((unsigned)(heads * B), (unsigned)((L + 32 * waves - 1) / (32 * waves))),
                     dim3(64 * waves), lds, s, (const T*)qkv, (T*)ctx, mask, pos_bias, L, H, heads, scale, drop_p, seed, rev, kmax, cu);
  OM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward, L <= 256: one workgroup per (sequence, head), one wave per 32-row block.
//   P = softmax(scale QK^T + mask), Pd = dropout(P)   (recomputed)
//   dPd = dO V^T ; dP = dropout'(dPd) ; dS = P o (dP - rowsum(P o dP)) * scale
//   dQ = dS K ; dK = dS^T Q ; dV = Pd^T dO
// BIAS: pos_bias [heads][Lm][Lm] is added to the scaled scores; drel [heads][2 Lm - 1] accumulates the gradient of the bias per
// offset key - query, summed over the batch (omk_t5_bias_bwd folds it into the bucket table) -- as attention_bwd_kernel does at D = 64.
template <typename T, int KT, bool BIAS>
__global__ __launch_bounds__(256) void attention_d32_bwd_kernel(
    const T* __restrict__ qkv, const T* __restrict__ dctx, T* __restrict__ dqkv, const int64_t* __restrict__ mask, int Lm, int H,
    int heads, float scale, float drop_p, uint64_t seed, const int* __restrict__ cu, const float* __restrict__ pos_bias,
    float* __restrict__ drel) {
  typedef D32<T> G;
  typedef typename MmaOps<T>::frag_t frag_t;
  constexpr int LP = KT * 32 + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sKt = (T*)smem;
  T* sQt = sKt + 32 * LP;
  T* sDOt = sQt + 32 * LP;
  float* sM = (float*)(sDOt + 32 * LP);        // additive key mask
  float* sMax = sM + KT * 32;                  // per query: row max, 1 / row sum, delta
  float* sInv = sMax + KT * 32;
  float* sDelta = sInv + KT * 32;
  float* sRel = sDelta + KT * 32;              // BIAS: this workgroup's share of drel [2 Lm - 1]

  const int h = blockIdx.x % heads;
  const int64_t b = blockIdx.x / heads;
  int64_t row0 = b * Lm;
  int L = Lm;
  if (cu) { row0 = cu[b]; L = cu[b + 1] - cu[b]; if (L <= 0) return; }
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (BIAS)
    for (int k = tid; k < 2 * Lm - 1; k += nthr) sRel[k] = 0.f;
  const int64_t ld = 3 * (int64_t)H;
  const T* base = qkv + row0 * ld + h * 32;
  const T* dob = dctx + row0 * H + h * 32;
  T* dbase = dqkv + row0 * ld + h * 32;
  const AttnDrop dr_(drop_p);
  const uint32_t thresh = dr_.thresh;
  const float keep_scale = dr_.keep_scale;

  for (int idx = tid; idx < KT * 32 * G::CPR; idx += nthr) {
    const int row = idx / G::CPR, c = idx % G::CPR;
    uint4 kv = make_uint4(0, 0, 0, 0), qv = kv, dv = kv;
    if (row < L) {
      qv = *(const uint4*)(base + (int64_t)row * ld + c * G::EPC);
      kv = *(const uint4*)(base + (int64_t)row * ld + H + c * G::EPC);
      dv = *(const uint4*)(dob + (int64_t)row * H + c * G::EPC);
    }
    const T* ke = (const T*)&kv; const T* qe = (const T*)&qv; const T* de = (const T*)&dv;
#pragma unroll
    for (int e = 0; e < G::EPC; ++e) {
      sKt[(c * G::EPC + e) * LP + row] = ke[e];
      sQt[(c * G::EPC + e) * LP + row] = qe[e];
      sDOt[(c * G::EPC + e) * LP + row] = de[e];
    }
  }
  for (int k = tid; k < KT * 32; k += nthr)
    sM[k] = k < L ? (mask[b * Lm + k] != 0 ? 0.f : kFinfoMin) : -INFINITY;
  __syncthreads();

  // up to four waves, each over every fourth 32-row block: one wave per SIMD, so a whole score row of 256 keys (s and dp: 256
  // registers) stays in the register file without scratch
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31, nw = nthr >> 6;

  // ------------------------------------------------------------------ phase A: lane <-> query
  for (int blk0 = wave * 32; blk0 < L; blk0 += nw * 32) {      // first query of the block
    const int myrow = (blk0 + l31) < L ? (blk0 + l31) : (L - 1);
    frag_t qf[G::NKK], dof[G::NKK];
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
      qf[kk] = *(const frag_t*)(base + (int64_t)myrow * ld + (kk * 2 + half) * G::EPC);
      dof[kk] = *(const frag_t*)(dob + (int64_t)myrow * H + (kk * 2 + half) * G::EPC);
    }
    // one key tile in registers at a time, three walks over the keys: the row statistics (online max / sum), delta = rowsum(P o dP),
    // then dS and dQ += dS K.  (A whole row of scores and dP -- 2 x 16 KT registers -- does not fit one wave at 256 keys.)
    // scale QK^T + mask of key tile t, transposed: lane <-> query, registers <-> keys
    auto s_tile = [&](int t, f32x16_t& v) {
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = 0.f;
      const int krow = (t * 32 + l31) < L ? (t * 32 + l31) : (L - 1);
      const T* kp = base + (int64_t)krow * ld + H;
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) MmaOps<T>::mma(*(const frag_t*)(kp + (kk * 2 + half) * G::EPC), qf[kk], v);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4_t mb = *(const f32x4_t*)(sM + t * 32 + 8 * g + 4 * half);
        if (BIAS) {
          const float* pr = pos_bias + ((int64_t)h * Lm + myrow) * Lm;
          const int k0 = t * 32 + 8 * g + 4 * half;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * g + e] = (v[4 * g + e] * scale + pr[(k0 + e) < Lm ? (k0 + e) : (Lm - 1)]) + mb[e];
        } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * g + e] = v[4 * g + e] * scale + mb[e];
        }
      }
    };
    // dropout'(dPd)^T of key tile t: dPd^T[key][query] = V dO^T, the forward's mask and 1 / (1 - p)
    auto dp_tile = [&](int t, f32x16_t& d) {
#pragma unroll
      for (int r = 0; r < 16; ++r) d[r] = 0.f;
      const int krow = (t * 32 + l31) < L ? (t * 32 + l31) : (L - 1);
      const T* vp = base + (int64_t)krow * ld + 2 * H;
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) MmaOps<T>::mma(*(const frag_t*)(vp + (kk * 2 + half) * G::EPC), dof[kk], d);
      if (thresh) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint64_t bits = attn_drop_bits(seed, b, h, heads, Lm, blk0 + l31, (t * 32 + 8 * g + 4 * half) >> 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) d[4 * g + e] = attn_drop_keep(bits, e, thresh) ? d[4 * g + e] * keep_scale : 0.f;
        }
      }
    };
    const int nt = (L + 31) >> 5;
    float mx = -INFINITY, sum = 0.f;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f32x16_t v;
      s_tile(t, v);
      float m_new = mx;
#pragma unroll
      for (int r = 0; r < 16; ++r) m_new = fmaxf(m_new, v[r]);
      if (m_new == -INFINITY) continue;                         // (this half's keys of the tile do not exist)
      float add = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) add += AttnGeom<T>::exp_(v[r] - m_new);
      sum = sum * AttnGeom<T>::exp_(mx - m_new) + add;
      mx = m_new;
    }
    {                                                           // merge the two halves of the row (lane ^ 32)
      const float mo = __shfl_xor(mx, 32, 64), so = __shfl_xor(sum, 32, 64);
      const float mm = fmaxf(mx, mo);                           // finite: key 0 exists
      sum = (mx == -INFINITY ? 0.f : sum * AttnGeom<T>::exp_(mx - mm)) + (mo == -INFINITY ? 0.f : so * AttnGeom<T>::exp_(mo - mm));
      mx = mm;
    }
    const float inv = 1.0f / sum;
    float delta = 0.f;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f32x16_t v, d;
      s_tile(t, v);
      dp_tile(t, d);
#pragma unroll
      for (int r = 0; r < 16; ++r) delta += AttnGeom<T>::exp_(v[r] - mx) * inv * d[r];
    }
    delta += __shfl_xor(delta, 32, 64);
    if (half == 0 && blk0 + l31 < L) { sMax[blk0 + l31] = mx; sInv[blk0 + l31] = inv; sDelta[blk0 + l31] = delta; }
    f32x16_t o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f32x16_t v, d;
      s_tile(t, v);
      dp_tile(t, d);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float dlogit = AttnGeom<T>::exp_(v[r] - mx) * inv * (d[r] - delta);      // d loss / d (scaled score + bias)
        if (BIAS) {
          const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, q = blk0 + l31;
          if (q < L && key < L) atomicAdd(&sRel[key - q + (Lm - 1)], dlogit);
        }
        v[r] = dlogit * scale;                                                          // dS
      }
      ContractT<T>::run(v, sKt + l31 * LP + t * 32 + 4 * half, LP, o);   // dQ^T += K^T dS^T
    }
    if (blk0 + l31 < L) store_row32<T>(dbase + (int64_t)(blk0 + l31) * ld, o, 1.f, half);
  }
  __syncthreads();
  if (BIAS)
    for (int k = tid; k < 2 * Lm - 1; k += nthr) atomicAdd(drel + (int64_t)h * (2 * Lm - 1) + k, sRel[k]);

  // ------------------------------------------------------------------ phase B: lane <-> key
  for (int blk0 = wave * 32; blk0 < L; blk0 += nw * 32) {      // first key of the block
  const int myrow = (blk0 + l31) < L ? (blk0 + l31) : (L - 1);
  const bool kvalid = (blk0 + l31) < L;
  const float mbk = sM[blk0 + l31];
  frag_t kf[G::NKK], vf[G::NKK];
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) {
    kf[kk] = *(const frag_t*)(base + (int64_t)myrow * ld + H + (kk * 2 + half) * G::EPC);
    vf[kk] = *(const frag_t*)(base + (int64_t)myrow * ld + 2 * H + (kk * 2 + half) * G::EPC);
  }
  f32x16_t dv, dk;
#pragma unroll
  for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; }
#pragma unroll 1
  for (int tq = 0; tq < KT; ++tq) {
    if (tq * 32 >= L) break;
    const int qr = (tq * 32 + l31) < L ? (tq * 32 + l31) : (L - 1);
    f32x16_t sb, dpb;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sb[r] = 0.f; dpb[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
      const frag_t qa = *(const frag_t*)(base + (int64_t)qr * ld + (kk * 2 + half) * G::EPC);
      const frag_t da = *(const frag_t*)(dob + (int64_t)qr * H + (kk * 2 + half) * G::EPC);
      MmaOps<T>::mma(qa, kf[kk], sb);        // S[query][key]
      MmaOps<T>::mma(da, vf[kk], dpb);       // dPd[query][key]
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int q4 = tq * 32 + 8 * g + 4 * half;
      const f32x4_t m4 = *(const f32x4_t*)(sMax + q4);
      const f32x4_t i4 = *(const f32x4_t*)(sInv + q4);
      const f32x4_t d4 = *(const f32x4_t*)(sDelta + q4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = q4 + e;
        float p = 0.f, pd = 0.f, dpp = 0.f;
        if (q < L && kvalid) {
          if (BIAS) p = AttnGeom<T>::exp_((sb[4 * g + e] * scale + pos_bias[((int64_t)h * Lm + q) * Lm + blk0 + l31]) + mbk - m4[e]) * i4[e];
          else
          p = AttnGeom<T>::exp_(sb[4 * g + e] * scale + mbk - m4[e]) * i4[e];
          pd = p; dpp = dpb[4 * g + e];
          if (thresh) {
            const bool keep = attn_drop_keep1(seed, b, h, heads, Lm, q, blk0 + l31, thresh);
            pd = keep ? p * keep_scale : 0.f;
            dpp = keep ? dpp * keep_scale : 0.f;
          }
        }
        sb[4 * g + e] = pd;                                                          // Pd[q][key]
        dpb[4 * g + e] = (q < L && kvalid) ? p * (dpp - d4[e]) * scale : 0.f;        // dS[q][key]
      }
    }
    ContractT<T>::run(sb, sDOt + l31 * LP + tq * 32 + 4 * half, LP, dv);    // dV^T += dO^T Pd
    ContractT<T>::run(dpb, sQt + l31 * LP + tq * 32 + 4 * half, LP, dk);    // dK^T += Q^T dS
  }
  if (kvalid) {
    store_row32<T>(dbase + (int64_t)(blk0 + l31) * ld + H, dk, 1.f, half);
    store_row32<T>(dbase + (int64_t)(blk0 + l31) * ld + 2 * H, dv, 1.f, half);
  }
  }
}

template <typename T, int KT, bool BIAS>
int launch_bwd(const void* qkv, const void* dctx, void* dqkv, const int64_t* mask, int64_t B, int L, int H, int heads, float scale,
               float drop_p, uint64_t seed, hipStream_t s, const int* cu, const float* pos_bias, float* drel) {
  constexpr int LP = KT * 32 + 4;
  const int lds = 3 * 32 * LP * (int)sizeof(T) + 4 * KT * 32 * 4 + (BIAS ? 2 * KT * 32 * 4 : 0);      // (by the tile count, like every other term: the attribute below is set once)
  if (attn_lds_once<attention_d32_bwd_kernel<T, KT, BIAS>>(lds)) return 1;
  hipLaunchKernelGGL((attention_d32_bwd_kernel<T, KT, BIAS>), dim3((unsigned)(heads * B)), dim3(64 * (L < 128 ? (L + 31) / 32 : 4)), lds, s, (const T*)qkv,
                     (const T*)dctx, (T*)dqkv, mask, L, H, heads, scale, drop_p, seed, cu, pos_bias, drel);
  OM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// launch only: attn_plan_fwd (attn_plan.h) has checked the arguments and chosen the tile count and the flags
int omk_attention_d32(const AttnPlan& p, int dtype, const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L,
                      int H, int heads, float scale, float drop_p, uint64_t seed, hipStream_t s, int reverse, const int* kmax, const int* cu) {
  return attn_with_type(dtype, [&](auto t) {
    return attn_with_kt<1, 2, 4, 6, 8>(p.kt, [&](auto kt) {      // (8: beyond 256 tokens too, in 256-key chunks)
      return attn_with_flags(p.bias, p.drop, [&](auto bias, auto drop) {
        return launch_fwd<decltype(t), kt(), drop(), bias()>(qkv, ctx, mask, pos_bias, B, L, H, heads, scale, drop_p, seed, s, reverse, kmax, cu);
      });
    });
  });
}

// launch only: attn_plan_bwd
int omk_attention_bwd_d32(const AttnPlan& p, int dtype, const void* qkv, const void* dctx, void* dqkv, const int64_t* mask, int64_t B, int L,
                          int H, int heads, float scale, float drop_p, uint64_t seed, hipStream_t s, const int* cu, const float* pos_bias,
                          float* drel) {
  return attn_with_type(dtype, [&](auto t) {
    return attn_with_kt<1, 2, 4, 6, 8>(p.kt, [&](auto kt) {
      if (p.bias) return launch_bwd<decltype(t), kt(), true>(qkv, dctx, dqkv, mask, B, L, H, heads, scale, drop_p, seed, s, cu, pos_bias, drel);
      return launch_bwd<decltype(t), kt(), false>(qkv, dctx, dqkv, mask, B, L, H, heads, scale, drop_p, seed, s, cu, nullptr, nullptr);
    });
  });
}
