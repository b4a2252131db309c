// HBM-bound helpers of the encoder: embedding gather + LayerNorm (K1), LayerNorm / RMSNorm
// (tails of K4/K6), pooling (K7), L2 normalise (K9), T5 relative-position bias, and the
// f32 -> f16 index shadow copy.  One wavefront (64 lanes) owns one row; 4 rows per block.
#include "common.h"
#include "kernels.h"
#include "ln_row.h"
#include "row_plan.h"
#include <type_traits>

#define ROWS_PER_BLOCK 4      // (4-element vectors per lane: row_max_vec, 4 up to H = 1024 and 8 up to 2048)

// Normalise the row held in x[][] (nv vectors per lane) and write it out.
// LayerNorm: two-pass mean / biased variance in f32 (torch.nn.LayerNorm);
// RMSNorm (T5LayerNorm, HF:models/t5/modeling_t5.py:59-72): x * rsqrt(mean(x^2)+eps) * g.
template <typename TOut, int MAX_VEC>
__device__ inline void norm_and_store(float (&x)[MAX_VEC][4], int nvec, int lane, int H,
                                      const float* __restrict__ g, const float* __restrict__ b,
                                      float eps, int rms, TOut* __restrict__ out, float* __restrict__ out32 = nullptr) {
  float mean, rstd;
  ln_row_stats<MAX_VEC>(x, nvec, lane, H, eps, rms, mean, rstd);
#pragma unroll
  for (int j = 0; j < MAX_VEC; ++j) {
    const int c = (lane + 64 * j) * 4;
    if (j < nvec && c < H) {
      float gv[4], y[4];
      Vec4<float>::load(g + c, gv);
      if (b) {
        float bv[4];
        Vec4<float>::load(b + c, bv);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = ln_affine(x[j][e], mean, rstd, gv[e], bv[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (x[j][e] - mean) * rstd * gv[e];
      }
      Vec4<TOut>::store(out + c, y);
      if (out32) Vec4<float>::store(out32 + c, y);      // the unrounded copy (16-bit training: what the next residual add reads)
    }
  }
}

template <typename TIn, typename TOut, int MAX_VEC>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void layernorm_kernel(
    const TIn* __restrict__ x, int64_t ldx, TOut* __restrict__ y, int64_t ldy,
    const float* __restrict__ g, const float* __restrict__ b, int64_t M, int H, float eps, int rms,
    const int* __restrict__ rows = nullptr, float* __restrict__ y32 = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= M) return;
  const int64_t src = rows ? (int64_t)rows[row] : row;      // gather (packed rows: the [CLS] row of every sequence)
  const int nvec = (H / 4 + 63) / 64;
  float v[MAX_VEC][4];
#pragma unroll
  for (int j = 0; j < MAX_VEC; ++j) {
    const int c = (lane + 64 * j) * 4;
    if (j < nvec && c < H) Vec4<TIn>::load(x + src * ldx + c, v[j]);
  }
  norm_and_store<TOut, MAX_VEC>(v, nvec, lane, H, g, b, eps, rms, y + row * ldy, y32 ? y32 + row * ldy : nullptr);
}

// bf16 rows with 16-byte accesses: 32 lanes own one row (two rows per wave), every lane holds NV
// vectors of 8 elements.  The 8-byte accesses of the generic kernel reach ~4.1 TB/s on
// [131072, 768]; 16-byte ones are what the memory path is built for (MI355X_MICROARCH.md).
template <int NV, typename TOut = bf16_t, typename TIn = bf16_t>      // TOut = float: the LAST normalisation before pooling (the reference's
__global__ __launch_bounds__(256) void layernorm_bf16x8_kernel(     // autocast runs layer_norm in fp32 and returns fp32); TIn: bf16_t or f16_t (round 6)
    const TIn* __restrict__ x, int64_t ldx, TOut* __restrict__ y, int64_t ldy,
    const float* __restrict__ g, const float* __restrict__ b, int64_t M, int H, float eps, int rms,
    const TIn* __restrict__ x_lo,             // x_lo: second plane of a two-plane residual stream (value = x + x_lo), or NULL
    const int* __restrict__ rows = nullptr,   // gather: output row r normalises input row rows[r]
    int lo8 = 0) {                            // 1: x_lo is the eight-bit plane (kernels.h omk_lo8_offset) of the [.., H] tensor x points into
  const int lane = threadIdx.x & 31;
  const int64_t orow = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (orow >= M) return;
  const int64_t row = rows ? (int64_t)rows[orow] : orow;
  const int nv8 = H / 8;
  float v[NV][8];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = lane + 32 * j;
    if (c < nv8) {
      const uint4 t = *(const uint4*)(x + row * ldx + c * 8);
      const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[j][2 * e] = Half16<TIn>::lo(w[e]); v[j][2 * e + 1] = Half16<TIn>::hi(w[e]); }
      if (x_lo && lo8) {       // the row's index in the [M, H] tensor the plane belongs to: row * ldx / H (ldx = L * H gathers the CLS rows)
        const int64_t trow = row * (ldx / H);
        const unsigned char* p8 = (const unsigned char*)x_lo;
        const uint32_t wa = *(const uint32_t*)(p8 + omk_lo8_offset(trow, c * 8, H)), wb = *(const uint32_t*)(p8 + omk_lo8_offset(trow, c * 8 + 4, H));
        const om_f32x2_t a01 = __builtin_amdgcn_cvt_pk_f32_bf8((int)wa, false), a23 = __builtin_amdgcn_cvt_pk_f32_bf8((int)wa, true);
        const om_f32x2_t b01 = __builtin_amdgcn_cvt_pk_f32_bf8((int)wb, false), b23 = __builtin_amdgcn_cvt_pk_f32_bf8((int)wb, true);
        const float l8[8] = {a01[0], a01[1], a23[0], a23[1], b01[0], b01[1], b23[0], b23[1]};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = fmaf(l8[e], 0.0009765625f, v[j][e]);
      } else if (x_lo) {
        const uint4 t2 = *(const uint4*)(x_lo + row * ldx + c * 8);
        const uint32_t w2[4] = {t2.x, t2.y, t2.z, t2.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[j][2 * e] += Half16<TIn>::lo(w2[e]); v[j][2 * e + 1] += Half16<TIn>::hi(w2[e]); }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
    }
  }
  auto half_sum = [](float t) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
  };
  float mean = 0.f;
  if (!rms) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[j][e];
    mean = half_sum(s) / (float)H;
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (lane + 32 * j < nv8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[j][e] - mean; ss += d * d; }
    }
  const float rstd = rsqrtf(half_sum(ss) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = lane + 32 * j;
    if (c < nv8) {
      float gv[8], bv[8];
      Vec4<float>::load(g + c * 8, *(float(*)[4])&gv[0]);
      Vec4<float>::load(g + c * 8 + 4, *(float(*)[4])&gv[4]);
      if (b) { Vec4<float>::load(b + c * 8, *(float(*)[4])&bv[0]); Vec4<float>::load(b + c * 8 + 4, *(float(*)[4])&bv[4]); }
      uint32_t w[4];
      float o[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float y0 = (v[j][2 * e] - mean) * rstd * gv[2 * e], y1 = (v[j][2 * e + 1] - mean) * rstd * gv[2 * e + 1];
        if (b) { y0 += bv[2 * e]; y1 += bv[2 * e + 1]; }
        o[2 * e] = y0; o[2 * e + 1] = y1;
        w[e] = Half16<TIn>::pack2(y0, y1);
      }
      if (sizeof(TOut) == 4) {
        Vec4<float>::store((float*)y + orow * ldy + c * 8, *(float(*)[4])&o[0]);
        Vec4<float>::store((float*)y + orow * ldy + c * 8 + 4, *(float(*)[4])&o[4]);
      } else {
        *(uint4*)(y + orow * ldy + c * 8) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
}

// Fold a LayerNorm into the bf16 weight that consumes its output (kernels.h, GemmEpilogue::ln_*):
//   W'[n,k] = bf16(W[n,k] gamma[k]),  s[n] = sum_k W'[n,k],  b'[n] = b[n] + sum_k beta[k] W[n,k]
// so that LN(y) W^T + b = rstd (y W'^T - mu s) + b'.  One wave per output row.
template <typename T>          // bf16_t or f16_t
__global__ __launch_bounds__(256) void ln_fold_kernel(const T* __restrict__ W, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ b,
                                                      T* __restrict__ Wf, float* __restrict__ colsum,
                                                      float* __restrict__ bf, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float s = 0.f, t = 0.f;
  for (int k = lane * 8; k < K; k += 64 * 8) {              // K % 8 == 0
    const uint4 w4 = *(const uint4*)(W + (int64_t)n * K + k);
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float w0 = Half16<T>::lo(w[e]), w1 = Half16<T>::hi(w[e]);
      o[e] = Half16<T>::pack2(w0 * gamma[k + 2 * e], w1 * gamma[k + 2 * e + 1]);
      s += Half16<T>::lo(o[e]) + Half16<T>::hi(o[e]);        // the column sum of what the GEMM will actually multiply
      if (beta) t += w0 * beta[k + 2 * e] + w1 * beta[k + 2 * e + 1];
    }
    *(uint4*)(Wf + (int64_t)n * K + k) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  s = wave_sum(s); t = wave_sum(t);
  if (lane == 0) { colsum[n] = s; bf[n] = (b ? b[n] : 0.f) + t; }
}

int omk_ln_fold(int dtype, const void* W, const float* gamma, const float* beta, const float* b, void* Wf,
                float* colsum, float* bf, int N, int K, hipStream_t s) {
  if (K % 8 != 0) OM_FAIL("K must be a multiple of 8");
  if (dtype == OM_F16)
    hipLaunchKernelGGL((ln_fold_kernel<f16_t>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const f16_t*)W, gamma, beta, b,
                       (f16_t*)Wf, colsum, bf, N, K);
  else
    hipLaunchKernelGGL((ln_fold_kernel<bf16_t>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const bf16_t*)W, gamma, beta, b,
                       (bf16_t*)Wf, colsum, bf, N, K);
  OM_LAUNCH_CHECK();
  return 0;
}

// BERT: LN(word[id] + type[tt] + pos[t])  (HF:models/bert/modeling_bert.py:68-108); any of the two tables may be missing.
// T5  : word[id]                          (shared embedding, no norm).
template <typename TOut, int MAX_VEC>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void embed_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ type_ids,
    const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
    const float* __restrict__ g, const float* __restrict__ b, TOut* __restrict__ out, int64_t M,
    int L, int H, int vocab, int type_vocab, float eps, int bert, const int* __restrict__ row_map, float* __restrict__ out32) {
  const int lane = threadIdx.x & 63;
  const int64_t orow = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (orow >= M) return;
  int64_t row = orow;
  if (row_map) {                                   // packed rows: output row t embeds token row_map[t]; pad rows are zero
    row = row_map[orow];
    if (row < 0) {
      for (int c = lane * 4; c < H; c += 256) { float z[4] = {0.f, 0.f, 0.f, 0.f}; Vec4<TOut>::store(out + orow * H + c, z); }
      return;
    }
  }
  int64_t id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const int nvec = (H / 4 + 63) / 64;
  float v[MAX_VEC][4];
  if (bert) {
    int64_t tt = type_ids ? type_ids[row] : 0;
    tt = tt < 0 ? 0 : (tt >= type_vocab ? type_vocab - 1 : tt);
    const int t = (int)(row % L);
#pragma unroll
    for (int j = 0; j < MAX_VEC; ++j) {
      const int c = (lane + 64 * j) * 4;
      if (j < nvec && c < H) {
        float w[4], ty[4], p[4];
        Vec4<float>::load(word + id * H + c, w);
        if (type && pos) {
          Vec4<float>::load(type + tt * H + c, ty);
          Vec4<float>::load(pos + (int64_t)t * H + c, p);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = (w[e] + ty[e]) + p[e];
        } else if (type) {         // NomicBERT: word + token type, no position table (the positions are rotary)
          Vec4<float>::load(type + tt * H + c, ty);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = w[e] + ty[e];
        } else if (pos) {          // DistilBERT, MPNet: word + position, no token-type table
          Vec4<float>::load(pos + (int64_t)t * H + c, p);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = w[e] + p[e];
        } else {                   // ModernBERT: LayerNorm of the word embedding alone (no position or token-type table)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = w[e];
        }
      }
    }
    norm_and_store<TOut, MAX_VEC>(v, nvec, lane, H, g, b, eps, 0, out + orow * H, out32 ? out32 + orow * H : nullptr);
  } else {
#pragma unroll
    for (int j = 0; j < MAX_VEC; ++j) {
      const int c = (lane + 64 * j) * 4;
      if (j < nvec && c < H) {
        Vec4<float>::load(word + id * H + c, v[j]);
        Vec4<TOut>::store(out + orow * H + c, v[j]);
      }
    }
  }
}

// pooling == FIRST: hidden[:,0,:] ; MEAN: sum(h*m)/clamp(sum(m),1e-9)  (utils.py:233-235)
template <typename T>
__global__ void pool_kernel(const T* __restrict__ x, const int64_t* __restrict__ mask,
                            float* __restrict__ out, int L, int H, int mode, const int* __restrict__ cu) {
  const int64_t b = blockIdx.x;
  const T* xb = x + (cu ? (int64_t)cu[b] : b * (int64_t)L) * H;
  const int Lb = cu ? cu[b + 1] - cu[b] : L;        // packed rows: this sequence's own length (the mask keeps pitch L)
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode == OM_POOL_FIRST) {
      Vec4<T>::load(xb + c, acc);
    } else {
      float cnt = 0.f;
      for (int t = 0; t < Lb; ++t) {
        const float m = (float)mask[b * L + t];
        float v[4];
        Vec4<T>::load(xb + (int64_t)t * H + c, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e] * m;
        cnt += m;
      }
      cnt = fmaxf(cnt, 1e-9f);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] / cnt;
    }
    Vec4<float>::store(out + b * H + c, acc);
  }
}

// F.normalize(x, dim=1): x / max(||x||_2, 1e-12)   (modeling/dense_retrieval_model.py:153-154)
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void l2norm_kernel(const float* __restrict__ x,
                                                                     float* __restrict__ y,
                                                                     int64_t M, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= M) return;
  float ss = 0.f;
  for (int c = lane; c < D; c += 64) { const float v = x[row * D + c]; ss += v * v; }
  const float denom = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int c = lane; c < D; c += 64) y[row * D + c] = x[row * D + c] / denom;
}

// T5 additive attention bias  bias[h][q][k] = table[bucket(k - q)][h]
// (HF:models/t5/modeling_t5.py compute_bias; the bucket LUT is built on the host).
__global__ void t5_bias_kernel(const float* __restrict__ table, const int* __restrict__ lut,
                               float* __restrict__ out, int L, int heads) {
  const int64_t n = (int64_t)heads * L * L;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % L), q = (int)((i / L) % L), h = (int)(i / ((int64_t)L * L));
    out[i] = table[lut[k - q + (L - 1)] * heads + h];
  }
}

// index.add(): f16 shadow rows + rounding statistics for the certified search margin.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void index_to_f16_kernel(
    const float* __restrict__ x, f16_t* __restrict__ y, int64_t N, int d,
    unsigned* stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= N) return;
  float e2 = 0.f, n2 = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = x[row * d + c];
    const f16_t r = (f16_t)v;             // round-to-nearest-even; |v| > 65504 -> inf -> margin inf
    const float rv = (float)r;
    y[row * d + c] = r;
    e2 += (v - rv) * (v - rv);
    n2 += rv * rv;
  }
  e2 = wave_sum(e2); n2 = wave_sum(n2);
  if (lane == 0) {
    // non-negative floats order like their bit patterns; round the norms UP a little
    const unsigned ue = __float_as_uint(sqrtf(e2) * 1.0001f), un = __float_as_uint(sqrtf(n2) * 1.0001f);
    if (ue > stats[0]) atomicMax(stats + 0, ue);     // monotone max: the plain read only skips
    if (un > stats[1]) atomicMax(stats + 1, un);     // atomics that cannot change the value
  }
}

// index.add() of a float16-only index (OM_SEARCH_F16_ONLY): the stored rows from float32 (round to nearest even) or float16 (bit for bit)
// input, one wave per row, one pass.  VEC: 16-byte accesses, eight values per lane and step (d % 8 == 0, both planes 16-byte aligned).
// The row norm of the STORED values is summed as index_to_f16_kernel sums it -- lane l adds columns l, l + 64, ... in that order -- so the
// same values leave the same stats[1] there and here: the vector path passes each 512-column step through a wave-private LDS slice to get
// from "eight consecutive columns per lane" to that order.  stats[0] is not written: the rows carry no rounding error against themselves.
#define ADD16_STEP 512      // columns of one vector step: 64 lanes x 8
template <typename TIn, bool VEC>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void index_add_f16_kernel(
    const TIn* __restrict__ x, f16_t* __restrict__ y, int64_t N, int d, unsigned* stats, unsigned* nonfinite) {
  __shared__ __attribute__((aligned(16))) f16_t stage[ROWS_PER_BLOCK][ADD16_STEP];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= N) return;                    // (a whole wave: nothing below synchronises across waves)
  const TIn* xr = x + row * d;
  f16_t* yr = y + row * d;
  float n2 = 0.f;
  float bad = 0.f;                         // stored values that are inf or NaN (a float: wave_sum adds it; at most d / 64 + 7 per lane)
  auto note = [&](f16_t r) { bad += ((__builtin_bit_cast(unsigned short, r) & 0x7c00u) == 0x7c00u) ? 1.f : 0.f; };
  if (VEC) {
    f16_t* st = stage[threadIdx.x >> 6];
    for (int c0 = 0; c0 < d; c0 += ADD16_STEP) {       // (wave-uniform trip count)
      const int c = c0 + lane * 8;
      if (c < d) {
        f16x8_t h;
        if constexpr (sizeof(TIn) == 4) {
          const float4 a = *(const float4*)(xr + c), b = *(const float4*)(xr + c + 4);
          h[0] = (f16_t)a.x; h[1] = (f16_t)a.y; h[2] = (f16_t)a.z; h[3] = (f16_t)a.w;
          h[4] = (f16_t)b.x; h[5] = (f16_t)b.y; h[6] = (f16_t)b.z; h[7] = (f16_t)b.w;
        } else {
          h = *(const f16x8_t*)(xr + c);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) note(h[i]);
        *(f16x8_t*)(yr + c) = h;
        *(f16x8_t*)(st + lane * 8) = h;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the slice is this wave's alone: its own writes, then its own reads
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int i = 0; i < ADD16_STEP / 64; ++i)
        if (c0 + lane + 64 * i < d) {
          const float rv = (float)st[lane + 64 * i];
          n2 += rv * rv;
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // read before the next step overwrites it
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  } else {
    for (int c = lane; c < d; c += 64) {
      const f16_t r = (f16_t)xr[c];
      const float rv = (float)r;
      note(r);
      yr[c] = r;
      n2 += rv * rv;
    }
  }
  n2 = wave_sum(n2); bad = wave_sum(bad);
  if (lane == 0) {
    const unsigned un = __float_as_uint(sqrtf(n2) * 1.0001f);
    if (un > stats[1]) atomicMax(stats + 1, un);      // (inf or NaN of a non-finite row orders above every norm: no margin certifies then)
    if (bad != 0.f) atomicAdd(nonfinite, (unsigned)bad);
  }
}

// ---- host launchers ---------------------------------------------------------
static thread_local int g_row_last = 0;     // the OM_ROW_* word of this thread's last normalisation launch (include/openmatch_hip.h)
void omk_row_note(int word) { g_row_last = word; }
extern "C" int om_debug_row_kernel_last(void) { return g_row_last; }

// The one forward launch of the four omk_layernorm* entries: what row_fwd_plan (row_plan.h) named, on these arguments.
struct RowFwdArgs {
  const void* x; int64_t ldx; void* y; int64_t ldy; const float* g; const float* b; int64_t M; int H; float eps; int rms;
  const void* x_lo;      // x8 body: the second plane, or NULL
  const int* rows;       // gather: output row r normalises input row rows[r], or NULL
  float* y32;            // generic body: the unrounded f32 copy of y (omk_layernorm_dual), or NULL
};
static inline bool row_aligned16(const void* a, const void* b, const void* c = nullptr) {      // (a NULL pointer is aligned)
  return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

template <typename TIn, typename TOut>
static void launch_row_fwd_as(const RowFwdPlan& p, const RowFwdArgs& a, hipStream_t s) {
  if constexpr (sizeof(TIn) == 2) {
    if (p.body == OM_ROW_FWD_X8) {
      auto x8 = [&](auto nv) {
        hipLaunchKernelGGL((layernorm_bf16x8_kernel<decltype(nv)::value, TOut, TIn>), dim3((unsigned)((a.M + 7) / 8)), dim3(256), 0, s, (const TIn*)a.x,
                           a.ldx, (TOut*)a.y, a.ldy, a.g, a.b, a.M, a.H, a.eps, a.rms, (const TIn*)a.x_lo, a.rows, (int)p.lo8);
      };
      if (p.nv == 1) x8(std::integral_constant<int, 1>());
      else if (p.nv == 2) x8(std::integral_constant<int, 2>());
      else if (p.nv == 3) x8(std::integral_constant<int, 3>());
      else x8(std::integral_constant<int, 4>());
      return;
    }
  }
  auto generic = [&](auto mv) {
    hipLaunchKernelGGL((layernorm_kernel<TIn, TOut, decltype(mv)::value>), dim3((unsigned)((a.M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)),
                       dim3(64 * ROWS_PER_BLOCK), 0, s, (const TIn*)a.x, a.ldx, (TOut*)a.y, a.ldy, a.g, a.b, a.M, a.H, a.eps, a.rms, a.rows, a.y32);
  };
  if (p.nv == 4) generic(std::integral_constant<int, 4>());
  else generic(std::integral_constant<int, 8>());
}

static int launch_row_fwd(const RowFwdPlan& p, const RowFwdArgs& a, hipStream_t s) {
  omk_row_note(row_fwd_word(p));
  const auto is = [&](int tin, int tout) { return p.tin == tin && p.tout == tout; };
  if (is(OM_BF16, OM_BF16)) launch_row_fwd_as<bf16_t, bf16_t>(p, a, s);
  else if (is(OM_F16, OM_F16)) launch_row_fwd_as<f16_t, f16_t>(p, a, s);
  else if (is(OM_BF16, OM_F32)) launch_row_fwd_as<bf16_t, float>(p, a, s);
  else if (is(OM_F16, OM_F32)) launch_row_fwd_as<f16_t, float>(p, a, s);
  else if (is(OM_F32, OM_BF16)) launch_row_fwd_as<float, bf16_t>(p, a, s);
  else if (is(OM_F32, OM_F16)) launch_row_fwd_as<float, f16_t>(p, a, s);
  else launch_row_fwd_as<float, float>(p, a, s);      // (the plan names these seven pairs and no other)
  OM_LAUNCH_CHECK();
  return 0;
}

// Row statistics from the slot partials a GEMM epilogue left (GemmEpilogue::stats_out): one thread per row adds the
// slots in slot order -- the same result whatever order the tiles ran in (round 2 accumulated with f32 atomics).
__global__ __launch_bounds__(256) void ln_stats_reduce_kernel(const float2* __restrict__ slots, int nslots, int64_t M, float2* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nslots; ++k) { const float2 v = slots[(int64_t)k * M + m]; s1 += v.x; s2 += v.y; }
  out[m] = make_float2(s1, s2);
}
int omk_ln_stats_reduce(const float* slots, int nslots, int64_t M, float* out, hipStream_t s) {
  if (M <= 0) return 0;
  hipLaunchKernelGGL(ln_stats_reduce_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const float2*)slots, nslots, M, (float2*)out);
  OM_LAUNCH_CHECK();
  return 0;
}

// Row gather of the [CLS] tail (kernels.h omk_gather_rows).  One thread per 16-byte vector of an output row: H / 8 consecutive threads
// copy one row of each plane (coalesced on both sides), the first of them also the row's statistics pair.  blockDim.x is a multiple of
// H / 8 up to 256, so a workgroup holds whole rows and the grid is Mc / (rows per workgroup): hundreds of workgroups for Mc >= 512.
struct GatherArgs { const uint4* src[3]; uint4* dst[3]; const float2* st_src; float2* st_dst; };
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherArgs a, const int* __restrict__ rows, int64_t B, int64_t L, int64_t Mc, int vec) {
  const int rpb = blockDim.x / vec;                      // rows per workgroup
  const int64_t r = (int64_t)blockIdx.x * rpb + threadIdx.x / vec;
  const int v = threadIdx.x % vec;
  if (r >= Mc) return;
  const int64_t b = r < B ? r : B - 1;
  const int64_t sr = rows ? (int64_t)rows[b] : b * L;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    if (a.src[p]) a.dst[p][r * vec + v] = a.src[p][sr * vec + v];
  if (v == 0 && a.st_src) a.st_dst[r] = a.st_src[sr];
}
int omk_gather_rows(const GatherPlane (&planes)[3], const float* stats_src, float* stats_dst, const int* rows, int64_t B, int64_t L, int64_t Mc,
                    int H, hipStream_t s) {
  if (B <= 0 || Mc <= 0) return 0;
  if (H < 8 || H % 8 || L < 1) OM_FAIL("row gather: rows of whole 16-byte vectors");
  GatherArgs a = {};
  uintptr_t align = (uintptr_t)stats_src | (uintptr_t)stats_dst;
  for (int p = 0; p < 3; ++p) {
    if (!planes[p].src || !planes[p].dst) continue;
    a.src[p] = (const uint4*)planes[p].src; a.dst[p] = (uint4*)planes[p].dst;
    align |= (uintptr_t)planes[p].src | (uintptr_t)planes[p].dst;
  }
  if (stats_src && stats_dst) { a.st_src = (const float2*)stats_src; a.st_dst = (float2*)stats_dst; }
  if (align & 15) OM_FAIL("row gather: 16-byte aligned buffers");
  const int vec = H / 8;
  const int threads = vec >= 256 ? vec : 256 / vec * vec;
  if (threads > 256) OM_FAIL("row gather: at most 2048 columns");
  const int64_t grid = (Mc + threads / vec - 1) / (threads / vec);
  if (grid > 0x7fffffffLL) OM_FAIL("row gather: too many rows for one launch");
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)grid), dim3(threads), 0, s, a, rows, B, L, Mc, vec);
  OM_LAUNCH_CHECK();
  return 0;
}
extern "C" int om_debug_gather_rows(const void* src0, void* dst0, const void* src1, void* dst1, const void* src2, void* dst2, const float* stats_src,
                                    float* stats_dst, const int* rows, int64_t B, int64_t L, int64_t Mc, int H, void* stream) {
  if (!src0 || !dst0) OM_FAIL("om_debug_gather_rows: null argument");
  if (B < 1 || Mc < B) OM_FAIL("om_debug_gather_rows: 1 <= B <= Mc");
  const GatherPlane planes[3] = {{src0, dst0}, {src1, dst1}, {src2, dst2}};
  return omk_gather_rows(planes, stats_src, stats_dst, rows, B, L, Mc, H, (hipStream_t)stream);
}

// x in f32 (a residual stream kept in f32 under a 16-bit compute format: encoder_causal.hip) -> y in the compute format
int omk_layernorm_from_f32(int dtype, const float* x, int64_t ldx, void* y, int64_t ldy, const float* g, const float* b, int64_t M, int H,
                           float eps, int rms, hipStream_t s) {
  const RowFwdPlan p = row_fwd_plan(ROW_FWD_FROM_F32, dtype, M, H, ldx, ldy, row_aligned16(x, y), row_aligned16(g, b), false, false);
  if (p.error) OM_FAIL(p.error);
  if (p.empty) return 0;
  return launch_row_fwd(p, RowFwdArgs{x, ldx, y, ldy, g, b, M, H, eps, rms, nullptr, nullptr, nullptr}, s);
}

// x[f32] += rms(h) * g: the RMSNorm of a sublayer OUTPUT h (compute format) added into a residual stream kept in f32 (Gemma3's
// post_attention_layernorm / post_feedforward_layernorm; g = 1 + w from the host).  One wave per row, the row arithmetic of ln_row.h:
// y = (h * rstd) * g in f32 as norm_and_store's RMS branch, then ONE f32 add.  The reference's autocast rounds y to the 16-bit format
// before that add; this kernel does not (the unrounded sum is the closer one to the fp32 model).
template <typename TIn, int MAX_VEC>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void rmsnorm_add_kernel(const TIn* __restrict__ h, int64_t ldh, float* __restrict__ x, int64_t ldx,
                                                                          const float* __restrict__ g, int64_t M, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nvec = (H / 4 + 63) / 64;
  float v[MAX_VEC][4];
#pragma unroll
  for (int j = 0; j < MAX_VEC; ++j) {
    const int c = (lane + 64 * j) * 4;
    if (j < nvec && c < H) Vec4<TIn>::load(h + row * ldh + c, v[j]);
  }
  float mean, rstd;
  ln_row_stats<MAX_VEC>(v, nvec, lane, H, eps, 1, mean, rstd);
  float* const xr = x + row * ldx;
#pragma unroll
  for (int j = 0; j < MAX_VEC; ++j) {
    const int c = (lane + 64 * j) * 4;
    if (j < nvec && c < H) {
      float gv[4], xv[4];
      Vec4<float>::load(g + c, gv);
      Vec4<float>::load(xr + c, xv);
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[e] = __fadd_rn(xv[e], __fmul_rn(__fmul_rn(v[j][e], rstd), gv[e]));
      Vec4<float>::store(xr + c, xv);
    }
  }
}

template <typename TIn>
static void launch_rmsnorm_add(const void* h, int64_t ldh, float* x, int64_t ldx, const float* g, int64_t M, int H, float eps, hipStream_t s) {
  const unsigned grid = (unsigned)((M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (row_max_vec(H) == 4) hipLaunchKernelGGL((rmsnorm_add_kernel<TIn, 4>), dim3(grid), dim3(64 * ROWS_PER_BLOCK), 0, s, (const TIn*)h, ldh, x, ldx, g, M, H, eps);
  else hipLaunchKernelGGL((rmsnorm_add_kernel<TIn, 8>), dim3(grid), dim3(64 * ROWS_PER_BLOCK), 0, s, (const TIn*)h, ldh, x, ldx, g, M, H, eps);
}

int omk_rmsnorm_add(int dtype, const void* h, int64_t ldh, float* x, int64_t ldx, const float* g, int64_t M, int H, float eps, hipStream_t s) {
  if (const char* why = row_width_error(H)) OM_FAIL(why);
  if (ldh % 4 || ldx % 4) OM_FAIL("norm-add: row pitches of whole four-element vectors");
  if (M <= 0) return 0;
  if (dtype == OM_BF16) launch_rmsnorm_add<bf16_t>(h, ldh, x, ldx, g, M, H, eps, s);
  else if (dtype == OM_F16) launch_rmsnorm_add<f16_t>(h, ldh, x, ldx, g, M, H, eps, s);
  else launch_rmsnorm_add<float>(h, ldh, x, ldx, g, M, H, eps, s);
  OM_LAUNCH_CHECK();
  return 0;
}

// x in the compute format (optionally two planes, bf16) -> y in f32
int omk_layernorm_f32out(int dtype, const void* x, int64_t ldx, float* y, int64_t ldy, const float* g, const float* b,
                         int64_t M, int H, float eps, int rms, hipStream_t s, const void* x_lo, const int* rows, int lo8) {
  const RowFwdPlan p = row_fwd_plan(ROW_FWD_F32OUT, dtype, M, H, ldx, ldy, row_aligned16(x, y, x_lo), row_aligned16(g, b), x_lo != nullptr, lo8 != 0);
  if (p.error) OM_FAIL(p.error);
  if (p.empty) return 0;
  return launch_row_fwd(p, RowFwdArgs{x, ldx, y, ldy, g, b, M, H, eps, rms, x_lo, rows, nullptr}, s);
}

// packed rows: more tokens than the caller's row bound -> every representation becomes NaN (never a silently truncated batch)
__global__ void pack_overflow_poison_kernel(const int* __restrict__ cu, int64_t B, int64_t rows, float* __restrict__ out, int64_t n) {
  if ((int64_t)cu[B + 1] <= rows) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = __int_as_float(0x7fc00000);
}
int omk_pack_overflow_poison(const int* cu, int64_t B, int64_t rows, float* out, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(pack_overflow_poison_kernel, dim3(64), dim3(256), 0, s, cu, B, rows, out, n);
  OM_LAUNCH_CHECK();
  return 0;
}

// f32 rows in -> the normalised rows in `dtype` (the next contraction's operand) AND in f32 (y32: what the next residual add reads):
// the LayerNorm of the 16-bit training forward, whose residual stream stays in f32 as the reference's autocast keeps it
int omk_layernorm_dual(int dtype, const float* x, int64_t ldx, void* y, float* y32, int64_t ldy, const float* g, const float* b,
                       int64_t M, int H, float eps, hipStream_t s) {
  const RowFwdPlan p = row_fwd_plan(ROW_FWD_DUAL, dtype, M, H, ldx, ldy, row_aligned16(x, y), row_aligned16(g, b), false, false);
  if (p.error) OM_FAIL(p.error);
  if (p.empty) return 0;
  return launch_row_fwd(p, RowFwdArgs{x, ldx, y, ldy, g, b, M, H, eps, 0, nullptr, nullptr, y32}, s);
}

int omk_layernorm(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, const float* g,
                  const float* b, int64_t M, int H, float eps, int rms, hipStream_t s, const void* x_lo, int lo8) {
  const RowFwdPlan p = row_fwd_plan(ROW_FWD_LAYERNORM, dtype, M, H, ldx, ldy, row_aligned16(x, y, x_lo), row_aligned16(g, b), x_lo != nullptr, lo8 != 0);
  if (p.error) OM_FAIL(p.error);
  if (p.empty) return 0;
  return launch_row_fwd(p, RowFwdArgs{x, ldx, y, ldy, g, b, M, H, eps, rms, x_lo, nullptr, nullptr}, s);
}

int omk_embed(int dtype, const int64_t* ids, const int64_t* type_ids, const float* word,
              const float* pos, const float* type, const float* g, const float* b, void* out,
              int64_t M, int L, int H, int vocab, int type_vocab, float eps, int bert,
              hipStream_t s, const int* row_map, float* out32) {
  if (const char* why = row_width_error(H)) OM_FAIL(why);
  if (M <= 0) return 0;
  if (out32 && (!bert || row_map)) OM_FAIL("embedding: the f32 copy goes with the BERT LayerNorm on unpacked rows");
  const unsigned grid = (unsigned)((M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const bool narrow = row_max_vec(H) == 4;
#define EMBED_LAUNCH(TT, NV)                                                                   \
  hipLaunchKernelGGL((embed_kernel<TT, NV>), dim3(grid), dim3(64 * ROWS_PER_BLOCK), 0, s, ids, \
                     type_ids, word, pos, type, g, b, (TT*)out, M, L, H, vocab, type_vocab, eps, bert, row_map, out32)
  if (dtype == OM_BF16) {
    if (narrow) EMBED_LAUNCH(bf16_t, 4); else EMBED_LAUNCH(bf16_t, 8);
  } else if (dtype == OM_F16) {
    if (narrow) EMBED_LAUNCH(f16_t, 4); else EMBED_LAUNCH(f16_t, 8);
  } else {
    if (narrow) EMBED_LAUNCH(float, 4); else EMBED_LAUNCH(float, 8);
  }
#undef EMBED_LAUNCH
  OM_LAUNCH_CHECK();
  return 0;
}

int omk_pool(int dtype, const void* x, const int64_t* mask, float* out, int64_t B, int L, int H,
             int mode, hipStream_t s, const int* cu) {
  if (B <= 0) return 0;
  if (H % 4 != 0) OM_FAIL("hidden size must be a multiple of 4");
  if (dtype == OM_BF16)
    hipLaunchKernelGGL((pool_kernel<bf16_t>), dim3((unsigned)B), dim3(256), 0, s, (const bf16_t*)x,
                       mask, out, L, H, mode, cu);
  else if (dtype == OM_F16)
    hipLaunchKernelGGL((pool_kernel<f16_t>), dim3((unsigned)B), dim3(256), 0, s, (const f16_t*)x,
                       mask, out, L, H, mode, cu);
  else
    hipLaunchKernelGGL((pool_kernel<float>), dim3((unsigned)B), dim3(256), 0, s, (const float*)x,
                       mask, out, L, H, mode, cu);
  OM_LAUNCH_CHECK();
  return 0;
}

int omk_l2norm(const float* x, float* y, int64_t M, int D, hipStream_t s) {
  if (M <= 0) return 0;
  const unsigned grid = (unsigned)((M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  hipLaunchKernelGGL(l2norm_kernel, dim3(grid), dim3(64 * ROWS_PER_BLOCK), 0, s, x, y, M, D);
  OM_LAUNCH_CHECK();
  return 0;
}

// NomicBERT's SwiGLU (HF:models/nomic_bert/modeling_nomic_bert.py NomicBertMLP): the one FFN1 contraction leaves [M, 2F] rows of
// (gate | up); out[m, j] = silu(in[m, j]) * in[m, F + j] in f32, rounded once, silu(g) = g / (1 + exp(-g)) (torch.nn.functional.silu).
// One thread per 16-byte vector of the output; the input row is read, never written.
template <typename T>
__global__ __launch_bounds__(256) void swiglu_rows_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t M, int F) {
  constexpr int N = 16 / (int)sizeof(T);                 // elements per 16-byte vector
  const int per_row = F / N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * per_row) return;
  const int64_t m = i / per_row;
  const int j = (int)(i % per_row) * N;
  const T* gp = in + m * 2 * (int64_t)F + j;
  const uint4 gq = *(const uint4*)gp, uq = *(const uint4*)(gp + F);
  const uint32_t gw[4] = {gq.x, gq.y, gq.z, gq.w}, uw[4] = {uq.x, uq.y, uq.z, uq.w};
  uint32_t o[4];
  auto act = [](float g, float u) { return g / (1.0f + expf(-g)) * u; };
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (sizeof(T) == 4) o[e] = __float_as_uint(act(__uint_as_float(gw[e]), __uint_as_float(uw[e])));
    else o[e] = Half16<T>::pack2(act(Half16<T>::lo(gw[e]), Half16<T>::lo(uw[e])), act(Half16<T>::hi(gw[e]), Half16<T>::hi(uw[e])));
  }
  *(uint4*)(out + m * (int64_t)F + j) = make_uint4(o[0], o[1], o[2], o[3]);
}

int omk_swiglu_rows(int dtype, const void* in, void* out, int64_t M, int F, hipStream_t s) {
  if (F < 64 || F % 64) OM_FAIL("SwiGLU rows: the inner width must be a positive multiple of 64");
  if (((uintptr_t)in | (uintptr_t)out) & 15) OM_FAIL("SwiGLU rows: 16-byte aligned buffers");
  if (M <= 0) return 0;
  const int64_t nvec = M * (F / (dtype == OM_F32 ? 4 : 8));
  if ((nvec + 255) / 256 > 0x7fffffffLL) OM_FAIL("SwiGLU rows: too many rows for one launch");
  const unsigned grid = (unsigned)((nvec + 255) / 256);
  if (dtype == OM_BF16) hipLaunchKernelGGL(swiglu_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)in, (bf16_t*)out, M, F);
  else if (dtype == OM_F16) hipLaunchKernelGGL(swiglu_rows_kernel<f16_t>, dim3(grid), dim3(256), 0, s, (const f16_t*)in, (f16_t*)out, M, F);
  else hipLaunchKernelGGL(swiglu_rows_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)in, (float*)out, M, F);
  OM_LAUNCH_CHECK();
  return 0;
}

extern "C" int om_debug_swiglu_rows(int dtype, const void* in, void* out, int64_t M, int F, void* stream) {
  if (!in || !out) OM_FAIL("om_debug_swiglu_rows: null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("SwiGLU rows: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (M < 0) OM_FAIL("SwiGLU rows: a negative row count");
  return omk_swiglu_rows(dtype, in, out, M, F, (hipStream_t)stream);
}

// ---- test hooks of the row kernels (include/openmatch_hip.h): argument checks, then the launcher as it is ----
// host only: the note word the entry would store for these arguments (0: nothing to do; -1: refused, the entry's text in om_last_error)
extern "C" int om_debug_row_fwd_plan(int entry, int dtype, int64_t M, int H, int64_t ldx, int64_t ldy, int data_aligned, int param_aligned, int plane,
                                     int lo8) {
  omk_row_note(0);
  const char* why = nullptr;
  if (entry < ROW_FWD_LAYERNORM || entry > ROW_FWD_DUAL) why = "entry must be 0 (layernorm), 1 (f32out), 2 (from_f32) or 3 (dual)";
  else if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) why = "dtype must be OM_F32, OM_BF16 or OM_F16";
  const RowFwdPlan p = why ? RowFwdPlan{} : row_fwd_plan(entry, dtype, M, H, ldx, ldy, data_aligned != 0, param_aligned != 0, plane != 0, lo8 != 0);
  if (why || p.error) {
    om_set_error(std::string("om_debug_row_fwd_plan: ") + (why ? why : p.error));
    return -1;
  }
  return p.empty ? 0 : row_fwd_word(p);
}
extern "C" int om_debug_layernorm(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, const float* g, const float* b, int64_t M, int H,
                                  float eps, int rms, const void* x_lo, int lo8, void* stream) {
  omk_row_note(0);
  if (!x || !y || !g) OM_FAIL("om_debug_layernorm: null argument");
  OM_DBG_DTYPE("om_debug_layernorm");
  return omk_layernorm(dtype, x, ldx, y, ldy, g, b, M, H, eps, rms, (hipStream_t)stream, x_lo, lo8);
}
extern "C" int om_debug_layernorm_f32out(int dtype, const void* x, int64_t ldx, float* y, int64_t ldy, const float* g, const float* b, int64_t M,
                                         int H, float eps, int rms, const void* x_lo, const int* rows, int lo8, void* stream) {
  omk_row_note(0);
  if (!x || !y || !g) OM_FAIL("om_debug_layernorm_f32out: null argument");
  OM_DBG_DTYPE("om_debug_layernorm_f32out");
  return omk_layernorm_f32out(dtype, x, ldx, y, ldy, g, b, M, H, eps, rms, (hipStream_t)stream, x_lo, rows, lo8);
}
/* x[f32] += rms(h) * g (Gemma3's norm of a sublayer output added into the f32 residual stream) */
extern "C" int om_debug_rmsnorm_add(int dtype, const void* h, int64_t ldh, float* x, int64_t ldx, const float* g, int64_t M, int H, float eps,
                                    void* stream) {
  if (!h || !x || !g) OM_FAIL("om_debug_rmsnorm_add: null argument");
  OM_DBG_DTYPE("om_debug_rmsnorm_add");
  return omk_rmsnorm_add(dtype, h, ldh, x, ldx, g, M, H, eps, (hipStream_t)stream);
}
extern "C" int om_debug_layernorm_from_f32(int dtype, const float* x, int64_t ldx, void* y, int64_t ldy, const float* g, const float* b,
                                           int64_t M, int H, float eps, int rms, void* stream) {
  omk_row_note(0);
  if (!x || !y || !g) OM_FAIL("om_debug_layernorm_from_f32: null argument");
  OM_DBG_DTYPE("om_debug_layernorm_from_f32");
  return omk_layernorm_from_f32(dtype, x, ldx, y, ldy, g, b, M, H, eps, rms, (hipStream_t)stream);
}
extern "C" int om_debug_layernorm_dual(int dtype, const float* x, int64_t ldx, void* y, float* y32, int64_t ldy, const float* g, const float* b,
                                       int64_t M, int H, float eps, void* stream) {
  omk_row_note(0);
  if (!x || !y || !y32 || !g) OM_FAIL("om_debug_layernorm_dual: null argument");
  OM_DBG_DTYPE16("om_debug_layernorm_dual");
  return omk_layernorm_dual(dtype, x, ldx, y, y32, ldy, g, b, M, H, eps, (hipStream_t)stream);
}
extern "C" int om_debug_pool(int dtype, const void* x, const int64_t* mask, float* out, int64_t B, int L, int H, int mode, const int* cu,
                             void* stream) {
  if (!x || !mask || !out) OM_FAIL("om_debug_pool: null argument");
  OM_DBG_DTYPE("om_debug_pool");
  return omk_pool(dtype, x, mask, out, B, L, H, mode, (hipStream_t)stream, cu);
}
extern "C" int om_debug_l2norm(const float* x, float* y, int64_t M, int D, void* stream) {
  if (!x || !y) OM_FAIL("om_debug_l2norm: null argument");
  return omk_l2norm(x, y, M, D, (hipStream_t)stream);
}
extern "C" int om_debug_ln_fold(int dtype, const void* W, const float* gamma, const float* beta, const float* b, void* Wf, float* colsum,
                                float* bf, int N, int K, void* stream) {
  if (!W || !gamma || !Wf || !colsum || !bf) OM_FAIL("om_debug_ln_fold: null argument");
  OM_DBG_DTYPE16("om_debug_ln_fold");
  return omk_ln_fold(dtype, W, gamma, beta, b, Wf, colsum, bf, N, K, (hipStream_t)stream);
}
extern "C" int om_debug_ln_stats_reduce(const float* slots, int nslots, int64_t M, float* out, void* stream) {
  if (!slots || !out) OM_FAIL("om_debug_ln_stats_reduce: null argument");
  return omk_ln_stats_reduce(slots, nslots, M, out, (hipStream_t)stream);
}

extern "C" int om_debug_embed(int dtype, const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                              const float* g, const float* b, void* out, int64_t M, int L, int H, int vocab, int type_vocab, float eps,
                              void* stream) {
  if (!ids || !word || !g || !b || !out) OM_FAIL("om_debug_embed: null argument");
  if (dtype != OM_F32 && dtype != OM_BF16 && dtype != OM_F16) OM_FAIL("embedding: dtype must be OM_F32, OM_BF16 or OM_F16");
  if (L < 1 || vocab < 1 || (type && type_vocab < 1)) OM_FAIL("embedding: L, vocab and the type table's rows must be at least 1");
  return omk_embed(dtype, ids, type_ids, word, pos, type, g, b, out, M, L, H, vocab, type_vocab, eps, 1, (hipStream_t)stream);
}

int omk_t5_bias(const float* table, const int* lut, float* out, int L, int heads, hipStream_t s) {
  hipLaunchKernelGGL(t5_bias_kernel, dim3(256), dim3(256), 0, s, table, lut, out, L, heads);
  OM_LAUNCH_CHECK();
  return 0;
}
extern "C" int om_debug_t5_bias(const float* table, const int* lut, float* out, int L, int heads, void* stream) {
  if (!table || !lut || !out) OM_FAIL("om_debug_t5_bias: null argument");
  if (L < 1 || heads < 1) OM_FAIL("om_debug_t5_bias: L and heads must be at least 1");
  return omk_t5_bias(table, lut, out, L, heads, (hipStream_t)stream);
}

extern "C" int om_index_to_f16(const float* rows_f32, int64_t N, int d, void* rows_f16,
                               float* stats, void* stream) {
  if (N <= 0) return 0;
  const unsigned grid = (unsigned)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  hipLaunchKernelGGL(index_to_f16_kernel, dim3(grid), dim3(64 * ROWS_PER_BLOCK), 0,
                     (hipStream_t)stream, rows_f32, (f16_t*)rows_f16, N, d, (unsigned*)stats);
  OM_LAUNCH_CHECK();
  return 0;
}

extern "C" int om_index_add_f16(int in_dtype, const void* rows, int64_t N, int d, void* rows_f16, float* stats, unsigned* nonfinite,
                                void* stream) {
  if (in_dtype != OM_F32 && in_dtype != OM_F16) OM_FAIL("om_index_add_f16: in_dtype must be OM_F32 or OM_F16");
  if (N <= 0) return 0;
  if (!rows || !rows_f16 || !stats || !nonfinite) OM_FAIL("om_index_add_f16: null argument");
  if (d < 1) OM_FAIL("om_index_add_f16: d must be at least 1");
  if (N > 0x7fffffffLL * ROWS_PER_BLOCK) OM_FAIL("om_index_add_f16: too many rows for one call");
  const unsigned grid = (unsigned)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const bool vec = d % 8 == 0 && (((uintptr_t)rows | (uintptr_t)rows_f16) & 15) == 0;
  const dim3 block(64 * ROWS_PER_BLOCK);
  const hipStream_t s = (hipStream_t)stream;
  f16_t* y = (f16_t*)rows_f16;
  unsigned* st = (unsigned*)stats;
  if (in_dtype == OM_F32) {
    if (vec) hipLaunchKernelGGL((index_add_f16_kernel<float, true>), dim3(grid), block, 0, s, (const float*)rows, y, N, d, st, nonfinite);
    else hipLaunchKernelGGL((index_add_f16_kernel<float, false>), dim3(grid), block, 0, s, (const float*)rows, y, N, d, st, nonfinite);
  } else {
    if (vec) hipLaunchKernelGGL((index_add_f16_kernel<f16_t, true>), dim3(grid), block, 0, s, (const f16_t*)rows, y, N, d, st, nonfinite);
    else hipLaunchKernelGGL((index_add_f16_kernel<f16_t, false>), dim3(grid), block, 0, s, (const f16_t*)rows, y, N, d, st, nonfinite);
  }
  OM_LAUNCH_CHECK();
  return 0;
}

// ---- self-check of ln_row.h's row reduction against the __shfl_xor butterfly (om_debug_wave_sum_check) ----
__global__ __launch_bounds__(256) void wave_sum_check_kernel(const float* __restrict__ in, float* __restrict__ a, float* __restrict__ b, int64_t groups) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;
  const float v = in[g * 64 + (threadIdx.x & 63)];
  const float s0 = wave_sum(v);
  float s1[1] = {v};
  ln_wave_sums<1>(s1);
  if ((threadIdx.x & 63) == (int)(g % 64)) { a[g] = s0; b[g] = s1[0]; }      // a different lane reports for every group: all lanes hold the sum
}
extern "C" int om_debug_wave_sum_check(const float* in, float* out_shuffle, float* out_dpp, int64_t groups, void* stream) {
  if (!in || !out_shuffle || !out_dpp || groups <= 0) OM_FAIL("om_debug_wave_sum_check: null argument");
  hipLaunchKernelGGL(wave_sum_check_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, (hipStream_t)stream, in, out_shuffle, out_dpp, groups);
  OM_LAUNCH_CHECK();
  return 0;
}
