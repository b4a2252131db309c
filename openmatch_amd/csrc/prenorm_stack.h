// What the f32-residual pre-norm stacks share -- Llama / Qwen2 and Qwen3 (encoder_causal.hip), Gemma3 (encoder_gemma3.hip) -- stated once:
// the workspace and how it is carved, the call's argument checks (prenorm_check), the launches in front of the layer loop
// (prenorm_begin: mask extents, packed rows, the embedding into the f32 residual stream), the launches behind it (prenorm_tail: final
// norm, pooling, head), the packed-rows rule, and the RUN / PrenormGemm helpers the loops are written in.  Each family keeps its
// check_cfg*, its per-layer pointer checks and its layer loop in its own file; a forward there reads
//
//   prenorm_check  ->  the family's per-layer checks  ->  prenorm_begin  ->  its layer loop  ->  prenorm_tail
//
// so that every refusal comes before the first launch: a refused call leaves nothing on the stream.
#pragma once
#include <string>

#include "kernels.h"

#define RUN(expr) do { if (expr) return 1; } while (0)

// Activation buffers ([M tokens] x width): x [M, H] f32 residual stream; in the compute dtype y normed input / sublayer output,
// qkv [M, P = (heads + 2 kv) * head_dim], ctx [M, A = heads * head_dim], ff / ff2 [M, F].
struct PrenormWs {
  char *x, *y, *qkv, *ctx, *ff, *ff2;
  float *pooled, *headout, *final32;
  int *kmax, *last_rows;          // last_rows: only where the family pools the last token (0 bytes otherwise)
  int *cu, *cls_rows, *row_map;   // packed rows: sequence offsets [B + 2], first row of each sequence [B], token of each row [packed_rows]
  int64_t M;        // token rows: packed_rows, or B * L
  int64_t Mp;       // row count the contractions run on: M rounded up to whole 256-row tiles for large 16-bit batches (as encoder.hip)
  int A, P;         // attention width (ctx rows, o_proj's contraction: it need not equal the hidden size) and the fused q | k | v width
  size_t total;
};

static PrenormWs prenorm_carve(const OmEncoderConfig* c, int n_kv_heads, int head_dim, bool want_last_rows, int64_t B, int64_t L, char* base,
                               int64_t packed_rows = 0) {
  const bool half = c->dtype == OM_BF16 || c->dtype == OM_F16;
  const size_t es = half ? 2 : 4;
  const size_t Mreal = packed_rows > 0 ? (size_t)packed_rows : (size_t)B * L, H = c->hidden, F = c->ffn;
  const size_t A = (size_t)c->n_heads * head_dim, P = (size_t)(c->n_heads + 2 * n_kv_heads) * head_dim;
  const size_t M = (half && Mreal >= 512) ? (Mreal + 255) / 256 * 256 : Mreal;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return base + o; };
  PrenormWs w;
  w.x = take(M * H * 4);
  w.y = take(M * H * es);
  w.qkv = take(M * P * es);
  w.ctx = take(M * A * es);
  w.ff = take(M * F * es);
  w.ff2 = take(M * F * es);
  w.pooled = (float*)take((size_t)B * H * 4);
  w.headout = (float*)take((size_t)B * (c->head_out > 0 ? c->head_out : 1) * 4);
  w.kmax = (int*)take((size_t)B * 4);
  w.last_rows = (int*)take(want_last_rows ? (size_t)B * 4 : 0);
  w.final32 = (float*)take(c->pooling == OM_POOL_MEAN ? Mreal * H * 4 : 0);      // mean pooling reads every row of the f32 final norm
  w.cu = (int*)take(packed_rows > 0 ? (size_t)(B + 2) * 4 : 0);
  w.cls_rows = (int*)take(packed_rows > 0 ? (size_t)B * 4 : 0);
  w.row_map = (int*)take(packed_rows > 0 ? (size_t)packed_rows * 4 : 0);
  w.M = (int64_t)Mreal;
  w.Mp = (int64_t)M;
  w.A = (int)A;
  w.P = (int)P;
  w.total = off;
  return w;
}

// Which (B, L, packed_rows) a packed entry takes: whole 256-row tiles, at least the family's `min_rows`, at most the padded count's tiles.
// Few rows: the padded entry's contractions take the weight-streaming kernel -- decided there on ITS row count B * L, so a batch whose
// PADDED form is that small is sent back (as om_encoder_packed_supported).
static bool prenorm_packed_rows_rule(int64_t B, int64_t L, int64_t packed_rows, int64_t min_rows) {
  if (B <= 0 || L <= 0 || L > 1024 || packed_rows <= 0) return false;
  if (packed_rows % 256 || packed_rows < min_rows || packed_rows > B * L + 255) return false;
  return B * L > (int64_t)om_option(OM_OPT_GEMM_SKINNY_M);
}

// How a family's refusals read
struct PrenormFamily {
  const char* tag;              // what the shared refusals begin with: "" (the Llama / Qwen2 / Qwen3 entries), "Gemma3"
  int64_t packed_floor;         // least packed_rows a forward takes: 512; 0 where only the family's rule bounds it from below (Gemma3)
  bool pools_last;              // OM_POOL_LAST is served: the workspace holds last_rows
  const char* layers_null;      // the refusal of a missing per-layer host table
  const char* emb_null;         // the refusal of a missing word_emb / final_ln_g
};

// Every check of a forward's arguments that is not the family's own, in one order, and the carved workspace; nothing is launched.
// layer_tables: the per-layer host arrays the family reads are all given.
static int prenorm_check(const PrenormFamily& fam, const OmEncoderConfig* c, int n_kv_heads, int head_dim, const OmEncoderWeights* w,
                         bool layer_tables, int64_t B, int64_t L, const void* out_hidden, const float* out_reps, void* workspace,
                         size_t workspace_bytes, int64_t packed_rows, PrenormWs* ws) {
  const std::string tag = fam.tag;
  if (L < 1 || L > 1024) OM_FAIL((tag.empty() ? tag : tag + ": ") + "sequence length must be in [1,1024]");
  if (packed_rows > 0) {
    const std::string pre = tag.empty() ? tag : tag + " ";
    if (c->pooling == OM_POOL_NONE || out_hidden) OM_FAIL(pre + "packed rows: representations only (a pooling, no out_hidden)");
    if (packed_rows % 256 || packed_rows < fam.packed_floor || packed_rows > B * L + 255)
      OM_FAIL(pre + (fam.packed_floor > 0 ? "packed_rows: a multiple of 256 in [" + std::to_string(fam.packed_floor) + ", B * L + 255]"
                                          : std::string("packed_rows: a multiple of 256, at most B * L + 255")));
  }
  if (!workspace || ((uintptr_t)workspace & 255)) OM_FAIL("workspace must be 256-byte aligned");
  *ws = prenorm_carve(c, n_kv_heads, head_dim, fam.pools_last, B, L, (char*)workspace, packed_rows);
  if (ws->total > workspace_bytes) OM_FAIL("workspace too small");
  if (c->pooling != OM_POOL_NONE && !out_reps) OM_FAIL("out_reps required when pooling is set");
  if (c->n_layers > 0 && !layer_tables) OM_FAIL(fam.layers_null);
  if (!w->word_emb || !w->final_ln_g) OM_FAIL(fam.emb_null);
  return 0;
}

// The launches in front of the layer loop: each row's mask extent, the packed layout, x = embed(ids) in f32 (through row_map when packed)
static int prenorm_begin(const OmEncoderConfig* c, const OmEncoderWeights* w, const PrenormWs& ws, const int64_t* input_ids,
                         const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows, hipStream_t s) {
  RUN(omk_mask_extent(attention_mask, B, (int)L, ws.kmax, s));
  if (packed_rows > 0) {
    RUN(omk_pack_rows(ws.kmax, B, (int)L, packed_rows, ws.cu, ws.cls_rows, ws.row_map, s));
    OM_HIP(hipMemsetAsync(ws.ctx, 0, (size_t)ws.M * ws.A * (c->dtype == OM_F32 ? 4 : 2), s));      // the tail rows: no attention workgroup writes them
  }
  return omk_embed(OM_F32, input_ids, nullptr, w->word_emb, nullptr, nullptr, nullptr, nullptr, ws.x, ws.M, (int)L, c->hidden, c->vocab, 1, c->ln_eps,
                   0, s, packed_rows > 0 ? ws.row_map : nullptr);
}

// One contraction of a layer loop, over the workspace's Mp rows: C (out_dt) = act(A W^T + bias) (+ or * res); operands in the compute dtype
struct PrenormGemm {
  int dt;
  int64_t Mg;
  hipStream_t s;
  int operator()(const void* A, int64_t lda, const void* W, int64_t ldw, int out_dt, void* C, int64_t ldc, int64_t N, int64_t K,
                 const float* bias = nullptr, const void* res = nullptr, int64_t ldr = 0, int act = OM_ACT_NONE) const {
    return om_gemm_nt(dt, A, lda, W, ldw, out_dt, C, ldc, Mg, N, K, bias, res, ldr, act, s);
  }
};

// rows[b] = the token row of sequence b's LAST unmasked token (kmax[b] = 1 + its index; L for a row without one: the last column)
static __global__ void last_rows_kernel(const int* __restrict__ kmax, int64_t B, int L, int* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rows[b] = (int)(b * L + kmax[b] - 1);
}

// packed rows: the row of sequence b's last unmasked token is cu[b] + kmax[b] - 1, clamped into the buffer as cls_rows is (a bound that
// was too small: the representations are poisoned afterwards)
static __global__ void last_rows_packed_kernel(const int* __restrict__ kmax, const int* __restrict__ cu, int64_t B, int rows_cap, int* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rows[b] = min(cu[b] + kmax[b] - 1, rows_cap - 1);
}

// The launches behind the layer loop.  norm: the hidden states in the compute dtype when asked for; the pooled rows ALWAYS as f32 rows of
// the normalisation of just the rows pooling reads (the reference's autocast leaves the norm's arithmetic in fp32), as the other stacks
// do.  Then the head, the l2 norm and, for packed rows, the overflow poison (omk_pooled_tail: a bound below the token count poisons the
// representations).  OM_POOL_LAST needs ws.last_rows: a family that did not ask for it refuses that pooling in its check_cfg.
static int prenorm_tail(const OmEncoderConfig* c, const OmEncoderWeights* w, const PrenormWs& ws, const int64_t* attention_mask, int64_t B,
                        int64_t L, void* out_hidden, float* out_reps, int64_t packed_rows, hipStream_t s) {
  const bool packed = packed_rows > 0;
  const int dt = c->dtype, H = c->hidden;
  const int64_t M = ws.M;
  const float* fg = w->final_ln_g;
  const float* xf = (const float*)ws.x;
  if (out_hidden) RUN(omk_layernorm_from_f32(dt, xf, H, out_hidden, H, fg, nullptr, M, H, c->ln_eps, 1, s));
  if (c->pooling == OM_POOL_NONE) return 0;
  float* pooled = c->head_in > 0 && w->head_w ? ws.pooled : out_reps;
  if (c->pooling == OM_POOL_FIRST) {
    if (packed) RUN(omk_layernorm_f32out(OM_F32, xf, H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s, nullptr, ws.cls_rows));
    else RUN(omk_layernorm_f32out(OM_F32, xf, L * H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s));
  } else if (c->pooling == OM_POOL_LAST) {
    const dim3 grid((unsigned)((B + 255) / 256));
    if (packed) hipLaunchKernelGGL(last_rows_packed_kernel, grid, dim3(256), 0, s, ws.kmax, ws.cu, B, (int)packed_rows, ws.last_rows);
    else hipLaunchKernelGGL(last_rows_kernel, grid, dim3(256), 0, s, ws.kmax, B, (int)L, ws.last_rows);
    OM_LAUNCH_CHECK();
    RUN(omk_layernorm_f32out(OM_F32, xf, H, pooled, H, fg, nullptr, B, H, c->ln_eps, 1, s, nullptr, ws.last_rows));
  } else {
    RUN(omk_layernorm_f32out(OM_F32, xf, H, ws.final32, H, fg, nullptr, M, H, c->ln_eps, 1, s));
    RUN(omk_pool(OM_F32, ws.final32, attention_mask, pooled, B, (int)L, H, OM_POOL_MEAN, s, packed ? ws.cu : nullptr));
  }
  return omk_pooled_tail(c, w, pooled, out_reps, B, packed ? ws.cu : nullptr, packed_rows, s);
}
