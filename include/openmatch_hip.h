/*
 * openmatch_hip.h — C ABI of the MI355X (gfx950) dense-retrieval hot path.
 *
 * The reference (thunlp/OpenMatch v2) has no native boundary of its own: every
 * FLOP of its hot path runs inside un-vendored third-party libraries
 * (HF transformers, torch ATen, faiss, NCCL).  This header is the boundary a
 * maintainer would bind instead of those libraries; each entry point names the
 * reference call site it replaces (paths relative to the reference tree,
 * `src/openmatch/...`; `HF:` = installed transformers 5.15).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *     pointers are borrowed, never owned or freed by the library;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     nothing synchronises the device unless the entry point says so;
 *   - no hidden allocation on the hot loop: scratch is a caller-provided
 *     workspace whose size comes from the matching *_workspace_bytes();
 *   - return value: 0 = OK, non-zero = error, message via om_last_error()
 *     (thread-local, valid until the next failing call on that thread);
 *   - matrices are row-major, leading dimensions in ELEMENTS.
 */
#ifndef OPENMATCH_HIP_H
#define OPENMATCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OM_ABI_VERSION 6   /* 6: OM_ARCH_MODERNBERT; rope / sliding-window fields appended to OmEncoderConfig, final_ln_b to OmEncoderWeights
                    * 5 (round 5): om_grad_sqnorm, om_adamw_step, om_loss_scale_update, om_encoder_packed_supported; OM_F16 training */

/* element types */
#define OM_F32 0
#define OM_BF16 1
#define OM_F16 2 /* IEEE half: the search shadow index; the inference encoder's float16 mode (OmEncoderConfig.dtype) */

/* GEMM epilogue activation */
#define OM_ACT_NONE 0
#define OM_ACT_GELU_ERF 1  /* HF "gelu"      (HF:activations.py GELUActivation)   */
#define OM_ACT_RELU 2      /* HF "relu"      (T5 DenseReluDense)                  */
#define OM_ACT_GELU_TANH 3 /* HF "gelu_new"  (T5 v1.1 gated act)                  */
#define OM_ACT_SILU 5      /* HF "silu": OmCausalConfig.base.act and OM_ARCH_NOMICBERT only -- those forwards apply it in an elementwise kernel of
                              their own (silu(gate) * up); NOT a GEMM epilogue: om_gemm_nt does not take it (4 is internal to the training epilogues) */
#define OM_ACT_MUL_RESID 0x100 /* flag: multiply by `resid` instead of adding it (gated FFN) */
#define OM_ACT_PRE_GRAD 0x200  /* flag (erf-GELU training epilogue, 16-bit output): `pre_act` receives gelu'(v) instead of the pre-activation
                                * v -- the backward's dgrad then multiplies by it (OM_ACT_MUL_RESID) instead of evaluating gelu' */

/* encoder architecture */
#define OM_ARCH_BERT 0 /* HF:models/bert/modeling_bert.py  BertModel -- the post-LayerNorm stack; also RoBERTa, and with two optional
                          parts: no token-type table (type_emb == NULL: DistilBERT, MPNet) and a relative-position bias added to the
                          scaled scores of every layer (rel_bias != NULL with rel_buckets > 0: MPNet) */
#define OM_ARCH_T5 1   /* HF:models/t5/modeling_t5.py      T5EncoderModel  */
#define OM_ARCH_MODERNBERT 2 /* HF:models/modernbert/modeling_modernbert.py  ModernBertModel (inference only):
                              * word embedding + LayerNorm; per layer x += Wo(attn(rope(Wqkv(LN1(x))))) (layer 0: no LN1,
                              * ln1_g == NULL), x += W2(gelu_erf(W1 LN2(x)) * Wg LN2(x)); final LayerNorm.  LayerNorm biases
                              * optional (norm_bias), no linear biases.  Attention at 1/sqrt(64) with rotary Q/K (rope_theta_global /
                              * rope_theta_local); layers flagged in sliding_layers see keys |q - k| <= half_window only. */

#define OM_ARCH_CAUSAL 3 /* HF:models/llama/modeling_llama.py LlamaModel, HF:models/qwen2/modeling_qwen2.py Qwen2Model (inference only):
                          * OmCausalConfig.base.arch, served by om_causal_encoder_forward alone (om_encoder_forward refuses it as unknown) */

#define OM_ARCH_NOMICBERT 4 /* HF:models/nomic_bert/modeling_nomic_bert.py NomicBertModel (nomic-embed-text-v1 / v1.5; inference only): the
                            * post-LayerNorm stack of OM_ARCH_BERT on its four layer loops with three differences -- no linear layer has a bias
                            * (every *_b is NULL), Q and K are rotated before attention (rotate_half pairs of 64-wide heads, theta in
                            * rope_theta_global, position = the token's column), and the feed-forward is SwiGLU: ffn1_w is [2F, H] rows
                            * gate_proj | up_proj (ONE contraction), down(silu(gate) * up) with ffn2_w [H, F].  The embedding is
                            * LayerNorm(word + token type): pos_emb is NULL, max_pos bounds L only.  act = OM_ACT_SILU; head_dim 64; hidden and
                            * ffn multiples of 64; rel_buckets and the other rotary / window fields are 0.  float16 as for OM_ARCH_BERT: nothing clamps. */

/* pooling — modeling/dense_retrieval_model.py:145-150 */
#define OM_POOL_NONE 0
#define OM_POOL_FIRST 1
#define OM_POOL_MEAN 2 /* utils.py:233-235 mean_pooling */
#define OM_POOL_LAST 3 /* the hidden state of each row's last unmasked token (right or left padding); om_causal_encoder_forward only */

/* search precision */
#define OM_SEARCH_F32 0           /* exact f32 MFMA scan                                   */
#define OM_SEARCH_F16_RESCORE 1   /* f16 MFMA candidate scan + exact f32 re-score (same ids)  */
#define OM_SEARCH_F16_ONLY 2      /* the float16 rows ARE the index (2 bytes per element): the same scan, the re-score and the
                                   * on-device redo read the float16 rows; index_f32 is not read and may be NULL */

const char* om_last_error(void);
int om_abi_version(void);

/* Number of HIP devices visible, or -1 with om_last_error() set. */
int om_device_count(void);

/* Measurement aid (bench.py's `roofline` object): while enabled, every launch of the dense
 * contraction kernel (class 0: bf16 encoder/scan GEMM, class 1: f32 GEMM, class 2: filtered
 * index scan) is bracketed by hipEvents on the launch stream.  om_kernel_timing_read()
 * synchronises those events, returns the summed kernel time / launch count / algorithmic
 * FLOPs (2*M*N*K) of the class since the last reset, and resets it. */
#define OM_TIMING_GEMM_BF16 0
#define OM_TIMING_GEMM_F32 1
#define OM_TIMING_SCAN 2
/* Debug hook: when `buf` is non-NULL every 256-row-tile GEMM workgroup writes 32 shader-clock
 * stamps (start, prologue, per-K-step, epilogue) to buf[32*block]; NULL switches it off. */
void om_debug_gemm_trace(unsigned long long* buf);
/* Debug hook for A/B measurements inside one process: 0 = default tile-generation selection; 6 = never the persistent
 * generation 7 (gemm_wide7.h); 70 = generation 7 with one tile per workgroup (no cross-tile prefetch). */
void om_debug_gemm_gen(int gen);
/* Test hook: the kernel family of the last GEMM launcher the calling thread reached.  Each launcher stores its code; omk_gemm
 * (under every om_gemm_nt call) stores 0 on entry, before any argument check, so an om_gemm_nt call that launches nothing --
 * an error, an empty problem -- reads 0.  Internal callers that reach a launcher without omk_gemm only store their family.
 * Lets a test assert that a case reached the family it names. */
#define OM_GEMM_FAMILY_V1 1          /* gemm_nt_kernel: 128 x 128 tiles, any M, N                                  */
#define OM_GEMM_FAMILY_V2 2          /* gemm_nt_kernel2: 256 x 128 tiles                                           */
#define OM_GEMM_FAMILY_V6 6          /* gemm_nt_kernel6: 256 x 256 tiles (gemm_wide6_*.hip)                          */
#define OM_GEMM_FAMILY_G7 7          /* gemm_nt_kernel7: persistent 256 x 256, the K ring restarts per tile         */
#define OM_GEMM_FAMILY_G7_ONE_TILE 70 /* gemm_nt_kernel7 with one tile per workgroup (om_debug_gemm_gen(70))       */
#define OM_GEMM_FAMILY_G7C16 71      /* gemm_nt_kernel7c16: continuous ring, no residual                            */
#define OM_GEMM_FAMILY_G7R16 72      /* gemm_nt_kernel7r16: continuous ring, residual                               */
#define OM_GEMM_FAMILY_SKINNY 9      /* gemm_skinny.hip: few rows, weight streaming                                 */
int om_debug_gemm_last(void);
/* Test hook: the family (OM_GEMM_FAMILY_*) an om_gemm_nt call with these arguments would launch at the current switches, 0 for an empty
 * problem, -1 for a call om_gemm_nt refuses.  Launches nothing and touches no GPU: the pointers are read as addresses only (alignment,
 * null), so the whole decision table can be walked with made-up addresses on a machine without a GPU. */
int om_debug_gemm_plan(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C, int64_t ldc,
                       int64_t M, int64_t N, int64_t K, const float* bias, const void* resid, int64_t ldr, int act);
/* Test hooks for the epilogues om_gemm_nt cannot express (tests/test_gemm_epilogues.py): the fused-LayerNorm and two-plane epilogues of
 * generation 7, the training epilogues (pre-activation tape, dropout; act may also be 4 = (acc + bias) * gelu'(resid), the backward
 * through erf-GELU), the f32-stream and pending-LayerNorm extras of the few-rows kernel.  OmDebugGemmEpilogue mirrors the internal
 * GemmEpilogue (csrc/kernels.h, which documents every field) except its trace pointer; zero-initialise it and set what the case needs.
 * om_debug_gemm_ex copies the struct field by field and calls the internal omk_gemm with every argument unchanged -- it checks nothing
 * but a NULL ep, so the planner's and the launchers' own refusals are what a test sees; om_debug_gemm_last() names the family.
 * om_debug_gemm_plan_ex is om_debug_gemm_plan for such a call: the family, 0 for an empty problem, -1 for a refusal; launches nothing,
 * reads every pointer as an address only.  om_debug_gemm_splitk forwards to the K-sliced weight-gradient contraction
 * C (f32) += A[M, K] B[N, K]^T (f32 atomics; K * sizeof(in) % 128 == 0). */
typedef struct OmDebugGemmEpilogue {
  const float* bias; const void* resid; int64_t ldr; int act;
  void* pre_act; int64_t ldp; float drop_p; uint64_t seed; const int* drop_rows;
  const float* ln_stats; const float* ln_colsum; const float* rln_stats; const float* rln_g; const float* rln_b; float* stats_out;
  const void* resid_lo; void* out_lo;
  const float* resid32; float* out32;
  const float* a_ln32; const float* a_ln_g; const float* a_ln_b; float* a_ln_stats_out; const float* rln32; const float* rln32_stats;
  int lo8; float ln_inv_h, ln_eps; int ln_rms; int reverse;
  const int* rows_dev;   /* a row count in device memory: generation 7 skips the rows from roundup256(clamp(count, 0, M)) on; others ignore it */
} OmDebugGemmEpilogue;
int om_debug_gemm_ex(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, const OmDebugGemmEpilogue* ep, void* stream);
int om_debug_gemm_plan_ex(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int out_dtype, void* C, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, const OmDebugGemmEpilogue* ep);
int om_debug_gemm_splitk(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                         int64_t N, int64_t K, void* stream);
/* Run-time switches for A/B measurements and tests (initialised from the environment variable of the same
 * name on first use): OM_OPT_ENCODER_FUSED_LN 1 = LayerNorm / RMSNorm fused across the encoder GEMMs where the
 * shapes allow (default), 0 = one normalisation kernel per site; OM_OPT_ENCODER_DEBUG 1 = log the path taken. */
#define OM_OPT_ENCODER_FUSED_LN 0
#define OM_OPT_ENCODER_DEBUG 1
#define OM_OPT_ATTENTION_FAST 2   /* bit mask (default 1), read once per call by the attention planners (csrc/attn_plan.h; DESIGN.md 4c lists the rules).
                                     bit 0: bfloat16 on the 16-bit kernels -- forward the low-instruction-count and chunked ones, backward the
                                     transposing-read one up to 128 tokens and the tile-at-a-time one from 193 (cleared: the generic kernels; float16
                                     has no others in the forward); bit 1 (tests): the kernels that serve more than 256 tokens -- online-softmax
                                     forward, tile-at-a-time backward -- at every length in the 16-bit formats; bit 2 (A/B): the first online-softmax
                                     forward kernel instead of the chunked 16-bit one */
#define OM_OPT_SCAN_GEN7 3        /* 1 (default): f16 index scan of wide query batches on the persistent generation-7 kernel; 0: generation 6 */
#define OM_OPT_SCAN_GROWTH 4      /* fast schedule of the index scan: rows scanned per round grow by this many percent of the rows already
                                    * scanned (default 60; smaller = more rounds, tighter thresholds, fewer appends per tile) */
#define OM_OPT_WGRAD_DEBUG 5     /* 0 (default); A/B switches of the weight-gradient kernel: bit 3 the register-staged kernel for everything, value >> 4 =
                                   * workgroups aimed at / 64.  Bits 1 (plain stores) and 2 (one step of the token loop) break the result: they are timing
                                   * probes and act only in a probe build (-DOM_PROBE_KERNELS); the shipped library ignores them (round 6) */
#define OM_OPT_GEMM_GROUP_M 6     /* row tiles per group of the persistent GEMM's tile walk (default 8): the group's A panels stay in an
                                   * XCD's L2 while its column tiles are swept */
#define OM_OPT_SCAN_QGROUP 7      /* query tiles (256 queries each) an XCD keeps resident in its L2 during the index scan (default 8) */
#define OM_OPT_TRAIN_WGRAD_STREAM 8 /* bit 0 (default 1): the BERT backward's weight-gradient GEMMs run on a second stream beside the data-gradient
                                    * chain (neither fills the GPU alone at training batch sizes); bit 1 (round 5, A/B, off): the weight transposes the
                                    * backward needs are launched by the training FORWARD on that stream -- measured 3 % SLOWER (the memory-bound transposes
                                    * take more from the forward's contractions than the 170 us they save: profiles/r05_train_ab_v2_*.jsonl);
                                    * bit 2 (A/B): the LayerNorm backward adds its d_gamma / d_beta sums with atomics, as before round 5 (default:
                                    * per-block partial sums + one reduce per layer group, a fixed order); bit 3 (A/B): that kernel without the
                                    * prefetch of the next row; bits 1-3 clear and bit 0 clear: everything on the caller's stream */
#define OM_OPT_ATTENTION_DEBUG 9  /* 0 (default); timing experiments on the bf16 attention kernel at L in (64, 128]: bit 0 no K / V fetch,
                                   * bit 1 no arithmetic, bit 2 no stores (results are garbage) */
#define OM_OPT_ENCODER_PINGPONG 10 /* 1 (default): the fused bf16 encoder's kernels alternate their walk direction over the token rows so
                                   * each starts on the rows its producer wrote last (memory-side cache hits); 0: always first to last */
#define OM_OPT_ENCODER_TWO_PLANE 11 /* bit mask (env OM_ENCODER_TWO_PLANE, default 3): the fused BERT encoder keeps its pre-LayerNorm residual stream in TWO
                                   * 16-bit planes (value = hi + lo; the reference's autocast keeps it in f32) for +2 bytes per element at the two
                                   * residual sites of a layer -- bit 0 bfloat16 (round 3: 1 - cos against the fp32 chain 1e-5 instead of 4.8e-5),
                                   * bit 1 float16 (round 6: the headline format inside the reference's own float16 autocast); bit 2 (opt-in, float16): the
                                   * second plane in EIGHT bits (e5m2 of the remainder * 2^10, a kernel-private layout) -- + 2.6 % passages/s at the same cosine / dot
                                   * ratios, one more swapped tie on the config-1 fixture's MRR@10; 0: one plane */
#define OM_OPT_GEMM_VARIANT 12     /* 0 (default): automatic tile-generation choice; 1 | 2 | 6 pin a generation (A/B measurements) */
#define OM_OPT_SEARCH_DEBUG 13     /* bit 0: om_sim_topk logs every round (rows done, chunk, list lengths) to stderr; bit 2 (A/B): the small-batch scan
                                    * fetches the index with the default cache policy instead of non-temporal loads (env OM_SEARCH_DEBUG) */
#define OM_OPT_TRAIN_WGRAD_BATCH 14 /* layers per deferred weight-gradient launch of the bf16 BERT backward (default 4; 0: one launch per
                                     * weight gradient as in round 2): the backward keeps every layer's dY and one om_gemm_tn_acc_batch
                                     * launch per group of layers computes their weight gradients (env OM_TRAIN_WGRAD_BATCH) */
#define OM_OPT_GEMM_MAX_GRID 15    /* 0 (default): the persistent 16-bit GEMM takes every CU; > 0: at most this many workgroups (one per CU) --
                                    * two half-batch encoder forwards on two streams share the chip with 128 each */
#define OM_OPT_GEMM_CONT 16        /* bit mask (env OM_GEMM_CONT, default 495 = bits 0-3, 5, 6, 7, 8) of the persistent 16-bit GEMM's continuous ring (the K loop of a tile
                                    * prefetches the next tile's first two steps; epilogue and accumulator initialisation of the next tile interleaved).
                                    * bit 0: the variants without a residual; bit 1: the one-plane residual variants; bit 2: (no effect any more: the index scan
                                    * of wide query batches is on the continuous ring wherever it fits, csrc/search_plan.h); bit 3: (no effect since round 5: the continuous GEMM kernels exist on 16 x 16 x 32 MFMAs only);
                                    * bit 4 (A/B, off): plain whole-tile bf16 shapes prefer the continuous kernels even when they leave CUs idle;
                                    * bit 5: the training forward's FFN1 (gelu + gelu' to the tape) on the continuous kernel with a two-output
                                    * epilogue; bit 6: generation 2 priced at its measured 0.55 of a 256 x 256 tile's rate when choosing between it and the
                                    * continuous kernel for plain whole-tile 16-bit shapes; bit 7 (round 5): plain float16 contractions follow the tile-choice model as
                                    * bfloat16 does (cleared: every whole-tile float16 shape on the persistent kernel); bits 8 / 9 (round 6): the float16 / bfloat16 TWO-plane residual variants on the continuous
                                    * ring (cleared -- bit 9 by default -- : the restart-per-tile kernel of round 3); a cleared bit 0 / 1: the ring restarts per tile as in round 3;
                                    * bit 10: (no effect any more: it put the wide index scan on 16 x 16 x 32 MFMAs, measured a wash -- profiles/r06_scan_16x16x32_ab.txt) */
#define OM_OPT_TRAIN_TAPE_GRAD 17  /* 1 (default): the bf16 BERT training forward keeps gelu'(f) on its tape instead of f (env OM_TRAIN_TAPE_GRAD) */
#define OM_OPT_TRAIN_RES32 18      /* 1 (default): the bf16 BERT training FORWARD keeps its residual stream in f32, as the reference's autocast does (layer_norm
                                    * runs and returns fp32): pre-LayerNorm sums in f32 on the tape, every LayerNorm output also unrounded for the next
                                    * residual add; 0: 16-bit residual stream as in rounds 1-4 (env OM_TRAIN_RES32; ~3 % faster, 2.4 x further from the
                                    * reference's fp32 gradients on tests/golden/train_base.npz) */
#define OM_OPT_GEMM_SKINNY_M 19    /* 16-bit contractions of at most this many rows run on the weight-streaming kernel (gemm_skinny.hip: one workgroup per
                                      16 output columns, K split over its waves) instead of the 128- / 256-column tiles, and the encoder forward takes its unfused path
                                      (normalisations as kernels) up to that many token rows; env OM_GEMM_SKINNY_M, default 1024, 0: off */
#define OM_OPT_GEMM_SKINNY_CFG 20  /* A/B: 0 (default) the kernel's own choice; MT * 10000 + NT * 100 + NW pins the tiles per wave and the K split (gemm_skinny.hip) */
#define OM_OPT_FEW_ROWS_LN_FUSE 21 /* round 6: 16-bit BERT forwards of at most this many token rows (default 64; env OM_FEW_ROWS_LN_FUSE; 0: off) launch no
                                      LayerNorm kernels between the embedding and the last layer: the contraction that consumes a LayerNorm's output
                                      normalises its operand rows itself, the one that adds it re-derives the element (gemm_skinny.hip; same bits) */
#define OM_OPT_ENCODER_SKIP_PAD 22  /* 1 (default; env OM_ENCODER_SKIP_PAD): om_encoder_forward skips a padded 16-bit batch's pad rows ON THE DEVICE where
                                      om_debug_encoder_skip_pad says so -- the rows up to each sequence's last unmasked token are packed back to back by
                                      a launch, and the persistent contractions read the token count from device memory (no copy to the host, no
                                      synchronisation); the representations keep their bits.  0 (A/B, tests): every contraction runs over all B * L rows */
#define OM_OPT_ENCODER_CLS_TAIL 23  /* 1 (default; env OM_ENCODER_CLS_TAIL): where om_debug_encoder_cls_tail says so, the fused BERT forward runs what follows
                                      its LAST layer's attention (out-proj, FFN1, FFN2, their row statistics) over the B [CLS] rows that pooling
                                      "first" reads -- gathered into roundup256(B) compact rows -- instead of every token row; the representations
                                      keep their bits.  0 (A/B, tests): the last layer runs over every row like the others */
#define OM_OPT_ENCODER_LANES 24  /* 65536 (default; env OM_ENCODER_LANES): the least PADDED token rows of a lane.  Where om_debug_encoder_lanes says so,
                                      om_encoder_forward runs a padded fused-BERT batch as two half-batches: sequences [0, B0) on the caller's stream,
                                      the rest on a stream the library owns (one per (device, caller stream), non-blocking, created on first use and
                                      kept for the life of the process), over two views of the one workspace, forked and joined with events so the
                                      caller's stream is ordered after both; the representations keep their bits.  Not while the stream is capturing,
                                      not under om_kernel_timing_enable(1), not without OmEncoderWeights::folded.  0 (A/B, tests): one chain */
#define OM_OPT_COUNT 25
int om_debug_option(int opt, int value);
/* the current value of a run-time switch (OM_OPT_*), so a test can restore exactly what it changed; -1 for an unknown option */
int om_debug_option_value(int opt);
/* the attention kernel alone (bf16 qkv [B*L, 3H] -> ctx [B*L, H]; mask [B, L] int64), for timing: csrc/kernels.h omk_attention */
int om_debug_attention(const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int H, int heads, void* stream);
/* Test hooks for the attention forward (tests/test_attention_kernels.py).  om_debug_attention_ex forwards every argument of the
 * internal launcher: qkv [rows, 3H] (q | k | v) and ctx [rows, H] of `dtype`, mask [B, L] int64, pos_bias [heads, L, L] f32 or NULL,
 * kmax [B] (om_debug_mask_extent) or NULL, cu [B + 2] (om_debug_pack_rows: packed rows, L stays the pitch of mask and pos_bias) or
 * NULL; w > 0 is the half window of banded attention (key k visible from q iff |q - k| <= w; no bias, dropout, cu or reverse there,
 * w >= L - 1 is full attention).  om_debug_attention is this with bf16, scale 0.125 and everything else off. */
int om_debug_attention_ex(int dtype, const void* qkv, void* ctx, const int64_t* mask, const float* pos_bias, int64_t B, int L, int H,
                          int heads, float scale, float drop_p, uint64_t seed, void* stream, int reverse, const int* kmax,
                          const int* cu, int w);
/* rotary positions in place on the Q and K columns of qkv [M, 3H], position = row % L (M need not be a multiple of L) */
int om_debug_rope(int dtype, void* qkv, int64_t M, int L, int H, float theta, void* stream);
/* the same pass over packed rows (OM_ARCH_NOMICBERT under om_encoder_forward_packed): the position of row t is row_map[t] % L, rows with
 * row_map[t] < 0 are left as they are (row_map [rows] as om_debug_pack_rows writes it) */
int om_debug_rope_rows(int dtype, void* qkv, int64_t rows, int L, int H, float theta, const int* row_map, void* stream);
/* SwiGLU of OM_ARCH_NOMICBERT: out[m, j] = silu(in[m, j]) * in[m, F + j] for M rows of in [M, 2F] (gate | up) into out [M, F], both of
 * `dtype`; f32 arithmetic, silu(g) = g / (1 + exp(-g)), rounded once.  F a multiple of 64. */
int om_debug_swiglu_rows(int dtype, const void* in, void* out, int64_t M, int F, void* stream);
/* the embedding launch alone: LayerNorm(word[id] + type[tt] (+ pos[row % L])) into out [M, H] of `dtype`; type_ids, pos and type may be
 * NULL (pos == NULL with a type table: OM_ARCH_NOMICBERT) */
int om_debug_embed(int dtype, const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                   const float* g, const float* b, void* out, int64_t M, int L, int H, int vocab, int type_vocab, float eps, void* stream);
/* Test hooks of the decoder-only stack (csrc/attention_causal.hip).  qkv is the grouped projection [rows, (n_heads + 2 n_kv_heads) * 64]
 * (q heads | k heads | v heads), ctx [rows, n_heads * 64]; query head h reads K / V head h / (n_heads / n_kv_heads).
 * om_debug_attention_causal: key k visible from query q iff k <= q and mask[b][k] != 0; it computes the key extents (one more small
 * launch) into a grow-only device buffer it keeps per device, so its first call on a device allocates.  om_debug_rope_gqa: rotary positions in place on the
 * q and k heads, position = row % L; inv_freq is a HOST array of 32 frequencies, cos / sin are multiplied by `scaling`.
 * The _packed / _rows forms are the kernels of om_causal_encoder_forward_packed alone, over the layout om_debug_mask_extent +
 * om_debug_pack_rows describe: sequence b is rows cu[b] .. cu[b + 1] - 1 of qkv / ctx (L stays the pitch of mask; rows outside are
 * neither read nor written), and the position of row t is row_map[t] % L (rows with row_map[t] < 0 are left as they are). */
int om_debug_attention_causal(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads, int n_kv_heads,
                              float scale, void* stream);
int om_debug_rope_gqa(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, const float* inv_freq, float scaling, void* stream);
int om_debug_attention_causal_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L, int n_heads,
                                     int n_kv_heads, float scale, void* stream);
int om_debug_rope_gqa_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, const float* inv_freq, float scaling,
                           const int* row_map, void* stream);
/* The same hooks with a head width: head_dim 64 runs the kernels above, head_dim 128 the 128-wide ones
 * over qkv [rows, (n_heads + 2 n_kv_heads) * 128] and ctx [rows, n_heads * 128].  om_debug_qknorm_rope: the per-head RMSNorm of the q
 * and k heads (x * rsqrt(mean(x^2) + eps) * g; q_norm_g / k_norm_g device arrays [head_dim] f32, NULL: no norm on that side) and the
 * rotary positions in one pass, in place; inv_freq is a HOST array of head_dim / 2 frequencies.  _packed / _rows as above. */
int om_debug_attention_causal_hd(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads, int n_kv_heads,
                                 int head_dim, float scale, void* stream);
int om_debug_attention_causal_hd_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L,
                                        int n_heads, int n_kv_heads, int head_dim, float scale, void* stream);
int om_debug_qknorm_rope(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, int head_dim, const float* q_norm_g,
                         const float* k_norm_g, float eps, const float* inv_freq, float scaling, void* stream);
int om_debug_qknorm_rope_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, int head_dim, const float* q_norm_g,
                              const float* k_norm_g, float eps, const float* inv_freq, float scaling, const int* row_map, void* stream);
/* Test hooks of the Gemma3 stack.  om_debug_attention_gqa_d256 (kernels: csrc/attention_d256.hip): bidirectional grouped-query attention over heads
 * of 256 columns, qkv [rows, (n_heads + 2 n_kv_heads) * 256], ctx [rows, n_heads * 256]; key k visible from query q iff mask[b][k] != 0
 * and, for 0 < w < L - 1, |q - k| <= w (w <= 0 or w >= L - 1: full attention).  om_debug_qknorm_rope_d256: om_debug_qknorm_rope at
 * head_dim 256 in Gemma3's form -- g = 1 + weight from the caller, the normalised value not rounded before the weight multiply;
 * inv_freq a HOST array of 128 frequencies.  om_debug_rmsnorm_add: x[f32] += (h * rsqrt(mean(h^2) + eps)) * g over M rows of H columns,
 * h in `dtype` with pitch ldh, x f32 with pitch ldx.
 * The _packed / _rows forms are the kernels of om_gemma3_encoder_forward_packed alone, over the layout om_debug_mask_extent +
 * om_debug_pack_rows describe: sequence b is rows cu[b] .. cu[b + 1] - 1 of qkv / ctx (L stays the pitch of mask and decides band or
 * full as above, so the packed launch runs the kernel body the padded launch of the batch runs; rows outside are neither read nor
 * written), and the position of row t is row_map[t] % L (rows with row_map[t] < 0 are left as they are). */
int om_debug_attention_gqa_d256(int dtype, const void* qkv, void* ctx, const int64_t* mask, int64_t B, int L, int n_heads, int n_kv_heads,
                                float scale, int w, void* stream);
int om_debug_qknorm_rope_d256(int dtype, void* qkv, int64_t M, int L, int n_heads, int n_kv_heads, const float* q_norm_g, const float* k_norm_g,
                              float eps, const float* inv_freq, float scaling, void* stream);
int om_debug_attention_gqa_d256_packed(int dtype, const void* qkv, void* ctx, const int64_t* mask, const int* cu, int64_t B, int L, int n_heads,
                                       int n_kv_heads, float scale, int w, void* stream);
int om_debug_qknorm_rope_d256_rows(int dtype, void* qkv, int64_t rows, int L, int n_heads, int n_kv_heads, const float* q_norm_g,
                                   const float* k_norm_g, float eps, const float* inv_freq, float scaling, const int* row_map, void* stream);
int om_debug_rmsnorm_add(int dtype, const void* h, int64_t ldh, float* x, int64_t ldx, const float* g, int64_t M, int H, float eps, void* stream);
/* kmax[b] = 1 + the last unmasked key of mask row b (L when it has none) */
int om_debug_mask_extent(const int64_t* mask, int64_t B, int L, int* kmax, void* stream);
/* cu [B + 2], cls_rows [B], row_map [rows] of the packed layout (csrc/kernels.h omk_pack_rows) */
int om_debug_pack_rows(const int* kmax, int64_t B, int L, int64_t rows, int* cu, int* cls_rows, int* row_map, void* stream);
/* The kernel family of the calling thread's last attention forward launch, family | key tiles << 8 (key tiles: 32-key tiles a
 * workgroup holds at once: the template's KT, 4 for the kernels that walk 128-key chunks).  The one forward entry (csrc/kernels.h
 * omk_attention) stores 0 on entry and its plan's code before it launches, so a call that launches nothing reads 0.  One host store
 * per launch, nothing on the device. */
#define OM_ATTN_FAMILY_GENERIC 1      /* attention_kernel: f32, and bf16 with OM_OPT_ATTENTION_FAST = 0, up to 256 tokens   */
#define OM_ATTN_FAMILY_FWD16 2        /* attention_fwd16_kernel: 16-bit, up to 256 tokens                                     */
#define OM_ATTN_FAMILY_FWD16_KMAX4 3  /* its KT = 4 body without bias / dropout under kmax or cu: trailing key tiles skipped   */
#define OM_ATTN_FAMILY_FWD16C 4       /* attention_fwd16c_kernel: 16-bit, 128-key chunks, online softmax                      */
#define OM_ATTN_FAMILY_LONG 5         /* attention_long_kernel: the first online-softmax kernel (f32 beyond 256 tokens; bf16 there
                                         with OM_OPT_ATTENTION_FAST = 0; both 16-bit formats under bit 2)                       */
#define OM_ATTN_FAMILY_D32 6          /* attention_d32_fwd_kernel: 32-wide heads                                              */
#define OM_ATTN_FAMILY_BAND16 7       /* attention_band16_kernel                                                              */
#define OM_ATTN_FAMILY_BAND32 8       /* attention_band32_kernel                                                              */
int om_debug_attention_last(void);
/* host only (no GPU needed): what the forward entry would launch for these arguments at the current switches (csrc/attn_plan.h
 * attn_plan_fwd; has_*: whether the optional pointer is given; w: the half window) -- family | key tiles << 8, 0 when nothing would
 * launch (an empty batch), -1 for a refusal with its reason in om_last_error.  Leaves the last-launch words alone. */
int om_debug_attention_plan(int dtype, int64_t B, int L, int H, int heads, int has_bias, float drop_p, int has_kmax, int has_cu, int w);
/* Grouped-query attention (csrc/kernels.h omk_attention_gqa, the one entry behind the six om_debug_attention_causal* / _gqa_d256* hooks
 * above and the Llama / Qwen2, Qwen3 and Gemma3 forwards): the families of its planner (csrc/attn_plan.h attn_plan_gqa; DESIGN.md 4c
 * lists the rules) and, host only, what it would launch -- causal: the triangle (head_dim 64 or 128, w must be <= 0), else the
 * bidirectional form (head_dim 256, w the half window); packed: rows packed by sequence; has_ext: whether kmax (padded rows, optional)
 * or cu (packed rows, required) is given.  out = {family, body (1 float32, 0 16-bit), grid x, grid y, dynamic LDS bytes}.  Returns 0,
 * every word zero when nothing would launch (an empty batch); -1 for a refusal with its reason in om_last_error. */
#define OM_ATTN_GQA_FAMILY_CAUSAL64 1   /* attention_causal16 / 32_kernel and their _packed forms                              */
#define OM_ATTN_GQA_FAMILY_CAUSAL128 2  /* attention_causal16 / 32_d128_kernel                                                 */
#define OM_ATTN_GQA_FAMILY_FULL256 3    /* attention_d256_16 / 32_kernel<AttnFull>: every unmasked key                         */
#define OM_ATTN_GQA_FAMILY_BAND256 4    /* attention_d256_16 / 32_kernel<AttnBand>: 0 < w < L - 1 on the padded L              */
int om_debug_attention_gqa_plan(int dtype, int64_t B, int L, int n_heads, int n_kv_heads, int head_dim, int causal, int w, int packed,
                                int has_ext, int64_t out[5]);
/* The same pair for the attention backward of a training step (csrc/train_kernels.h omk_attention_bwd, attn_plan_bwd; packed: the
 * step runs over packed rows).  The last-launch word is the PROCESS's, not the thread's: torch's autograd engine runs a backward on
 * a thread of its own. */
#define OM_ATTN_BWD_FAMILY_BWD16 1    /* attention_bwd16_kernel: transposing LDS reads, 16-bit, up to 128 tokens                 */
#define OM_ATTN_BWD_FAMILY_GENERIC 2  /* attention_bwd_kernel: a whole score row in registers, up to 256 tokens (float32: 192)    */
#define OM_ATTN_BWD_FAMILY_LONG 3     /* attention_bwd_long_a / _b_kernel: two passes, one score tile at a time, 16-bit, up to 512 */
#define OM_ATTN_BWD_FAMILY_D32 4      /* attention_d32_bwd_kernel: 32-wide heads, up to 256 tokens                               */
int om_debug_attention_bwd_last(void);
int om_debug_attention_bwd_plan(int dtype, int64_t B, int L, int H, int heads, int has_bias, int has_drel, int has_cu, int packed);
/* Test hook for the attention backward (tests/test_attention_bwd_kernels.py): every argument of the one backward entry, forwarded as
 * given (the hook chooses no kernel; a refused call leaves the last-launch word 0).  qkv [rows, 3H] and dqkv [rows, 3H] (dq | dk | dv),
 * dctx [rows, H] and ctx [rows, H] (the forward's output) of `dtype`; mask [B, L] int64; pos_bias [heads, L, L] f32 or NULL; drel
 * [heads, 2L - 1] f32 or NULL: the gradient of the bias per relative position key - query + (L - 1), ACCUMULATED into what the buffer
 * holds; ctx and stats (om_debug_attention_bwd_stats_bytes(B, heads) bytes of scratch) are read and written by the LONG family only and
 * may be NULL for every other; cu [B + 2] (om_debug_pack_rows) or NULL, with packed != 0 for a step over packed rows: sequence b is rows
 * cu[b] .. cu[b + 1] - 1, L stays the pitch of mask, pos_bias and drel, and rows of dqkv from cu[B] on are not written.  The dK / dV rows
 * of a padded key are zero whenever its sequence has an unmasked key. */
int om_debug_attention_bwd_ex(int dtype, const void* qkv, const void* ctx, const void* dctx, void* dqkv, const int64_t* mask,
                              const float* pos_bias, float* drel, float* stats, int64_t B, int L, int H, int heads, float scale,
                              float drop_p, uint64_t seed, const int* cu, int packed, void* stream);
size_t om_debug_attention_bwd_stats_bytes(int64_t B, int heads);
/* host only (no GPU needed): which layer loop om_encoder_forward (packed_rows == 0) or om_encoder_forward_packed would run for this
 * call at the current switches (csrc/encoder_plan.h encoder_plan; DESIGN.md 4d lists the rules).  gated_ffn, has_rel_bias: what the
 * forward reads from the weights (layers_host[0].ffn1g_w, rel_bias); a type_emb table is assumed where type_vocab > 0.  Returns
 * path | few_rows << 8 | two << 9 | lo8 << 10 (few_rows: the contractions run on the few-rows kernel; two / lo8: the fused BERT path's
 * second residual plane, and that plane in eight bits), 0 for an empty batch, -1 for a refusal with its reason in om_last_error. */
/* (OM_ARCH_NOMICBERT runs the four BERT loops under their codes) */
#define OM_ENC_PATH_BERT_FUSED 1       /* LayerNorm fused across the contractions (16-bit, >= 512 rows, widths of 256)          */
#define OM_ENC_PATH_BERT_PENDING_LN 2  /* few rows (<= OM_OPT_FEW_ROWS_LN_FUSE), f32 residual stream, LayerNorms inside the contractions */
#define OM_ENC_PATH_BERT_FEW32 3       /* few rows (<= OM_OPT_GEMM_SKINNY_M), f32 residual stream, LayerNorms as kernels          */
#define OM_ENC_PATH_BERT_PLAIN 4       /* one normalisation kernel per site: float32, and every other 16-bit shape                 */
#define OM_ENC_PATH_MODERNBERT 5
#define OM_ENC_PATH_T5_FUSED 6         /* RMSNorm fused across the contractions                                                    */
#define OM_ENC_PATH_T5_PLAIN 7         /* one normalisation kernel per site (float32, few rows, gated feed-forwards)               */
struct OmEncoderConfig;
int om_debug_encoder_plan(const struct OmEncoderConfig* cfg, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                          int want_hidden);
/* host only (no GPU needed): what om_encoder_train_forward[_packed|_hidden] (backward == 0) or om_encoder_train_backward[_packed|_hidden]
 * would run for this call at the current switches (csrc/train_plan.h train_plan; DESIGN.md 4g lists the rules).  want_hidden: the
 * _hidden entries; has_rel_bias: OmEncoderWeights::rel_bias is given; tape_flags: -1, or for a backward what its forward wrote on the
 * tape (1: f32 pre-LayerNorm sums, 2: gelu'(f) in place of f).  Returns
 *   tail (0 hidden states, 1 plain, 2 f32 from the [CLS] rows, 3 f32 mean) | t5 << 2 | gated << 3 | rel << 4 | packed << 5 | bert16 << 6 |
 *   res32 << 7 | pre_grad << 8 | keep << 9 | early_wt << 10 | lane << 11 | ln_atomics << 12 | wbatch << 16
 * (keep: the workspace holds keep slices; early_wt: the forward transposes the weights on the side stream / the backward may reuse them;
 * lane, ln_atomics, wbatch: the BERT backward's side stream, LayerNorm sums by atomics, layers per deferred weight-gradient launch),
 * 0 for an empty batch, -1 for a refusal with its reason in om_last_error. */
int om_debug_train_plan(const struct OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows, int want_hidden, int has_rel_bias,
                        int backward, int tape_flags);
/* host only: 1 if om_encoder_forward (packed_rows == 0) would skip this call's pad rows on the device at the current switches
 * (csrc/encoder_plan.h encoder_skip_pad): OM_OPT_ENCODER_SKIP_PAD is set, no hidden states are wanted, a pooling is set,
 * the call plans OM_ENC_PATH_BERT_FUSED or OM_ENC_PATH_T5_FUSED, and om_encoder_packed_supported takes the bound roundup256(B * L).
 * 0 otherwise (a call the forward refuses included), -1 for a NULL cfg.  The plan word above does not change with it. */
int om_debug_encoder_skip_pad(const struct OmEncoderConfig* cfg, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int want_hidden);
/* host only: 1 if om_encoder_forward (packed_rows == 0) or om_encoder_forward_packed would run its last layer's per-row tail over the
 * [CLS] rows alone at the current switches (csrc/encoder_plan.h encoder_cls_tail): OM_OPT_ENCODER_CLS_TAIL is set, the
 * call plans OM_ENC_PATH_BERT_FUSED without the eight-bit plane, pooling is OM_POOL_FIRST, no hidden states are wanted, n_layers >= 2,
 * B >= 512 and 4 * roundup256(B) is at most the call's token rows in whole tiles.  0 otherwise (a call the forward refuses included),
 * -1 for a NULL cfg.  The plan word and the workspace size do not change with it. */
int om_debug_encoder_cls_tail(const struct OmEncoderConfig* cfg, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                              int want_hidden);
/* host only: 1 if om_encoder_forward would run this padded call as two lanes at the current switches (csrc/encoder_plan.h
 * encoder_lanes), with lane 0's sequence count in *B0 (B0 may be NULL): OM_OPT_ENCODER_LANES is not 0, packed_rows is 0,
 * a pooling is set, no hidden states are wanted, the call plans OM_ENC_PATH_BERT_FUSED without a relative-position bias, B0 -- the
 * largest count <= B / 2 with B0 * L a multiple of 256 -- and B - B0 both have at least that many token rows and fewer than 131 072 (measured slower from there on), and each lane planned
 * as a call of its own gets the whole's path, planes and walk and the whole's om_debug_encoder_skip_pad / om_debug_encoder_cls_tail
 * answers.  0 otherwise, -1 for a NULL cfg.  The forward itself declines as well while its stream is capturing, in timing mode, without
 * OmEncoderWeights::folded, or where a contraction would plan another GEMM family at a lane's height.  The plan word and the workspace
 * size do not change with it. */
int om_debug_encoder_lanes(const struct OmEncoderConfig* cfg, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int64_t packed_rows,
                           int want_hidden, int64_t* B0);
/* host only: the byte ranges of lane `lane` (0 | 1) inside the workspace of the call (B, L), as (offset, bytes) pairs in out[0 .. 2 n):
 * x, y, x1, qkv, ctx, ff, ff2, pooled, headout, kmax, final32, stats, slots, y_lo, x1_lo (n = 15; a field the configuration does not
 * use has 0 bytes).  Returns n, or -1 where om_debug_encoder_lanes is not 1 or cap < 2 n. */
#define OM_ENCODER_LANE_RANGES 15
int om_debug_encoder_lane_ranges(const struct OmEncoderConfig* cfg, int gated_ffn, int has_rel_bias, int64_t B, int64_t L, int lane,
                                 int64_t* out, int cap);
/* how many forwards have forked into two lanes since the library was loaded */
int64_t om_debug_encoder_lane_forks(void);
/* Test hook of the row gather behind it (csrc/kernels.h omk_gather_rows): output row r < Mc of every given destination copies source row
 * idx(min(r, B - 1)), idx(b) = rows ? rows[b] : b * L.  Up to three 16-bit planes of H columns (src_i / dst_i, NULL pairs are skipped; H
 * a multiple of 8, 16-byte aligned buffers) and one [., 2] f32 array (stats_src / stats_dst, or NULL). */
int om_debug_gather_rows(const void* src0, void* dst0, const void* src1, void* dst1, const void* src2, void* dst2, const float* stats_src,
                         float* stats_dst, const int* rows, int64_t B, int64_t L, int64_t Mc, int H, void* stream);
/* host only: 1 if attention-probability dropout keeps (b, h, q, key) at rate p under `seed`; Lm is the mask's row pitch */
int om_debug_attn_drop_keep(uint64_t seed, int64_t b, int h, int heads, int Lm, int q, int key, float p);
/* self-check of the LayerNorm row reduction (csrc/ln_row.h): every group of 64 consecutive floats of `in` summed by the __shfl_xor butterfly
 * (out_shuffle[g]) and by its DPP / permlane form (out_dpp[g]); the two must agree bit for bit (tests/test_gpu_parity.py) */
int om_debug_wave_sum_check(const float* in, float* out_shuffle, float* out_dpp, int64_t groups, void* stream);
/* Test hooks for the row kernels (tests/test_row_kernels.py): normalisation forward and backward, pooling, L2 normalisation, dropout,
 * the bias-gradient column sum, the LayerNorm fold and the two deterministic reductions.  Each checks its own pointers for NULL and
 * its dtype (OM_F32 | OM_BF16 | OM_F16; om_debug_ln_fold and om_debug_layernorm_dual: the two 16-bit ones), then forwards EVERY
 * argument to the internal launcher of the same name (csrc/kernels.h, csrc/train_kernels.h) and adds nothing of its own.
 * Optional pointers (NULL allowed): b, x_lo, rows, add, dx_drop, db, dy32 / x32 (then dy / x may be NULL), partial (then dg may be
 * NULL), partial_blocks, drop_rows, type_ids, type with dtype_, cu, beta, the fold's b.
 * om_debug_row_kernel_last(): which kernel the calling thread's last normalisation launch ran -- one host store per launch, 0 after
 * a hook call that launched nothing (a refusal, an empty problem):
 *   forward : OM_ROW_FWD_GENERIC | OM_ROW_FWD_X8, NV (x8: 1..4) or MAX_VEC (generic: 4 | 8) << 4, input dtype << 8,
 *             output dtype << 12, second plane read << 16, and that plane in eight bits << 17
 *   backward: OM_ROW_LN_BWD, NV (3 | 4 | 8) << 4, MODE << 8, waves per block << 12, prefetch << 16, per-block partial sums << 17 */
#define OM_ROW_FWD_GENERIC 1
#define OM_ROW_FWD_X8 2
#define OM_ROW_LN_BWD 3
int om_debug_row_kernel_last(void);
/* Host only (csrc/row_plan.h): the word a normalisation call WOULD note, without a launch or a device -- 0 when there is
 * nothing to do (M <= 0), -1 with the launcher's own refusal in om_last_error; both set the thread's note word to 0.
 * om_debug_row_fwd_plan: entry 0 om_debug_layernorm, 1 _f32out, 2 _from_f32, 3 _dual; data_aligned: x, y and x_lo (where given) are
 * 16-byte aligned; param_aligned: g and b (where given) are; plane: x_lo is given.
 * om_debug_row_bwd_plan: mode 0 om_debug_norm_bwd / om_debug_ln_bwd_drop (L is not read), 1 om_debug_embed_bwd, at the current
 * OM_OPT_TRAIN_WGRAD_STREAM; out = {grid, threads per block, dynamic LDS bytes, the value *partial_blocks receives}. */
int om_debug_row_fwd_plan(int entry, int dtype, int64_t M, int H, int64_t ldx, int64_t ldy, int data_aligned, int param_aligned, int plane,
                          int lo8);
int om_debug_row_bwd_plan(int dtype, int mode, int64_t M, int H, int L, int has_x32, int has_dy32, int has_partial, int64_t out[4]);
int om_debug_layernorm(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, const float* g, const float* b, int64_t M, int H,
                       float eps, int rms, const void* x_lo, int lo8, void* stream);
int om_debug_layernorm_f32out(int dtype, const void* x, int64_t ldx, float* y, int64_t ldy, const float* g, const float* b, int64_t M,
                              int H, float eps, int rms, const void* x_lo, const int* rows, int lo8, void* stream);
int om_debug_layernorm_from_f32(int dtype, const float* x, int64_t ldx, void* y, int64_t ldy, const float* g, const float* b, int64_t M,
                                int H, float eps, int rms, void* stream);
int om_debug_layernorm_dual(int dtype, const float* x, int64_t ldx, void* y, float* y32, int64_t ldy, const float* g, const float* b,
                            int64_t M, int H, float eps, void* stream);
int om_debug_norm_bwd(int dtype, const void* dy, const void* x, const float* g, void* dx, float* dg, float* db, int64_t M, int H,
                      float eps, int rms, const void* add, void* stream);
int om_debug_ln_bwd_drop(int dtype, const void* dy, const void* x, const float* g, void* dx, void* dx_drop, float drop_p,
                         uint64_t drop_seed, float* dg, float* db, int64_t M, int H, float eps, const float* dy32, const float* x32,
                         float* partial, int* partial_blocks /* host */, const int* drop_rows, void* stream);
/* one LayerNorm site of om_debug_ln_param_reduce: dg[c] += sum over b < blocks of partial[b][0][c], db (may be NULL) likewise [1] */
typedef struct OmLnSite { const float* partial; float* dg; float* db; int blocks; } OmLnSite;
int om_debug_ln_param_reduce(const OmLnSite* sites /* host */, int n, int H, void* stream);
int om_debug_embed_bwd(int dtype, const void* dy, const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos,
                       const float* type, const float* g, float* dword, float* dpos, float* dtype_, float* dg, float* db, int64_t M,
                       int L, int H, int vocab, int type_vocab, float eps, const int* cu, void* stream);
int om_debug_pool(int dtype, const void* x, const int64_t* mask, float* out, int64_t B, int L, int H, int mode, const int* cu,
                  void* stream);
int om_debug_pool_bwd(int dtype, const float* dp, const int64_t* mask, void* dh, int64_t B, int L, int H, int mode, const int* cu,
                      void* stream);
int om_debug_l2norm(const float* x, float* y, int64_t M, int D, void* stream);
int om_debug_l2norm_bwd(const float* x, const float* dy, float* dx, int64_t M, int D, void* stream);
int om_debug_colsum(int dtype, const void* x, int64_t ld, int64_t M, int N, float* out, void* stream);
int om_debug_dropout(int dtype, const void* x, void* y, int64_t n, float p, uint64_t seed, const int* rows, int H, void* stream);
int om_debug_ln_fold(int dtype, const void* W, const float* gamma, const float* beta, const float* b, void* Wf, float* colsum,
                     float* bf, int N, int K, void* stream);
int om_debug_ln_stats_reduce(const float* slots, int nslots, int64_t M, float* out, void* stream);
/* Test hooks of the remaining training kernels (tests/test_train_leftover_kernels.py), in the same manner: pointers and dtype checked,
 * every argument forwarded.  om_debug_transpose: out[c][r] = op(in[r][c]) for r < R, zero for R <= r < Rp (op 0 copy, 1 erf-GELU);
 * om_debug_transpose_batch: n dense transposes, 40 to a launch; om_debug_zero_rows_from: rows [*first, M) of a row-major tensor <- 0,
 * `first` in device memory; the T5 feed-forward activation (kind 0 relu, 1 gelu_new(f) * f2) and its backward; the T5 embedding
 * backward (ids clamped to [0, vocab - 1]; row_map NULL or a token per row of dy, < 0: the row is skipped); the relative-position bias
 * gather out[h][q][k] = table[lut[k - q + L - 1]][h] and its backward dtable[lut[r]][h] += drel[h][r]. */
int om_debug_transpose(int dtype, const void* in, int64_t ldi, int64_t R, int C, void* out, int64_t ldo, int64_t Rp, int op, void* stream);
int om_debug_transpose_batch(int dtype, const void* const* in, void* const* out, const int* R, const int* C, int n, void* stream);
int om_debug_zero_rows_from(void* p, int64_t row_bytes, const int* first, int64_t M, void* stream);
int om_debug_t5_act_fwd(int dtype, const void* f, const void* f2, void* g, int64_t n, int kind, void* stream);
int om_debug_t5_act_bwd(int dtype, const void* dg, const void* f, const void* f2, void* df, void* df2, int64_t n, int kind, void* stream);
int om_debug_t5_embed_bwd(int dtype, const void* dy, const int64_t* ids, float* dword, int64_t M, int H, int vocab, const int* row_map,
                          void* stream);
int om_debug_t5_bias(const float* table, const int* lut, float* out, int L, int heads, void* stream);
int om_debug_t5_bias_bwd(const float* drel, const int* lut, float* dtable, int L, int heads, void* stream);
/* Test hooks of the T5 decoder position's own kernels (csrc/decoder.hip, tests/test_decoder_kernels.py), in the same manner: pointers,
 * dtype and ranges checked (L in [1, 1024], H == heads * 64, drop_p in [0, 1)), every argument forwarded to the launcher that
 * om_t5_decoder_step and the train pair call.  q, ctx, dctx, dq: [B, H]; kv, dkv: [B, L, 2H] (K | V); mask: [B, L] int64.
 * om_debug_dec_cross: single-query cross attention without the 1/sqrt(d) scale, dropout of the probabilities keyed on
 * (b heads + h) L + l; om_debug_dec_cross_bwd: its backward (every row l < L of dkv is written); om_debug_dec_final: RMSNorm to f32;
 * om_debug_dec_head_drop: v[b, h, :] scaled or zeroed by ONE draw per (b, h), in place; om_debug_dec_start: x[b, :] = emb[:];
 * om_debug_dec_cast: f32 -> dtype.  om_debug_dec_site (host only, launches nothing): the seed of dropout site `site` of `layer`. */
int om_debug_dec_cross(int dtype, const void* q, const void* kv, const int64_t* mask, void* ctx, int64_t B, int L, int H, int heads,
                       float drop_p, uint64_t seed, void* stream);
int om_debug_dec_cross_bwd(int dtype, const void* q, const void* kv, const int64_t* mask, const void* dctx, void* dq, void* dkv, int64_t B,
                           int L, int H, int heads, float drop_p, uint64_t seed, void* stream);
int om_debug_dec_final(int dtype, const void* x, const float* g, float* out, int64_t B, int H, float eps, void* stream);
int om_debug_dec_head_drop(int dtype, void* v, int64_t B, int H, float p, uint64_t seed, void* stream);
int om_debug_dec_start(int dtype, const float* emb, void* x, int64_t B, int H, void* stream);
int om_debug_dec_cast(int dtype, const float* x, void* y, int64_t n, void* stream);
uint64_t om_debug_dec_site(uint64_t seed, int layer, int site);
int om_kernel_timing_enable(int enable);
int om_kernel_timing_read(int kernel_class, double* total_ms, int64_t* launches, double* flops);

/* ------------------------------------------------------------------------
 * Dense contraction  C[M,N] = act(A[M,K] · B[N,K]^T + bias[N]) + resid[M,N]
 * (torch.nn.Linear layout: B is the [out,in] weight).  Replaces the ATen/BLAS
 * GEMMs under every nn.Linear of HF BertLayer / T5Block and linear.py:22-23.
 * in_dtype: OM_F32 (exact f32 MFMA, k-ordered fmaf chain), OM_BF16 or OM_F16 (16-bit MFMA, f32 accumulate;
 * OM_F16 with out_dtype OM_F16 or OM_F32, inference epilogues only).  bias (f32) and resid (out_dtype) may be NULL.
 * Requires K * sizeof(in) % 128 == 0.
 * ------------------------------------------------------------------------ */
int om_gemm_nt(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
               int out_dtype, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
               const float* bias, const void* resid, int64_t ldr, int act, void* stream);

/* ------------------------------------------------------------------------
 * Weight-gradient contraction  C[N,K] += A[M,N]^T · B[M,K],  bias[N] += column sums of A
 * (A = dY, B = X, both row-major bf16 as the backward pass holds them; C, bias f32,
 * ACCUMULATED into -- zero them first for a plain product).  Replaces autograd's
 * dW = dY^T X / db = sum(dY) of every nn.Linear under DRModel.forward + backward
 * (modeling/dense_retrieval_model.py:89-131).  Requires N % 128 == 0, K % 128 == 0,
 * lda / ldb multiples of 8 and below 2^25 elements, 16-byte aligned operands; bias may be NULL.
 * ------------------------------------------------------------------------ */
int om_gemm_tn_acc(int in_dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
                   float* C, int64_t ldc, float* bias, int64_t M, int64_t N, int64_t K, void* stream);

/* The same contraction for MANY (A, B, C, bias) quadruples over one token count M in ONE launch (round 3): what the
 * training backward uses for the weight gradients of a whole group of layers -- autograd's dW = dY^T X of every nn.Linear,
 * deferred to the end of the group (modeling/dense_retrieval_model.py:89-131 + loss.backward()).  256 x 256 output tiles
 * over the whole token axis, no split and no atomics: every C / bias element is read, added to and written by exactly one
 * workgroup, so C and bias must not be touched by anything else while the launch runs.  Requires N % 256 == 0,
 * K % 256 == 0, M >= 32 (tokens past the last multiple of 32 go through the om_gemm_tn_acc kernels on the same stream),
 * lda / ldb multiples of 8, 16-byte aligned operands; bias may be NULL. */
typedef struct OmTnProblem {
  const void* A; const void* B; float* C; float* bias;   /* dY [M,N], X [M,K] (bf16), dW [N,K], db [N] (f32, accumulated) */
  int64_t lda, ldb, ldc, N, K;
} OmTnProblem;
int om_gemm_tn_acc_batch(int in_dtype, const OmTnProblem* problems, int n, int64_t M, void* stream);
/* Test hooks (tests/test_gemm_tn_kernels.py).  om_debug_gemm_tn_last: what the calling thread's last om_gemm_tn_acc or
 * om_gemm_tn_acc_batch launched, eight words --
 *   [0] bit mask: 1 the LDS-DMA kernel, 2 the register-staged kernel, 4 the 256 x 256 kernel; 0: nothing was launched (a refusal too)
 *   om_gemm_tn_acc:        [1] rows of the DMA kernel  [2] its slices  [3] its 64-token steps per slice
 *                          [4] rows of the register-staged kernel  [5] its slices  [6] its rows per slice  [7] 0
 *   om_gemm_tn_acc_batch:  [1] whole 32-token steps  [2] 256 x 256 tiles over all problems  [3] tiles per XCD (chunk) of the last launch
 *                          [4] launches (48 problems each)  [5] tail rows  [6] slices and [7] rows per slice of the last problem's tail
 * om_debug_gemm_tn_plan: the same words for the call that WOULD be made at the current switches (OM_OPT_WGRAD_DEBUG) -- batch 0:
 * om_gemm_tn_acc; batch n > 0: om_gemm_tn_acc_batch over n problems of this shape.  Returns 0, all words zero for an empty problem, -1
 * for a refusal with its reason in om_last_error().  Host only: no GPU is touched and om_debug_gemm_tn_last keeps its value. */
int om_debug_gemm_tn_last(int64_t out[8]);
int om_debug_gemm_tn_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int batch, int64_t out[8]);

/* ------------------------------------------------------------------------
 * Encoder forward:  ids -> hidden [B,L,H] -> pooled/head/normalised reps [B,D]
 * Replaces  lm(**items) + pooling + head + F.normalize  in
 * modeling/dense_retrieval_model.py:133-155 (DRModel.encode), i.e. the whole
 * HF BertModel.forward (HF:models/bert/modeling_bert.py:623-684),
 * T5Stack.forward (HF:models/t5/modeling_t5.py), ModernBertModel.forward or
 * NomicBertModel.forward (OM_ARCH_*) in eval mode.
 * ------------------------------------------------------------------------ */
typedef struct OmLayerWeights {
  /* matrices: compute dtype (OM_F32 / OM_BF16 / OM_F16), [out,in] row-major */
  const void* qkv_w;   /* [3H,H]  rows: query | key | value                       */
  const float* qkv_b;  /* [3H] or NULL (T5)                                       */
  const void* o_w;     /* [H,H]                                                   */
  const float* o_b;    /* [H] or NULL                                             */
  const float* ln1_g;  /* BERT: attention.output.LayerNorm ; T5: layer[0].layer_norm ; ModernBERT: attn_norm (NULL in layer 0) ;
                          NomicBERT: post_attention_layernorm (ln2: post_mlp_layernorm) */
  const float* ln1_b;  /* NULL for T5 (RMSNorm)                                   */
  const void* ffn1_w;  /* [F,H]   BERT intermediate.dense / T5 wi (wi_0 if gated) ; NomicBERT: [2F,H] rows gate_proj | up_proj */
  const float* ffn1_b; /* [F] or NULL                                             */
  const void* ffn1g_w; /* [F,H]   T5 v1.1 wi_1 (linear gate) or NULL ; ModernBERT: Wi rows F..2F-1 (ffn1_w: rows 0..F-1) */
  const void* ffn2_w;  /* [H,F]                                                   */
  const float* ffn2_b; /* [H] or NULL                                             */
  const float* ln2_g;  /* BERT: output.LayerNorm ; T5: layer[1].layer_norm        */
  const float* ln2_b;
} OmLayerWeights;

typedef struct OmEncoderConfig {
  int arch;          /* OM_ARCH_*                                                 */
  int dtype;         /* compute dtype of matrices/activations: OM_F32 | OM_BF16 | OM_F16 (OM_F16: om_encoder_forward only,
                      * BERT-family erf-GELU encoders -- the reference's `--fp16` is torch.cuda.amp
                      * float16, retriever/dense_retriever.py:76; same kernels and MFMA rate as OM_BF16, 11-bit mantissas) */
  int hidden;        /* H                                                         */
  int n_layers;
  int n_heads;
  int head_dim;      /* 64; BERT family: 32 or 64 (n_heads * head_dim == hidden)   */
  int ffn;           /* F                                                         */
  int vocab;
  int max_pos;       /* BERT position table rows ; NomicBERT: max_position_embeddings (bounds L; no table) */
  int type_vocab;    /* BERT token-type table rows; 0 with type_emb == NULL: word + position only (DistilBERT, MPNet) */
  int act;           /* OM_ACT_*                                                  */
  float ln_eps;      /* 1e-12 BERT, 1e-6 T5                                       */
  int rel_buckets;   /* T5 / MPNet relative_attention_num_buckets (32); OM_ARCH_BERT: 0 = no relative bias */
  int rel_max_dist;  /* T5 relative_attention_max_distance (128); MPNet: 128, fixed in its modelling code */
  int pooling;       /* OM_POOL_*                                                 */
  int head_in;       /* LinearHead input dim  (0 = no head)                       */
  int head_out;      /* LinearHead output dim                                     */
  int normalize;     /* F.normalize(reps, dim=1)                                  */
  /* ---- ABI v6, OM_ARCH_MODERNBERT (OM_ARCH_NOMICBERT: rope_theta_global alone, the rest zero; zero for BERT / T5) ---- */
  float rope_theta_global; /* rope_parameters["full_attention"]["rope_theta"] (160 000) ; OM_ARCH_NOMICBERT: rope_parameters["rope_theta"] (1 000) */
  float rope_theta_local;  /* rope_parameters["sliding_attention"]["rope_theta"] (10 000)   */
  int half_window;         /* local_attention // 2: key k visible from query q iff |q - k| <= half_window (sliding layers) */
  uint64_t sliding_layers; /* bit l set: layer l is a sliding-window layer (config.layer_types[l] == "sliding_attention") */
} OmEncoderConfig;

typedef struct OmEncoderWeights {
  const float* word_emb;  /* [vocab,H] f32                                        */
  const float* pos_emb;   /* [max_pos,H] f32 (BERT); NULL: NomicBERT (rotary positions)       */
  const float* type_emb;  /* [type_vocab,H] f32 (BERT); NULL: no token types (DistilBERT, MPNet) */
  const float* emb_ln_g;  /* BERT embeddings.LayerNorm ; ModernBERT embeddings.norm */
  const float* emb_ln_b;
  const OmLayerWeights* layers_host; /* HOST array [n_layers] of device pointers  */
  const float* final_ln_g; /* T5 final_layer_norm.weight ; ModernBERT final_norm.weight */
  const float* rel_bias;   /* relative_attention_bias [buckets,heads] f32, one table for all layers: T5 block[0]; OM_ARCH_BERT: MPNet's
                              encoder.relative_attention_bias (bias[h][q][k] = table[bucket(k - q)][h], T5's bidirectional rule), else NULL */
  const float* head_w;     /* LinearHead weight [head_out,head_in] f32, or NULL   */
  const void* folded;      /* LayerNorm-folded weights made by om_encoder_fold_weights (ABI v4), or NULL: folded per forward */
  const float* final_ln_b; /* ModernBERT final_norm.bias, or NULL (norm_bias = False) (ABI v6)                          */
} OmEncoderWeights;

/* LayerNorm / RMSNorm folded into the weights that consume the normalised tensor (the 16-bit fused path): size of the
 * buffer (0 when the configuration has no fused path) and the one-off computation into a caller-owned, 256-byte aligned
 * device buffer.  Redo it whenever an encoder weight changes; om_encoder_forward reads it through OmEncoderWeights::folded. */
size_t om_encoder_fold_bytes(const OmEncoderConfig* cfg);
int om_encoder_fold_weights(const OmEncoderConfig* cfg, const OmEncoderWeights* w, void* folded, size_t bytes, void* stream);

size_t om_encoder_workspace_bytes(const OmEncoderConfig* cfg, int64_t B, int64_t L);

/* T5 relative-position bucket of `relative_position` = key_pos - query_pos, bidirectional
 * (HF:models/t5/modeling_t5.py T5Attention._relative_position_bucket).  Host function. */
int om_t5_relative_bucket(int relative_position, int num_buckets, int max_distance);

/* input_ids / attention_mask / token_type_ids: int64 [B,L] as the reference's
 * collators produce them (dataset/data_collator.py:27-38,78-83); token_type_ids
 * may be NULL (treated as 0; always ignored for T5).
 * out_hidden: [B,L,H] in cfg->dtype, or NULL.  out_reps: f32 [B,D]
 * (D = head_out if head else H), or NULL when pooling == OM_POOL_NONE.
 * Pad rows: a 16-bit call that returns representations only and plans a fused path (om_debug_encoder_skip_pad == 1) does not compute
 * the rows past each sequence's last unmasked token.  It packs the remaining rows on the device as om_encoder_forward_packed does,
 * with the bound roundup256(B * L), and its contractions read the token count from device memory: no copy to the host and no
 * synchronisation, the same bits, the workspace of om_encoder_workspace_bytes.  The packing arrays (4 * (roundup256(B * L) + 2 B + 2)
 * bytes) live in a buffer the library keeps per (device, stream); it is allocated by the first such call on a stream and grows only,
 * and a call that would have to allocate it while its stream is capturing runs over all B * L rows instead.  What follows from that:
 * the first call on a stream, and every call that grows the buffer, allocates and synchronises the device -- make it outside any
 * stream capture of the process (it would invalidate a capture another thread has open in global mode); a graph captured with the
 * skip keeps the buffer's address, shares the buffer with later eager calls on that stream, and must be replayed on the stream it
 * was captured on; buffers are kept per stream handle for the life of the process (about 0.5 MB for the 1024 x 128 batch).
 * OM_OPT_ENCODER_SKIP_PAD = 0 turns this off. */
int om_encoder_forward(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                       const int64_t* input_ids, const int64_t* attention_mask,
                       const int64_t* token_type_ids, int64_t B, int64_t L,
                       void* out_hidden, float* out_reps, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The same representations from PACKED rows: the reference pads every sequence of a batch to one length
 * (dataset/data_collator.py:27-38 `padding='max_length'`, or the longest of the batch) and HF runs every layer over the
 * padding; a padded key is masked out of every softmax, so the rows of a sequence up to its last unmasked token do not
 * depend on what follows them.  This entry keeps only those rows, back to back ([CLS] of sequence b at row cu[b]), runs
 * the embedding, all contractions and the normalisations over `packed_rows` rows instead of B * L, attention per
 * sequence over its own rows, and pools from them: the representations om_encoder_forward returns, for
 * sum(lengths) / (B * L) of the work.  16-bit configurations with the fused path (hidden, ffn multiples of 256;
 * BERT-family: erf-GELU, float16 or bfloat16; NomicBERT (a row's rotary position stays its token's column); T5 encoders: no gated feed-forward), L <= 1024 (round 6; was 256), pooling set (no out_hidden).
 * packed_rows: the caller's bound on the token count -- sum over sequences of (1 + index of the last unmasked token) --
 * rounded up to a multiple of 256, >= 512.  The bound is checked on the device: a batch that holds more tokens returns
 * NaN in every representation (no host synchronisation, never a truncated batch).
 * Workspace: om_encoder_workspace_bytes_packed(cfg, B, L, packed_rows). */
/* 1 when om_encoder_forward_packed takes (cfg, B, L, packed_rows) under the current run-time switches (OM_OPT_*), else 0:
 * the host layer asks before choosing the packed entry and falls back to om_encoder_forward.  gated_ffn: T5 v1.1 layers (ffn1g_w). */
int om_encoder_packed_supported(const OmEncoderConfig* cfg, int gated_ffn, int64_t B, int64_t L, int64_t packed_rows);
size_t om_encoder_workspace_bytes_packed(const OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
int om_encoder_forward_packed(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                              const int64_t* input_ids, const int64_t* attention_mask,
                              const int64_t* token_type_ids, int64_t B, int64_t L, int64_t packed_rows,
                              float* out_reps, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Decoder-only backbones as encoders (inference): HF LlamaModel / Qwen2Model.forward in eval mode without a KV cache
 * (HF:models/llama/modeling_llama.py, HF:models/qwen2/modeling_qwen2.py) + pooling + head + normalise, what
 * modeling/dense_retrieval_model.py:133-155 computes when AutoModel returns one of them.  A grouped-query backbone needs a K / V head
 * count that OmEncoderConfig has no field for, so these entries take a config struct of their own that EMBEDS the encoder's (its
 * layout and OM_ABI_VERSION are unchanged).  base: arch = OM_ARCH_CAUSAL, head_dim = 64 with n_heads * 64 == hidden (<= 2048), hidden
 * and ffn multiples of 64, act = OM_ACT_SILU, ln_eps = rms_norm_eps, pooling OM_POOL_NONE / FIRST / MEAN / LAST; the position, type,
 * relative-bias, rope-theta and window fields are ignored.
 * Weights: OmLayerWeights / OmEncoderWeights as they are --
 *   qkv_w  [(n_heads + 2 n_kv_heads) * 64, H] rows q_proj | k_proj | v_proj, qkv_b alongside or NULL (Qwen2: biases; Llama attention_bias)
 *   o_w    [H, H] o_proj, o_b or NULL;  ln1_g input_layernorm, ln2_g post_attention_layernorm (RMSNorm: no biases)
 *   ffn1_w [F, H] gate_proj, ffn1g_w [F, H] up_proj, ffn2_w [H, F] down_proj (no biases);  word_emb embed_tokens, final_ln_g norm.
 * Key k is visible from query q iff k <= q and attention_mask[b][k] != 0; positions are 0 .. L - 1 whatever the padding (HF's
 * arange).  L <= 1024.  out_hidden [B, L, H] in base.dtype or NULL; out_reps f32 [B, D].  No training entry.
 *
 * om_causal_encoder_forward_packed: the same representations from PACKED rows, under the contract of om_encoder_forward_packed --
 * each sequence's rows up to its last unmasked token, back to back; ids and mask keep their [B, L] layout; packed_rows is the caller's
 * bound on the token count, a multiple of 256 in [512, B * L + 255]; a batch that holds more tokens returns NaN in every
 * representation (checked on the device, nothing is read or written out of range).  The same launch sequence over packed_rows rows
 * instead of B * L, in f32, f16 and bf16; a position is the token's COLUMN (HF's arange), so rotary phases survive packing; a
 * sequence with leading pad tokens keeps them inside its extent, masked.  Representations only: a pooling, no out_hidden.
 * om_causal_encoder_packed_supported: 1 when the packed entry takes (cfg, B, L, packed_rows), else 0 -- the host layer asks and falls
 * back to om_causal_encoder_forward (0 also where B * L is at or below OM_OPT_GEMM_SKINNY_M: the padded entry's contractions take the
 * few-rows kernels there).  Workspace: om_causal_encoder_workspace_bytes_packed.
 * ------------------------------------------------------------------------ */
typedef struct OmCausalConfig {
  OmEncoderConfig base;
  int n_kv_heads;               /* config.num_key_value_heads: divides n_heads (n_heads: MHA, 1: MQA)                          */
  float rope_attention_scaling; /* rotary_emb.attention_scaling: cos and sin are multiplied by it (1 for default / linear / llama3) */
  float inv_freq[32];           /* rotary_emb.inv_freq, read on the host: serves the rope types whose frequencies do not depend on L */
} OmCausalConfig;
size_t om_causal_encoder_workspace_bytes(const OmCausalConfig* cfg, int64_t B, int64_t L);
int om_causal_encoder_forward(const OmCausalConfig* cfg, const OmEncoderWeights* w, const int64_t* input_ids,
                              const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps,
                              void* workspace, size_t workspace_bytes, void* stream);
int om_causal_encoder_packed_supported(const OmCausalConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
size_t om_causal_encoder_workspace_bytes_packed(const OmCausalConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
int om_causal_encoder_forward_packed(const OmCausalConfig* cfg, const OmEncoderWeights* w, const int64_t* input_ids,
                                     const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows, float* out_reps,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Qwen3 embedders (HF Qwen3Model, HF:models/qwen3/modeling_qwen3.py; Qwen3-Embedding): the stack above with three things more --
 * heads of 128 columns, an attention width A = n_heads * head_dim that need not equal `hidden`, and an RMSNorm over each q and k head
 * before the rotation (q_norm, k_norm).  The entries are the five above with a config that EMBEDS OmCausalConfig (no layout above
 * changes, OM_ABI_VERSION stays) and one more argument, a HOST array of n_layers OmCausalQkNorm (may be NULL when qk_norm is 0).
 * Rules: base.base.head_dim is 64 or 128; A a multiple of 64; hidden and ffn multiples of 64, hidden <= 2048 (the row-norm, embedding
 * and pooling kernels hold a row in 8 vectors per lane); n_kv_heads divides n_heads; act = OM_ACT_SILU; L <= 1024; pooling NONE /
 * FIRST / MEAN / LAST.  The rotary frequencies are inv_freq[64] below when head_dim is 128 and base.inv_freq[32] when it is 64; the
 * norm's eps is base.base.ln_eps (rms_norm_eps).
 * Weights as above with the attention width in place of H where a head count sets it:
 *   qkv_w [(n_heads + 2 n_kv_heads) * head_dim, H], qkv_b alongside or NULL;  o_w [H, A].
 * Packed rows: the rule of om_causal_encoder_packed_supported (a multiple of 256 rows in [512, B * L + 255], a padded form above
 * OM_OPT_GEMM_SKINNY_M).
 * ------------------------------------------------------------------------ */
typedef struct OmCausalConfig2 {
  OmCausalConfig base;          /* at offset 0: arch, widths, n_kv_heads, rope_attention_scaling, the 32 frequencies of head_dim 64 */
  int qk_norm;                  /* 1: RMSNorm over each q and k head before the rotation, weights in OmCausalQkNorm                   */
  int reserved;                 /* 0                                                                                                    */
  float inv_freq[64];           /* rotary_emb.inv_freq when head_dim is 128                                                             */
} OmCausalConfig2;
typedef struct OmCausalQkNorm {
  const float* q_norm_g;        /* self_attn.q_norm.weight [head_dim] f32, device */
  const float* k_norm_g;        /* self_attn.k_norm.weight [head_dim] f32, device */
} OmCausalQkNorm;
size_t om_causal2_encoder_workspace_bytes(const OmCausalConfig2* cfg, int64_t B, int64_t L);
int om_causal2_encoder_forward(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                               const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden,
                               float* out_reps, void* workspace, size_t workspace_bytes, void* stream);
int om_causal2_encoder_packed_supported(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows);
size_t om_causal2_encoder_workspace_bytes_packed(const OmCausalConfig2* cfg, int64_t B, int64_t L, int64_t packed_rows);
int om_causal2_encoder_forward_packed(const OmCausalConfig2* cfg, const OmEncoderWeights* w, const OmCausalQkNorm* qk_norm_host,
                                      const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows,
                                      float* out_reps, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * EmbeddingGemma (HF Gemma3TextModel with use_bidirectional_attention, HF:models/gemma3/modeling_gemma3.py; inference): the f32-residual
 * pre-norm loop above with heads of 256 columns, grouped K / V, an RMSNorm over each q and k head before the rotation, rotary
 * frequencies per layer TYPE, bidirectional attention -- full layers see every unmasked key, sliding layers key k from query q iff
 * |q - k| <= half_window -- a tanh-GELU gated feed-forward, and FOUR RMSNorms per layer, two of which act on a sublayer's OUTPUT before
 * the residual add.  An entry and a config struct of its own that EMBEDS OmCausalConfig (no layout above changes, OM_ABI_VERSION stays).
 * Rules: base.base.arch = OM_ARCH_GEMMA3; head_dim 256 only (the attention width n_heads * 256 need not equal hidden); hidden and ffn
 * multiples of 64, hidden <= 2048; n_kv_heads divides n_heads; act = OM_ACT_GELU_TANH ("gelu_pytorch_tanh"); no projection has a bias
 * (attention_bias False); attn_logit_softcapping 0 (None); bidirectional 1 (a causal Gemma3 is refused); at most 64 layers; L <= 1024;
 * pooling NONE / FIRST / MEAN; ln_eps = rms_norm_eps.  base.rope_attention_scaling and base.inv_freq are ignored.
 * Weights: OmLayerWeights / OmEncoderWeights as they are, every norm weight handed over as g = 1 + weight in f32 (Gemma3RMSNorm
 * multiplies by 1 + weight) --
 *   word_emb = embed_tokens.weight * float32(sqrt(hidden)) (the f32 multiply HF applies to the looked-up row), final_ln_g = 1 + norm.weight
 *   qkv_w [(n_heads + 2 n_kv_heads) * 256, H] rows q_proj | k_proj | v_proj;  o_w [H, n_heads * 256]
 *   ln1_g = 1 + input_layernorm.weight, ln2_g = 1 + pre_feedforward_layernorm.weight
 *   ffn1_w [F, H] gate_proj, ffn1g_w [F, H] up_proj, ffn2_w [H, F] down_proj
 * and a HOST array of n_layers OmGemma3Norms (device pointers, f32, each 1 + weight).
 *
 * om_gemma3_encoder_forward_packed: the same representations from PACKED rows, under the contract of om_causal_encoder_forward_packed --
 * each sequence's rows up to its last unmasked token, back to back; ids and mask keep their [B, L] layout; packed_rows is the caller's
 * bound on the token count, a multiple of 256, at most B * L + 255; a batch that holds more tokens returns NaN in every representation
 * (checked on the device, nothing is read or written out of range).  The same launch sequence (one layer loop serves both entries)
 * over packed_rows rows instead of B * L, in f32, f16 and bf16; a position is the token's COLUMN, so rotary phases survive packing; a
 * sequence with leading pad tokens keeps them inside its extent, masked; a sliding layer takes the band kernel exactly when the padded
 * entry would (decided on L, not on a sequence's extent).  Representations only: pooling FIRST or MEAN, no out_hidden.
 * om_gemma3_encoder_packed_supported: 1 when the packed entry takes (cfg, B, L, packed_rows), else 0 -- the host layer asks and falls
 * back to om_gemma3_encoder_forward.  1 iff the config passes the rules above, L <= 1024, packed_rows is a multiple of 256 and at most
 * B * L + 255, and BOTH B * L and packed_rows lie above OM_OPT_GEMM_SKINNY_M: all five contractions of a layer are format-in /
 * format-out, so a 16-bit call of at most that many rows plans the few-rows kernel where the padded call plans a wide tile.  Where
 * the planner picks the same kernel family for both row counts on every contraction the two entries agree bit for bit (DESIGN.md
 * section 8 lists the row counts where the families part).  Workspace: om_gemma3_encoder_workspace_bytes_packed (0 for a refused config).
 * Not built: the on-device pad skip of the padded 16-bit entries (it rests on a row count only the whole-tile generation-7 kernels
 * read; EmbeddingGemma's feed-forward width 1152 is no multiple of 256, so its contractions run on the generic tiles) and training.
 * ------------------------------------------------------------------------ */
#define OM_ARCH_GEMMA3 5 /* OmGemma3Config.base.base.arch, served by the om_gemma3_* entries alone */
typedef struct OmGemma3Config {
  OmCausalConfig base;           /* at offset 0: arch, widths, n_kv_heads                                                             */
  float attn_scale;              /* config.query_pre_attn_scalar ** -0.5: a field of its own, not head_dim ** -0.5                   */
  int half_window;               /* config.sliding_window - 1, read AFTER construction (the config has already halved the window)    */
  uint64_t sliding_layers;       /* bit l set: config.layer_types[l] == "sliding_attention"                                           */
  float full_scaling;            /* rotary_emb.full_attention_scaling                                                                   */
  float sliding_scaling;         /* rotary_emb.sliding_attention_scaling                                                                */
  float attn_logit_softcapping;  /* 0: None (anything else is refused)                                                                  */
  int bidirectional;             /* config.use_bidirectional_attention: 1 (0 is refused)                                                */
  float full_inv_freq[128];      /* rotary_emb.full_attention_inv_freq, read on the host                                                */
  float sliding_inv_freq[128];   /* rotary_emb.sliding_attention_inv_freq                                                               */
} OmGemma3Config;
typedef struct OmGemma3Norms {
  const float* q_norm_g;                /* 1 + self_attn.q_norm.weight [256] f32, device     */
  const float* k_norm_g;                /* 1 + self_attn.k_norm.weight [256]                 */
  const float* post_attention_norm_g;   /* 1 + post_attention_layernorm.weight [hidden]      */
  const float* post_feedforward_norm_g; /* 1 + post_feedforward_layernorm.weight [hidden]    */
} OmGemma3Norms;
size_t om_gemma3_encoder_workspace_bytes(const OmGemma3Config* cfg, int64_t B, int64_t L);
int om_gemma3_encoder_forward(const OmGemma3Config* cfg, const OmEncoderWeights* w, const OmGemma3Norms* norms_host, const int64_t* input_ids,
                              const int64_t* attention_mask, int64_t B, int64_t L, void* out_hidden, float* out_reps, void* workspace,
                              size_t workspace_bytes, void* stream);
int om_gemma3_encoder_packed_supported(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows);
size_t om_gemma3_encoder_workspace_bytes_packed(const OmGemma3Config* cfg, int64_t B, int64_t L, int64_t packed_rows);
int om_gemma3_encoder_forward_packed(const OmGemma3Config* cfg, const OmEncoderWeights* w, const OmGemma3Norms* norms_host,
                                     const int64_t* input_ids, const int64_t* attention_mask, int64_t B, int64_t L, int64_t packed_rows,
                                     float* out_reps, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * One decoder position of a T5 encoder-decoder over the encoder's output (inference):
 * what the reference computes for T5 backbones that are not --encoder_only --
 * DRModel.encode modeling/dense_retrieval_model.py:137-141 (decoder_input_ids = zeros([B,1]),
 * reps = decoder last_hidden_state[:, 0]) and the monoT5 scores of RRModel.encode
 * modeling/reranking_model.py:110-114 (two columns of the LM head over that state).
 * cfg: the ENCODER's config (hidden, heads, ffn, act, ln_eps, dtype); matrices in cfg->dtype,
 * [out,in] row-major, no biases (T5).  Self-attention over a single position needs only Wv, Wo.
 * enc_hidden: [B,L,H] in cfg->dtype = om_encoder_forward's out_hidden (after the final norm).
 * out_hidden: f32 [B,H], the decoder stack's output after its final RMSNorm. */
typedef struct OmT5DecoderLayer {
  const void* sa_v_w;    /* [H,H] layer[0].SelfAttention.v                                   */
  const void* sa_o_w;    /* [H,H] layer[0].SelfAttention.o                                   */
  const float* sa_ln_g;  /* layer[0].layer_norm                                              */
  const void* ca_q_w;    /* [H,H] layer[1].EncDecAttention.q                                 */
  const void* ca_kv_w;   /* [2H,H] rows: EncDecAttention.k | EncDecAttention.v               */
  const void* ca_o_w;    /* [H,H] layer[1].EncDecAttention.o                                 */
  const float* ca_ln_g;  /* layer[1].layer_norm                                              */
  const void* ffn1_w;    /* [F,H] wi (wi_0 if gated)                                         */
  const void* ffn1g_w;   /* [F,H] wi_1 or NULL                                               */
  const void* ffn2_w;    /* [H,F] wo                                                         */
  const float* ffn_ln_g; /* layer[2].layer_norm                                              */
} OmT5DecoderLayer;
typedef struct OmT5DecoderWeights {
  const float* start_emb;   /* [H] f32: shared.weight[decoder_start_token_id]                */
  const float* final_ln_g;  /* decoder.final_layer_norm.weight                               */
  const OmT5DecoderLayer* layers_host; /* HOST array [n_layers] of device pointers           */
  int n_layers;
} OmT5DecoderWeights;
size_t om_t5_decoder_workspace_bytes(const OmEncoderConfig* cfg, int64_t B, int64_t L);
int om_t5_decoder_step(const OmEncoderConfig* cfg, const OmT5DecoderWeights* w, const void* enc_hidden,
                       const int64_t* attention_mask, int64_t B, int64_t L, float* out_hidden,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Training through the decoder position (reference: autograd under DRModel.encode :137-141 / RRModel.encode :110-114 in
 * train mode).  `dropout` = HF config.dropout_rate (0 in eval), applied at HF's sites from hashes of (seed, site,
 * index); the forward keeps a caller-owned tape, the backward ADDS weight gradients into caller-zeroed f32 buffers laid
 * out like the weights and WRITES d_enc_hidden [B,L,H] (cfg->dtype), the gradient w.r.t. enc_hidden, which
 * om_encoder_train_backward_hidden takes.  start_emb [H]: gradient of the one embedding row the decoder reads (point it
 * at row decoder_start of the shared table's gradient; NULL skips it). */
typedef struct OmT5DecoderLayerGrads {
  float* sa_v_w;  float* sa_o_w; float* sa_ln_g;
  float* ca_q_w;  float* ca_kv_w; float* ca_o_w; float* ca_ln_g;
  float* ffn1_w;  float* ffn1g_w; float* ffn2_w; float* ffn_ln_g;
} OmT5DecoderLayerGrads;
typedef struct OmT5DecoderGrads {
  float* start_emb;
  float* final_ln_g;
  const OmT5DecoderLayerGrads* layers_host;   /* HOST array [n_layers] of device pointers */
} OmT5DecoderGrads;
size_t om_t5_decoder_tape_bytes(const OmEncoderConfig* cfg, int n_layers, int64_t B, int64_t L);
size_t om_t5_decoder_train_workspace_bytes(const OmEncoderConfig* cfg, int n_layers, int64_t B, int64_t L);
int om_t5_decoder_train_forward(const OmEncoderConfig* cfg, const OmT5DecoderWeights* w, const void* enc_hidden,
                                const int64_t* attention_mask, int64_t B, int64_t L, float dropout, uint64_t seed,
                                void* tape, size_t tape_bytes, float* out_hidden, void* workspace,
                                size_t workspace_bytes, void* stream);
int om_t5_decoder_train_backward(const OmEncoderConfig* cfg, const OmT5DecoderWeights* w, const void* enc_hidden,
                                 const int64_t* attention_mask, int64_t B, int64_t L, float dropout, uint64_t seed,
                                 const void* tape, const float* d_out, const OmT5DecoderGrads* grads,
                                 void* d_enc_hidden, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of y[B,D] = x[B,K] W[D,K]^T in f32 (om_gemm_nt forward): dw [D,K] = dy^T x (written), dx [B,K] = dy W.
 * Either output may be NULL.  The LinearHead / LM-head rows behind a trained T5 decoder position. */
int om_linear_f32_backward(const float* dy, const float* x, const float* w, float* dw, float* dx, int B, int D, int K,
                           void* stream);

/* ------------------------------------------------------------------------
 * Encoder forward + backward for training (BERT; sequence length <= 128).
 * Replaces the autograd graph HF builds under DRModel.forward in train mode
 * (modeling/dense_retrieval_model.py:89-131 -> HF BertModel with dropout) and
 * `loss.backward()` through it (trainer/dense_trainer.py:102-108).
 *
 * The forward saves one "tape" of activations (caller-provided memory); dropout masks are
 * regenerated from (seed, element index) in the backward, never stored.  Gradients are ADDED
 * (f32 atomics: split-K weight gradients, bias / LayerNorm / embedding reductions) into
 * caller-provided f32 buffers laid out like the weights; ZERO them before the call (or pass the
 * same buffers to several calls to accumulate).
 * ------------------------------------------------------------------------ */
typedef struct OmLayerGrads {
  float* qkv_w;  float* qkv_b;  float* o_w;    float* o_b;   float* ln1_g; float* ln1_b;
  float* ffn1_w; float* ffn1_b; float* ffn2_w; float* ffn2_b; float* ln2_g; float* ln2_b;
  float* ffn1g_w;                   /* T5 v1.1 gate projection wi_1 (ABI v2)          */
} OmLayerGrads;

typedef struct OmEncoderGrads {
  float* word_emb; float* pos_emb; float* type_emb; float* emb_ln_g; float* emb_ln_b;
  const OmLayerGrads* layers_host;  /* HOST array [n_layers] of device pointers */
  float* head_w;                    /* [head_out, head_in] or NULL              */
  float* final_ln_g;                /* T5: final RMSNorm weight [hidden] (ABI v2)     */
  float* rel_bias;                  /* T5, MPNet: relative_attention_bias [buckets, heads] (summed over layers) */
} OmEncoderGrads;

size_t om_encoder_tape_bytes(const OmEncoderConfig* cfg, int64_t B, int64_t L);
size_t om_encoder_train_workspace_bytes(const OmEncoderConfig* cfg, int64_t B, int64_t L);

/* hidden_dropout / attn_dropout: HF config hidden_dropout_prob / attention_probs_dropout_prob
 * (0 disables).  out_reps: f32 [B,D] as om_encoder_forward.  Sequence length: up to 512 tokens in the 16-bit formats (round 6: above 256 the
 * attention runs on kernels that keep one score tile in registers; the reference trains at whatever length its collator pads to,
 * dataset/data_collator.py:13-24), up to 192 in float32. */
int om_encoder_train_forward(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                             const int64_t* input_ids, const int64_t* attention_mask,
                             const int64_t* token_type_ids, int64_t B, int64_t L,
                             float hidden_dropout, float attn_dropout, uint64_t seed, void* tape,
                             size_t tape_bytes, float* out_reps, void* workspace,
                             size_t workspace_bytes, void* stream);

/* d_reps: f32 [B,D] gradient of the loss w.r.t. out_reps.  Same ids / mask / dropout / seed /
 * tape as the matching forward call. */
int om_encoder_train_backward(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                              const int64_t* input_ids, const int64_t* attention_mask,
                              const int64_t* token_type_ids, int64_t B, int64_t L,
                              float hidden_dropout, float attn_dropout, uint64_t seed,
                              const void* tape, const float* d_reps, const OmEncoderGrads* grads,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Packed rows in TRAINING (round 5; the training-side counterpart of om_encoder_forward_packed).  The reference's train collator pads
 * every query to q_max_len and every passage to p_max_len (dataset/data_collator.py:13-24) and the model computes over the padding;
 * here the contractions, normalisations, the tape and the weight gradients run over `packed_rows` rows -- each sequence's tokens up
 * to its last unmasked one, back to back.  ids / mask / token types keep their [B, L] layout; packed_rows is a multiple of 256 that
 * is >= the token count (computed on the host from the collator's lengths) and < B * L.  16-bit BERT-family and (round 6) T5 encoder
 * configurations with widths of 256, L <= 256, pooling first / mean: ask om_encoder_train_packed_supported.  Same representations and gradients as the
 * padded pair up to the order of the sums over rows; a bound below the token count turns out_reps into NaN. */
int om_encoder_train_packed_supported(const OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
size_t om_encoder_tape_bytes_packed(const OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
size_t om_encoder_train_workspace_bytes_packed(const OmEncoderConfig* cfg, int64_t B, int64_t L, int64_t packed_rows);
int om_encoder_train_forward_packed(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                                    const int64_t* input_ids, const int64_t* attention_mask,
                                    const int64_t* token_type_ids, int64_t B, int64_t L, int64_t packed_rows,
                                    float hidden_dropout, float attn_dropout, uint64_t seed,
                                    void* tape, size_t tape_bytes, float* out_reps,
                                    void* workspace, size_t workspace_bytes, void* stream);
int om_encoder_train_backward_packed(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                                     const int64_t* input_ids, const int64_t* attention_mask,
                                     const int64_t* token_type_ids, int64_t B, int64_t L, int64_t packed_rows,
                                     float hidden_dropout, float attn_dropout, uint64_t seed,
                                     const void* tape, const float* d_reps, const OmEncoderGrads* grads,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* The same pair with the stack's output / its gradient at the boundary instead of pooled representations: out_hidden
 * and d_hidden are [B,L,H] in cfg->dtype (T5: after the final RMSNorm and its dropout).  cfg->pooling / head / normalize
 * are ignored.  What the T5 decoder position (om_t5_decoder_train_*) sits on. */
int om_encoder_train_forward_hidden(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                                    const int64_t* input_ids, const int64_t* attention_mask,
                                    const int64_t* token_type_ids, int64_t B, int64_t L,
                                    float hidden_dropout, float attn_dropout, uint64_t seed, void* tape,
                                    size_t tape_bytes, void* out_hidden, void* workspace,
                                    size_t workspace_bytes, void* stream);
int om_encoder_train_backward_hidden(const OmEncoderConfig* cfg, const OmEncoderWeights* w,
                                     const int64_t* input_ids, const int64_t* attention_mask,
                                     const int64_t* token_type_ids, int64_t B, int64_t L,
                                     float hidden_dropout, float attn_dropout, uint64_t seed,
                                     const void* tape, const void* d_hidden, const OmEncoderGrads* grads,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* Gradient all-reduce overlapped with the backward (multi-GPU training): hand the NEXT om_encoder_train_backward on this
 * thread an array of n_layers + 1 hipEvent_t.  events[l] (l = n_layers-1 .. 0) is recorded on the backward's stream once
 * every kernel that writes layer l's gradients has been enqueued, events[n_layers] after the embedding gradients: a
 * side stream that waits for events[l] can all-reduce layer l's slice of the gradient arena while the rest of the
 * backward still runs.  NULL entries are skipped; the array is consumed by one backward. */
int om_encoder_train_set_layer_events(void* const* events, int n);

/* ------------------------------------------------------------------------
 * Optimizer step of the training loop: global-norm gradient clipping + AdamW + refresh of the packed compute-dtype
 * copies of the updated weights, for a whole model in three launches.  Replaces what the reference inherits from HF
 * Trainer.train per optimizer step (trainer/dense_trainer.py:27-108: torch.nn.utils.clip_grad_norm_(max_grad_norm),
 * torch.optim.AdamW.step) and the re-packing of the encoder's 16-bit weight matrices that would follow it here.
 *
 * tensors / chunks are DEVICE arrays the caller builds once per set of buffers: `tensors[t]` describes one parameter
 * (p, g, m, v: f32 [n]; g == NULL: the parameter received no gradient and is left alone; shadow0 / shadow1: up to two
 * copies of p in shadow*_dtype (OM_F32 | OM_BF16 | OM_F16) that are rewritten with the updated values -- the packed
 * weights OmLayerWeights points at -- or NULL); `chunks[2 c], chunks[2 c + 1]` = (tensor index, chunk index within it)
 * for every OM_ADAM_CHUNK elements of every tensor, one workgroup each.
 *   om_grad_sqnorm   out_sq[0] = sum over all tensors of |g|^2 (f32; fixed summation order); partial: n_chunks floats of scratch
 *   om_adamw_step    torch.optim.AdamW's update with bias corrections for `step` (counted from 1) on
 *                    g' = g * grad_scale * min(1, max_norm / (|g * grad_scale|_2 + 1e-6))   (max_norm <= 0: no clipping);
 *                    gnorm_sq = om_grad_sqnorm's out_sq (required when clipping).  skip_nonfinite != 0: an inf / nan norm
 *                    leaves every buffer untouched (the skipped step of a float16 GradScaler); om_loss_scale_update reads the same scalar.
 * ------------------------------------------------------------------------ */
#define OM_ADAM_CHUNK 16384
typedef struct OmAdamTensor {
  float* p; const float* g; float* m; float* v;
  void* shadow0; void* shadow1;
  int64_t n;
  float weight_decay;
  int shadow0_dtype, shadow1_dtype, reserved;
} OmAdamTensor;
int om_grad_sqnorm(const OmAdamTensor* tensors, const int32_t* chunks, int n_chunks, float* partial, float* out_sq, void* stream);
int om_adamw_step(const OmAdamTensor* tensors, const int32_t* chunks, int n_chunks, float lr, float beta1, float beta2, float eps,
                  int64_t step, const float* gnorm_sq, float max_norm, float grad_scale, int skip_nonfinite,
                  const float* scale_state /* NULL, or state4 of om_loss_scale_update: gradients are multiplied by state4[1] as well, and the
                                              bias corrections use step - state4[3] (GradScaler does not call step() on a skipped step) */,
                  void* stream);
/* Dynamic loss scale of float16 training (torch.cuda.amp.GradScaler.update; the reference's --fp16 through HF Trainer,
 * trainer/dense_trainer.py:141-149) on the device: state4 = {scale, 1 / scale, clean steps, skipped steps}; a non-finite
 * gnorm_sq[0] (om_grad_sqnorm of the SCALED gradients) halves the scale, `growth_interval` finite steps in a row double it. */
int om_loss_scale_update(const float* gnorm_sq, float* state4, int growth_interval, void* stream);

/* ------------------------------------------------------------------------
 * Exact inner-product search.  Replaces faiss.IndexFlatIP.add / .search
 * (retriever/dense_retriever.py:38-41,105,180) and faiss-GPU sharding (:43-58).
 * ------------------------------------------------------------------------ */

/* index.add(): make the 16-bit shadow copy of rows [0,N) and accumulate the rounding
 * statistics the certified candidate margin needs.  The shadow is IEEE f16, not bf16: same
 * MFMA rate, 8x smaller rounding error, which is what keeps the certified margin (and with it
 * the candidate lists) narrow on anisotropic embedding sets.  (OM_SEARCH_F16_ONLY keeps no float32 rows at all: om_index_add_f16.)
 * stats: device float[2] = {max_i ||p_i - f16(p_i)||_2 , max_i ||f16(p_i)||_2}, updated with
 * max (initialise to 0 before the first add; +inf if a value overflows f16 -> f32 scan). */
int om_index_to_f16(const float* rows_f32, int64_t N, int d, void* rows_f16, float* stats,
                    void* stream);

/* index.add() of a float16-only index (OM_SEARCH_F16_ONLY): rows [N, d] in in_dtype -- OM_F32: rounded to nearest even, the bits of
 * torch.Tensor.half(); OM_F16: copied bit for bit -- stored to rows_f16 [N, d].  No float32 copy is made or needed.
 * stats: device float[2] as above; stats[1] is max-updated with the 2-norm of the STORED float16 rows (the reduction om_index_to_f16 uses:
 * the same values leave the same word), stats[0] is never written and stays 0 -- the rows carry no rounding error against themselves, so
 * the certified margin keeps only the query-rounding term ||q - f16(q)|| * stats[1] and the accumulation slop.
 * nonfinite: device unsigned, not NULL; the number of stored values that are inf or NaN (a float32 input beyond +-65504 rounds to inf) is
 * ADDED to it: zero it before the call, read it after the stream has passed.  A non-finite row leaves stats[1] inf or NaN, which no
 * margin certifies.  One wave per row; 16-byte accesses when d % 8 == 0 and both planes are 16-byte aligned.  rows and rows_f16 must
 * not overlap. */
int om_index_add_f16(int in_dtype, const void* rows, int64_t N, int d, void* rows_f16, float* stats, unsigned* nonfinite, void* stream);

size_t om_sim_topk_workspace_bytes(int64_t n_queries, int d, int k);

/* D,I = index.search(x, k):  scores[Q,k] f32 sorted descending, ids[Q,k] int64 =
 * id_offset + row, padded with (-3.4028235e38, -1) when N < k (faiss semantics).
 * Ties are ordered by ascending row.  mode OM_SEARCH_F16_RESCORE needs
 * index_f16 + stats from om_index_to_f16; returned scores are always the
 * exact f32 inner products.  k <= 2048.
 * NOT stream-ordered for the host: om_sim_topk synchronises `stream` ONCE per call (it reads the
 * overflow flags back at the end of its fast schedule; more often on the rare careful path), so
 * it blocks its caller, cannot be captured in a graph and cannot overlap a second search of the
 * same thread.  om_sim_topk_async below is the entry that only enqueues.
 * mode OM_SEARCH_F16_ONLY: the exact top-k of <q, widen(index_f16)> with float32 queries -- bit for bit what OM_SEARCH_F16_RESCORE
 * returns over index_f32 = widen(index_f16) when it took no float32 retry.  index_f32 is not read and may be NULL; index_f16 and stats
 * (om_index_add_f16) are required.  There is no float32 plane to retry on: the entry enqueues om_sim_topk_async's chain -- certified
 * scan, re-score from the float16 rows, on-device redo of every query with an overflowed list, a too-wide or non-finite margin or a list
 * beyond the re-score's cover -- and synchronises once.  It needs the workspace of om_sim_topk_async_workspace_bytes, and like that
 * entry it refuses d > 16384 and OM_OPT_SCAN_GEN7 = 0.  A redone query costs seven passes over the index on the VALU per block of
 * queries -- far more than the float32 scan the two-copy mode falls back to; om_sim_topk_info [4] and [7] tell when it was paid. */
int om_sim_topk(int mode, const float* queries, int64_t n_queries, const float* index_f32,
                const void* index_f16, const float* stats, int64_t N, int d, int k,
                int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                size_t workspace_bytes, void* stream);

/* The same search, stream-ordered: arguments, argument checks, output layout, padding and tie rule of om_sim_topk, but the entry only
 * ENQUEUES work on `stream` -- no stream / device / event synchronisation, no blocking copy, no allocation, no host read of device
 * memory.  After one eager call has set the kernels' function attributes it is legal on a capturing stream.  What om_sim_topk decides
 * on the host from its flags is decided per query on the device: a query whose candidate list overflowed (masses of exact ties:
 * duplicated rows), whose certified f16 margin was too wide, or whose list outgrew the re-score is recomputed exactly by an on-device
 * radix select over all rows (csrc/search.hip, "on-device redo"); the other queries of the batch keep the bits om_sim_topk returns.
 * A redone query's scores are the f32 dot products of the f16 mode's re-score, in both modes.
 * status: device memory, 8 x int64, not NULL, written by the last kernel of the chain: [0] scan precision as om_sim_topk_info reports it
 * (1 f16+rescore, 0 f32; a too-wide margin does not change it here), [1] rounds, [2] queries redone on the device, [3] longest list,
 * [4] queries whose certified margin was too wide, [5] OM_SCAN_FAMILY_* of the last filtered round, [6] 1, written last (0 from the
 * start of the chain), [7] 0.  Refuses when OM_OPT_SCAN_GEN7 = 0 has switched the fast schedule off, and d > 16384.
 * workspace: om_sim_topk_async_workspace_bytes (>= om_sim_topk_workspace_bytes; 0 for n_queries <= 0), 256-byte aligned, owned by the
 * call until the stream has passed it: two searches in flight need two workspaces.  om_sim_topk_info is not touched.
 * mode OM_SEARCH_F16_ONLY: as described at om_sim_topk; the chain is this one with the re-score and the redo reading the float16 rows,
 * status[0] = 1, and the two refusals above name the mode. */
size_t om_sim_topk_async_workspace_bytes(int64_t n_queries, int d, int k);
int om_sim_topk_async(int mode, const float* queries, int64_t n_queries, const float* index_f32,
                      const void* index_f16, const float* stats, int64_t N, int d, int k,
                      int64_t id_offset, float* out_scores, int64_t* out_ids, int64_t* status,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The fast schedule both entries run (csrc/search_plan.h search_schedule: no launch, no HIP call): behind the dense bootstrap of the
 * first 4096 rows, *n filtered rounds; chunks[i], i < min(*n, cap), is the number of rows of round i, the first of which starts at row
 * 4096.  N <= 4096 has no rounds.  mode: OM_SEARCH_*; under the calling thread's switches (OM_OPT_SCAN_GROWTH). */
int om_debug_search_schedule(int mode, int64_t nq, int64_t N, int k, int64_t* chunks, int cap, int* n);

/* Filtered exact search: the top-k over the ALLOWED rows of the shard only -- per query exactly what om_sim_topk_async of the same mode
 * returns over an index that holds only the allowed rows in their original order: the same scores (the re-score's bits in the two
 * 16-bit modes), ties by ascending row, ids = id_offset + the ORIGINAL row, (-3.4028235e38, -1) padding when fewer than k rows are allowed.
 * allow_bits: device memory, (N + 31) / 32 uint32 words, bit r & 31 of word r >> 5 is row r; one bitmap for all queries of the call; bits
 * at and beyond N are ignored.  n_allowed: the number of set bits among [0, N), as the host knows it -- it sizes the schedule only; the
 * rank of the redo's select comes from a count taken on the device at the head of the chain, so a stale value costs speed, never
 * correctness.  The entry only ENQUEUES, as om_sim_topk_async does, and runs that entry's chain: the scan kernels do not know the
 * filter -- a disallowed row above the threshold enters a list like any row -- and a small kernel drops the disallowed keys of every
 * list in front of EVERY selection (the dense bootstrap's included), so thresholds, certified margins and the re-score only ever see
 * allowed rows.  The lists therefore fill as those of a search for k_eff = ceil(k N / n_allowed): the schedule below sizes its rounds
 * for that, and scores a longer head of the shard densely.  A query whose list overflows all the same is redone on the device, and the
 * redo skips disallowed rows.  A filter whose allowed rows are scarce at the head of [0, N) and dense later defeats the bootstrap (no
 * threshold exists before k allowed rows were seen): every query is then redone by seven VALU passes over the index; status[2] tells.
 * status: as om_sim_topk_async's, but may be NULL.  Refuses what om_sim_topk_async refuses (OM_OPT_SCAN_GEN7 = 0, d > 16384, k > 2048),
 * a null bitmap and n_allowed outside [0, N].  workspace: om_sim_topk_filtered_workspace_bytes, 256-byte aligned. */
size_t om_sim_topk_filtered_workspace_bytes(int64_t n_queries, int d, int k);
int om_sim_topk_filtered(int mode, const float* queries, int64_t n_queries, const float* index_f32,
                         const void* index_f16, const float* stats, int64_t N, int d, int k,
                         int64_t id_offset, const uint32_t* allow_bits, int64_t n_allowed, float* out_scores,
                         int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The filtered search with a bitmap PER QUERY: per query exactly what om_sim_topk_filtered returns for that query alone under its
 * bitmap -- the same scores (the re-score's bits in the two 16-bit modes), ties by ascending row, ids = id_offset + the ORIGINAL row,
 * (-3.4028235e38, -1) padding when fewer than k rows are allowed -- in ONE chain, so one pass over the index serves every filter.
 * allow_bits: device memory; bitmap f is the (N + 31) / 32 words at allow_bits + f * words_pitch (words_pitch >= (N + 31) / 32: a padded
 * pitch is legal, bits at and beyond N and the padding are ignored).  filter_of: device [n_queries] int32, query q is searched under
 * bitmap filter_of[q]; a value below 0 is "no filter" -- the query returns what om_sim_topk_async returns for it, so filtered and
 * unfiltered queries share a batch; a value >= n_filters is "nothing allowed" and is never used as an address.  filter_of == NULL: query q
 * is under bitmap q, and n_filters must equal n_queries.  n_allowed_min: the host's count of set bits among [0, N) of the SPARSEST bitmap
 * the call uses, N when every query is unfiltered.  It sizes the schedule only (om_debug_search_schedule_filtered with this count): the
 * lists of a query under a denser bitmap fill more slowly than planned, which costs nothing; the rank of the redo's select is
 * min(k, a count of the query's own bitmap taken on the device), so a stale value costs speed, never correctness.
 * The chain is om_sim_topk_filtered's: the drop in front of every selection, the count and the redo read the bitmap of their query.
 * Enqueues only; legal on a capturing stream after one eager call.  status: as om_sim_topk_async's, may be NULL.
 * Refuses what om_sim_topk_filtered refuses, n_filters outside [1, 65535], words_pitch below (N + 31) / 32, a NULL filter_of with
 * n_filters != n_queries, and n_allowed_min outside [0, N].  workspace: om_sim_topk_filtered_multi_workspace_bytes, 256-byte aligned. */
size_t om_sim_topk_filtered_multi_workspace_bytes(int64_t n_queries, int d, int k, int64_t n_filters);
int om_sim_topk_filtered_multi(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                               const float* stats, int64_t N, int d, int k, int64_t id_offset, const uint32_t* allow_bits,
                               int64_t words_pitch, int64_t n_filters, const int32_t* filter_of, int64_t n_allowed_min, float* out_scores,
                               int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The search with an EXCLUSION LIST per query (hard-negative mining: every row but the query's few known positives): per query exactly
 * what om_sim_topk_async of the same mode returns over an index without the excluded rows -- the same scores (the re-score's bits in the
 * two 16-bit modes), descending, ties by ascending row, ids = id_offset + the ORIGINAL row, (-3.4028235e38, -1) padding when fewer than k
 * rows remain.  excl: device memory, int32 [n_queries][pitch]; row q holds the rows query q must not return -- ASCENDING, WITHOUT REPEATS,
 * padded at the end with -1.  pitch is at most */
#define OM_EXCLUDE_MAX 4096
/* ids (16 KiB: the drop stages one list in LDS).  An id at or beyond N is legal and matches nothing.  A list that breaks the contract
 * (unsorted, repeats, a negative other than the padding) may drop the wrong rows or return a short result; it never makes the entry read
 * outside [excl, excl + n_queries * pitch) or outside the index: every probe of the binary search stays inside the list's own pitch
 * words, and no value of a list is used as an address.
 * The chain is om_sim_topk_filtered_multi's with the list in the bitmap's place: in front of EVERY selection a small kernel drops the
 * excluded keys of every list (one workgroup per query, one binary search per key), so thresholds, certified margins and the re-score
 * only ever see rows that may be returned; the redo skips the excluded (row, query) pairs and takes its rank, min(k, N - the list's
 * entries below N), from a count taken on the device.  The schedule is om_debug_search_exclude_schedule's.  Lists that exclude most of
 * the head of the index act like a clustered bitmap: no threshold exists behind the bootstrap and the queries are redone (status[2]).
 * Enqueues only; legal on a capturing stream after one eager call.  status: as om_sim_topk_async's, may be NULL.  pitch == 0 is the
 * unfiltered search, and excl is not read.  Refuses what om_sim_topk_filtered refuses, pitch outside [0, OM_EXCLUDE_MAX], and a NULL excl
 * with pitch > 0.  workspace: om_sim_topk_excluding_workspace_bytes, 256-byte aligned. */
size_t om_sim_topk_excluding_workspace_bytes(int64_t n_queries, int d, int k, int64_t pitch);
int om_sim_topk_excluding(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16,
                          const float* stats, int64_t N, int d, int k, int64_t id_offset, const int32_t* excl, int64_t pitch,
                          float* out_scores, int64_t* out_ids, int64_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The schedule of om_sim_topk_excluding (csrc/search_plan.h search_schedule_excluding: no launch, no HIP call):
 * om_debug_search_schedule_filtered's for n_allowed = N - pitch, the fewest rows any query of the call may be returned -- a planning
 * number only.  pitch == 0: om_debug_search_schedule's; N - pitch < 1: every row is scored densely. */
int om_debug_search_exclude_schedule(int mode, int64_t nq, int64_t N, int k, int64_t pitch, int64_t* chunks, int cap, int* n, int64_t* boot);
/* The exact top-k of every query over its OWN candidate rows (dense re-ranking of a first-stage run): cand [n_queries][cand_pitch] int32 on
 * the device, cand[q][j] a row number; any value outside [0, N) is a hole -- skipped, never dereferenced.  Rows must be DISTINCT within a
 * query: a repeated row is returned twice (openmatch_amd/index.py removes repeats before the call).  Scores are the re-score's dot product
 * over the rows the mode's re-score reads -- the float32 rows for OM_SEARCH_F32 and OM_SEARCH_F16_RESCORE (index_f16 is not read), the
 * float16 rows for OM_SEARCH_F16_ONLY (index_f32 is not read) -- so in the two 16-bit modes the bits are those a filtered search returns
 * for the same rows.  Ties by ascending row, ids = id_offset + row, (-3.4028235e38, -1) padding.  No scan, no margin, no redo: the
 * chain is fixed by cand_pitch alone -- per block of 4096 candidate columns one scoring kernel (a wavefront per (query, candidate)) and one
 * sorting selection -- and costs n_queries * cand_pitch * d whatever N.  Enqueues only; capturable after one eager call.
 * Refuses k outside [1, 2048], d no multiple of 64, more than 65535 queries, N above 2^31 - 1, a misaligned workspace, cand_pitch < 1, a
 * NULL cand, and a NULL plane of the kind the mode reads.  workspace: om_sim_topk_candidates_workspace_bytes, 256-byte aligned. */
size_t om_sim_topk_candidates_workspace_bytes(int64_t n_queries, int d, int k);
int om_sim_topk_candidates(int mode, const float* queries, int64_t n_queries, const float* index_f32, const void* index_f16, int64_t N, int d,
                           int k, int64_t id_offset, const int32_t* cand, int64_t cand_pitch, float* out_scores, int64_t* out_ids,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The schedule of om_sim_topk_filtered (csrc/search_plan.h search_schedule_filtered: no launch, no HIP call): *boot dense chunks of 4096
 * rows -- the smallest count whose expected allowed rows reach 2 k, at most all rows -- then *n filtered rounds of chunks[i] rows, the
 * first of which starts at row *boot * 4096, sized from the list estimate of k_eff.  n_allowed == N: om_debug_search_schedule's. */
int om_debug_search_schedule_filtered(int mode, int64_t nq, int64_t N, int k, int64_t n_allowed, int64_t* chunks, int cap, int* n,
                                      int64_t* boot);
/* What decides between scanning under the bitmap and gathering the allowed rows (openmatch_amd/index.py filter_route): *list_eff, the
 * list estimate that schedule sizes its rounds from -- that of k_eff = ceil(k N / n_allowed) in the mode's own formula -- and *list_max,
 * the longest list a selection may leave.  N >= 1, n_allowed in [1, N].  Pure: no launch, no HIP call. */
int om_debug_search_filter_estimate(int mode, int64_t N, int k, int64_t n_allowed, int64_t* list_eff, int64_t* list_max);
/* The row-typed kernels of the re-score and the redo over a caller's candidates, without a search: rows [N, d] in row_dtype (OM_F32 |
 * OM_F16), queries [n_queries, d] f32, cand [n_queries][m] row numbers (uint32, device; repeats allowed; a number >= N is not followed and
 * scores NaN), out_scores [n_queries][m] f32.  kernel 0: rescore_kernel, 1: rescore_strided_kernel -- out[q][j] = <query q, row cand[q][j]>;
 * 2: the redo's collect pass over ALL rows (cand is not read and may be NULL, m must be N <= 8192) -- out[q][r] = <query q, row r>.
 * The float16 and the float32 form return the same bits on rows that hold the same values.  d a multiple of 64, at most 16384;
 * workspace: om_sim_topk_async_workspace_bytes(n_queries, d, 1), 256-byte aligned. */
int om_debug_rescore_rows(int kernel, int row_dtype, const void* rows, int64_t N, int d, const float* queries, int64_t n_queries,
                          const uint32_t* cand, int m, float* out_scores, void* workspace, size_t workspace_bytes, void* stream);
/* The list kernels of a search -- everything between the scan's appends and (D, I) -- over a caller's lists, without a search; each is
 * launched as the search launches it (grid, block, dynamic LDS, the workspace's own arrays).
 * Lists in: scores / rows [n_queries][m] (f32 / uint32, device); list q gets pack_key(scores[q][j], rows[q][j]) in slot j < m and STALE keys
 * (score +inf, row 0xf0000000 + slot) in the slots m .. 8191 of its 8192-slot stride.  counts [n_queries] (uint32, device) is written to the
 * list counters as it is: a count above m names stale slots, one above 8192 is a round whose appends were dropped (at most 16384 is taken).
 * Before the kernel: cnt_prev = 0xffffffff, thr = NaN (bits 0x7fc00000), flag[0..15] = 0, qstat = 0.
 * op: */
#define OM_DEBUG_LISTS_RADIX 0     /* select_radix_kernel(k, margin, cap: 4096 | 8192)                                                  */
#define OM_DEBUG_LISTS_SORT 1      /* select_kernel(k, margin)                                                                          */
#define OM_DEBUG_LISTS_DROP 2      /* drop_disallowed_kernel(allow: (nrows + 31) / 32 words on the device, nrows >= 1)                  */
#define OM_DEBUG_LISTS_APPEND 3    /* append_dense_kernel(S [n_queries][ldS] f32, 1 <= n <= 4096, ldS >= n, row_base), then check_overflow_kernel(cover) */
#define OM_DEBUG_LISTS_EMIT 4      /* emit_kernel(k, id_offset) into emit_scores / emit_ids [n_queries][k]                              */
/* margin [n_queries] (f32, device) or NULL: certified or exact mode of the two selections (copied into the workspace's margins).
 * use_qstat 0: the kernels get a null qstat, as on om_sim_topk's path.  Arguments an op does not take are not read.
 * Lists out (any of the three may be NULL): out_scores / out_rows [n_queries][8192], the whole stride of every list, stale slots included;
 * out_state [n_queries][4] uint32 = {cnt, cnt_prev, bits of thr, qstat}, followed by flag[0..3].
 * 1 to 65535 queries, k in [1, 2048], m in [1, 8192]; workspace: om_sim_topk_async_workspace_bytes(n_queries, 64, 1), 256-byte aligned. */
int om_debug_select_lists(int op, int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int k,
                          const float* margin, int use_qstat, int cap, const uint32_t* allow, uint32_t nrows, const float* S, int64_t ldS,
                          int n, uint32_t row_base, uint32_t cover, int64_t id_offset, float* emit_scores, int64_t* emit_ids,
                          float* out_scores, uint32_t* out_rows, uint32_t* out_state, void* workspace, size_t workspace_bytes, void* stream);
/* OM_DEBUG_LISTS_DROP with the bitmaps of om_sim_topk_filtered_multi: drop_disallowed_kernel launched as that entry launches it, over
 * lists put and read back as om_debug_select_lists does (the same stale keys, counts and out_* layout).  allow / words_pitch / n_filters /
 * filter_of: as om_sim_topk_filtered_multi's, over rows [0, nrows).  A query under no filter keeps its list (a count above 8192 is
 * clamped and marked all the same), one with nothing allowed ends with count 0. */
int om_debug_drop_lists_multi(int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int use_qstat,
                              const uint32_t* allow, uint32_t nrows, int64_t words_pitch, int64_t n_filters, const int32_t* filter_of,
                              float* out_scores, uint32_t* out_rows, uint32_t* out_state, void* workspace, size_t workspace_bytes,
                              void* stream);
/* The drop under the exclusion lists of om_sim_topk_excluding: drop_excluded_kernel launched as that entry launches it, over lists put
 * and read back as om_debug_select_lists does (the same stale keys, counts and out_* layout).  excl [n_queries][pitch] as that entry's,
 * pitch in [1, OM_EXCLUDE_MAX], over rows [0, nrows): a key is kept, in its order, when its row is below nrows and not in the query's
 * list.  A query whose list is empty keeps its list as it is (a count above 8192 is clamped and marked all the same). */
int om_debug_drop_lists_excluding(int64_t n_queries, int m, const float* scores, const uint32_t* rows, const uint32_t* counts, int use_qstat,
                                  const int32_t* excl, int64_t pitch, uint32_t nrows, float* out_scores, uint32_t* out_rows,
                                  uint32_t* out_state, void* workspace, size_t workspace_bytes, void* stream);
/* query_prep_kernel on the grid of the search: queries [n_queries][d] f32 and stats[2] = {max ||p - f16(p)||, max ||f16(p)||} on the
 * device -> out_q16 [round_up(n_queries, 256)][d] float16 (rows beyond n_queries zero) and the certified margins out_margin [n_queries]. */
int om_debug_query_prep(const float* queries, int64_t n_queries, int d, const float* stats, void* out_q16, float* out_margin, void* stream);

/* Diagnostics of the calling thread's last om_sim_topk: out[0] = scan precision that produced
 * the result (0 f32, 1 f16+rescore), [1] = scan rounds, [2] = overflow fallbacks (chunks redone
 * densely), [3] = longest candidate list, [4] = 1 if the certified f16 margin was too wide and
 * the call fell back to the f32 scan, [5] = OM_SCAN_FAMILY_* of the last filtered-scan round
 * (0: every row was scored densely), [6] = OM_SCAN_KERNEL_* of that round's main launch (its tail's
 * where the round held no whole tile; 0: every row was scored densely), [7] = 0.  Written by
 * om_sim_topk alone, on every return behind its argument checks.
 * OM_SEARCH_F16_ONLY: [0] = 1, [2] = 0 (nothing is ever started over), [4] = the NUMBER of queries whose certified margin was too wide
 * (they were redone on the device, there is no float32 scan), [7] = queries redone on the device for any reason. */
void om_sim_topk_info(int64_t out[8]);

/* Which kernel a filtered-scan round of om_sim_topk runs (csrc/search_plan.h scan_plan: no launch, no HIP call, no pointer read). */
#define OM_SCAN_FAMILY_GENERIC 1   /* sim_filter_kernel: the 128-query tile of generation 2 (also the ragged tail behind a stream kernel)      */
#define OM_SCAN_FAMILY_WIDE 2      /* more than 128 queries: the 256 x 256 kernels (generation 7 / 7c over whole tiles, generation 6)         */
#define OM_SCAN_FAMILY_STREAM32 3  /* sim_stream_reg_kernel: 32-query blocks resident in registers, f16 index, 256 <= d <= 1024, <= 128 queries */
#define OM_SCAN_FAMILY_STREAM16 4  /* sim_stream_reg_kernel<.., 32, 16>: 16-query blocks on 16 x 16 x 32 MFMAs, 1088 <= d <= 2048, <= 64 queries         */
/* half: the 16-bit index (OM_SEARCH_F16_RESCORE) or the float32 one.  out = {family, queries per resident block (32 | 16 | 0), resident
 * blocks per workgroup (1 | 2 | 4 | 0), K steps of 64 columns compiled in (12 | 16 | 32 | 0)}, under the calling thread's switches. */
int om_debug_scan_plan(int half, int64_t nq, int d, int out[4]);
/* The launches of one filtered round (csrc/search_plan.h scan_round: no launch, no HIP call, no pointer read). */
#define OM_SCAN_KERNEL_TILE2 1     /* sim_filter_kernel: 256 rows x 128 queries per workgroup, generation 2, both index formats                */
#define OM_SCAN_KERNEL_TILE6 2     /* sim_filter_kernel6: 256 rows x 256 queries per workgroup, generation 6, both index formats               */
#define OM_SCAN_KERNEL_WIDE7 3     /* sim_filter_kernel7: persistent over 256 x 256 tiles, the ring restarted per tile, 16-bit index           */
#define OM_SCAN_KERNEL_WIDE7C 4    /* sim_filter_kernel7c: the same on the continuous ring (rows of at least three 128-byte K steps)           */
#define OM_SCAN_KERNEL_STREAM 5    /* sim_stream_reg_kernel: the instantiation om_debug_scan_plan names by qblock, nb and nkmax                */
/* The round over `rows` index rows of a search of nq queries of width d on a device of `cus` compute units: a main launch and a ragged
 * tail, either of which may be empty (all four words 0).  out = {main kernel OM_SCAN_KERNEL_*, rows, grid, group, tail kernel, rows,
 * grid, group}; the tail starts behind the main launch's rows; group is the kernel's last argument (tile kernels: group_m | qgroup << 8;
 * stream kernel: 1 = non-temporal index loads).  Under the calling thread's switches (OM_OPT_SCAN_GEN7, OM_OPT_SCAN_QGROUP,
 * OM_OPT_SEARCH_DEBUG).  Refuses a grid above 2^31 - 1 workgroups, as the search does. */
int om_debug_scan_round(int half, int64_t nq, int d, int64_t rows, int cus, int64_t out[8]);
/* One launch of exactly the stream instantiation om_debug_scan_plan names for (nq, d): rows16 [nrows, d] f16 with nrows a multiple of 128
 * (row r has id row_base + r), queries16 [>= nq, d] f16 as om_sim_topk's query preparation leaves them, thr[q] the score a row must
 * reach (128 floats, +inf beyond nq), keys [nq][8192] and cnt [nq] the candidate lists (cnt counts every survivor, keys holds the
 * first 8192 as (orderable score) << 32 | ~id), on `grid` persistent workgroups.  Refuses a shape the plan sends elsewhere. */
int om_debug_sim_stream(const void* rows16, int64_t nrows, uint32_t row_base, const void* queries16, int64_t nq, int d, const float* thr,
                        uint64_t* keys, unsigned* cnt, int grid, void* stream);
/* One launch of a tile kernel of the scan's kernel table, as a filtered round of om_sim_topk launches it: kernel = OM_SCAN_KERNEL_TILE2,
 * TILE6, WIDE7 or WIDE7C, half = 0 the float32 plane, 1 the float16 plane (rows and queries in that format), rows [nrows, d] with ids
 * from row_base, grid and group as om_debug_scan_round returns them (generation 7: group = group_m | qgroup << 8).  Survivors
 * (score >= thr[q]) are APPENDED: cnt[q] counts every one, keys[q] holds those whose position is below 8192.
 * Refused, with nothing launched: a null argument; a kernel the table does not hold (generation 7 on the float32 plane, 0, STREAM);
 * d <= 0 or d % 64 != 0; nrows < 1 or nq < 1; grid outside [1, 2^31 - 1]; group_m = 0; WIDE7 / WIDE7C with nrows % 256 != 0 (whole row
 * tiles only); WIDE7C with d < 192; TILE2 / TILE6 with a grid other than one workgroup per (256-row tile, 128- / 256-query tile).
 * NOT checked, the caller's to keep: for TILE6, WIDE7 and WIDE7C queries holds round_up(nq, 256) rows, zero beyond nq; thr is readable
 * for round_up(nq, 256) + 256 entries and +inf beyond nq; keys is [nq][8192]; cnt is [nq] and is not cleared. */
int om_debug_scan_kernel(int kernel, int half, const void* rows, int64_t nrows, uint32_t row_base, const void* queries, int64_t nq, int d,
                         const float* thr, uint64_t* keys, unsigned* cnt, int64_t grid, int group, void* stream);

/* Merge W partial results (utils.py:215-229 merge_retrieval_results_by_score /
 * faiss shard merge): parts are [W][Q,k_in] row-major, each row descending;
 * entries with id < 0 are padding.  Output [Q,k_out] descending; ties keep
 * (part, position) order (python's stable sorted(reverse=True)). */
int om_topk_merge(const float* part_scores, const int64_t* part_ids, int W, int64_t n_queries,
                  int k_in, int k_out, float* out_scores, int64_t* out_ids, void* stream);

/* ------------------------------------------------------------------------
 * In-batch-negatives contrastive loss, forward + backward in one call.
 * Replaces  scores = q @ p.T ; CrossEntropyLoss(mean)(scores, arange(Q)*n_psg)
 * (modeling/dense_retrieval_model.py:113-122, loss.py:9-15) and its autograd.
 *   q [Qg,d], p [Pg,d] f32 (already all-gathered when negatives_x_device);
 *   loss = loss_scale * mean_i CE(scores[i,:], i*n_psg);
 *   d_q [q_rows,d], d_p [p_rows,d]: gradient of loss w.r.t. the LOCAL slices
 *   q[q_row0 : q_row0+q_rows], p[p_row0 : p_row0+p_rows] (the reference's
 *   all_gather re-inserts only the local tensor: :247-258).
 * scores (f32 [Qg,Pg]) may be NULL; d_q / d_p may be NULL (forward only).
 * Any d >= 1; q and p need the alignment of a float only.
 * workspace: (2*Qg*Pg + Qg) floats.
 * ------------------------------------------------------------------------ */
int om_contrastive_fwd_bwd(const float* q, const float* p, int Qg, int Pg, int d, int n_psg,
                           float loss_scale, int q_row0, int q_rows, int p_row0, int p_rows,
                           float* loss, float* scores, float* d_q, float* d_p, float* workspace,
                           void* stream);

/* The same with the full call surface of `F.cross_entropy(logits, target, reduction=...)` that the reference's
 * loss callables expose (loss.py:9-15: `target=None, reduction='mean'` are parameters of SimpleContrastiveLoss.__call__;
 * :27-31 forwards them through DistributedContrastiveLoss):
 *   target   int64 [Qg] class index per row, or NULL for the in-batch positive i*n_psg; -100 rows are ignored
 *            (torch's ignore_index: loss 0, no gradient, not counted by the mean);
 *   reduction 0 mean | 1 sum | 2 none (loss is then [Qg]; row_grad [Qg], or NULL for ones, is the upstream
 *            gradient of each row's loss -- call once with d_q = d_p = NULL for the forward, again for the backward).
 * workspace: (2*Qg*Pg + Qg + 1) floats. */
int om_contrastive_fwd_bwd_ex(const float* q, const float* p, int Qg, int Pg, int d, const int64_t* target, int n_psg,
                              int reduction, const float* row_grad, float loss_scale, int q_row0, int q_rows,
                              int p_row0, int p_rows, float* loss, float* scores, float* d_q, float* d_p,
                              float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * Multi-GPU collectives over RCCL / xGMI (one process per GPU).  What the reference does through torch.distributed
 * + NCCL and faiss-GPU, behind plain pointers:
 *   om_allgather_rows   DRModel.dist_gather_tensor (modeling/dense_retrieval_model.py:247-258; loss.py:33-38):
 *                       recv[w*rows:(w+1)*rows] = rank w's rows, rank-major
 *   om_allreduce_grads  the gradient averaging DistributedDataParallel does under HF Trainer
 *                       (trainer/dense_trainer.py:27-108): in place over one flat f32 buffer
 *   om_exchange_topk    the shard-merge traffic of the faiss-GPU index (retriever/dense_retriever.py:43-58),
 *                       re-cut by query range: block w of this shard's [world][q_block][k] candidates goes to rank w
 *                       (follow with om_topk_merge on the received [world][q_block][k])
 * A communicator is created from a 128-byte unique id: rank 0 calls om_comm_unique_id, the host layer broadcasts it
 * over whatever rendezvous it has (openmatch_amd: the torch.distributed store), every rank calls om_comm_init with
 * its HIP device current.  RCCL is bound at run time; all calls are asynchronous on `stream`.
 * ------------------------------------------------------------------------ */
#define OM_COMM_ID_BYTES 128
int om_comm_unique_id(void* id128);
int om_comm_init(const void* id128, int world, int rank, void** comm);
int om_comm_destroy(void* comm);
int om_comm_count(void* comm, int* count);   /* ranks of the communicator as RCCL reports them (ncclCommCount) */
int om_allgather_rows(void* comm, const void* send, void* recv, int64_t rows, int64_t row_bytes, void* stream);
int om_allreduce_grads(void* comm, float* buf, int64_t n, int average, void* stream);
int om_exchange_topk(void* comm, int world, const float* D, const int64_t* I, int64_t q_block, int k, float* recvD,
                     int64_t* recvI, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENMATCH_HIP_H */
