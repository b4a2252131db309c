// Native GPU self-test + micro-benchmark of libopenmatch_hip.so (no Python, starts in
// milliseconds on a fresh box).  Every kernel is compared with a straightforward double-
// precision host loop on random, asymmetric data.  Usage: selftest [quick|full|bench]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../include/openmatch_hip.h"
#include <stdlib.h>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)
#define OMCK(x) do { if (x) { printf("OM error: %s  (%s:%d)\n", om_last_error(), __FILE__, __LINE__); g_fail++; } } while (0)

static int g_fail = 0;
static std::mt19937 rng(20260925);

typedef unsigned short bf16;
static bf16 f2b(float f) { unsigned u; memcpy(&u, &f, 4); unsigned lsb = (u >> 16) & 1; return (bf16)((u + 0x7fff + lsb) >> 16); }
static float b2f(bf16 b) { unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }

template <typename T> T* dalloc(size_t n) { T* p; CK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T))); return p; }
template <typename T> T* upload(const std::vector<T>& v) { T* p = dalloc<T>(v.size()); CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); return p; }
template <typename T> std::vector<T> download(const T* p, size_t n) { std::vector<T> v(n); CK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }

static std::vector<float> randn(size_t n, float scale = 1.f) { std::normal_distribution<float> d(0.f, scale); std::vector<float> v(n); for (auto& x : v) x = d(rng); return v; }
static std::vector<bf16> to_bf16(const std::vector<float>& v) { std::vector<bf16> o(v.size()); for (size_t i = 0; i < v.size(); ++i) o[i] = f2b(v[i]); return o; }
static std::vector<float> round_bf16(const std::vector<float>& v) { std::vector<float> o(v.size()); for (size_t i = 0; i < v.size(); ++i) o[i] = b2f(f2b(v[i])); return o; }

static void report(const char* name, double maxerr, double tol, const char* extra = "") {
  const bool ok = maxerr <= tol && std::isfinite(maxerr);
  printf("[%s] %-58s max_err=%.3e tol=%.1e %s\n", ok ? " OK " : "FAIL", name, maxerr, tol, extra);
  if (!ok) g_fail++;
}

static double act_ref(double x, int act) {
  if (act == OM_ACT_GELU_ERF) return 0.5 * x * (1.0 + erf(x / sqrt(2.0)));
  if (act == OM_ACT_RELU) return x > 0 ? x : 0;
  if (act == OM_ACT_GELU_TANH) return 0.5 * x * (1.0 + tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)));
  return x;
}

// ---------------------------------------------------------------- GEMM
static void test_gemm(int dtype, int64_t M, int64_t N, int64_t K, bool bias, bool resid, int act, int out_dtype) {
  auto A = randn(M * K), B = randn(N * K, 0.05f), bs = randn(N), R = randn(M * N);
  if (dtype == OM_BF16) { A = round_bf16(A); B = round_bf16(B); }
  if (out_dtype == OM_BF16) R = round_bf16(R);
  void *dA, *dB, *dC, *dR = nullptr;
  if (dtype == OM_BF16) { dA = upload(to_bf16(A)); dB = upload(to_bf16(B)); } else { dA = upload(A); dB = upload(B); }
  if (out_dtype == OM_BF16) { dC = dalloc<bf16>(M * N); if (resid) dR = upload(to_bf16(R)); } else { dC = dalloc<float>(M * N); if (resid) dR = upload(R); }
  CK(hipMemset(dC, 0xff, M * N * (out_dtype == OM_BF16 ? 2 : 4)));
  float* dbias = bias ? upload(bs) : nullptr;
  OMCK(om_gemm_nt(dtype, dA, K, dB, K, out_dtype, dC, N, M, N, K, dbias, dR, N, act, nullptr));
  CK(hipDeviceSynchronize());
  std::vector<float> C(M * N);
  if (out_dtype == OM_BF16) { auto t = download((bf16*)dC, M * N); for (size_t i = 0; i < C.size(); ++i) C[i] = b2f(t[i]); } else C = download((float*)dC, M * N);
  double maxerr = 0; int64_t bi = -1, bj = -1;
  for (int64_t i = 0; i < M; ++i) for (int64_t j = 0; j < N; ++j) {
    double acc = 0; for (int64_t k = 0; k < K; ++k) acc += (double)A[i * K + k] * B[j * K + k];
    if (bias) acc += bs[j];
    acc = act_ref(acc, act & 0xff);
    if (resid) acc = (act & OM_ACT_MUL_RESID) ? acc * R[i * N + j] : acc + R[i * N + j];
    double e = fabs(acc - C[i * N + j]) / (1.0 + fabs(acc));
    if (!(e <= maxerr)) { maxerr = e; bi = i; bj = j; }
  }
  char name[160], extra[80];
  snprintf(name, sizeof name, "gemm %s->%s M=%ld N=%ld K=%ld bias=%d resid=%d act=0x%x", dtype ? "bf16" : "f32", out_dtype ? "bf16" : "f32", (long)M, (long)N, (long)K, bias, resid, act);
  snprintf(extra, sizeof extra, "worst@(%ld,%ld)", (long)bi, (long)bj);
  report(name, maxerr, out_dtype == OM_BF16 ? 1e-2 : (dtype == OM_BF16 ? 2e-5 : 2e-5), extra);
  hipFree(dA); hipFree(dB); hipFree(dC); if (dR) hipFree(dR); if (dbias) hipFree(dbias);
}

// ---------------------------------------------------------------- encoder (tiny, vs host double)
struct HostBert {
  int H, F, nl, nh, vocab, maxpos, L; float eps;
  std::vector<float> word, pos, type, eg, eb;
  struct Layer { std::vector<float> qkv_w, qkv_b, o_w, o_b, g1, b1, w1, bb1, w2, bb2, g2, b2; };
  std::vector<Layer> layers;
};
static void ln_ref(std::vector<double>& x, int H, const std::vector<float>& g, const std::vector<float>& b, double eps) {
  size_t M = x.size() / H;
  for (size_t i = 0; i < M; ++i) { double m = 0, v = 0; for (int c = 0; c < H; ++c) m += x[i * H + c]; m /= H; for (int c = 0; c < H; ++c) v += (x[i * H + c] - m) * (x[i * H + c] - m); v /= H; double r = 1.0 / sqrt(v + eps); for (int c = 0; c < H; ++c) x[i * H + c] = (x[i * H + c] - m) * r * g[c] + b[c]; }
}
static std::vector<double> linear_ref(const std::vector<double>& x, size_t M, int K, const std::vector<float>& W, const std::vector<float>& b, int N) {
  std::vector<double> y(M * N);
  for (size_t i = 0; i < M; ++i) for (int j = 0; j < N; ++j) { double a = b.empty() ? 0 : b[j]; for (int k = 0; k < K; ++k) a += x[i * K + k] * W[(size_t)j * K + k]; y[i * N + j] = a; }
  return y;
}
static std::vector<double> bert_ref(const HostBert& m, const std::vector<int64_t>& ids, const std::vector<int64_t>& mask, const std::vector<int64_t>& tt, int B) {
  const int H = m.H, L = m.L; size_t M = (size_t)B * L;
  std::vector<double> x(M * H);
  for (size_t r = 0; r < M; ++r) for (int c = 0; c < H; ++c) x[r * H + c] = (double)m.word[ids[r] * H + c] + m.type[tt[r] * H + c] + m.pos[(r % L) * H + c];
  ln_ref(x, H, m.eg, m.eb, m.eps);
  for (auto& lw : m.layers) {
    auto qkv = linear_ref(x, M, H, lw.qkv_w, lw.qkv_b, 3 * H);
    std::vector<double> ctx(M * H, 0.0);
    for (int b = 0; b < B; ++b) for (int h = 0; h < m.nh; ++h) for (int qi = 0; qi < L; ++qi) {
      std::vector<double> s(L); double mx = -1e300;
      for (int kj = 0; kj < L; ++kj) { double a = 0; for (int d = 0; d < 64; ++d) a += qkv[((size_t)b * L + qi) * 3 * H + h * 64 + d] * qkv[((size_t)b * L + kj) * 3 * H + H + h * 64 + d]; a = a / 8.0 + (mask[b * L + kj] ? 0.0 : -1e30); s[kj] = a; mx = std::max(mx, a); }
      double sum = 0; for (int kj = 0; kj < L; ++kj) { s[kj] = exp(s[kj] - mx); sum += s[kj]; }
      for (int d = 0; d < 64; ++d) { double a = 0; for (int kj = 0; kj < L; ++kj) a += s[kj] / sum * qkv[((size_t)b * L + kj) * 3 * H + 2 * H + h * 64 + d]; ctx[((size_t)b * L + qi) * H + h * 64 + d] = a; }
    }
    auto y = linear_ref(ctx, M, H, lw.o_w, lw.o_b, H);
    for (size_t i = 0; i < y.size(); ++i) y[i] += x[i];
    ln_ref(y, H, lw.g1, lw.b1, m.eps);
    auto f = linear_ref(y, M, H, lw.w1, lw.bb1, m.F);
    for (auto& v : f) v = act_ref(v, OM_ACT_GELU_ERF);
    auto z = linear_ref(f, M, m.F, lw.w2, lw.bb2, H);
    for (size_t i = 0; i < z.size(); ++i) z[i] += y[i];
    ln_ref(z, H, lw.g2, lw.b2, m.eps);
    x = z;
  }
  return x;
}

static void test_encoder(int dtype, int B, int L, int pooling, bool normalize, bool head) {
  HostBert m; m.H = 128; m.F = 256; m.nl = 2; m.nh = 2; m.vocab = 500; m.maxpos = 256; m.L = L; m.eps = 1e-12f;
  const int H = m.H, F = m.F;
  auto rb = [&](size_t n, float s) { auto v = randn(n, s); return dtype == OM_BF16 ? round_bf16(v) : v; };
  m.word = randn((size_t)m.vocab * H, 0.5f); m.pos = randn((size_t)m.maxpos * H, 0.5f); m.type = randn(2 * H, 0.5f);
  m.eg = randn(H, 0.2f); for (auto& v : m.eg) v += 1.f; m.eb = randn(H, 0.1f);
  m.layers.resize(m.nl);
  for (auto& lw : m.layers) {
    lw.qkv_w = rb((size_t)3 * H * H, 0.08f); lw.qkv_b = randn(3 * H, 0.1f); lw.o_w = rb((size_t)H * H, 0.08f); lw.o_b = randn(H, 0.1f);
    lw.g1 = randn(H, 0.2f); for (auto& v : lw.g1) v += 1.f; lw.b1 = randn(H, 0.1f);
    lw.w1 = rb((size_t)F * H, 0.08f); lw.bb1 = randn(F, 0.1f); lw.w2 = rb((size_t)H * F, 0.08f); lw.bb2 = randn(H, 0.1f);
    lw.g2 = randn(H, 0.2f); for (auto& v : lw.g2) v += 1.f; lw.b2 = randn(H, 0.1f);
  }
  std::vector<int64_t> ids((size_t)B * L), mask((size_t)B * L), tt((size_t)B * L);
  for (int b = 0; b < B; ++b) { int len = 1 + rng() % L; if (b == 0) len = L; for (int t = 0; t < L; ++t) { ids[b * L + t] = t < len ? 1 + rng() % (m.vocab - 1) : 0; mask[b * L + t] = t < len; tt[b * L + t] = (t < len && t > len / 2) ? 1 : 0; } }
  auto ref = bert_ref(m, ids, mask, tt, B);
  std::vector<float> headw = randn((size_t)H * H, 0.1f);
  // reps reference
  std::vector<double> reps((size_t)B * H);
  for (int b = 0; b < B; ++b) for (int c = 0; c < H; ++c) {
    if (pooling == OM_POOL_FIRST) reps[b * H + c] = ref[((size_t)b * L) * H + c];
    else { double a = 0, n = 0; for (int t = 0; t < L; ++t) { a += ref[((size_t)b * L + t) * H + c] * mask[b * L + t]; n += mask[b * L + t]; } reps[b * H + c] = a / std::max(n, 1e-9); }
  }
  if (head) { std::vector<double> r2((size_t)B * H); for (int b = 0; b < B; ++b) for (int j = 0; j < H; ++j) { double a = 0; for (int k = 0; k < H; ++k) a += reps[b * H + k] * headw[(size_t)j * H + k]; r2[b * H + j] = a; } reps = r2; }
  if (normalize) for (int b = 0; b < B; ++b) { double n = 0; for (int c = 0; c < H; ++c) n += reps[b * H + c] * reps[b * H + c]; n = std::max(sqrt(n), 1e-12); for (int c = 0; c < H; ++c) reps[b * H + c] /= n; }

  OmEncoderConfig cfg; memset(&cfg, 0, sizeof cfg);
  cfg.arch = OM_ARCH_BERT; cfg.dtype = dtype; cfg.hidden = H; cfg.n_layers = m.nl; cfg.n_heads = m.nh; cfg.head_dim = 64; cfg.ffn = F; cfg.vocab = m.vocab; cfg.max_pos = m.maxpos; cfg.type_vocab = 2; cfg.act = OM_ACT_GELU_ERF; cfg.ln_eps = m.eps; cfg.pooling = pooling; cfg.head_in = head ? H : 0; cfg.head_out = head ? H : 0; cfg.normalize = normalize;
  std::vector<OmLayerWeights> lws(m.nl);
  auto upw = [&](const std::vector<float>& v) -> void* { return dtype == OM_BF16 ? (void*)upload(to_bf16(v)) : (void*)upload(v); };
  for (int l = 0; l < m.nl; ++l) { auto& lw = m.layers[l]; OmLayerWeights& o = lws[l]; memset(&o, 0, sizeof o); o.qkv_w = upw(lw.qkv_w); o.qkv_b = upload(lw.qkv_b); o.o_w = upw(lw.o_w); o.o_b = upload(lw.o_b); o.ln1_g = upload(lw.g1); o.ln1_b = upload(lw.b1); o.ffn1_w = upw(lw.w1); o.ffn1_b = upload(lw.bb1); o.ffn2_w = upw(lw.w2); o.ffn2_b = upload(lw.bb2); o.ln2_g = upload(lw.g2); o.ln2_b = upload(lw.b2); }
  OmEncoderWeights W; memset(&W, 0, sizeof W);
  W.word_emb = upload(m.word); W.pos_emb = upload(m.pos); W.type_emb = upload(m.type); W.emb_ln_g = upload(m.eg); W.emb_ln_b = upload(m.eb); W.layers_host = lws.data(); W.head_w = head ? upload(headw) : nullptr;
  size_t wsb = om_encoder_workspace_bytes(&cfg, B, L);
  char* ws = dalloc<char>(wsb);
  auto dids = upload(ids); auto dmask = upload(mask); auto dtt = upload(tt);
  size_t es = dtype == OM_BF16 ? 2 : 4;
  char* dhid = dalloc<char>((size_t)B * L * H * es); float* dreps = dalloc<float>((size_t)B * H);
  OMCK(om_encoder_forward(&cfg, &W, dids, dmask, dtt, B, L, dhid, dreps, ws, wsb, nullptr));
  CK(hipDeviceSynchronize());
  std::vector<float> hid((size_t)B * L * H);
  if (dtype == OM_BF16) { auto t = download((bf16*)dhid, hid.size()); for (size_t i = 0; i < hid.size(); ++i) hid[i] = b2f(t[i]); } else hid = download((float*)dhid, hid.size());
  auto greps = download(dreps, (size_t)B * H);
  double e1 = 0, e2 = 0;
  for (int b = 0; b < B; ++b) for (int t = 0; t < L; ++t) if (mask[b * L + t] || pooling == OM_POOL_FIRST) for (int c = 0; c < H; ++c) { size_t i = ((size_t)b * L + t) * H + c; double e = fabs(hid[i] - ref[i]); if (!(e <= e1)) e1 = e; }
  for (size_t i = 0; i < greps.size(); ++i) { double e = fabs(greps[i] - reps[i]) / (1 + fabs(reps[i])); if (!(e <= e2)) e2 = e; }
  char name[160];
  snprintf(name, sizeof name, "encoder(bert tiny) %s B=%d L=%d pool=%d norm=%d head=%d hidden", dtype ? "bf16" : "f32", B, L, pooling, normalize, head);
  report(name, e1, dtype == OM_BF16 ? 1.5e-1 : 2e-4);
  snprintf(name, sizeof name, "encoder(bert tiny) %s B=%d L=%d pool=%d norm=%d head=%d reps", dtype ? "bf16" : "f32", B, L, pooling, normalize, head);
  report(name, e2, dtype == OM_BF16 ? 1e-1 : 2e-4);
}

// ---------------------------------------------------------------- search
static void test_search(int mode, int64_t N, int Q, int d, int k, int order /*0 random,1 ascending (adversarial)*/, bool clustered) {
  auto P = randn((size_t)N * d, 0.3f), Qv = randn((size_t)Q * d, 0.3f);
  if (clustered) { auto mean = randn(d, 1.0f); for (int64_t i = 0; i < N; ++i) for (int c = 0; c < d; ++c) P[i * d + c] = mean[c] + 0.05f * P[i * d + c]; for (int i = 0; i < Q; ++i) for (int c = 0; c < d; ++c) Qv[i * d + c] = mean[c] + 0.05f * Qv[i * d + c]; }
  if (order == 1) {  // sort rows by score against query 0 ascending: every chunk beats the running threshold
    std::vector<std::pair<double, int64_t>> sc(N);
    for (int64_t i = 0; i < N; ++i) { double a = 0; for (int c = 0; c < d; ++c) a += (double)P[i * d + c] * Qv[c]; sc[i] = {a, i}; }
    std::sort(sc.begin(), sc.end());
    std::vector<float> P2(P.size()); for (int64_t i = 0; i < N; ++i) memcpy(&P2[i * d], &P[sc[i].second * d], d * 4); P = P2;
  }
  float* dP = upload(P); float* dQ = upload(Qv);
  bf16* dPb = dalloc<bf16>((size_t)N * d); float* dstats = dalloc<float>(2); CK(hipMemset(dstats, 0, 8));
  OMCK(om_index_to_f16(dP, N, d, dPb, dstats, nullptr));
  size_t wsb = om_sim_topk_workspace_bytes(Q, d, k); char* ws = dalloc<char>(wsb);
  float* dD = dalloc<float>((size_t)Q * k); int64_t* dI = dalloc<int64_t>((size_t)Q * k);
  auto t0 = std::chrono::steady_clock::now();
  OMCK(om_sim_topk(mode, dQ, Q, dP, dPb, dstats, N, d, k, 1000, dD, dI, ws, wsb, nullptr));
  CK(hipDeviceSynchronize());
  double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  auto D = download(dD, (size_t)Q * k); auto I = download(dI, (size_t)Q * k);
  // reference: double scores, top-k set; ties/near-ties adjudicated with a 1e-5 relative band
  int bad_sets = 0, bad_order = 0, near_tie_only = 0; double maxdiff = 0;
  std::vector<double> sc(N); std::vector<int64_t> idx(N);
  for (int qi = 0; qi < Q; ++qi) {
    for (int64_t i = 0; i < N; ++i) { double a = 0; for (int c = 0; c < d; ++c) a += (double)P[i * d + c] * Qv[(size_t)qi * d + c]; sc[i] = a; }
    std::iota(idx.begin(), idx.end(), 0);
    const int64_t kk = std::min<int64_t>(k, N);
    std::partial_sort(idx.begin(), idx.begin() + kk, idx.end(), [&](int64_t a, int64_t b) { return sc[a] > sc[b] || (sc[a] == sc[b] && a < b); });
    const double kth = sc[idx[kk - 1]];
    std::vector<char> in_ref(N, 0); for (int64_t j = 0; j < kk; ++j) in_ref[idx[j]] = 1;
    bool set_ok = true, tie_only = true;
    for (int64_t j = 0; j < k; ++j) {
      int64_t id = I[(size_t)qi * k + j]; float s = D[(size_t)qi * k + j];
      if (j >= kk) { if (id != -1) set_ok = false, tie_only = false; continue; }
      id -= 1000;
      if (id < 0 || id >= N) { set_ok = false; tie_only = false; continue; }
      maxdiff = std::max(maxdiff, fabs(s - sc[id]) / (1 + fabs(sc[id])));
      if (!in_ref[id]) { set_ok = false; if (fabs(sc[id] - kth) > 1e-5 * (1 + fabs(kth))) tie_only = false; }
      if (j > 0 && D[(size_t)qi * k + j] > D[(size_t)qi * k + j - 1]) bad_order++;
    }
    if (!set_ok) { bad_sets++; if (tie_only) near_tie_only++; }
  }
  char name[200], extra[260];
  snprintf(name, sizeof name, "sim_topk mode=%d N=%ld Q=%d d=%d k=%d order=%d clustered=%d", mode, (long)N, Q, d, k, order, clustered);
  int64_t info[8]; om_sim_topk_info(info);
  snprintf(extra, sizeof extra, "id-set mismatches=%d (near-tie only=%d) unsorted=%d %.1f ms [used=%ld rounds=%ld ovf=%ld list=%ld wide=%ld]", bad_sets, near_tie_only, bad_order, ms, (long)info[0], (long)info[1], (long)info[2], (long)info[3], (long)info[4]);
  const bool ok = (bad_sets - near_tie_only) == 0 && bad_order == 0;
  report(name, ok ? maxdiff : 1e9, 1e-5, extra);
  hipFree(dP); hipFree(dQ); hipFree(dPb); hipFree(dstats); hipFree(ws); hipFree(dD); hipFree(dI);
}

static void test_merge() {
  const int W = 4, Q = 7, kin = 50, kout = 60;
  std::vector<float> ps((size_t)W * Q * kin); std::vector<int64_t> pi(ps.size());
  for (int w = 0; w < W; ++w) for (int q = 0; q < Q; ++q) {
    std::vector<float> v(kin); for (auto& x : v) x = (float)(rng() % 40) * 0.25f;  // many ties
    std::sort(v.begin(), v.end(), std::greater<float>());
    int valid = (w == 3) ? 5 : kin;
    for (int j = 0; j < kin; ++j) { size_t o = ((size_t)w * Q + q) * kin + j; ps[o] = j < valid ? v[j] : -3.4028235e38f; pi[o] = j < valid ? (int64_t)w * 100000 + j : -1; }
  }
  float* dps = upload(ps); int64_t* dpi = upload(pi); float* dos = dalloc<float>(Q * kout); int64_t* doi = dalloc<int64_t>(Q * kout);
  OMCK(om_topk_merge(dps, dpi, W, Q, kin, kout, dos, doi, nullptr)); CK(hipDeviceSynchronize());
  auto os = download(dos, Q * kout); auto oi = download(doi, Q * kout);
  int bad = 0;
  for (int q = 0; q < Q; ++q) {
    std::vector<std::pair<float, int64_t>> all;
    for (int w = 0; w < W; ++w) for (int j = 0; j < kin; ++j) { size_t o = ((size_t)w * Q + q) * kin + j; if (pi[o] >= 0) all.push_back({ps[o], pi[o]}); }
    std::stable_sort(all.begin(), all.end(), [](auto& a, auto& b) { return a.first > b.first; });
    for (int j = 0; j < kout; ++j) { if (j < (int)all.size()) { if (os[q * kout + j] != all[j].first || oi[q * kout + j] != all[j].second) bad++; } else if (oi[q * kout + j] != -1) bad++; }
  }
  report("topk_merge W=4 (ties keep part/position order, padding)", bad, 0);
}

static void test_contrastive() {
  const int Qg = 16, n_psg = 4, Pg = 64, d = 128; const float scale = 2.f;
  auto q = randn(Qg * d, 0.3f), p = randn(Pg * d, 0.3f);
  float *dq = upload(q), *dp = upload(p), *dl = dalloc<float>(1), *ds = dalloc<float>(Qg * Pg), *gq = dalloc<float>(8 * d), *gp = dalloc<float>(32 * d), *ws = dalloc<float>(2 * Qg * Pg + Qg + 1);
  OMCK(om_contrastive_fwd_bwd(dq, dp, Qg, Pg, d, n_psg, scale, 8, 8, 32, 32, dl, ds, gq, gp, ws, nullptr)); CK(hipDeviceSynchronize());
  std::vector<double> S(Qg * Pg), dS(Qg * Pg); double loss = 0;
  for (int i = 0; i < Qg; ++i) { double mx = -1e300; for (int j = 0; j < Pg; ++j) { double a = 0; for (int c = 0; c < d; ++c) a += (double)q[i * d + c] * p[j * d + c]; S[i * Pg + j] = a; mx = std::max(mx, a); } double sum = 0; for (int j = 0; j < Pg; ++j) sum += exp(S[i * Pg + j] - mx); loss += mx + log(sum) - S[i * Pg + i * n_psg]; for (int j = 0; j < Pg; ++j) dS[i * Pg + j] = (exp(S[i * Pg + j] - mx) / sum - (j == i * n_psg)) * scale / Qg; }
  loss = loss / Qg * scale;
  auto gl = download(dl, 1); auto gs = download(ds, Qg * Pg); auto ggq = download(gq, 8 * d); auto ggp = download(gp, 32 * d);
  double e = fabs(gl[0] - loss), es = 0, eq = 0, ep = 0;
  for (int i = 0; i < Qg * Pg; ++i) es = std::max(es, fabs(gs[i] - S[i]));
  for (int i = 0; i < 8; ++i) for (int c = 0; c < d; ++c) { double a = 0; for (int j = 0; j < Pg; ++j) a += dS[(8 + i) * Pg + j] * p[j * d + c]; eq = std::max(eq, fabs(a - ggq[i * d + c])); }
  for (int j = 0; j < 32; ++j) for (int c = 0; c < d; ++c) { double a = 0; for (int i = 0; i < Qg; ++i) a += dS[i * Pg + 32 + j] * q[i * d + c]; ep = std::max(ep, fabs(a - ggp[j * d + c])); }
  report("contrastive loss", e, 1e-5); report("contrastive scores", es, 1e-5); report("contrastive d_q (local rows)", eq, 1e-6); report("contrastive d_p (local rows)", ep, 1e-6);
}

// The C-ABI collectives on a ONE-rank communicator (every box so far had one GPU): om_comm_unique_id -> om_comm_init -> om_allgather_rows ->
// om_allreduce_grads -> om_exchange_topk -> om_topk_merge, the call sequence of a sharded search and of cross-device negatives, with no
// Python in between (include/openmatch_hip.h:561-573; reference: modeling/dense_retrieval_model.py:247-258, retriever/dense_retriever.py:43-58).
static void test_collectives_one_rank() {
  unsigned char id[OM_COMM_ID_BYTES];
  if (om_comm_unique_id(id)) { printf("%-64s SKIPPED (RCCL not loadable: %s)\n", "collectives on a one-rank communicator", om_last_error()); return; }
  void* comm = nullptr;
  OMCK(om_comm_init(id, 1, 0, &comm));
  int count = 0; OMCK(om_comm_count(comm, &count));
  report("comm: one rank as RCCL counts them", count == 1 ? 0 : 1, 0);
  const int rows = 37, d = 96;
  auto x = randn((size_t)rows * d);
  float* dx = upload(x); float* dg = dalloc<float>((size_t)rows * d);
  OMCK(om_allgather_rows(comm, dx, dg, rows, (int64_t)d * 4, nullptr)); CK(hipDeviceSynchronize());
  auto g = download(dg, (size_t)rows * d);
  double e = 0; for (size_t i = 0; i < g.size(); ++i) e = std::max(e, (double)fabs(g[i] - x[i]));
  report("allgather_rows (world 1: the rows themselves)", e, 0);
  OMCK(om_allreduce_grads(comm, dg, (int64_t)rows * d, 1, nullptr)); CK(hipDeviceSynchronize());
  g = download(dg, (size_t)rows * d);
  e = 0; for (size_t i = 0; i < g.size(); ++i) e = std::max(e, (double)fabs(g[i] - x[i]));
  report("allreduce_grads average (world 1: unchanged)", e, 0);
  // a shard's candidates [world = 1][q_block][k] -> the owner of the query block, then the merge
  const int Q = 6, k = 16;
  std::vector<float> D((size_t)Q * k); std::vector<int64_t> I(D.size());
  for (int q = 0; q < Q; ++q) { std::vector<float> v(k); for (auto& t : v) t = (float)(rng() % 1000) * 0.01f; std::sort(v.begin(), v.end(), std::greater<float>());
    for (int j = 0; j < k; ++j) { D[q * k + j] = v[j]; I[q * k + j] = 1000 * q + j; } }
  float* dD = upload(D); int64_t* dI = upload(I); float* rD = dalloc<float>(D.size()); int64_t* rI = dalloc<int64_t>(I.size());
  OMCK(om_exchange_topk(comm, 1, dD, dI, Q, k, rD, rI, nullptr));
  float* mD = dalloc<float>((size_t)Q * k); int64_t* mI = dalloc<int64_t>((size_t)Q * k);
  OMCK(om_topk_merge(rD, rI, 1, Q, k, k, mD, mI, nullptr)); CK(hipDeviceSynchronize());
  auto oD = download(mD, D.size()); auto oI = download(mI, I.size());
  int bad = 0; for (size_t i = 0; i < D.size(); ++i) bad += (oD[i] != D[i]) || (oI[i] != I[i]);
  report("exchange_topk + topk_merge (world 1: the shard's own lists)", bad, 0);
  OMCK(om_comm_destroy(comm));
  hipFree(dx); hipFree(dg); hipFree(dD); hipFree(dI); hipFree(rD); hipFree(rI); hipFree(mD); hipFree(mI);
}

// ---------------------------------------------------------------- micro-benchmarks
static void bench_gemm(int dtype, int64_t M, int64_t N, int64_t K, int act) {
  size_t es = dtype == OM_BF16 ? 2 : 4;
  std::vector<float> hA = randn(std::min<size_t>((size_t)M * K, 1 << 22)), hB = randn((size_t)N * K, 0.05f);
  char* A = dalloc<char>(M * K * es); char* B = dalloc<char>(N * K * es); char* C = dalloc<char>(M * N * es); float* bias = upload(randn(N));
  // fill with random data (random operands clock lower than zeros: do not bench on zeros)
  if (dtype == OM_BF16) { auto t = to_bf16(hA); for (size_t o = 0; o < (size_t)M * K; o += t.size()) CK(hipMemcpy(A + o * 2, t.data(), std::min(t.size(), (size_t)M * K - o) * 2, hipMemcpyHostToDevice)); auto tb = to_bf16(hB); CK(hipMemcpy(B, tb.data(), tb.size() * 2, hipMemcpyHostToDevice)); }
  else { for (size_t o = 0; o < (size_t)M * K; o += hA.size()) CK(hipMemcpy(A + o * 4, hA.data(), std::min(hA.size(), (size_t)M * K - o) * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(B, hB.data(), hB.size() * 4, hipMemcpyHostToDevice)); }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) OMCK(om_gemm_nt(dtype, A, K, B, K, dtype, C, N, M, N, K, bias, nullptr, 0, act, nullptr));
  const int it = 20;
  CK(hipEventRecord(e0, nullptr));
  for (int i = 0; i < it; ++i) OMCK(om_gemm_nt(dtype, A, K, B, K, dtype, C, N, M, N, K, bias, nullptr, 0, act, nullptr));
  CK(hipEventRecord(e1, nullptr)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= it;
  printf("[BENCH] gemm %s M=%ld N=%ld K=%ld act=%d : %.3f ms  %.1f TFLOP/s\n", dtype ? "bf16" : "f32", (long)M, (long)N, (long)K, act, ms, 2.0 * M * N * K / ms / 1e9);
  hipFree(A); hipFree(B); hipFree(C); hipFree(bias);
}

static void bench_search(int mode, int64_t N, int Q, int d, int k) {
  std::vector<float> hP = randn(1 << 22, 0.3f);
  float* dP = dalloc<float>((size_t)N * d);
  for (size_t o = 0; o < (size_t)N * d; o += hP.size()) CK(hipMemcpy(dP + o, hP.data(), std::min(hP.size(), (size_t)N * d - o) * 4, hipMemcpyHostToDevice));
  // de-duplicate the repeated block a little: add a per-row ramp on column 0 via a second upload is
  // overkill for a timing run; ties only stress the tie-break path.
  float* dQ = upload(randn((size_t)Q * d, 0.3f));
  bf16* dPb = dalloc<bf16>((size_t)N * d); float* dstats = dalloc<float>(2); CK(hipMemset(dstats, 0, 8));
  OMCK(om_index_to_f16(dP, N, d, dPb, dstats, nullptr));
  size_t wsb = om_sim_topk_workspace_bytes(Q, d, k); char* ws = dalloc<char>(wsb);
  float* dD = dalloc<float>((size_t)Q * k); int64_t* dI = dalloc<int64_t>((size_t)Q * k);
  for (int rep = 0; rep < 2; ++rep) {
    CK(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    OMCK(om_sim_topk(mode, dQ, Q, dP, dPb, dstats, N, d, k, 0, dD, dI, ws, wsb, nullptr));
    CK(hipDeviceSynchronize());
    double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int64_t info[8]; om_sim_topk_info(info);
    printf("[BENCH] sim_topk mode=%d N=%ld Q=%d d=%d k=%d : %.2f ms  %.1f q/s  %.1f TFLOP/s-equivalent [used=%ld rounds=%ld ovf=%ld list=%ld wide=%ld]\n", mode, (long)N, Q, d, k, ms, Q / ms * 1e3, 2.0 * N * Q * d / ms / 1e9, (long)info[0], (long)info[1], (long)info[2], (long)info[3], (long)info[4]);
  }
  hipFree(dP); hipFree(dQ); hipFree(dPb); hipFree(dstats); hipFree(ws); hipFree(dD); hipFree(dI);
}

// per-block phase timelines of one GEMM launch (shader clocks); `warm` launches first (200: sustained clocks)
static void run_trace(int64_t N, int64_t K, int64_t M, int64_t ld, int warm, bool dump_blocks) {
    char* A = dalloc<char>(M * K * 2); char* B = dalloc<char>(N * K * 2); char* C = dalloc<char>(M * N * 2);
    { auto t = to_bf16(randn(1 << 22)); for (size_t o = 0; o < (size_t)M * K; o += t.size()) CK(hipMemcpy(A + o * 2, t.data(), std::min(t.size(), (size_t)M * K - o) * 2, hipMemcpyHostToDevice)); auto tb = to_bf16(randn((size_t)N * K, 0.05f)); CK(hipMemcpy(B, tb.data(), tb.size() * 2, hipMemcpyHostToDevice)); }
    const size_t nblk = 8192; unsigned long long* tr = dalloc<unsigned long long>(nblk * 32);
    for (int i = 0; i < warm; ++i) OMCK(om_gemm_nt(OM_BF16, A, ld, B, ld, OM_BF16, C, N, M, N, K, nullptr, nullptr, 0, 0, nullptr));
    CK(hipMemset(tr, 0, nblk * 32 * 8)); om_debug_gemm_trace(tr);
    OMCK(om_gemm_nt(OM_BF16, A, ld, B, ld, OM_BF16, C, N, M, N, K, nullptr, nullptr, 0, 0, nullptr));
    CK(hipDeviceSynchronize()); om_debug_gemm_trace(nullptr);
    auto h = download(tr, nblk * 32);
    unsigned long long t0 = ~0ull; size_t used = 0;
    for (size_t b = 0; b < nblk; ++b) if (h[b * 32]) { t0 = std::min(t0, h[b * 32]); used = b + 1; }
    printf("trace M=%ld N=%ld K=%ld ld=%ld blocks=%zu (cycles since first block start)\n", (long)M, (long)N, (long)K, (long)ld, used);
    {   // averages over all blocks: prologue [1]->[3], K loop [3]->[15] (ideal = K * 32 MFMA cycles per wave), epilogue [15]->[28]
      double pro = 0, loop = 0, epi = 0, tot = 0; size_t n = 0;
      for (size_t b = 0; b < used; ++b) if (h[b * 32] && h[b * 32 + 28] && h[b * 32 + 15] && h[b * 32 + 3]) {
        pro += (double)(h[b * 32 + 3] - h[b * 32 + 1]); loop += (double)(h[b * 32 + 15] - h[b * 32 + 3]);
        epi += (double)(h[b * 32 + 28] - h[b * 32 + 15]); tot += (double)(h[b * 32 + 28] - h[b * 32]); ++n;
      }
      if (n) printf("avg over %zu blocks: prologue %.0f  K loop %.0f (MFMA time %ld, x%.3f)  epilogue %.0f  whole tile %.0f (memtime ticks)\n", n, pro / n, loop / n, (long)(K * 32), loop / n / (K * 32.0), epi / n, tot / n);
      // effective shader clock: s_memtime ticks against the constant 100 MHz s_memrealtime counter, first start -> last end
      unsigned long long c0 = ~0ull, c1 = 0, w0 = ~0ull, w1 = 0;
      for (size_t b = 0; b < used; ++b) if (h[b * 32] && h[b * 32 + 28]) { c0 = std::min(c0, h[b * 32]); c1 = std::max(c1, h[b * 32 + 28]); w0 = std::min(w0, h[b * 32 + 30]); w1 = std::max(w1, h[b * 32 + 31]); }
      if (w1 > w0) printf("kernel span: %llu shader ticks in %.1f us (100 MHz wall counter) -> %.3f GHz effective shader clock; tiles per CU %.2f\n", c1 - c0, (w1 - w0) / 100.0, (double)(c1 - c0) / ((w1 - w0) * 10.0), used / 256.0);
    }
    if (dump_blocks) for (size_t b = 0; b < used; b += std::max<size_t>(1, used / 8)) {
      printf("blk %5zu:", b);
      for (int i = 0; i < 30; ++i) if (h[b * 32 + i] && i != 29) printf(" [%d]%llu", i, h[b * 32 + i] - t0);
      printf("\n");
    }
    hipFree(A); hipFree(B); hipFree(C); hipFree(tr);
}

int main(int argc, char** argv) {
  std::string what = argc > 1 ? argv[1] : "quick";
  int ndev = om_device_count();
  printf("openmatch_hip ABI v%d, %d device(s)\n", om_abi_version(), ndev);
  if (ndev <= 0) { printf("no GPU: %s\n", om_last_error()); return 3; }
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  printf("device: %s  CUs=%d  clock=%d MHz  mem=%.1f GB  LDS/block=%zu\n", prop.name, prop.multiProcessorCount, prop.clockRate / 1000, prop.totalGlobalMem / 1e9, prop.sharedMemPerBlock);

  if (what != "bench" && what != "prof" && what != "trace" && what != "shapes" && what != "layer" && what != "gen7" && what != "scantrace" && what != "tn" && what != "groupm") {
    // GEMM: aligned, ragged M/N tails, every epilogue, both dtypes
    test_gemm(OM_F32, 128, 128, 32, false, false, OM_ACT_NONE, OM_F32);
    test_gemm(OM_BF16, 128, 128, 64, false, false, OM_ACT_NONE, OM_F32);
    test_gemm(OM_F32, 256, 384, 256, true, false, OM_ACT_NONE, OM_F32);
    test_gemm(OM_BF16, 256, 384, 256, true, false, OM_ACT_NONE, OM_F32);
    test_gemm(OM_F32, 130, 200, 96, true, true, OM_ACT_GELU_ERF, OM_F32);
    test_gemm(OM_BF16, 130, 200, 192, true, true, OM_ACT_GELU_ERF, OM_BF16);
    test_gemm(OM_BF16, 1000, 70, 128, true, true, OM_ACT_RELU, OM_F32);
    test_gemm(OM_F32, 77, 300, 64, false, true, OM_ACT_GELU_TANH | OM_ACT_MUL_RESID, OM_F32);
    test_gemm(OM_BF16, 4099, 768, 768, true, false, OM_ACT_GELU_ERF, OM_BF16);
    test_gemm(OM_F32, 1030, 768, 768, true, true, OM_ACT_NONE, OM_F32);
    test_gemm(OM_BF16, 1000, 200, 128, true, true, OM_ACT_RELU, OM_BF16);        // v2 tile, ragged M and N tile
    test_gemm(OM_BF16, 513, 2304, 768, true, false, OM_ACT_NONE, OM_BF16);
    test_gemm(OM_BF16, 2048, 768, 3072, true, true, OM_ACT_NONE, OM_BF16);       // 48 K steps through the ring
    test_gemm(OM_F32, 777, 132, 64, false, true, OM_ACT_GELU_TANH | OM_ACT_MUL_RESID, OM_F32);
    test_gemm(OM_BF16, 600, 128, 64, false, false, OM_ACT_NONE, OM_F32);         // single K step
    // encoder end to end (embedding, attention incl. ragged L, LN, FFN, pooling, head, normalise)
    test_encoder(OM_F32, 5, 128, OM_POOL_FIRST, false, false);
    test_encoder(OM_F32, 3, 32, OM_POOL_MEAN, true, true);
    test_encoder(OM_F32, 3, 50, OM_POOL_MEAN, true, false);
    test_encoder(OM_F32, 2, 162, OM_POOL_FIRST, false, false);
    test_encoder(OM_F32, 2, 200, OM_POOL_FIRST, false, false);
    test_encoder(OM_BF16, 5, 128, OM_POOL_FIRST, true, false);
    test_encoder(OM_BF16, 3, 50, OM_POOL_MEAN, true, true);
    // search
    test_search(OM_SEARCH_F32, 3000, 9, 64, 10, 0, false);       // N < dense chunk
    test_search(OM_SEARCH_F32, 500, 5, 64, 1000, 0, false);      // N < k: padding
    test_search(OM_SEARCH_F32, 50000, 33, 128, 100, 0, false);
    test_search(OM_SEARCH_F32, 50000, 33, 128, 1000, 0, true);
    test_search(OM_SEARCH_F16_RESCORE, 50000, 33, 128, 100, 0, false);
    test_search(OM_SEARCH_F16_RESCORE, 50000, 33, 128, 1000, 0, true);
    test_search(OM_SEARCH_F32, 60000, 4, 64, 1000, 1, false);    // adversarial order -> overflow fallback
    test_search(OM_SEARCH_F16_RESCORE, 60000, 4, 64, 1000, 1, false);
    if (what == "full") {
      test_search(OM_SEARCH_F32, 300000, 130, 768, 1000, 0, true);
      test_search(OM_SEARCH_F16_RESCORE, 300000, 130, 768, 1000, 0, true);
    }
    test_merge();
    test_contrastive();
    test_collectives_one_rank();
  }
  if (what == "trace") {
    const int64_t N = argc > 2 ? atoi(argv[2]) : 768, K = argc > 3 ? atoi(argv[3]) : 768, M = argc > 4 ? atoll(argv[4]) : 32768;
    const int64_t ld = (argc > 5 && atoll(argv[5]) > 0) ? atoll(argv[5]) : K;   // leading dimension (0 / absent: K)
    run_trace(N, K, M, ld, argc > 6 ? atoi(argv[6]) : 3, true);
    return 0;
  }
  if (what == "gen7") {     // generation 7 (persistent, 128-byte K steps) against generation 6: correctness, layer shapes, tile traces
    for (int gen : {0, 70}) {
      om_debug_gemm_gen(gen);
      printf("-- generation 7%s\n", gen == 70 ? ", one tile per workgroup" : " (default selection)");
      test_gemm(OM_BF16, 512, 256, 128, false, false, OM_ACT_NONE, OM_BF16);       // two K steps, two tiles
      test_gemm(OM_BF16, 512, 256, 64, true, false, OM_ACT_NONE, OM_BF16);         // a single K step
      test_gemm(OM_BF16, 1024, 512, 192, true, true, OM_ACT_NONE, OM_BF16);        // three steps, residual ring
      test_gemm(OM_BF16, 4096, 768, 768, true, false, OM_ACT_GELU_ERF, OM_BF16);
      test_gemm(OM_BF16, 2048, 768, 3072, true, true, OM_ACT_NONE, OM_BF16);       // 24 steps through the unit rotation
      test_gemm(OM_BF16, 70 * 256, 1024, 256, true, true, OM_ACT_NONE, OM_BF16);   // 280 tiles: more than one per workgroup
      test_gemm(OM_BF16, 70 * 256, 768, 128, true, false, OM_ACT_RELU, OM_BF16);
      if (gen != 0) continue;
      // the continuous ring (round 4: no residual, >= 3 K steps): several tiles per workgroup, the ring carried across them
      test_gemm(OM_BF16, 70 * 256, 1024, 192, true, false, OM_ACT_GELU_ERF, OM_BF16);  // three steps: the prefetch reaches exactly one tile ahead
      test_gemm(OM_BF16, 70 * 256, 768, 768, true, false, OM_ACT_NONE, OM_BF16);       // 840 tiles on 256 workgroups, 12 steps
      test_gemm(OM_BF16, 70 * 256, 768, 256, false, false, OM_ACT_NONE, OM_BF16);      // four steps (ring period 5 against 4), no bias
      test_gemm(OM_BF16, 2048, 768, 3072, true, false, OM_ACT_RELU, OM_BF16);          // 48 steps, one tile per workgroup
      test_gemm(OM_BF16, 256, 256, 448, true, false, OM_ACT_NONE, OM_BF16);            // one tile, one workgroup, seven steps
    }
    const int64_t M = argc > 2 ? atoll(argv[2]) : 131072;
    for (int rep = 0; rep < 2; ++rep)
      for (int gen : {6, 70, 0}) {
        om_debug_gemm_gen(gen);
        printf("-- %s\n", gen == 6 ? "generation 6" : (gen == 70 ? "generation 7, one tile per workgroup" : "generation 7 (persistent)"));
        bench_gemm(OM_BF16, M, 2304, 768, 0);
        bench_gemm(OM_BF16, M, 768, 768, 0);
        bench_gemm(OM_BF16, M, 3072, 768, OM_ACT_GELU_ERF);
        bench_gemm(OM_BF16, M, 768, 3072, 0);
        bench_gemm(OM_BF16, 8192, 8192, 8192, 0);
      }
    for (int gen : {6, 70, 0}) {
      om_debug_gemm_gen(gen);
      printf("-- traces, %s\n", gen == 6 ? "generation 6" : (gen == 70 ? "generation 7, one tile per workgroup" : "generation 7 (persistent)"));
      run_trace(3072, 768, M, 768, 50, false);
      run_trace(768, 3072, M, 3072, 50, false);
    }
    om_debug_gemm_gen(0);
    printf("%s: %d failure(s)\n", g_fail ? "SELFTEST FAILED" : "SELFTEST PASSED", g_fail);
    return g_fail ? 1 : 0;
  }
  if (what == "tn") {       // weight-gradient contraction: time per shape under the debug variants of OM_OPT_WGRAD_DEBUG
    const int64_t M = argc > 2 ? atoll(argv[2]) : 9216;
    const int shapes[4][2] = {{768, 768}, {768, 3072}, {3072, 768}, {2304, 768}};
    for (auto& sh : shapes) {
      const int N = sh[0], K = sh[1];
      bf16* dA = upload(to_bf16(randn((size_t)M * N, 1.f)));
      bf16* dB = upload(to_bf16(randn((size_t)M * K, 1.f)));
      float* dC = dalloc<float>((size_t)N * K); float* db = dalloc<float>(N);
      std::vector<int> variants = {0, 8, 2, 4};      // DMA-fed (default), register-staged, plain stores, one step
      if (argc > 3) { variants.clear(); for (int a = 3; a < argc; ++a) variants.push_back(atoi(argv[a])); }
      for (int variant : variants) {
        om_debug_option(OM_OPT_WGRAD_DEBUG, variant);
        CK(hipMemset(dC, 0, (size_t)N * K * 4)); CK(hipMemset(db, 0, N * 4));
        for (int r = 0; r < 3; ++r) OMCK(om_gemm_tn_acc(OM_BF16, dA, N, dB, K, dC, K, db, M, N, K, nullptr));
        CK(hipDeviceSynchronize());
        auto t0 = std::chrono::steady_clock::now();
        const int reps = 20;
        for (int r = 0; r < reps; ++r) OMCK(om_gemm_tn_acc(OM_BF16, dA, N, dB, K, dC, K, db, M, N, K, nullptr));
        CK(hipDeviceSynchronize());
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
        printf("[BENCH] gemm_tn M=%ld N=%d K=%d variant=%d (%s%s%s, ~%d workgroups): %.1f us  %.1f TFLOP/s\n", (long)M, N, K, variant, "128x128",
               (variant & 2) ? ", plain stores" : "", (variant & 4) ? ", one step" : "", (variant >> 4) * 64, us, 2.0 * M * N * K / us * 1e-6);
      }
      om_debug_option(OM_OPT_WGRAD_DEBUG, 0);
      CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dC)); CK(hipFree(db));
    }
    // the batched launch (om_gemm_tn_acc_batch): the four contractions of `layers` bert-base layers at once, every layer
    // with its own operands (as the backward keeps them); checked against the per-shape kernel on layer 0
    for (int layers : {1, 2, 4, 12}) {
      std::vector<OmTnProblem> probs;
      std::vector<void*> owned;
      double flops = 0.0;
      std::vector<bf16> hA[4], hB[4];
      for (int l = 0; l < layers; ++l)
        for (int si = 0; si < 4; ++si) {
          const int N = shapes[si][0], K = shapes[si][1];
          if (l == 0) { hA[si] = to_bf16(randn((size_t)M * N, 1.f)); hB[si] = to_bf16(randn((size_t)M * K, 1.f)); }
          bf16* dA = upload(hA[si]); bf16* dB = upload(hB[si]);
          float* dC = dalloc<float>((size_t)N * K); float* db = dalloc<float>(N);
          CK(hipMemset(dC, 0, (size_t)N * K * 4)); CK(hipMemset(db, 0, N * 4));
          OmTnProblem q; q.A = dA; q.B = dB; q.C = dC; q.bias = db; q.lda = N; q.ldb = K; q.ldc = K; q.N = N; q.K = K;
          probs.push_back(q);
          owned.push_back(dA); owned.push_back(dB); owned.push_back(dC); owned.push_back(db);
          flops += 2.0 * M * N * K;
        }
      OMCK(om_gemm_tn_acc_batch(OM_BF16, probs.data(), (int)probs.size(), M, nullptr));
      CK(hipDeviceSynchronize());
      if (layers == 1) {                                   // one accumulation so far: compare with the split kernel
        for (int si = 0; si < 4; ++si) {
          const int N = shapes[si][0], K = shapes[si][1];
          float* dC = dalloc<float>((size_t)N * K); float* db = dalloc<float>(N);
          CK(hipMemset(dC, 0, (size_t)N * K * 4)); CK(hipMemset(db, 0, N * 4));
          OMCK(om_gemm_tn_acc(OM_BF16, probs[si].A, N, probs[si].B, K, dC, K, db, M, N, K, nullptr));
          const std::vector<float> want = download(dC, (size_t)N * K), got = download(probs[si].C, (size_t)N * K);
          const std::vector<float> wb = download(db, (size_t)N), gb = download(probs[si].bias, (size_t)N);
          double worst = 0.0, wbias = 0.0;
          for (size_t e = 0; e < want.size(); ++e) worst = std::max(worst, (double)fabsf(want[e] - got[e]));
          for (size_t e = 0; e < wb.size(); ++e) wbias = std::max(wbias, (double)fabsf(wb[e] - gb[e]));
          const bool ok = worst < 2e-5 * sqrt((double)M) * 8 && wbias < 2e-5 * sqrt((double)M) * 8;
          printf("[%s] gemm_tn batch vs split kernel N=%d K=%d: max |dC| %.3g, max |dbias| %.3g\n", ok ? "OK" : "FAIL", N, K, worst, wbias);
          if (!ok) ++g_fail;
          CK(hipFree(dC)); CK(hipFree(db));
        }
      }
      for (int r = 0; r < 2; ++r) OMCK(om_gemm_tn_acc_batch(OM_BF16, probs.data(), (int)probs.size(), M, nullptr));
      CK(hipDeviceSynchronize());
      auto t0 = std::chrono::steady_clock::now();
      const int reps = 10;
      for (int r = 0; r < reps; ++r) OMCK(om_gemm_tn_acc_batch(OM_BF16, probs.data(), (int)probs.size(), M, nullptr));
      CK(hipDeviceSynchronize());
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
      printf("[BENCH] gemm_tn batch M=%ld, %d layer(s) x 4 contractions (256x256 tiles, whole token axis): %.1f us  %.1f TFLOP/s\n",
             (long)M, layers, us, flops / us * 1e-6);
      for (void* q : owned) CK(hipFree(q));
    }
    printf("%s: %d failure(s)\n", g_fail ? "SELFTEST FAILED" : "SELFTEST PASSED", g_fail);
    return g_fail ? 1 : 0;
  }
  if (what == "attn") {        // bf16 attention kernel alone under the OM_OPT_ATTENTION_DEBUG variants
    const int64_t B = argc > 2 ? atoll(argv[2]) : 1024; const int L = argc > 3 ? atoi(argv[3]) : 128, H = 768, heads = 12;
    bf16* dqkv = upload(to_bf16(randn((size_t)B * L * 3 * H, 1.f)));
    bf16* dctx = dalloc<bf16>((size_t)B * L * H);
    std::vector<int64_t> hm((size_t)B * L, 1);
    int64_t* dmask = upload(hm);
    for (int variant : {0, 1, 2, 3, 4, 5, 6, 7, 0}) {
      om_debug_option(OM_OPT_ATTENTION_DEBUG, variant);
      for (int r = 0; r < 3; ++r) OMCK(om_debug_attention(dqkv, dctx, dmask, B, L, H, heads, nullptr));
      CK(hipDeviceSynchronize());
      auto t0 = std::chrono::steady_clock::now();
      const int reps = 20;
      for (int r = 0; r < reps; ++r) OMCK(om_debug_attention(dqkv, dctx, dmask, B, L, H, heads, nullptr));
      CK(hipDeviceSynchronize());
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
      printf("[BENCH] attention B=%ld L=%d heads=%d variant=%d (%s%s%s): %.1f us  %.2f TB/s of qkv + ctx\n", (long)B, L, heads, variant,
             (variant & 1) ? "no K/V fetch " : "", (variant & 2) ? "no arithmetic " : "", (variant & 4) ? "no stores" : "", us,
             (double)B * L * H * 2 * 4 / us * 1e-6);
    }
    om_debug_option(OM_OPT_ATTENTION_DEBUG, 0);
    return 0;
  }
  if (what == "groupm") {      // persistent GEMM: tile-walk group size vs throughput on the encoder's shapes
    const int64_t M = 131072;
    for (int gm : {8, 1, 2, 4, 16, 32}) {
      om_debug_option(OM_OPT_GEMM_GROUP_M, gm);
      printf("-- group_m = %d\n", gm);
      bench_gemm(OM_BF16, M, 2304, 768, 0);
      bench_gemm(OM_BF16, M, 768, 768, 0);
      bench_gemm(OM_BF16, M, 3072, 768, OM_ACT_GELU_ERF);
      bench_gemm(OM_BF16, M, 768, 3072, 0);
    }
    om_debug_option(OM_OPT_GEMM_GROUP_M, 8);
    return 0;
  }
  if (what == "scantrace") {     // tile phase timeline of the generation-7 index scan (first 8192 tiles of the last round)
    const int64_t N = argc > 2 ? atoll(argv[2]) : 2000000; const int Q = argc > 3 ? atoi(argv[3]) : 6980, d = 768, k = 1000;
    std::vector<float> hP = randn(1 << 22, 0.3f);
    float* dP = dalloc<float>((size_t)N * d);
    for (size_t o = 0; o < (size_t)N * d; o += hP.size()) CK(hipMemcpy(dP + o, hP.data(), std::min(hP.size(), (size_t)N * d - o) * 4, hipMemcpyHostToDevice));
    float* dQ = upload(randn((size_t)Q * d, 0.3f));
    bf16* dPb = dalloc<bf16>((size_t)N * d); float* dstats = dalloc<float>(2); CK(hipMemset(dstats, 0, 8));
    OMCK(om_index_to_f16(dP, N, d, dPb, dstats, nullptr));
    size_t wsb = om_sim_topk_workspace_bytes(Q, d, k); char* ws = dalloc<char>(wsb);
    float* dD = dalloc<float>((size_t)Q * k); int64_t* dI = dalloc<int64_t>((size_t)Q * k);
    OMCK(om_sim_topk(OM_SEARCH_F16_RESCORE, dQ, Q, dP, dPb, dstats, N, d, k, 0, dD, dI, ws, wsb, nullptr));
    const size_t nblk = 8192; unsigned long long* tr = dalloc<unsigned long long>(nblk * 32);
    for (int a = 4; a < std::max(argc, 5); ++a) {      // remaining arguments: OM_OPT_SCAN_GROWTH values to compare
      if (a < argc) om_debug_option(OM_OPT_SCAN_GROWTH, atoi(argv[a]));
      for (int rep = 0; rep < 2; ++rep) OMCK(om_sim_topk(OM_SEARCH_F16_RESCORE, dQ, Q, dP, dPb, dstats, N, d, k, 0, dD, dI, ws, wsb, nullptr));
      CK(hipDeviceSynchronize());
      auto u0 = std::chrono::steady_clock::now();
      for (int rep = 0; rep < 3; ++rep) OMCK(om_sim_topk(OM_SEARCH_F16_RESCORE, dQ, Q, dP, dPb, dstats, N, d, k, 0, dD, dI, ws, wsb, nullptr));
      CK(hipDeviceSynchronize());
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count() / 3;
      int64_t info[8] = {0}; om_sim_topk_info(info);
      printf("scan: N=%ld Q=%d growth=%s : %.2f ms/search  %.0f q/s  [rounds=%ld ovf=%ld list=%ld]\n", (long)N, Q, a < argc ? argv[a] : "default", ms,
             Q / ms * 1e3, (long)info[1], (long)info[2], (long)info[3]);
      CK(hipMemset(tr, 0, nblk * 32 * 8)); om_debug_gemm_trace(tr);
      OMCK(om_sim_topk(OM_SEARCH_F16_RESCORE, dQ, Q, dP, dPb, dstats, N, d, k, 0, dD, dI, ws, wsb, nullptr));
      CK(hipDeviceSynchronize()); om_debug_gemm_trace(nullptr);
      auto h = download(tr, nblk * 32);
      double wait = 0, init = 0, loop = 0, filt = 0, tot = 0; size_t n = 0;
      for (size_t b = 0; b < nblk; ++b) if (h[b * 32] && h[b * 32 + 28] && h[b * 32 + 15] && h[b * 32 + 3]) {
        wait += (double)(h[b * 32 + 1] - h[b * 32]); init += (double)(h[b * 32 + 3] - h[b * 32 + 1]);
        loop += (double)(h[b * 32 + 15] - h[b * 32 + 3]); filt += (double)(h[b * 32 + 28] - h[b * 32 + 15]); tot += (double)(h[b * 32 + 28] - h[b * 32]);
        ++n;
      }
      {
        double ph[6] = {0}; double surv = 0; size_t m = 0;
        for (size_t b = 0; b < nblk; ++b) if (h[b * 32 + 16] && h[b * 32 + 21] && h[b * 32 + 28]) {
          const unsigned long long* t = &h[b * 32];
          ph[0] += (double)(t[16] - t[15]); ph[1] += (double)(t[17] - t[16]); ph[2] += (double)(t[18] - t[17]);
          ph[3] += (double)(t[19] - t[18]); ph[4] += (double)(t[21] - t[19]); ph[5] += (double)(t[28] - t[21]); surv += (double)t[20]; ++m;
        }
        if (m) printf("   filter phase (continuous-ring scan), avg over %zu tiles: pending atomics + A(1) issue %.0f | filter rows 0-1 %.0f | rows 2-3 %.0f | "
                      "flush + pending reload %.0f | wait vmcnt(0) %.0f | B(1) issue %.0f ; survivors of wave 0 per tile %.1f\n",
                      m, ph[0] / m, ph[1] / m, ph[2] / m, ph[3] / m, ph[4] / m, ph[5] / m, surv / m);
      }
      if (n) printf("   last round, avg over %zu tiles: start+wait %.0f  init %.0f  K loop %.0f (MFMA time %d, x%.3f)  prefetch+filter %.0f  whole tile %.0f (memtime ticks)\n",
                    n, wait / n, init / n, loop / n, d * 32, loop / n / (d * 32.0), filt / n, tot / n);
    }
    return 0;
  }
  if (what == "shapes") {   // the encoder's own GEMM shapes at a small token count, every dtype
    for (int dt : {OM_F32, OM_BF16}) {
      test_gemm(dt, 1024, 2304, 768, true, false, OM_ACT_NONE, dt);
      test_gemm(dt, 1024, 768, 768, true, true, OM_ACT_NONE, dt);
      test_gemm(dt, 1024, 3072, 768, true, false, OM_ACT_GELU_ERF, dt);
      test_gemm(dt, 1024, 768, 3072, true, true, OM_ACT_NONE, dt);
    }
    printf("%s: %d failure(s)\n", g_fail ? "SELFTEST FAILED" : "SELFTEST PASSED", g_fail);
    return g_fail ? 1 : 0;
  }
  if (what == "layer") {    // the four contractions of one bert-base layer at the bench's token count
    const int64_t M = argc > 2 ? atoll(argv[2]) : 131072;
    bench_gemm(OM_BF16, M, 2304, 768, 0);
    bench_gemm(OM_BF16, M, 768, 768, 0);
    bench_gemm(OM_BF16, M, 3072, 768, OM_ACT_GELU_ERF);
    bench_gemm(OM_BF16, M, 768, 3072, 0);
    return 0;
  }
  if (what == "prof") {     // short run for rocprofv3 --pmc passes
    bench_gemm(OM_BF16, 32768, 768, 768, 0);
    bench_gemm(OM_BF16, 32768, 3072, 768, OM_ACT_GELU_ERF);
    bench_gemm(OM_BF16, 32768, 768, 3072, 0);
    bench_gemm(OM_BF16, 8192, 8192, 8192, 0);
    return 0;
  }
  if (what == "bench" || what == "full") {
    bench_gemm(OM_BF16, 32768, 2304, 768, 0);
    bench_gemm(OM_BF16, 32768, 768, 768, 0);
    bench_gemm(OM_BF16, 32768, 3072, 768, OM_ACT_GELU_ERF);
    bench_gemm(OM_BF16, 32768, 768, 3072, 0);
    bench_gemm(OM_BF16, 8192, 8192, 8192, 0);
    bench_gemm(OM_F32, 32768, 768, 768, 0);
    bench_gemm(OM_F32, 8192, 3072, 768, OM_ACT_GELU_ERF);
    bench_search(OM_SEARCH_F16_RESCORE, 2000000, 1024, 768, 1000);
    bench_search(OM_SEARCH_F32, 2000000, 1024, 768, 1000);
  }
  printf("%s: %d failure(s)\n", g_fail ? "SELFTEST FAILED" : "SELFTEST PASSED", g_fail);
  return g_fail ? 1 : 0;
}
