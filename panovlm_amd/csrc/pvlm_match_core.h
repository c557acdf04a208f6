// Statement of K33: the brute-force 2-NN SIFT matching of MatchSIFT (util/SIFT.cpp:130-162, the cv::cuda knnMatch(..., 2) branch) and the pair filter of
// SfM::MatchImagePairs (sfm/SfM.cpp:266-275).  Host / device: csrc/pvlm_match.hip wraps it in kernels, the host mirror compiles it for MatchSIFT and the host
// loop, and a host compile (tests/cpp/match_core_check.cpp) is what the CPU tests compare with numpy and the GPU tests compare with bit for bit.
// Compile with -ffp-contract=off: the only fused operations are the fmaf calls written here.
//
// The definition.  Descriptors are rows of 128 float.  d2(a, b): c = 0; for k = 0..127 ascending { t = a[k] - b[k]; c = fmaf(t, t, c); }.  distance = sqrtf(d2),
// correctly rounded.  2-NN of a query: the two train rows with the smallest (d2, train index), compared lexicographically (an exact tie goes to the lower index).
// Ratio test: distance0 < ratio * distance1 in float, strictly (util/SIFT.cpp:158).  Fewer than two train rows: no match (upstream reads raw_matches[i][1]
// out of bounds with one train row: the deliberate divergence documented in pvlm.h).  Pair filter: see pair_filter below.
// [recalled] This is the direct sum of squared differences a brute-force L2 matcher computes; the summation order of cv::cuda's and cv::BFMatcher's kernels is
// not pinned (there is no OpenCV build to pin it against).  The FLANN branch of MatchSIFT is approximate and not mirrored.
//
// The screening bound.  The fast path ranks train rows by s = (na + nb) - 2 dot with na, nb = norm2() of the rows and dot an fp32 fmaf chain over the 128
// products in some fixed order (the matrix core).  With u = 2^-24, g_n = n u / (1 - n u), N = |a|^2 + |b|^2 in real arithmetic:
//   |na_c - na| <= g_128 na, |nb_c - nb| <= g_128 nb  (128 roundings, all terms >= 0);  |dot_c - dot| <= g_128 sum |a_k b_k| <= g_128 N / 2;
//   t = fl(na_c + nb_c): <= u (1 + g_128) N;   s = fl(t - 2 dot_c) (one fmaf): <= u (|t| + 2 |dot_c|) <= 2 u (1 + g_129) N;
//   |s - sum (a_k - b_k)^2| <= (2 g_128 + 3 u (1 + g_129)) N <= g_131 * 2 N.
// screen_bound evaluates 264 u (na_c + nbmax_c) in float: N <= (na_c + nb_c) / (1 - g_128), two float roundings, 262.002 u -> 264 u covers them.
// The definition's own error: d2_c = D (1 + th), |th| <= g_130 (the difference, its square inside the fmaf, 128 accumulations; all terms >= 0).
// certified(): a train row outside the C screened candidates has s_j >= s_C, so D_j >= s_C - E and d2_c(j) >= (s_C - E)(1 - g_130); when that is strictly
// above the exact second-best d2 of the candidates, no outside row can enter or tie the exact top two.  lo2 = lo - lo 2^-16 with lo = fl(s_C - E):
// (1 - 2^-16)(1 + u) <= (1 - u)(1 - g_130), so the float evaluation stays below the real bound; lo < 2^-100 (where lo 2^-16 could be inexact) is not certified.
#pragma once
#include <cmath>
#include <cstdint>
#if !defined(__HIPCC__) && defined(__x86_64__)
#include <immintrin.h>
#endif

#ifndef PVLM_EQ_UD
#if defined(__HIPCC__)
#define PVLM_EQ_UD __host__ __device__ __forceinline__
#else
#define PVLM_EQ_UD inline
#endif
#endif

namespace pvlm_matching {

constexpr int kDim = 128;      // floats per descriptor
constexpr int kCand = 4;       // C: screened candidates per query

PVLM_EQ_UD float fma_f(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmaf_rn(a, b, c);
#else
  return __builtin_fmaf(a, b, c);
#endif
}
PVLM_EQ_UD float sqrt_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ::sqrtf(x);              // correctly rounded (the fast __fsqrt_rn intrinsic is not)
#else
  return __builtin_sqrtf(x);
#endif
}
PVLM_EQ_UD float inf_f() { return __builtin_huge_valf(); }

PVLM_EQ_UD float d2_exact(const float* a, const float* b) {
  float c = 0.0f;
  for (int k = 0; k < kDim; ++k) { const float t = a[k] - b[k]; c = fma_f(t, t, c); }
  return c;
}
// the squared norm the screening uses: c = fmaf(a[k], a[k], c), k ascending
PVLM_EQ_UD float norm2(const float* a) {
  float c = 0.0f;
  for (int k = 0; k < kDim; ++k) c = fma_f(a[k], a[k], c);
  return c;
}

struct Knn2 { float d2[2]; int idx[2]; };
PVLM_EQ_UD Knn2 knn2_empty() { Knn2 r; r.d2[0] = r.d2[1] = inf_f(); r.idx[0] = r.idx[1] = -1; return r; }
PVLM_EQ_UD bool lex_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }
// (d2, j) into the two smallest; j >= 0.  An empty slot (inf, -1) loses to every finite d2 and to (inf, j) by the explicit test.
PVLM_EQ_UD void knn2_push(Knn2& r, float d2, int j) {
  if (r.idx[1] >= 0 && !lex_less(d2, j, r.d2[1], r.idx[1])) return;
  if (r.idx[0] < 0 || lex_less(d2, j, r.d2[0], r.idx[0])) { r.d2[1] = r.d2[0]; r.idx[1] = r.idx[0]; r.d2[0] = d2; r.idx[0] = j; }
  else { r.d2[1] = d2; r.idx[1] = j; }
}
PVLM_EQ_UD Knn2 knn2_row(const float* a, const float* B, int n2) {
  Knn2 r = knn2_empty();
  for (int j = 0; j < n2; ++j) knn2_push(r, d2_exact(a, B + (size_t)j * kDim), j);
  return r;
}
// the ratio test on the two distances; false with fewer than two neighbours
PVLM_EQ_UD bool ratio_keep(const Knn2& r, float ratio, float* distance0) {
  if (r.idx[1] < 0) return false;
  const float d0 = sqrt_f(r.d2[0]), d1 = sqrt_f(r.d2[1]);
  *distance0 = d0;
  const float rhs = ratio * d1;
  return d0 < rhs;
}
// it->distance < 0.8 * it_max->distance: the product is a double (sfm/SfM.cpp:272)
PVLM_EQ_UD bool filter_keep(float distance, float dmax) { return (double)distance < 0.8 * (double)dmax; }

PVLM_EQ_UD float screen_value(float na, float nb, float dot) { return fma_f(-2.0f, dot, na + nb); }
PVLM_EQ_UD float screen_bound(float na, float nb_max) { return (na + nb_max) * (264.0f * 0x1p-24f); }
PVLM_EQ_UD bool certified(float s_c, float E, float d2_second) {
  if (!(E < inf_f())) return false;
  const float lo = s_c - E;
  if (!(lo >= 0x1p-100f)) return false;
  const float lo2 = lo - lo * 0x1p-16f;
  return lo2 > d2_second;
}

#if !defined(__HIPCC__)
// ---- host loops (the host mirror's MatchSIFT, the bench's baseline, the tests' reference compile) ----
struct Match { int query, train; float distance; };

// Eight train rows at a time, transposed once per block (bt[k][v]) and shared by all queries, so that the eight chains of a query are the lanes of one
// 8-wide fused multiply-add per k: each lane is still the definition's chain in the definition's order, and a query still meets the rows in ascending index.
// chains8: c[v] = d2 of query row a against train row v of the transposed block
inline void chains8_scalar(const float* a, const float* bt, float* c) {
  for (int v = 0; v < 8; ++v) c[v] = 0.0f;
  for (int k = 0; k < kDim; ++k)
    for (int v = 0; v < 8; ++v) { const float t = a[k] - bt[k * 8 + v]; c[v] = __builtin_fmaf(t, t, c[v]); }
}
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) inline void chains8_avx2(const float* a, const float* bt, float* c) {
  __m256 acc = _mm256_setzero_ps();
  for (int k = 0; k < kDim; ++k) { const __m256 t = _mm256_sub_ps(_mm256_set1_ps(a[k]), _mm256_load_ps(bt + k * 8)); acc = _mm256_fmadd_ps(t, t, acc); }
  _mm256_store_ps(c, acc);
}
#endif
inline void knn2_rows(const float* A, int q_begin, int q_end, const float* B, int n2, Knn2* out) {
#if defined(__x86_64__)
  const bool wide = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#endif
  for (int i = q_begin; i < q_end; ++i) out[i] = knn2_empty();
  alignas(32) float bt[kDim * 8];
  alignas(32) float c[8];
  int j = 0;
  for (; j + 8 <= n2; j += 8) {
    for (int v = 0; v < 8; ++v)
      for (int k = 0; k < kDim; ++k) bt[k * 8 + v] = B[(size_t)(j + v) * kDim + k];
    for (int i = q_begin; i < q_end; ++i) {
#if defined(__x86_64__)
      if (wide) chains8_avx2(A + (size_t)i * kDim, bt, c); else
#endif
      chains8_scalar(A + (size_t)i * kDim, bt, c);
      for (int v = 0; v < 8; ++v) knn2_push(out[i], c[v], j + v);
    }
  }
  for (; j < n2; ++j)
    for (int i = q_begin; i < q_end; ++i) knn2_push(out[i], d2_exact(A + (size_t)i * kDim, B + (size_t)j * kDim), j);
}

// the pair filter of sfm/SfM.cpp:266-275 on the ratio-test matches of one pair, in place; returns whether the pair survives.
// matches_threshold >= 0 (a negative one is PVLM_ERR_ARG at the entry points: upstream's first comparison converts it to size_t and drops every pair)
template <class Vec>
inline bool pair_filter(Vec& matches, int matches_threshold) {
  if ((long long)matches.size() < (long long)matches_threshold) { matches.clear(); return false; }
  float dmax = 0.0f;
  for (const Match& m : matches) if (m.distance > dmax) dmax = m.distance;
  size_t n = 0;
  for (size_t i = 0; i < matches.size(); ++i) if (filter_keep(matches[i].distance, dmax)) matches[n++] = matches[i];
  matches.resize(n);
  if ((long long)n < (long long)matches_threshold) { matches.clear(); return false; }
  return true;
}
#endif

}  // namespace pvlm_matching
