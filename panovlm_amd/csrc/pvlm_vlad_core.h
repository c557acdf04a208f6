// Statement of K35: the VLAD image retrieval of sfm/VLAD.cpp (Kmeans :46-95, ComputeVLADEmbedding :97-154, FindNeighbors :156-183) that SfM::InitImagePairs
// (sfm/SfM.cpp:74-97) turns into image pairs.  Host / device: csrc/pvlm_vlad.hip wraps it in kernels, the host mirror compiles the host loops below for
// InitImagePairsHost, and a host compile (tests/cpp/vlad_core_check.cpp) is what the CPU tests compare with numpy and the GPU tests compare with bit for bit.
// Compile with -ffp-contract=off: the only fused operations are the fmaf calls of pvlm_match_core.h.
//
// [recalled] Upstream leaves every summation to OpenCV (cv::BFMatcher::match for the nearest centre, Mat += and Mat /= for the means and the blocks, cv::norm for
// the norms, Mat::dot for the similarity); their orders are not pinned (there is no OpenCV build to pin them against).  This file fixes its own orders.
//
// Nearest centre.  Of the ALIVE centres the one with the smallest (d2_exact(row, centre), centre index), lexicographically (pvlm_matching::lex_less).  The alive
// centres are handed around packed in ascending index order with an index map, so the packed order is the index order and ties survive the packing.
//
// k-means.  assign[i] = 0 for every training row (upstream's resize(rows, 0) is part of its "changed" test); the initial centres are copies of the training rows
// init_rows names.  A pass: changed = false; every row gets its nearest alive centre (changed when that differs from assign[i]); every alive centre is recomputed.
// Passes repeat while changed and fewer than max_iterations have run.  Mean of a centre with count > 0 members: (float)(S_k / (double)count) per component, S_k an
// fp64 sum in a fixed order: members in ascending training-row order, cut into runs of kSumChunk = 256 members, every run an ascending chain from 0.0, the run sums
// added in ascending order from 0.0.  (For integer-valued descriptors the sum is exact whatever the order.)  Deliberate divergence: upstream accumulates in float.
// A centre with count == 0 is DEAD: alive = 0, its codebook row is zeros, it is never a candidate again, its VLAD block stays zero (upstream: 0/0 = NaN, never
// chosen by a comparison-based search: the same outcome, stated).  max_iterations == 0 returns the initial rows.
//
// Embedding of a frame, rows in ascending keypoint order: c = nearest alive centre; r_k = row[k] - centre[k] in float.  Type 2: n = sqrt(sum (double)r_k^2), an
// fp64 chain with k ascending; n == 0: the row contributes nothing (divergence: upstream's 0/0 makes the frame's whole vector NaN); else r_k = (float)((double)r_k
// / n).  block[c][k] += r_k in float, rows ascending.  Per block: type 0 sign * sqrtf(|v|); type 1 (float)((double)v / norm(block)), the norm the fp64 chain above,
// a zero block stays zero (divergence); type 2 sign * (float)root5((double)|v|).  Whole vector: N = sqrt(sum over blocks of the block sums), a block sum the
// ascending fp64 chain of its 128 squares from 0.0, the block sums added in ascending order from 0.0; v = (float)((double)v / N); a zero vector stays zero
// (divergence: upstream gives NaN for a frame without descriptors).
//
// root5(x), x > 0 finite and normal: the fifth root in fp64 by IEEE + * / only, so that host and device give the same bits.  x = m 2^e with m in [0.5, 1);
// e = 5 q + r with r in 0..4; m' = m 2^r in [0.5, 16); y = 0.8 + 0.065 m'; kRoot5Steps = 6 Newton steps y <- (4 y + m' / y^4) / 5 (y^4 = (y y)(y y)); result
// y 2^q.  Measured against (float)pow((double)x, 0.2) of glibc over every non-negative finite float (tests/cpp/vlad_core_check.cpp, chk_root5_sweep; 2 139 095 040
// values): 3 floats differ, each by one float ulp.
//
// Neighbours.  sim(i, j) = the fp64 chain s = s + (double)v_i[k] * (double)v_j[k] over all 128 * book_size components, k ascending, from 0.0.  The products are
// exact (two 24-bit significands), so the chain is symmetric in i and j.  Row i lists the first min(neighbor_size, n) frames in ascending (-sim, index); the frame
// itself is included wherever it lands (upstream does the same; InitImagePairs skips it).
#pragma once
#include <cstring>
#if !defined(__HIPCC__)
#include <algorithm>
#include <atomic>
#include <vector>

#include "pvlm_workers.h"
#endif

#include "pvlm_match_core.h"

namespace pvlm_vlad {

using pvlm_matching::kDim;
constexpr int kSumChunk = 256;        // members per run of a centre's fp64 sum
constexpr int kRoot5Steps = 6;
constexpr int kMaxBook = 4096;        // the entry points' limit on book_size (the grouping keeps one counter per (tile, centre))

PVLM_EQ_UD double sqrt_d(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ::sqrt(x);                   // fp64 square root: correctly rounded on the device
#else
  return __builtin_sqrt(x);
#endif
}

PVLM_EQ_UD double root5(double x) {
  if (!(x > 0.0)) return 0.0;
  unsigned long long b; __builtin_memcpy(&b, &x, 8);
  const int e = (int)((b >> 52) & 0x7ff) - 1022;                      // x = m 2^e, m in [0.5, 1)
  int q = e / 5, r = e - 5 * q;
  if (r < 0) { r += 5; q -= 1; }
  unsigned long long mb = (b & 0x000fffffffffffffull) | ((unsigned long long)(1022 + r) << 52);
  double m; __builtin_memcpy(&m, &mb, 8);                             // m' = m 2^r in [0.5, 16)
  double y = 0.8 + 0.065 * m;
  for (int i = 0; i < kRoot5Steps; ++i) { const double y2 = y * y; y = (4.0 * y + m / (y2 * y2)) / 5.0; }
  const unsigned long long sb = (unsigned long long)(1023 + q) << 52;
  double s; __builtin_memcpy(&s, &sb, 8);
  return y * s;
}

// the nearest of n_alive packed centres: its packed index (-1 when there is none)
PVLM_EQ_UD int nearest_packed(const float* row, const float* packed, int n_alive) {
  int best = -1; float bd = pvlm_matching::inf_f();
  for (int c = 0; c < n_alive; ++c) {
    const float d = pvlm_matching::d2_exact(row, packed + (size_t)c * kDim);
    if (best < 0 || pvlm_matching::lex_less(d, c, bd, best)) { bd = d; best = c; }
  }
  return best;
}

// the ascending fp64 chain of the squares of r[0..127]
PVLM_EQ_UD double sq_chain(const float* r) {
  double s = 0.0;
  for (int k = 0; k < kDim; ++k) { const double d = (double)r[k]; s = s + d * d; }
  return s;
}

// the normalised residual component of a row against its centre (type 2: n = sqrt(sq_chain(residual)); other types: n is ignored)
PVLM_EQ_UD float residual_k(float x, float c, int type, double n) {
  float r = x - c;
  if (type == 2) r = (float)((double)r / n);
  return r;
}

// the per-block step on one component (a zero stays what it is); bn = sqrt(sq_chain(block)) for type 1
PVLM_EQ_UD float block_step(float v, int type, double bn) {
  if (v == 0.0f) return v;
  if (type == 0) return v > 0.0f ? pvlm_matching::sqrt_f(v) : -pvlm_matching::sqrt_f(-v);
  if (type == 1) return bn == 0.0 ? v : (float)((double)v / bn);
  return v > 0.0f ? (float)root5((double)v) : -(float)root5((double)-v);
}

// neighbour order: (-sim, index) ascending
PVLM_EQ_UD bool sim_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

#if !defined(__HIPCC__)
// ---- host loops (InitImagePairsHost, the bench's baseline, the tests' reference compile) ----
struct Packed { std::vector<float> rows; std::vector<int> map; };     // the alive centres in ascending index order, and their indices
inline Packed pack_alive(const float* codebook, const unsigned char* alive, int book_size) {
  Packed p;
  for (int c = 0; c < book_size; ++c)
    if (!alive || alive[c]) { p.map.push_back(c); p.rows.insert(p.rows.end(), codebook + (size_t)c * kDim, codebook + (size_t)(c + 1) * kDim); }
  return p;
}

// nearest[i] = the nearest alive centre of row_at(i), i in [0, n), the rows spread over the worker pool
template <class RowAt>
inline void assign_rows(const RowAt& row_at, long long n, const Packed& P, size_t n_threads, int* nearest) {
  const int na = (int)P.map.size();
  std::atomic<long long> next{0};
  const long long step = 256;
  pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads, (size_t)((n + step - 1) / step) + 1)), [&]() {
    for (long long a = next.fetch_add(step); a < n; a = next.fetch_add(step))
      for (long long i = a; i < std::min(n, a + step); ++i) { const int c = nearest_packed(row_at(i), P.rows.data(), na); nearest[i] = c < 0 ? -1 : P.map[(size_t)c]; }
  });
}

// the means of the alive centres from the assignment; a centre without members dies
template <class RowAt>
inline void update_centres(const RowAt& row_at, long long n, const int* assign, int book_size, float* codebook, unsigned char* alive) {
  std::vector<std::vector<long long>> members((size_t)book_size);
  for (long long i = 0; i < n; ++i) members[(size_t)assign[i]].push_back(i);
  for (int c = 0; c < book_size; ++c) {
    if (!alive[c]) continue;
    const std::vector<long long>& M = members[(size_t)c];
    float* out = codebook + (size_t)c * kDim;
    if (M.empty()) { alive[c] = 0; for (int k = 0; k < kDim; ++k) out[k] = 0.0f; continue; }
    double total[kDim];
    for (int k = 0; k < kDim; ++k) total[k] = 0.0;
    for (size_t a = 0; a < M.size(); a += (size_t)kSumChunk) {
      double run[kDim];
      for (int k = 0; k < kDim; ++k) run[k] = 0.0;
      for (size_t m = a; m < std::min(M.size(), a + (size_t)kSumChunk); ++m) { const float* r = row_at(M[m]); for (int k = 0; k < kDim; ++k) run[k] = run[k] + (double)r[k]; }
      for (int k = 0; k < kDim; ++k) total[k] = total[k] + run[k];
    }
    for (int k = 0; k < kDim; ++k) out[k] = (float)(total[k] / (double)M.size());
  }
}

// k-means over n rows.  codebook: book_size x 128; alive: book_size; assign: n.  Returns the passes run.
template <class RowAt>
inline int kmeans(const RowAt& row_at, long long n, int book_size, int max_iterations, const long long* init_rows, size_t n_threads, float* codebook, unsigned char* alive,
                  int* assign) {
  for (long long i = 0; i < n; ++i) assign[i] = 0;
  for (int c = 0; c < book_size; ++c) { alive[c] = 1; std::memcpy(codebook + (size_t)c * kDim, row_at(init_rows[c]), kDim * sizeof(float)); }
  std::vector<int> nearest((size_t)std::max<long long>(n, 1));
  bool changed = true; int iter = 0;
  for (; iter < max_iterations && changed; ++iter) {
    changed = false;
    const Packed P = pack_alive(codebook, alive, book_size);
    assign_rows(row_at, n, P, n_threads, nearest.data());
    for (long long i = 0; i < n; ++i) if (nearest[(size_t)i] != assign[i]) { assign[i] = nearest[(size_t)i]; changed = true; }
    update_centres(row_at, n, assign, book_size, codebook, alive);
  }
  return iter;
}

// the VLAD vector of one frame (out: 128 * book_size floats)
inline void embed_frame(const float* rows, int n, const float* codebook, const Packed& P, int book_size, int type, float* out) {
  const size_t D = (size_t)kDim * (size_t)book_size;
  for (size_t k = 0; k < D; ++k) out[k] = 0.0f;
  const int na = (int)P.map.size();
  for (int i = 0; i < n; ++i) {
    const float* row = rows + (size_t)i * kDim;
    const int pc = nearest_packed(row, P.rows.data(), na);
    if (pc < 0) continue;
    const int c = P.map[(size_t)pc];
    const float* cen = codebook + (size_t)c * kDim;
    double nrm = 1.0;
    if (type == 2) {
      float r[kDim];
      for (int k = 0; k < kDim; ++k) r[k] = row[k] - cen[k];
      nrm = sqrt_d(sq_chain(r));
      if (nrm == 0.0) continue;
    }
    float* blk = out + (size_t)c * kDim;
    for (int k = 0; k < kDim; ++k) blk[k] += residual_k(row[k], cen[k], type, nrm);
  }
  double total = 0.0;
  for (int c = 0; c < book_size; ++c) {
    float* blk = out + (size_t)c * kDim;
    const double bn = type == 1 ? sqrt_d(sq_chain(blk)) : 0.0;
    for (int k = 0; k < kDim; ++k) blk[k] = block_step(blk[k], type, bn);
    total = total + sq_chain(blk);
  }
  const double N = sqrt_d(total);
  if (N == 0.0) return;
  for (size_t k = 0; k < D; ++k) out[k] = (float)((double)out[k] / N);
}

inline double sim_chain(const float* a, const float* b, size_t D) {
  double s = 0.0;
  for (size_t k = 0; k < D; ++k) s = s + (double)a[k] * (double)b[k];
  return s;
}

// sim: n x n (both triangles written from one evaluation); neighbors: n x min(neighbor_size, n)
inline void neighbors(const float* vlad, int n, size_t D, int neighbor_size, size_t n_threads, int* out, double* sim) {
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads, (size_t)std::max(n, 1))), [&]() {
    for (int i = next++; i < n; i = next++)
      for (int j = i; j < n; ++j) { const double s = sim_chain(vlad + (size_t)i * D, vlad + (size_t)j * D, D); sim[(size_t)i * n + j] = s; sim[(size_t)j * n + i] = s; }
  });
  const int m = std::min(neighbor_size, n);
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) order[(size_t)j] = j;
    const double* s = sim + (size_t)i * n;
    std::sort(order.begin(), order.end(), [s](int a, int b) { return sim_before(s[a], a, s[b], b); });
    for (int k = 0; k < m; ++k) out[(size_t)i * m + k] = order[(size_t)k];
  }
}
#endif

}  // namespace pvlm_vlad
