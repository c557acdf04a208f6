// pvlm_host_vlad.hpp — K35 on the host: the k-means codebook, the VLAD embedding and the neighbour lists of sfm/VLAD.cpp over the frames' descriptor arrays, on the
// host compile of csrc/pvlm_vlad_core.h, spread over the worker pool.  It serves pvlm::InitImagePairsHost (the baseline tools/vlad_bench.py times) and the tests'
// reference (tests/cpp/vlad_core_check.cpp).  Not installed; not part of the interface.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../csrc/pvlm_vlad_core.h"

namespace pvlm {
namespace vlad_detail {

using pvlm_vlad::kDim;

// the concatenation of the train frames' rows, in list order
struct TrainRows {
  std::vector<const float*> base; std::vector<long long> start;       // per train frame; start has one more entry: the row count
  TrainRows(const float* const* desc, const int* rows, int n_train, const int* train_frames) {
    start.push_back(0);
    for (int t = 0; t < n_train; ++t) { base.push_back(desc[train_frames[t]]); start.push_back(start.back() + rows[train_frames[t]]); }
  }
  long long size() const { return start.back(); }
  const float* operator()(long long i) const {
    const size_t t = (size_t)(std::upper_bound(start.begin(), start.end(), i) - start.begin()) - 1;
    return base[t] + (size_t)(i - start[t]) * kDim;
  }
};

// the argument rules of pvlm_vlad_kmeans; 0 or -1 (PVLM_ERR_ARG)
inline int CheckKmeansArgs(int n_frames, const int* rows, int n_train, const int* train_frames, int book_size, int max_iterations, const long long* init_rows) {
  if (book_size < 1 || book_size > pvlm_vlad::kMaxBook || max_iterations < 0 || n_train < 0) return -1;
  long long n = 0;
  for (int t = 0; t < n_train; ++t) { if (train_frames[t] < 0 || train_frames[t] >= n_frames) return -1; n += rows[train_frames[t]]; }
  if ((long long)book_size > n) return -1;
  for (int c = 0; c < book_size; ++c) if (init_rows[c] < 0 || init_rows[c] >= n) return -1;
  return 0;
}

inline int KmeansHost(int n_frames, const float* const* desc, const int* rows, int n_train, const int* train_frames, int book_size, int max_iterations,
                      const long long* init_rows, size_t n_threads, float* codebook, unsigned char* alive, int* assign_or_null, int* iterations, int* dead_centres) {
  if (CheckKmeansArgs(n_frames, rows, n_train, train_frames, book_size, max_iterations, init_rows)) return -1;
  const TrainRows R(desc, rows, n_train, train_frames);
  std::vector<int> own;
  int* assign = assign_or_null;
  if (!assign) { own.resize((size_t)R.size()); assign = own.data(); }
  const int it = pvlm_vlad::kmeans(R, R.size(), book_size, max_iterations, init_rows, n_threads, codebook, alive, assign);
  if (iterations) *iterations = it;
  if (dead_centres) { *dead_centres = 0; for (int c = 0; c < book_size; ++c) *dead_centres += alive[c] ? 0 : 1; }
  return 0;
}

// one k-means pass's assignment alone (what the bench times on the host): nearest alive centre of every training row
inline void AssignHost(const float* const* desc, const int* rows, int n_train, const int* train_frames, int book_size, const float* codebook, const unsigned char* alive,
                       size_t n_threads, int* nearest) {
  const TrainRows R(desc, rows, n_train, train_frames);
  pvlm_vlad::assign_rows(R, R.size(), pvlm_vlad::pack_alive(codebook, alive, book_size), n_threads, nearest);
}

// the argument rules of pvlm_vlad_embed on the codebook
inline int CheckEmbedArgs(int book_size, const float* codebook, const unsigned char* alive_or_null, int normalization) {
  if (book_size < 1 || book_size > pvlm_vlad::kMaxBook || normalization < 0 || normalization > 2) return -1;
  for (int c = 0; c < book_size; ++c)
    if (!alive_or_null || alive_or_null[c])
      for (int k = 0; k < kDim; ++k) if (!std::isfinite(codebook[(size_t)c * kDim + k])) return -1;
  return 0;
}

// out: n_frames x 128 book_size
inline int EmbedHost(int n_frames, const float* const* desc, const int* rows, int book_size, const float* codebook, const unsigned char* alive_or_null, int normalization,
                     size_t n_threads, float* out) {
  if (CheckEmbedArgs(book_size, codebook, alive_or_null, normalization)) return -1;
  const pvlm_vlad::Packed P = pvlm_vlad::pack_alive(codebook, alive_or_null, book_size);
  const size_t D = (size_t)kDim * (size_t)book_size;
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads, (size_t)std::max(n_frames, 1))), [&]() {
    for (int f = next++; f < n_frames; f = next++) pvlm_vlad::embed_frame(desc[f], rows[f], codebook, P, book_size, normalization, out + (size_t)f * D);
  });
  return 0;
}

// neighbors: n x min(neighbor_size, n); sim_or_null: n x n
inline int NeighborsHost(const float* vlad, int n, int book_size, int neighbor_size, size_t n_threads, int* neighbors, double* sim_or_null) {
  if (neighbor_size < 1) return -1;
  std::vector<double> own;
  double* sim = sim_or_null;
  if (!sim) { own.resize((size_t)n * (size_t)n); sim = own.data(); }
  pvlm_vlad::neighbors(vlad, n, (size_t)kDim * (size_t)book_size, neighbor_size, n_threads, neighbors, sim);
  return 0;
}

// SplitMix64: the seeded generator of the mirror's draws (upstream: an unseeded std::mt19937; there is nothing to be equal to)
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
};
// `count` distinct values of [0, n), unsorted (util/Tools.h CreateRandomArray): the first `count` places of a Fisher-Yates shuffle
inline std::vector<long long> DrawDistinct(long long count, long long n, Rng& rng) {
  std::vector<long long> v((size_t)n);
  for (long long i = 0; i < n; ++i) v[(size_t)i] = i;
  count = std::min(count, n);
  for (long long i = 0; i < count; ++i) { const long long j = i + (long long)(rng.next() % (uint64_t)(n - i)); std::swap(v[(size_t)i], v[(size_t)j]); }
  v.resize((size_t)count);
  return v;
}

}  // namespace vlad_detail
}  // namespace pvlm
