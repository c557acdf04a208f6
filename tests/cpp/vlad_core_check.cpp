// Host-compiled check of K35: the definition of panovlm_amd/csrc/pvlm_vlad_core.h (nearest alive centre, k-means with the chunked fp64 means, the three embeddings,
// root5, the similarity chain and the neighbour order) through the host loops of panovlm_amd/host/pvlm_host_vlad.hpp.  tests/test_vlad_cpu.py compares them with
// tests/vlad_ref.py without a GPU; tests/test_vlad_gpu.py compares the device calls with them bit for bit.  TEST INFRASTRUCTURE ONLY.  Built with -ffp-contract=off.
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_vlad.hpp"

using namespace pvlm::vlad_detail;

namespace {
std::vector<const float*> frame_ptrs(int n_frames, const int* rows, const float* desc) {
  std::vector<const float*> ptr((size_t)n_frames);
  size_t at = 0;
  for (int f = 0; f < n_frames; ++f) { ptr[(size_t)f] = desc + at * kDim; at += (size_t)rows[f]; }
  return ptr;
}
}  // namespace

extern "C" {

int chk_vlad_sum_chunk() { return pvlm_vlad::kSumChunk; }

// desc: the frames' rows one frame after the other.  Returns 0, or -1 (PVLM_ERR_ARG).
int chk_vlad_kmeans(int n_frames, const int* rows, const float* desc, int n_train, const int* train_frames, int book_size, int max_iterations, const long long* init_rows,
                    int n_threads, float* codebook, unsigned char* alive, int* assign, int* iterations, int* dead_centres) {
  const std::vector<const float*> ptr = frame_ptrs(n_frames, rows, desc);
  return KmeansHost(n_frames, ptr.data(), rows, n_train, train_frames, book_size, max_iterations, init_rows, (size_t)n_threads, codebook, alive, assign, iterations, dead_centres);
}

int chk_vlad_embed(int n_frames, const int* rows, const float* desc, int book_size, const float* codebook, const unsigned char* alive_or_null, int normalization, int n_threads,
                   float* out) {
  const std::vector<const float*> ptr = frame_ptrs(n_frames, rows, desc);
  return EmbedHost(n_frames, ptr.data(), rows, book_size, codebook, alive_or_null, normalization, (size_t)n_threads, out);
}

int chk_vlad_neighbors(const float* vlad, int n, int book_size, int neighbor_size, int n_threads, int* neighbors, double* sim) {
  return NeighborsHost(vlad, n, book_size, neighbor_size, (size_t)n_threads, neighbors, sim);
}

double chk_root5(double x) { return pvlm_vlad::root5(x); }

// (float)root5((double)x) against (float)pow((double)x, 0.2) for every non-negative finite float: the number that differ and the largest difference in float ulps
void chk_root5_sweep(int n_threads, long long* differing, int* max_ulp) {
  const uint32_t end = 0x7f800000u, step = 1u << 20;
  std::atomic<uint32_t> next{0};
  std::atomic<long long> diff{0};
  std::atomic<int> worst{0};
  pvlm_run_workers((size_t)std::max(n_threads, 1), [&]() {
    long long d = 0; int w = 0;
    for (uint32_t a = next.fetch_add(step); a < end; a = next.fetch_add(step))
      for (uint32_t b = a; b < a + step && b < end; ++b) {
        float x; std::memcpy(&x, &b, 4);
        const float got = (float)pvlm_vlad::root5((double)x), want = (float)std::pow((double)x, 0.2);
        if (got != want) {
          uint32_t gb, wb; std::memcpy(&gb, &got, 4); std::memcpy(&wb, &want, 4);
          ++d; w = std::max(w, (int)std::min<uint32_t>(gb > wb ? gb - wb : wb - gb, 1u << 30));
        }
      }
    diff += d;
    int cur = worst.load();
    while (w > cur && !worst.compare_exchange_weak(cur, w)) {}
  });
  *differing = diff.load(); *max_ulp = worst.load();
}

}  // extern "C"
