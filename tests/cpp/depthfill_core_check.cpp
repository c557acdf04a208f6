// Host-compiled check of K37: the definition of panovlm_amd/csrc/pvlm_depthfill_core.h (the stages, the median network, exp_neg, the bilateral, the uint16 conversion,
// the whole-image host loop and the host splat).  tests/test_depthfill_cpu.py compares them with tests/depthfill_ref.py without a GPU; tests/test_depthfill_gpu.py
// compares the device calls with them bit for bit.  TEST INFRASTRUCTURE ONLY.  Built with -ffp-contract=off.  With -DDEPTHFILL_CHECK_MAIN it is a stand-alone
// program (the form that runs under -fsanitize=address,undefined): the host loop on the odd shapes, single against batch, and every value finite and >= 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_depthfill_core.h"

namespace df = pvlm_depthfill;

extern "C" {

// Returns 0, or -1 for what the entry points refuse
int chk_depth_completion(int rows, int cols, int n_images, const unsigned short* in_u16, const float* in_f32, float max_depth, float* dense, unsigned short* u16,
                         int n_threads, long long* stats2) {
  if (rows <= 0 || cols <= 0 || n_images < 0 || (in_u16 != nullptr) == (in_f32 != nullptr) || (!dense && !u16) || !std::isfinite(max_depth) || !(max_depth > 0.f)) return -1;
  if (in_f32) for (size_t i = 0; i < (size_t)rows * cols * n_images; ++i) if (!df::input_ok(in_f32[i])) return -1;
  df::HostStats s;
  df::complete_host_batch(rows, cols, n_images, in_u16, in_f32, max_depth, dense, u16, (size_t)n_threads, &s);
  if (stats2) { stats2[0] = s.valid_in; stats2[1] = s.valid_out; }
  return 0;
}

int chk_depth_images(int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl, unsigned size, float max_depth,
                     unsigned short* depth_u16, int n_threads) {
  if (rows <= 0 || cols <= 0 || n_scans < 0 || !T_cl || !std::isfinite(max_depth) || !(max_depth > 0.f)) return -1;
  if (n_scans > 0 && first_point[0] != 0) return -1;
  for (int s = 0; s < n_scans; ++s) if (first_point[s + 1] < first_point[s]) return -1;
  df::depth_images_host(rows, cols, n_scans, first_point, xyz, T_cl, size, max_depth, depth_u16, (size_t)n_threads);
  return 0;
}

void chk_splat(int rows, int cols, long long n, const float* xyz, const double* T_cl, unsigned size, unsigned short* img) { df::splat_host(rows, cols, n, xyz, T_cl, size, img); }
void chk_exp_neg(long long n, const double* x, double* out) { for (long long i = 0; i < n; ++i) out[i] = df::exp_neg(x[i]); }
float chk_median25(const float* v) { float p[25]; std::memcpy(p, v, sizeof(p)); return df::median25(p); }
void chk_to_u16(long long n, const float* x, unsigned short* out) { for (long long i = 0; i < n; ++i) out[i] = df::to_u16(x[i]); }
int chk_reflect101(int i, int n) { return df::reflect101(i, n); }

}  // extern "C"

#if defined(DEPTHFILL_CHECK_MAIN)
namespace {
unsigned long long g_state = 7;
unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

// a sparse image of the tests' kind: a share of the pixels gets one of the boundary depths, the top fifth and a stripe stay empty
std::vector<unsigned short> sparse_image(int rows, int cols, unsigned per_mille) {
  static const float depths[10] = {2.f, 8.f, 15.f, 20.f, 30.f, 33.f, 39.99f, 45.f, 26.f / 256.f, 25.f / 256.f};
  std::vector<unsigned short> img((size_t)rows * cols, 0);
  for (int r = rows / 5; r < rows; ++r)
    for (int c = 0; c < cols; ++c)
      if (rnd() % 1000 < per_mille && !(c >= cols / 2 && c < cols / 2 + 3)) img[(size_t)r * cols + c] = (unsigned short)(depths[rnd() % 10] * 256.f);
  return img;
}
}  // namespace

int main() {
  const int shapes[][2] = {{96, 160}, {67, 131}, {5, 7}, {1, 9}, {9, 1}, {1, 1}, {33, 65}};
  int bad = 0;
  for (const auto& s : shapes) {
    const int rows = s[0], cols = s[1];
    const size_t n = (size_t)rows * cols;
    std::vector<unsigned short> in;
    for (int k = 0; k < 3; ++k) { const std::vector<unsigned short> one = sparse_image(rows, cols, k == 0 ? 10 : k == 1 ? 300 : 0); in.insert(in.end(), one.begin(), one.end()); }
    std::vector<float> dense(3 * n), single(n);
    std::vector<unsigned short> u16(3 * n), single16(n);
    long long st[2];
    if (chk_depth_completion(rows, cols, 3, in.data(), nullptr, 40.f, dense.data(), u16.data(), 3, st)) { std::printf("refused %d x %d\n", rows, cols); return 1; }
    long long filled = 0;
    for (int k = 0; k < 3; ++k) {
      chk_depth_completion(rows, cols, 1, in.data() + k * n, nullptr, 40.f, single.data(), single16.data(), 1, nullptr);
      if (std::memcmp(single.data(), dense.data() + k * n, n * sizeof(float)) || std::memcmp(single16.data(), u16.data() + k * n, n * 2)) { std::printf("batch != single at %d x %d image %d\n", rows, cols, k); ++bad; }
    }
    for (size_t i = 0; i < 3 * n; ++i) { if (!std::isfinite(dense[i]) || dense[i] < 0.f || dense[i] > 40.f) ++bad; filled += dense[i] > df::kValid; }
    std::printf("%3d x %3d: valid in %lld, valid out %lld (%lld)\n", rows, cols, st[0], st[1], filled);
    if (filled != st[1]) ++bad;
  }
  // exp_neg at its corners
  const double xs[] = {0.0, 1e-300, 0.3465735902799726, 0.34657359027997270, 1.0, 707.9999999999999, 708.0, 1e300};
  for (double x : xs) { const double got = df::exp_neg(x), want = std::exp(-x); if (x < 708.0 ? std::fabs(got - want) > std::ldexp(want, -50) : got != 0.0) { std::printf("exp_neg(%g) = %a, exp = %a\n", x, got, want); ++bad; } }
  std::printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
#endif
