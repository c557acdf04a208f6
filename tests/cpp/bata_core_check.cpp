// Host-compiled check of K44: the definition of panovlm_amd/csrc/pvlm_bata_core.h behind the host backend of panovlm_amd/host/pvlm_host_bata.hpp (the kernels' work
// done by loops, a dense host Cholesky in place of the library's solver).  tests/test_bata_cpu.py compares it with the independent numpy reference of
// tests/bata_ref.py without a GPU; tests/test_bata_gpu.py compares pvlm_transavg_bata with it.  With -DBATA_CHECK_MAIN it is a stand-alone program (the sanitizer
// build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_bata.hpp"

namespace bt = pvlm_bata;

extern "C" {

int chk_bata_group_size() { return bt::pg::kGroup; }

// Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, k > 0, -1 or -2; the outputs are written only when it is 0.
int chk_bata_solve(int n_cameras, int P, const int* first, const int* second, const double* dir, const double* scales0, double delta, int init_iteration, int inner_iteration,
                   int outer_iteration, double robust_threshold, double* centres, double* lud_centres, double* scales_out, int* info) {
  bt::Params prm;
  prm.delta = delta; prm.init_iteration = init_iteration; prm.inner_iteration = inner_iteration; prm.outer_iteration = outer_iteration; prm.robust_threshold = robust_threshold;
  return pvlm::bata_detail::SolveHost(n_cameras, P, first, second, dir, scales0, &prm, centres, lud_centres, scales_out, info);
}

}  // extern "C"

#ifdef BATA_CHECK_MAIN
// n cameras on a helix, each paired with its next 3 (exact unit directions, the true lengths as start scales, every seventh pair's direction reversed); with
// split = true the pairs across the middle are left out (two components: not positive definite).  Prints the result.
static int helix(int n, bool split) {
  std::vector<int> first, second; std::vector<double> dir, s0, pos((size_t)3 * n);
  for (int c = 0; c < n; ++c) { pos[3 * (size_t)c] = std::cos(0.7 * c) * 4; pos[3 * (size_t)c + 1] = std::sin(0.7 * c) * 4; pos[3 * (size_t)c + 2] = 0.1 * c; }
  for (int c = 0; c < n; ++c)
    for (int k = 1; k <= 3 && c + k < n; ++k) {
      if (split && c < n / 2 && c + k >= n / 2) continue;
      double d[3], len = 0;
      for (int a = 0; a < 3; ++a) { d[a] = pos[3 * (size_t)c + a] - pos[3 * (size_t)(c + k) + a]; len += d[a] * d[a]; }
      len = std::sqrt(len);
      const double sign = first.size() % 7 == 6 ? -1.0 : 1.0;
      first.push_back(c); second.push_back(c + k); s0.push_back(len);
      for (int a = 0; a < 3; ++a) dir.push_back(sign * d[a] / len);
    }
  const int P = (int)first.size();
  std::vector<double> out((size_t)3 * n, -7.0), lud((size_t)3 * n, -7.0), s((size_t)P, -7.0);
  int info = -7;
  const int rc = chk_bata_solve(n, P, first.data(), second.data(), dir.data(), s0.data(), 1e-6, 10, 10, 10, 0.1, out.data(), lud.data(), s.data(), &info);
  // the centres against the truth up to one common factor (fitted on camera 1) and camera 0's shift
  double err = 0;
  if (rc == 0 && info == 0 && n > 1) {
    double num = 0, den = 0;
    for (int a = 0; a < 3; ++a) { const double v = pos[3 + a] - pos[a]; num += out[3 + a] * v; den += v * v; }
    const double f = num / den;
    for (int c = 0; c < n; ++c) for (int a = 0; a < 3; ++a) err = std::fmax(err, std::fabs(out[3 * (size_t)c + a] - f * (pos[3 * (size_t)c + a] - pos[a])));
  }
  std::printf("n = %d pairs %d split %d: rc %d info %d untouched %d distance %.3e\n", n, P, split ? 1 : 0, rc, info, out[0] == -7.0 ? 1 : 0, err);
  if (split) return !(rc == 0 && info > 0 && out[0] == -7.0 && lud[0] == -7.0 && s[0] == -7.0);
  return !(rc == 0 && info == 0 && std::isfinite(err));
}
int main() { return helix(3, false) | helix(9, false) | helix(70, false) | helix(100, false) | helix(40, true); }      // 100 cameras: 294 pairs, a tree of two levels
#endif
