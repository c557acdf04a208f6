// Host-compiled check of K46: the definition of panovlm_amd/csrc/pvlm_transdir_core.h behind the host backend of panovlm_amd/host/pvlm_host_transdir.hpp (the
// kernels' work done by loops, a dense host Cholesky in place of the library's solver).  tests/test_transdir_cpu.py compares it with the independent numpy reference
// of tests/transdir_ref.py without a GPU; tests/test_transdir_gpu.py compares pvlm_transavg_chordal / pvlm_transavg_lud with it.  With -DTRANSDIR_CHECK_MAIN it is
// a stand-alone program (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_transdir.hpp"

namespace pg = pvlm_pairgraph;

static void put(const pg::Summary& s, double* summary5) {
  summary5[0] = s.initial_cost; summary5[1] = s.final_cost; summary5[2] = s.successful_steps; summary5[3] = s.unsuccessful_steps; summary5[4] = s.termination;
}

extern "C" {

int chk_transdir_group_size() { return pg::kGroup; }

// summary5: initial cost, final cost, accepted steps, rejected steps, termination.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
int chk_transdir_chordal(int F, int P, const int* first, const int* second, const double* dir, int origin, double* centres, double loss_a, int max_num_iterations,
                         double* summary5) {
  pg::Summary s;
  if (!summary5) return -1;
  const int rc = pvlm::transdir_detail::ChordalHost(F, P, first, second, dir, origin, centres, loss_a, max_num_iterations, &s);
  if (rc) return rc;
  put(s, summary5);
  return 0;
}

int chk_transdir_lud(int F, int P, const int* first, const int* second, const double* dir, double* scales, double* weight, int origin, double* centres, double upper_ratio,
                     double lower_ratio, int max_num_iterations, double* sum_e, double* summary5) {
  pg::Summary s;
  if (!summary5) return -1;
  const int rc = pvlm::transdir_detail::LudHost(F, P, first, second, dir, scales, weight, origin, centres, upper_ratio, lower_ratio, max_num_iterations, sum_e, &s);
  if (rc) return rc;
  put(s, summary5);
  return 0;
}

}  // extern "C"

#ifdef TRANSDIR_CHECK_MAIN
// a ring of n cameras, each paired with its next 3 (exact directions but one, which is turned; every third pair without a length); the start is the truth moved by
// a tenth of a metre per camera.  Runs the chordal problem and two LUD solves and prints the summaries
static int ring(int n) {
  std::vector<int> first, second; std::vector<double> dir, scales, pos((size_t)3 * n), x((size_t)3 * n);
  for (int c = 0; c < n; ++c) { pos[3 * (size_t)c] = std::cos(0.7 * c) * 4 - 4; pos[3 * (size_t)c + 1] = std::sin(0.7 * c) * 4; pos[3 * (size_t)c + 2] = 0.1 * c; }
  for (int c = 0; c < n; ++c)
    for (int k = 1; k <= 3 && c + k < n; ++k) {
      first.push_back(c); second.push_back(c + k);
      double d[3], len = 0;
      for (int a = 0; a < 3; ++a) { d[a] = pos[3 * (size_t)c + a] - pos[3 * (size_t)(c + k) + a]; len += d[a] * d[a]; }
      len = std::sqrt(len);
      if (first.size() == 2) { const double t = d[0]; d[0] = -d[1]; d[1] = t; }
      for (int a = 0; a < 3; ++a) dir.push_back(d[a] / len);
      scales.push_back(first.size() % 3 == 0 ? 1.0 : len);
    }
  const int P = (int)first.size();
  for (int c = 0; c < n; ++c) for (int a = 0; a < 3; ++a) x[3 * (size_t)c + a] = c == 0 ? 0.0 : pos[3 * (size_t)c + a] + 0.1 * std::sin(1.3 * c + a);
  std::vector<double> y(x), weight((size_t)P, 1.0);
  double sc[5] = {0, 0, 0, 0, 0}, sl[5] = {0, 0, 0, 0, 0}, sum_e = 0;
  int rc = chk_transdir_chordal(n, P, first.data(), second.data(), dir.data(), 0, x.data(), 0.5, 300, sc);
  for (int pass = 0; pass < 2; ++pass) rc |= chk_transdir_lud(n, P, first.data(), second.data(), dir.data(), scales.data(), weight.data(), 0, y.data(), 1.3, 0.9, 50, &sum_e, sl);
  std::printf("n = %d pairs %d: rc %d chordal %.6e -> %.6e steps %d + %d termination %d; lud %.6e -> %.6e steps %d + %d termination %d sum_e %.6e\n", n, P, rc, sc[0], sc[1],
              (int)sc[2], (int)sc[3], (int)sc[4], sl[0], sl[1], (int)sl[2], (int)sl[3], (int)sl[4], sum_e);
  return rc || !(sc[1] <= sc[0]) || !(sl[1] <= sl[0]);
}
int main() { return ring(1) | ring(3) | ring(9) | ring(70) | ring(300); }
#endif
