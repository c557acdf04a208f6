// Host-compiled check of K42: the definition of panovlm_amd/csrc/pvlm_transavg_core.h behind the host backend of panovlm_amd/host/pvlm_host_transavg.hpp (the kernels'
// work done by loops, a dense host Cholesky in place of the library's solver).  tests/test_transavg_cpu.py compares it with the independent numpy reference of
// tests/transavg_ref.py without a GPU; tests/test_transavg_gpu.py compares pvlm_transavg_solve / pvlm_transavg_dlt with it.  With -DTRANSAVG_CHECK_MAIN it is a
// stand-alone program (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_transavg.hpp"

namespace ta = pvlm_transavg;

extern "C" {

int chk_transavg_group_size() { return ta::kGroup; }

// Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, or k > 0 when the system is not positive definite (out untouched).
int chk_transavg_dlt(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* out, int* info) {
  return pvlm::transavg_detail::DltHost(F, P, first, second, R, t21, out, info);
}

// summary5: initial cost, final cost, accepted steps, rejected steps, termination.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
int chk_transavg_solve(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* scales, int origin, double* translations, double* weight,
                       double loss_a, double upper_ratio, double lower_ratio, int max_num_iterations, double* summary5) {
  ta::Summary s;
  if (!summary5) return -1;
  const int rc = pvlm::transavg_detail::SolveHost(F, P, first, second, R, t21, scales, origin, translations, weight, loss_a, upper_ratio, lower_ratio, max_num_iterations, &s);
  if (rc) return rc;
  summary5[0] = s.initial_cost; summary5[1] = s.final_cost; summary5[2] = s.successful_steps; summary5[3] = s.unsuccessful_steps; summary5[4] = s.termination;
  return 0;
}

}  // extern "C"

#ifdef TRANSAVG_CHECK_MAIN
// a ring of n cameras, each paired with its next 3 (identity rotations, exact relative translations, one pair's length wrong tenfold); prints the summary
static int ring(int n) {
  std::vector<int> first, second; std::vector<double> R, t21, pos((size_t)3 * n);
  for (int c = 0; c < n; ++c) { pos[3 * (size_t)c] = std::cos(0.7 * c) * 4; pos[3 * (size_t)c + 1] = std::sin(0.7 * c) * 4; pos[3 * (size_t)c + 2] = 0.1 * c; }
  for (int c = 0; c < n; ++c)
    for (int k = 1; k <= 3 && c + k < n; ++k) {
      first.push_back(c); second.push_back(c + k);
      const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      R.insert(R.end(), I, I + 9);
      for (int a = 0; a < 3; ++a) t21.push_back((pos[3 * (size_t)(c + k) + a] - pos[3 * (size_t)c + a]) * (first.size() == 2 ? 10.0 : 1.0));
    }
  const int P = (int)first.size();
  std::vector<double> scales((size_t)P), weight((size_t)P, 1.0), x((size_t)3 * n, 0.0);
  for (int p = 0; p < P; ++p) scales[(size_t)p] = std::sqrt(t21[3 * (size_t)p] * t21[3 * (size_t)p] + t21[3 * (size_t)p + 1] * t21[3 * (size_t)p + 1] + t21[3 * (size_t)p + 2] * t21[3 * (size_t)p + 2]);
  int info = -1; double sum[5];
  int rc = chk_transavg_dlt(n, P, first.data(), second.data(), R.data(), t21.data(), x.data(), &info);
  if (n > 0) x[0] = x[1] = x[2] = 0.0;
  if (n > 0) rc |= chk_transavg_solve(n, P, first.data(), second.data(), R.data(), t21.data(), scales.data(), 0, x.data(), weight.data(), 0.01, 1.3, 0.9, 50, sum);
  else sum[0] = sum[1] = sum[2] = sum[3] = sum[4] = 0;
  std::printf("n = %d pairs %d: rc %d info %d cost %.6e -> %.6e steps %d + %d termination %d\n", n, P, rc, info, sum[0], sum[1], (int)sum[2], (int)sum[3], (int)sum[4]);
  return rc || !(sum[1] <= sum[0]);
}
int main() { return ring(1) | ring(3) | ring(9) | ring(70) | ring(300); }
#endif
