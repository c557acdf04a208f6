// Host-compiled check of K40: the definition of panovlm_amd/csrc/pvlm_rotavg_core.h behind the host backends of panovlm_amd/host/pvlm_host_rotavg.hpp (the kernels'
// work done by loops, a dense host Cholesky in place of the library's solvers).  tests/test_rotavg_cpu.py compares it with the independent numpy reference of
// tests/rotavg_ref.py without a GPU; tests/test_rotavg_gpu.py compares pvlm_rotavg_l1 / pvlm_rotavg_l2 with it.  With -DROTAVG_CHECK_MAIN it is a stand-alone
// program (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_rotavg.hpp"

namespace ra = pvlm_rotavg;
namespace ta = pvlm_transavg;

extern "C" {

int chk_rotavg_group_size() { return ra::kGroup; }
int chk_rotavg_tile() { return ra::kTile; }

// summary4: L1 outer iterations, ADMM iterations in all, IRLS iterations, info.
// Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
int chk_rotavg_l1(int F, int P, const int* first, const int* second, const double* R21, int start, double* rotations, int* summary4) {
  ra::L1Summary s;
  if (!summary4) return -1;
  const int rc = pvlm::rotavg_detail::L1Host(F, P, first, second, R21, start, rotations, &s);
  if (rc) return rc;
  summary4[0] = s.l1_iterations; summary4[1] = s.admm_iterations; summary4[2] = s.irls_iterations; summary4[3] = s.info;
  return 0;
}

// summary5: initial cost, final cost, accepted steps, rejected steps, termination.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
int chk_rotavg_l2(int F, int P, const int* first, const int* second, const double* R21, double* rotations, double loss_a, int max_num_iterations, double* summary5) {
  ta::Summary s;
  if (!summary5) return -1;
  const int rc = pvlm::rotavg_detail::L2Host(F, P, first, second, R21, rotations, loss_a, max_num_iterations, &s);
  if (rc) return rc;
  summary5[0] = s.initial_cost; summary5[1] = s.final_cost; summary5[2] = s.successful_steps; summary5[3] = s.unsuccessful_steps; summary5[4] = s.termination;
  return 0;
}

// the L2 residual of one pair and its two analytic Jacobians (row-major 3 x 3: d r / d aa_1, d r / d aa_2)
void chk_rotavg_l2_pair(const double* aa1, const double* aa2, const double* R21, double* r, double* J1, double* J2) {
  double M[9];
  ra::l2_residual(aa1, aa2, R21, r, M);
  ra::l2_jacobians(aa1, aa2, r, M, J1, J2);
}

}  // extern "C"

#ifdef ROTAVG_CHECK_MAIN
// n cameras turning about a tilted axis, each paired with its next 3; relative rotations exact but for one pair that is off by 0.5 rad; the start is the chain of
// the first pair of every camera; prints the summaries
static int ring(int n) {
  std::vector<int> first, second; std::vector<double> R21, truth((size_t)9 * n), rot((size_t)9 * n);
  for (int c = 0; c < n; ++c) { const double a[3] = {0.05 * c, 0.11 * c, -0.03 * c}; ra::exp_rotation(a, &truth[9 * (size_t)c]); }
  for (int c = 0; c < n; ++c)
    for (int k = 1; k <= 3 && c + k < n; ++k) {
      first.push_back(c); second.push_back(c + k);
      double R[9];
      ra::mul_nt(&truth[9 * (size_t)(c + k)], &truth[9 * (size_t)c], R);
      if (first.size() == 2) { const double off[3] = {0.5, 0, 0}; ra::apply_update(R, off); }
      R21.insert(R21.end(), R, R + 9);
    }
  const int P = (int)first.size();
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int c = 0; c < n; ++c) {
    if (c == 0) { for (int k = 0; k < 9; ++k) rot[(size_t)k] = I[k]; continue; }
    for (int p = 0; p < P; ++p) if (second[(size_t)p] == c && first[(size_t)p] == c - 1) ra::mul_nn(&R21[9 * (size_t)p], &rot[9 * (size_t)(c - 1)], &rot[9 * (size_t)c]);
  }
  int s4[4] = {0, 0, 0, 0}; double s5[5] = {0, 0, 0, 0, 0};
  int rc = chk_rotavg_l1(n, P, first.data(), second.data(), R21.data(), 0, rot.data(), s4);
  rc |= chk_rotavg_l2(n, P, first.data(), second.data(), R21.data(), rot.data(), 0.07, 50, s5);
  std::printf("n = %d pairs %d: rc %d L1 %d ADMM %d IRLS %d info %d; L2 cost %.6e -> %.6e steps %d + %d termination %d\n", n, P, rc, s4[0], s4[1], s4[2], s4[3], s5[0], s5[1],
              (int)s5[2], (int)s5[3], (int)s5[4]);
  return rc || !(s5[1] <= s5[0]);
}
int main() { return ring(1) | ring(3) | ring(9) | ring(70) | ring(200); }
#endif
