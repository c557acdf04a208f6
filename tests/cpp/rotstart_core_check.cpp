// Host-compiled check of K45: the definition of panovlm_amd/csrc/pvlm_rotstart_core.h behind the host backend of panovlm_amd/host/pvlm_host_rotstart.hpp (the kernels'
// work done by loops, a dense host Cholesky in place of the library's solver).  tests/test_rotstart_cpu.py compares it with the independent numpy reference of
// tests/rotstart_ref.py without a GPU; tests/test_rotstart_gpu.py compares pvlm_rotavg_least_square with it.  With -DROTSTART_CHECK_MAIN it is a stand-alone program
// (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_rotstart.hpp"

namespace rs = pvlm_rotstart;

extern "C" {

// Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  summary: iterations, solves, info; values: residual, theta[3].  rotations is written only when info is 0.
int chk_rotstart_solve(int F, int P, const int* first, const int* second, const double* R21, double* rotations, double shift_rel, double tol, int max_iterations,
                       int* summary, double* values) {
  rs::Params prm;
  prm.shift_rel = shift_rel; prm.tol = tol; prm.max_iterations = max_iterations;
  rs::Summary s;
  const int rc = pvlm::rotstart_detail::LeastSquareHost(F, P, first, second, R21, rotations, &prm, summary && values ? &s : nullptr);
  if (rc == 0) { summary[0] = s.iterations; summary[1] = s.solves; summary[2] = s.info; values[0] = s.residual; for (int k = 0; k < 3; ++k) values[1 + k] = s.theta[k]; }
  return rc;
}

}  // extern "C"

#ifdef ROTSTART_CHECK_MAIN
// n cameras whose true rotations turn about a fixed tilted axis, each paired with its next `reach`; every pair's R_21 is exact but for a rotation of `noise` radians
// about an axis that changes with the pair, every third pair is stored flipped (first > second, R_21^T).  The start is the chain of the reach-1 pairs.  With
// max_iterations = 1 the call must end with info -2 and the rotations untouched.  Prints the result.
static void rot_axis(const double* axis, double angle, double* R) { const double v[3] = {axis[0] * angle, axis[1] * angle, axis[2] * angle}; rs::ra::exp_rotation(v, R); }
static int band(int n, int reach, double noise, int max_iterations) {
  const double tilt[3] = {0.6, 0.0, 0.8};
  std::vector<double> truth(9 * (size_t)n), R21, start(9 * (size_t)n);
  std::vector<int> first, second;
  for (int c = 0; c < n; ++c) rot_axis(tilt, 0.3 * c, &truth[9 * (size_t)c]);
  for (int c = 0; c < n; ++c)
    for (int k = 1; k <= reach && c + k < n; ++k) {
      const size_t p = first.size();
      const double ax[3] = {std::cos(1.0 * p), std::sin(1.0 * p) * 0.6, std::sin(1.0 * p) * 0.8};
      double N[9], E[9], R[9];
      rot_axis(ax, noise, N);
      rs::ra::mul_nt(&truth[9 * (size_t)(c + k)], &truth[9 * (size_t)c], E);      // R_jw R_iw^T
      rs::ra::mul_nn(N, E, R);
      if (p % 3 == 2) { first.push_back(c + k); second.push_back(c); for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) R21.push_back(R[3 * b + a]); }
      else { first.push_back(c); second.push_back(c + k); R21.insert(R21.end(), R, R + 9); }
    }
  const int P = (int)first.size();
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::copy(eye, eye + 9, start.begin());
  for (int c = 1; c < n; ++c)
    for (int p = 0; p < P; ++p) {
      if (first[(size_t)p] == c - 1 && second[(size_t)p] == c) rs::ra::mul_nn(&R21[9 * (size_t)p], &start[9 * (size_t)(c - 1)], &start[9 * (size_t)c]);
      if (first[(size_t)p] == c && second[(size_t)p] == c - 1) rs::ra::mul_tn(&R21[9 * (size_t)p], &start[9 * (size_t)(c - 1)], &start[9 * (size_t)c]);
    }
  std::vector<double> rot(start);
  int summary[3] = {-7, -7, -7};
  double values[4] = {-7, -7, -7, -7};
  const int rc = chk_rotstart_solve(n, P, first.data(), second.data(), R21.data(), rot.data(), 1e-9, 1e-12, max_iterations, summary, values);
  double err = 0;      // against the truth in camera 0's frame, the largest entry
  for (int c = 0; c < n; ++c) { double T[9]; rs::ra::mul_nt(&truth[9 * (size_t)c], &truth[0], T); for (int k = 0; k < 9; ++k) err = std::fmax(err, std::fabs(T[k] - rot[9 * (size_t)c + k])); }
  std::printf("n = %d pairs %d noise %g: rc %d info %d iterations %d solves %d residual %.3e distance %.3e\n", n, P, noise, rc, summary[2], summary[0], summary[1], values[0], err);
  if (max_iterations == 1 && noise > 0) return !(rc == 0 && summary[2] == rs::kInfoMaxIterations && rot == start);
  return !(rc == 0 && summary[2] == 0 && err <= (noise > 0 ? 20 * noise : 1e-12));
}
int main() { return band(2, 1, 0.01, 100) | band(40, 3, 0.0, 100) | band(70, 3, 0.01, 100) | band(70, 3, 0.01, 1); }
#endif
