// Host-compiled check of K47: the definition of panovlm_amd/csrc/pvlm_translp_core.h behind the host backend of panovlm_amd/host/pvlm_host_translp.hpp (the kernels'
// work done by loops, a dense host Cholesky in place of the library's solver).  tests/test_translp_cpu.py compares it with the independent transcription of
// tests/translp_ref.py under HiGHS without a GPU; tests/test_translp_gpu.py compares pvlm_transavg_l1 with it.  With -DTRANSLP_CHECK_MAIN it is a stand-alone
// program (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_translp.hpp"

namespace lp = pvlm_translp;

extern "C" {

int chk_translp_group_size() { return pvlm_pairgraph::kGroup; }

// summary10: gamma, dual objective, gap, primal residual, dual residual, iterations, bumps, n_components, n_loose, termination.  duals (19 per triplet), lambdas (one
// per triplet) and gaps (s^T z at every evaluation, at most gaps_capacity of them, their number in *n_gaps) may be null.  Returns 0, or -1 (PVLM_ERR_ARG) with
// nothing written.
int chk_translp_l1(int F, int P, const int* first, const int* second, const double* R21, const double* t21, int T, const int* trip_pairs, int origin, double* translations,
                   double* duals, double* lambdas, int max_iterations, double gap_tol, double feas_tol, double* summary10, double* gaps, int gaps_capacity, int* n_gaps) {
  if (!summary10) return -1;
  lp::Params prm; prm.max_iterations = max_iterations; prm.gap_tol = gap_tol; prm.feas_tol = feas_tol;
  lp::Summary s;
  std::vector<double> g;
  const int rc = pvlm::translp_detail::L1Host(F, P, first, second, R21, t21, T, trip_pairs, origin, translations, duals, &prm, &s, lambdas, &g);
  if (rc) return rc;
  const double v[10] = {s.gamma, s.dual_objective, s.gap, s.primal_residual, s.dual_residual, (double)s.iterations, (double)s.bumps, (double)s.n_components, (double)s.n_loose,
                        (double)s.termination};
  for (int k = 0; k < 10; ++k) summary10[k] = v[k];
  if (gaps && n_gaps) { *n_gaps = 0; for (size_t i = 0; i < g.size() && (int)i < gaps_capacity; ++i) gaps[(*n_gaps)++] = g[i]; }
  return 0;
}

}  // extern "C"

#ifdef TRANSLP_CHECK_MAIN
// n cameras on a helix, every camera paired with its next 3 (exact relative poses but one translation, which is turned); every triplet of the pair graph.  Prints the
// summary
static int helix(int n) {
  std::vector<int> first, second, trips; std::vector<double> R, t, pos((size_t)3 * n), ang((size_t)n);
  for (int c = 0; c < n; ++c) { pos[3 * (size_t)c] = std::cos(0.7 * c) * 4; pos[3 * (size_t)c + 1] = std::sin(0.7 * c) * 4; pos[3 * (size_t)c + 2] = 0.1 * c; ang[(size_t)c] = 0.3 * c; }
  std::vector<std::vector<int>> id((size_t)n, std::vector<int>((size_t)n, -1));
  for (int a = 0; a < n; ++a)
    for (int k = 1; k <= 3 && a + k < n; ++k) {
      const int b = a + k;
      id[(size_t)a][(size_t)b] = (int)first.size();
      first.push_back(a); second.push_back(b);
      // rotations about z: R_cw(c) = Rz(ang), t_cw = -R_cw pos; R_21 = R_b R_a^T, t_21 = t_b - R_21 t_a
      const double d = ang[(size_t)b] - ang[(size_t)a], cd = std::cos(d), sd = std::sin(d);
      const double R21[9] = {cd, -sd, 0, sd, cd, 0, 0, 0, 1};
      auto tcw = [&](int c, double* o) { const double ca = std::cos(ang[(size_t)c]), sa = std::sin(ang[(size_t)c]); const double* p = &pos[3 * (size_t)c];
                                        o[0] = -(ca * p[0] - sa * p[1]); o[1] = -(sa * p[0] + ca * p[1]); o[2] = -p[2]; };
      double ta[3], tb[3], t21[3];
      tcw(a, ta); tcw(b, tb);
      for (int r = 0; r < 3; ++r) t21[r] = tb[r] - (R21[3 * r] * ta[0] + R21[3 * r + 1] * ta[1] + R21[3 * r + 2] * ta[2]);
      if (first.size() == 2) { const double x = t21[0]; t21[0] = -t21[1]; t21[1] = x; }
      for (double v : R21) R.push_back(v);
      for (double v : t21) t.push_back(v);
    }
  for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) for (int c = b + 1; c < n; ++c)
    if (id[(size_t)a][(size_t)b] >= 0 && id[(size_t)b][(size_t)c] >= 0 && id[(size_t)a][(size_t)c] >= 0) { trips.push_back(id[(size_t)a][(size_t)b]); trips.push_back(id[(size_t)b][(size_t)c]); trips.push_back(id[(size_t)a][(size_t)c]); }
  const int P = (int)first.size(), T = (int)trips.size() / 3;
  std::vector<double> x((size_t)3 * n, 0.0), duals((size_t)19 * T + 1), lam((size_t)T + 1), gaps(128);
  double sm[10] = {0}; int ng = 0;
  const int rc = chk_translp_l1(n, P, first.data(), second.data(), R.data(), t.data(), T, trips.data(), 0, x.data(), duals.data(), lam.data(), 60, 1e-9, 1e-9, sm, gaps.data(), 128, &ng);
  std::printf("n = %d pairs %d triplets %d: rc %d gamma %.12e dual %.12e gap %.3e rp %.3e rd %.3e iterations %d bumps %d components %d loose %d termination %d\n", n, P, T, rc, sm[0],
              sm[1], sm[2], sm[3], sm[4], (int)sm[5], (int)sm[6], (int)sm[7], (int)sm[8], (int)sm[9]);
  return rc || (T > 0 && sm[9] != 0) || (T == 0 && sm[9] != 6);
}
int main() { return helix(3) | helix(4) | helix(9) | helix(70) | helix(200); }
#endif
