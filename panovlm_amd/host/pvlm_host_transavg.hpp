// K42 on the host: the definition of csrc/pvlm_transavg_core.h (translation averaging) behind a host backend that does what the kernels of csrc/pvlm_transavg.hip do —
// the per-pair linearisation, the fixed reduction tree, the back-substitution — on the host's pair-graph layer (pvlm_host_pairgraph.hpp: the per-camera gather over
// kGroup lanes and their butterfly, a dense host Cholesky of the camera system in place of the library's solver).  No device, no dependency on the rest of the host
// mirror: the equality partner of pvlm_transavg_solve / pvlm_transavg_dlt (tests/cpp/transavg_core_check.cpp) and the `host` route of EstimateGlobalTranslation
// (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_transavg_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace transavg_detail {

namespace ta = pvlm_transavg;
namespace pg = pvlm_pairgraph;

// the LM backend on the host's layer over the device's pair model; finite_pivot = false: the pivot test of the library's factorisation (d > 0 alone), which this
// twin exists to equal
using Backend = pairgraph_detail::LmPairHost<ta::Model>;

// pvlm_transavg_dlt on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, or k > 0 when the system is not positive definite (out untouched).
inline int DltHost(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* out, int* info) {
  if (!info || (F > 0 && !out) || ta::check_pairs(F, P, first, second, R, t21)) return -1;
  if (P == 0) { *info = F <= 1 ? 0 : 1; if (F == 1) out[0] = out[1] = out[2] = 0.0; return 0; }
  const std::vector<double> zeros(3 * (size_t)F + 4 * (size_t)P, 0.0);
  pg::Options opt;
  Backend be(ta::Model{R, t21, zeros.data(), true}, opt, F, P, first, second, zeros.data(), zeros.data(), 0, false);
  be.damped = false;
  be.linearise(1.0, true);
  const bool ok = be.solve(1.0);
  *info = be.info;
  if (ok) std::memcpy(out, be.step.data(), 3 * (size_t)F * sizeof(double));
  return 0;
}

// pvlm_transavg_solve on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int SolveHost(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* scales, int origin, double* translations, double* weight,
                     double loss_a, double upper_ratio, double lower_ratio, int max_num_iterations, pg::Summary* summary) {
  if (!summary || !translations || (P > 0 && (!scales || !weight)) || ta::check_pairs(F, P, first, second, R, t21)) return -1;
  if (origin < 0 || origin >= F || max_num_iterations < 0) return -1;
  if (!pg::finite_all(translations, 3 * (size_t)F) || !pg::finite_all(scales, (size_t)P) || !std::isfinite(loss_a) || !std::isfinite(upper_ratio) || !std::isfinite(lower_ratio)) return -1;
  for (int k = 0; k < 3; ++k) if (translations[3 * (size_t)origin + k] != 0.0) return -1;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P > 0) {
    std::vector<double> d(3 * (size_t)P), bnd(4 * (size_t)P);
    for (int p = 0; p < P; ++p) { ta::direction(t21 + 3 * (size_t)p, &d[3 * (size_t)p]); ta::bounds(scales[p], upper_ratio, lower_ratio, &bnd[4 * (size_t)p]); }
    pg::Options opt;
    opt.loss_a = loss_a; opt.max_num_iterations = max_num_iterations;
    Backend be(ta::Model{R, d.data(), bnd.data(), false}, opt, F, P, first, second, translations, scales, origin, false);
    pg::lm_solve(be, opt, &s);
    std::memcpy(translations, be.x[be.cur].data(), 3 * (size_t)F * sizeof(double));
    std::memcpy(scales, be.s[be.cur].data(), (size_t)P * sizeof(double));
    for (int p = 0; p < P; ++p)
      weight[p] = ta::final_weight(R + 9 * (size_t)p, t21 + 3 * (size_t)p, &translations[3 * (size_t)first[p]], &translations[3 * (size_t)second[p]], scales[p]);
  }
  *summary = s;
  return 0;
}

}  // namespace transavg_detail
}  // namespace pvlm
