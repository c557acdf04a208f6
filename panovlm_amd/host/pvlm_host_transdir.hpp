// K46 on the host: the definition of csrc/pvlm_transdir_core.h (translation averaging on world-frame directions: the chordal problem and one LUD solve) behind the
// host's LM backend, which does what the device's does — the per-pair linearisation, the fixed reduction tree, the back-substitution — on the host's pair-graph
// layer (pvlm_host_pairgraph.hpp), each problem over the device's pair model.  No device, no dependency on the rest of the host mirror: the equality partner of pvlm_transavg_chordal /
// pvlm_transavg_lud (tests/cpp/transdir_core_check.cpp) and the `host` route of TranslationAveragingL2Chordal / TranslationAveragingLUD (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_transdir_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace transdir_detail {

namespace td = pvlm_transdir;
namespace pg = pvlm_pairgraph;

using pairgraph_detail::LmPairHost;       // finite_pivot = false below: the pivot test of the library's factorisation, which these twins exist to equal

// pvlm_transavg_chordal on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int ChordalHost(int F, int P, const int* first, const int* second, const double* dir, int origin, double* centres, double loss_a, int max_num_iterations,
                       pg::Summary* summary) {
  if (!summary || !centres || td::check_pairs(F, P, first, second, dir) || td::check_centres(F, origin, centres)) return -1;
  if (max_num_iterations < 0 || !std::isfinite(loss_a)) return -1;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P > 0) {
    const pg::Options opt = td::chordal_options(loss_a, max_num_iterations);
    LmPairHost<td::Chordal> be(td::Chordal{dir}, opt, F, P, first, second, centres, nullptr, origin, false);
    pg::lm_solve(be, opt, &s);
    if (s.termination != pg::kCostNotFinite) std::memcpy(centres, be.x[be.cur].data(), 3 * (size_t)F * sizeof(double));
  }
  *summary = s;
  return 0;
}

// pvlm_transavg_lud on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int LudHost(int F, int P, const int* first, const int* second, const double* dir, double* scales, double* weight, int origin, double* centres, double upper_ratio,
                   double lower_ratio, int max_num_iterations, double* sum_e, pg::Summary* summary) {
  if (!summary || !centres || !sum_e || (P > 0 && (!scales || !weight)) || td::check_pairs(F, P, first, second, dir) || td::check_centres(F, origin, centres)) return -1;
  if (max_num_iterations < 0 || !pg::finite_all(scales, (size_t)P) || !pg::finite_all(weight, (size_t)P) || !std::isfinite(upper_ratio) || !std::isfinite(lower_ratio)) return -1;
  for (int p = 0; p < P; ++p) if (!(weight[p] > 0.0)) return -1;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P > 0) {
    std::vector<double> bnd(4 * (size_t)P), m((size_t)P);
    for (int p = 0; p < P; ++p) td::lud_bounds(scales[p], upper_ratio, lower_ratio, &bnd[4 * (size_t)p]);
    pg::Options opt;
    opt.max_num_iterations = max_num_iterations;
    LmPairHost<td::Lud> be(td::Lud{dir, bnd.data(), weight}, opt, F, P, first, second, centres, scales, origin, false);
    pg::lm_solve(be, opt, &s);
    if (s.termination != pg::kCostNotFinite) {
      std::memcpy(centres, be.x[be.cur].data(), 3 * (size_t)F * sizeof(double));
      std::memcpy(scales, be.s[be.cur].data(), (size_t)P * sizeof(double));
      for (int p = 0; p < P; ++p) weight[p] = td::final_weight(dir + 3 * (size_t)p, &centres[3 * (size_t)first[p]], &centres[3 * (size_t)second[p]], scales[p], &m[(size_t)p]);
      *sum_e = pg::tree_reduce_host<false>(m.data(), P);
    }
  }
  *summary = s;
  return 0;
}

}  // namespace transdir_detail
}  // namespace pvlm
