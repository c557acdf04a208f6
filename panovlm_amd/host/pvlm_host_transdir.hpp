// K46 on the host: the definition of csrc/pvlm_transdir_core.h (translation averaging on world-frame directions: the chordal problem and one LUD solve) behind a
// host backend that does what the kernels of csrc/pvlm_transdir.hip do — the per-pair linearisation, the fixed reduction tree, the back-substitution — on the host's
// pair-graph layer (pvlm_host_pairgraph.hpp).  No device, no dependency on the rest of the host mirror: the equality partner of pvlm_transavg_chordal /
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

// the LM backend of both problems on the host's layer; finite_pivot = false: the pivot test of the library's factorisation, which this twin exists to equal.
// bnd, w and s0 are null for kChordal.
struct HostBackend : pairgraph_detail::LmHost {
  int model;
  const double* dir;
  std::vector<double> bnd, w, sigma, rec, terms, gs;
  std::vector<double> x[2], s[2];
  int cur = 0;

  HostBackend(int model_, const pg::Options& o, int F_, int P_, const int* fi, const int* se, const double* dir_, const double* bnd_, const double* w_, const double* c0,
              const double* s0, int origin) : LmHost(o, F_, P_, fi, se, nullptr, origin, false), model(model_), dir(dir_) {
    bnd.assign(4 * (size_t)P, 0.0); w.assign((size_t)P, 1.0); s[0].assign((size_t)P, 0.0);
    if (model == td::kLud) { bnd.assign(bnd_, bnd_ + 4 * (size_t)P); w.assign(w_, w_ + (size_t)P); s[0].assign(s0, s0 + (size_t)P); }
    s[1] = s[0];
    sigma.assign((size_t)P, 0.0); rec.assign((size_t)td::kPairSlots * P, 0.0); terms.assign((size_t)td::kPairTerms * P, 0.0); gs.assign((size_t)P, 0.0);
    x[0].assign(c0, c0 + 3 * (size_t)F); x[1] = x[0];
  }
  double initial_cost() {
    for (int p = 0; p < P; ++p)
      terms[(size_t)p] = td::pair_cost(model, dir + 3 * (size_t)p, &bnd[4 * (size_t)p], w[(size_t)p], &x[cur][3 * (size_t)first[p]], &x[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a);
    return pg::tree_reduce_host<false>(terms.data(), P);
  }
  double linearise(double radius, bool first_time) {
    for (int p = 0; p < P; ++p) {
      td::linearise_pair(model, dir + 3 * (size_t)p, &bnd[4 * (size_t)p], w[(size_t)p], &x[cur][3 * (size_t)first[p]], &x[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a, radius,
                         opt.min_lm_diagonal, opt.max_lm_diagonal, first_time, &sigma[(size_t)p], &rec[(size_t)p], P, off_block(p));
      gs[(size_t)p] = std::fabs(rec[(size_t)td::kGs * P + p]);
    }
    gather(rec);
    if (first_time) sys.set_sigma(cam.data());
    return std::fmax(pg::tree_reduce_host<true>(gs.data(), P), sys.gradient_max(cam.data()));
  }
  bool solve(double radius) { return LmHost::solve(radius, true); }
  pg::Scalars candidate() {
    std::vector<double>& xc = x[cur ^ 1];
    step_cameras(x[cur], xc);
    for (int p = 0; p < P; ++p) {
      const size_t i = (size_t)first[p], j = (size_t)second[p];
      td::step_pair(model, dir + 3 * (size_t)p, &bnd[4 * (size_t)p], w[(size_t)p], &rec[(size_t)p], P, &step[3 * i], &step[3 * j], &xc[3 * i], &xc[3 * j], s[cur][(size_t)p], opt.loss_a,
                    &s[cur ^ 1][(size_t)p], &terms[(size_t)p], P);
    }
    double pt[td::kPairTerms];
    for (int k = 0; k < td::kPairTerms; ++k) pt[k] = pg::tree_reduce_host<false>(&terms[(size_t)k * P], P);
    return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], pt[td::kTermStep2] + camera_term(0), pt[td::kTermX2] + camera_term(1)};
  }
  void accept() { cur ^= 1; }
};

// pvlm_transavg_chordal on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int ChordalHost(int F, int P, const int* first, const int* second, const double* dir, int origin, double* centres, double loss_a, int max_num_iterations,
                       pg::Summary* summary) {
  if (!summary || !centres || td::check_pairs(F, P, first, second, dir) || td::check_centres(F, origin, centres)) return -1;
  if (max_num_iterations < 0 || !std::isfinite(loss_a)) return -1;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P > 0) {
    const pg::Options opt = td::chordal_options(loss_a, max_num_iterations);
    HostBackend be(td::kChordal, opt, F, P, first, second, dir, nullptr, nullptr, centres, nullptr, origin);
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
    HostBackend be(td::kLud, opt, F, P, first, second, dir, bnd.data(), weight, centres, scales, origin);
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
