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

// the LM backend on the host's layer; finite_pivot = false: the pivot test of the library's factorisation (d > 0 alone), which this twin exists to equal
struct HostBackend : pairgraph_detail::LmHost {
  bool dlt = false;
  std::vector<double> d, bnd, sigma, rec, terms, gs;
  std::vector<double> t[2], s[2];
  int cur = 0;

  HostBackend(const pg::Options& o, int F_, int P_, const int* fi, const int* se, const double* R_, const double* d_, const double* bnd_, const double* t0, const double* s0,
              int origin) : LmHost(o, F_, P_, fi, se, R_, origin, false), d(d_, d_ + 3 * (size_t)P_), bnd(bnd_, bnd_ + 4 * (size_t)P_) {
    sigma.assign((size_t)P, 0.0); rec.assign((size_t)ta::kPairSlots * P, 0.0); terms.assign((size_t)ta::kPairTerms * P, 0.0); gs.assign((size_t)P, 0.0);
    t[0].assign(t0, t0 + 3 * (size_t)F); t[1] = t[0]; s[0].assign(s0, s0 + (size_t)P); s[1] = s[0];
  }
  double initial_cost() {
    for (int p = 0; p < P; ++p)
      terms[(size_t)p] = ta::pair_cost(R21 + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &t[cur][3 * (size_t)first[p]], &t[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a);
    return pg::tree_reduce_host<false>(terms.data(), P);
  }
  double linearise(double radius, bool first_time) {
    for (int p = 0; p < P; ++p) {
      ta::linearise_pair(R21 + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &t[cur][3 * (size_t)first[p]], &t[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a,
                         radius, opt.min_lm_diagonal, opt.max_lm_diagonal, first_time, dlt, &sigma[(size_t)p], &rec[(size_t)p], P, off_block(p));
      gs[(size_t)p] = std::fabs(rec[(size_t)ta::kGs * P + p]);
    }
    gather(rec);
    if (first_time && !dlt) sys.set_sigma(cam.data());
    return std::fmax(pg::tree_reduce_host<true>(gs.data(), P), sys.gradient_max(cam.data()));
  }
  bool solve(double radius) { return LmHost::solve(radius, !dlt); }
  pg::Scalars candidate() {
    std::vector<double>& tc = t[cur ^ 1];
    step_cameras(t[cur], tc);
    for (int p = 0; p < P; ++p) {
      const size_t i = (size_t)first[p], j = (size_t)second[p];
      ta::step_pair(R21 + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &rec[(size_t)p], P, &step[3 * i], &step[3 * j], &tc[3 * i], &tc[3 * j], s[cur][(size_t)p], opt.loss_a,
                    &s[cur ^ 1][(size_t)p], &terms[(size_t)p], P);
    }
    double pt[ta::kPairTerms];
    for (int k = 0; k < ta::kPairTerms; ++k) pt[k] = pg::tree_reduce_host<false>(&terms[(size_t)k * P], P);
    return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], pt[ta::kTermStep2] + camera_term(0), pt[ta::kTermX2] + camera_term(1)};
  }
  void accept() { cur ^= 1; }
};

// pvlm_transavg_dlt on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, or k > 0 when the system is not positive definite (out untouched).
inline int DltHost(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* out, int* info) {
  if (!info || (F > 0 && !out) || ta::check_pairs(F, P, first, second, R, t21)) return -1;
  if (P == 0) { *info = F <= 1 ? 0 : 1; if (F == 1) out[0] = out[1] = out[2] = 0.0; return 0; }
  const std::vector<double> zeros(3 * (size_t)F + 4 * (size_t)P, 0.0);
  pg::Options opt;
  HostBackend be(opt, F, P, first, second, R, t21, zeros.data(), zeros.data(), zeros.data(), 0);
  be.dlt = true;
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
    HostBackend be(opt, F, P, first, second, R, d.data(), bnd.data(), translations, scales, origin);
    pg::lm_solve(be, opt, &s);
    std::memcpy(translations, be.t[be.cur].data(), 3 * (size_t)F * sizeof(double));
    std::memcpy(scales, be.s[be.cur].data(), (size_t)P * sizeof(double));
    for (int p = 0; p < P; ++p)
      weight[p] = ta::final_weight(R + 9 * (size_t)p, t21 + 3 * (size_t)p, &translations[3 * (size_t)first[p]], &translations[3 * (size_t)second[p]], scales[p]);
  }
  *summary = s;
  return 0;
}

}  // namespace transavg_detail
}  // namespace pvlm
