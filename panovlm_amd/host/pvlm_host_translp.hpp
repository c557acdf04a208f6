// K47 on the host: the definition of csrc/pvlm_translp_core.h (TranslationAveragingL1: the triplet minimax programme by an interior-point method) behind a host
// backend that does what the kernels of csrc/pvlm_translp.hip do — the per-triplet evaluation, both gathers over kGroup lanes and their butterfly, the fixed
// reduction tree, the back-substitution — with the dense host Cholesky of pvlm_host_pairgraph.hpp in place of the library's solver.  No device, no dependency on the
// rest of the host mirror: the one-thread baseline and the equality partner of pvlm_transavg_l1 (tests/cpp/translp_core_check.cpp) and the `host` route of
// TranslationAveragingL1 (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_translp_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace translp_detail {

namespace lp = pvlm_translp;
namespace pg = pvlm_pairgraph;

struct HostBackend {
  lp::Problem& prob;
  const int* trip_pairs; const double* R21; const double* t21;
  int F, P, T;
  std::vector<double> s, z, ds, dz, lam, dlam, x, rec, terms, blocks, camv, camrhs;

  HostBackend(lp::Problem& pr, const int* tp, const double* R, const double* t) : prob(pr), trip_pairs(tp), R21(R), t21(t), F(pr.F), P(pr.P), T(pr.T) {
    lam = prob.lam0;
    s.assign((size_t)lp::kRows * T, 0.0); z = s;
    for (int t = 0; t < T; ++t) {
      lp::Trip tr; double sv[lp::kRows], zv[lp::kRows];
      lp::load_trip(t, trip_pairs, R21, t21, prob.lo.data(), &tr);
      lp::start_rows(tr, lam[(size_t)t], prob.gamma0, prob.z0, sv, zv);
      lp::store_rows(s.data(), T, t, sv); lp::store_rows(z.data(), T, t, zv);
    }
    ds.assign(s.size(), 0.0); dz.assign(s.size(), 0.0); dlam.assign((size_t)T, 0.0); x.assign(3 * (size_t)F, 0.0);
    rec.assign((size_t)lp::kRecSlots * T, 0.0); terms.assign((size_t)lp::kTerms * T, 0.0);
    blocks.assign(36 * ((size_t)F + P), 0.0); camv.assign((size_t)lp::kCamRec * F, 0.0); camrhs.assign(3 * (size_t)F, 0.0);
  }
  const double* cam() const { return camv.data(); }
  const double* cam_rhs() const { return camrhs.data(); }

  // one row of a CSR through the lanes and their butterfly
  template <int N> void gather_row(const std::vector<int>& off, const std::vector<int>& ent, int row, int slot0, int per_slot, double* out) const {
    double part[pg::kGroup][N];
    for (int l = 0; l < pg::kGroup; ++l) lp::gather_lane<N>(rec.data(), T, ent.data(), off[(size_t)row], off[(size_t)row + 1], l, slot0, per_slot, part[l]);
    pairgraph_detail::butterfly<pg::kGroup, N>(part);
    for (int k = 0; k < N; ++k) out[k] = part[0][k];
  }
  bool evaluate(double gam, double* roots) {
    for (int t = 0; t < T; ++t) {
      lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], xc[3][3];
      lp::load_trip(t, trip_pairs, R21, t21, prob.lo.data(), &tr);
      lp::load_rows(s.data(), T, t, sv); lp::load_rows(z.data(), T, t, zv); lp::load_cams(x.data(), prob.trip_cam.data(), t, xc);
      lp::assemble_triplet(tr, xc, lam[(size_t)t], gam, sv, zv, &rec[(size_t)t], T, &terms[(size_t)t], T);
    }
    for (int c = 0; c < F; ++c) {
      gather_row<lp::kCamRec>(prob.cam_off, prob.cam_ent, c, 0, lp::kCamRec, &camv[(size_t)lp::kCamRec * c]);
      pg::diagonal_block(&camv[(size_t)lp::kCamRec * c], &blocks[36 * (size_t)c]);
    }
    for (int p = 0; p < P; ++p) {
      double v[9];
      gather_row<9>(prob.pair_off, prob.pair_ent, p, lp::kRecOff, 9, v);
      lp::off_block(v, &blocks[36 * ((size_t)F + p)]);
    }
    for (int k = 0; k < lp::kTerms; ++k)
      roots[k] = k < lp::kTermRp ? pg::tree_reduce_host<false>(&terms[(size_t)k * T], T) : pg::tree_reduce_host<true>(&terms[(size_t)k * T], T);
    return true;
  }
  bool rhs(int mode, double gam, double sigma_mu, double* gamma_share) {
    for (int t = 0; t < T; ++t) {
      lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows], xc[3][3];
      lp::load_trip(t, trip_pairs, R21, t21, prob.lo.data(), &tr);
      lp::load_rows(s.data(), T, t, sv); lp::load_rows(z.data(), T, t, zv); lp::load_rows(ds.data(), T, t, dsv); lp::load_rows(dz.data(), T, t, dzv);
      lp::load_cams(x.data(), prob.trip_cam.data(), t, xc);
      terms[(size_t)t] = lp::rhs_triplet(mode, tr, xc, lam[(size_t)t], gam, sv, zv, dsv, dzv, sigma_mu, &rec[(size_t)t], T);
    }
    for (int c = 0; c < F; ++c) gather_row<3>(prob.cam_off, prob.cam_ent, c, lp::kRecRhs, 3, &camrhs[3 * (size_t)c]);
    *gamma_share = pg::tree_reduce_host<false>(terms.data(), T);
    return true;
  }
  // the pivot test of the library's factorisation (finite_pivot = false), which this twin exists to equal
  bool solve(int* info) { *info = pairgraph_detail::solve_camera_system(&prob.sys, blocks, false); return true; }
  bool direction(int mode, double gam, const std::vector<double>& dx, double dgam, double sigma_mu, double* ratio) {
    for (int t = 0; t < T; ++t) {
      lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows], xc[3][3], dxc[3][3], r[2];
      lp::load_trip(t, trip_pairs, R21, t21, prob.lo.data(), &tr);
      lp::load_rows(s.data(), T, t, sv); lp::load_rows(z.data(), T, t, zv); lp::load_rows(ds.data(), T, t, dsv); lp::load_rows(dz.data(), T, t, dzv);
      lp::load_cams(x.data(), prob.trip_cam.data(), t, xc); lp::load_cams(dx.data(), prob.trip_cam.data(), t, dxc);
      lp::direction_triplet(mode, tr, xc, lam[(size_t)t], gam, sv, zv, dxc, dgam, sigma_mu, &rec[(size_t)t], T, dsv, dzv, &dlam[(size_t)t], r);
      lp::store_rows(ds.data(), T, t, dsv); lp::store_rows(dz.data(), T, t, dzv);
      terms[(size_t)t] = r[0]; terms[(size_t)T + t] = r[1];
    }
    for (int k = 0; k < 2; ++k) ratio[k] = pg::tree_reduce_host<true>(&terms[(size_t)k * T], T);
    return true;
  }
  bool mu_aff(double ap, double ad, double* sum) {
    for (int t = 0; t < T; ++t) {
      double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows];
      lp::load_rows(s.data(), T, t, sv); lp::load_rows(z.data(), T, t, zv); lp::load_rows(ds.data(), T, t, dsv); lp::load_rows(dz.data(), T, t, dzv);
      terms[(size_t)t] = lp::mu_aff_triplet(sv, zv, dsv, dzv, ap, ad);
    }
    *sum = pg::tree_reduce_host<false>(terms.data(), T);
    return true;
  }
  bool update(double ap, double ad, const std::vector<double>& dx) {
    for (size_t i = 0; i < s.size(); ++i) { s[i] += ap * ds[i]; z[i] += ad * dz[i]; }
    for (int t = 0; t < T; ++t) lam[(size_t)t] += ap * dlam[(size_t)t];
    for (size_t i = 0; i < x.size(); ++i) x[i] += ap * dx[i];
    return true;
  }
};

// pvlm_transavg_l1 on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  lambdas (one per triplet) and gaps (s^T z at every evaluation) are the host
// compile's extras for the tests; each may be null.
inline int L1Host(int F, int P, const int* first, const int* second, const double* R21, const double* t21, int T, const int* trip_pairs, int origin, double* translations,
                  double* duals, const lp::Params* prm, lp::Summary* summary, double* lambdas = nullptr, std::vector<double>* gaps = nullptr) {
  if (!summary || lp::check_args(F, P, first, second, R21, t21, T, trip_pairs, origin, translations, prm)) return -1;
  lp::Summary s{0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, lp::kNoTriplets};
  if (T > 0) {
    lp::Problem prob;
    prob.init(F, P, first, second, R21, t21, T, trip_pairs, origin);
    HostBackend be(prob, trip_pairs, R21, t21);
    lp::run(be, prob, *prm, &s, gaps);
    if (s.termination == lp::kConverged || s.termination == lp::kIterationLimit) {
      std::vector<double> zt((size_t)lp::kRows * T);
      for (int t = 0; t < T; ++t) for (int r = 0; r < lp::kRows; ++r) zt[(size_t)lp::kRows * t + r] = be.z[(size_t)r * T + t];
      s.dual_objective = lp::dual_objective(prob, &be.z[(size_t)lp::kBound * T]);
      std::memcpy(translations, be.x.data(), be.x.size() * sizeof(double));
      if (duals) std::memcpy(duals, zt.data(), zt.size() * sizeof(double));
      if (lambdas) std::memcpy(lambdas, be.lam.data(), (size_t)T * sizeof(double));
    }
  }
  *summary = s;
  return 0;
}

}  // namespace translp_detail
}  // namespace pvlm
