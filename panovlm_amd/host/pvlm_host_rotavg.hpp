// K40 on the host: the definition of csrc/pvlm_rotavg_core.h (rotation averaging) behind host backends that do what the kernels of csrc/pvlm_rotavg.hip do — the
// per-pair work, the per-camera gathers over kGroup lanes and the dense product over kTile lanes with their butterflies, the fixed reduction tree — on the host's
// pair-graph layer (pvlm_host_pairgraph.hpp), whose dense Cholesky stands in for the library's solvers.  No device, no dependency on the rest of the host mirror: the equality partner of pvlm_rotavg_l1 /
// pvlm_rotavg_l2 (tests/cpp/rotavg_core_check.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_rotavg_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace rotavg_detail {

namespace ra = pvlm_rotavg;
namespace pg = pvlm_pairgraph;
using pairgraph_detail::butterfly;
using pairgraph_detail::dense_spd_solve;
using pairgraph_detail::solve_camera_system;

struct L1HostBackend {
  int F, P, start, n;
  const int *first, *second; const double* R21;
  std::vector<double> rot, rec, G, g, X, terms, cterms, cam, blocks;
  std::vector<int> off, ent;
  pg::CameraSystem sys;
  int info_g = 0;

  L1HostBackend(int F_, int P_, const int* fi, const int* se, const double* R21_, int start_, const double* rotations)
      : F(F_), P(P_), start(start_), n(F_ - 1), first(fi), second(se), R21(R21_), rot(rotations, rotations + 9 * (size_t)F_) {
    pg::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, start);
    rec.assign((size_t)ra::kL1Slots * P, 0.0); g.assign(3 * (size_t)n, 0.0); X.assign(3 * (size_t)F, 0.0);
    terms.assign((size_t)ra::kL1Terms * P, 0.0); cterms.assign(2 * (size_t)F, 0.0); cam.assign(6 * (size_t)F, 0.0); blocks.assign(36 * ((size_t)F + P), 0.0);
    // G = (2 L)^-1, stored as the solver leaves it: the solution for the unit vector e_i at G[i * n ..]
    std::vector<double> A;
    ra::laplacian2(F, P, first, second, start, &A);
    G.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) G[(size_t)i * n + i] = 1.0;
    info_g = dense_spd_solve(n, A, n, G.data(), true);
  }
  bool failed() const { return false; }
  int camera_of(int row) const { return row + (row >= start); }
  int row_of(int c) const { return c - (c > start); }

  void gather_admm() {
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][9];
      for (int l = 0; l < pg::kGroup; ++l) pg::gather_lane<9>(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, ra::kW, 0x1ffu, part[l]);
      butterfly<pg::kGroup, 9>(part);
      if (c == start) { cterms[(size_t)c] = 0.0; cterms[(size_t)F + c] = 0.0; continue; }
      double gc[3];
      ra::admm_camera(part[0], gc, &cterms[(size_t)c], &cterms[(size_t)F + c]);
      for (int k = 0; k < 3; ++k) g[(size_t)k * n + row_of(c)] = gc[k];
    }
  }
  double admm_begin() {
    for (int p = 0; p < P; ++p) ra::admm_begin_pair(&rot[9 * (size_t)first[p]], &rot[9 * (size_t)second[p]], R21 + 9 * (size_t)p, &rec[(size_t)p], P, &terms[(size_t)p]);
    gather_admm();
    return pg::tree_reduce_host<false>(terms.data(), P);
  }
  ra::AdmmNorms admm_iterate() {
    for (int i = 0; i < n; ++i) {                                // X = G g: row i over kTile lanes, then their butterfly
      double part[ra::kTile][3];
      for (int l = 0; l < ra::kTile; ++l) {
        part[l][0] = part[l][1] = part[l][2] = 0.0;
        for (int j = l; j < n; j += ra::kTile) { const double a = G[(size_t)i * n + j]; for (int k = 0; k < 3; ++k) part[l][k] += a * g[(size_t)k * n + j]; }
      }
      butterfly<ra::kTile, 3>(part);
      for (int k = 0; k < 3; ++k) X[(size_t)k * F + camera_of(i)] = part[0][k];
    }
    for (int p = 0; p < P; ++p) {
      const double xi[3] = {X[(size_t)first[p]], X[(size_t)F + first[p]], X[2 * (size_t)F + first[p]]}, xj[3] = {X[(size_t)second[p]], X[(size_t)F + second[p]], X[2 * (size_t)F + second[p]]};
      ra::admm_pair(xi, xj, &rec[(size_t)p], P, &terms[(size_t)p], P);
    }
    gather_admm();
    ra::AdmmNorms nm;
    nm.r2 = pg::tree_reduce_host<false>(&terms[(size_t)ra::kTermR2 * P], P); nm.ax2 = pg::tree_reduce_host<false>(&terms[(size_t)ra::kTermAx2 * P], P);
    nm.z2 = pg::tree_reduce_host<false>(&terms[(size_t)ra::kTermZ2 * P], P);
    nm.s2 = pg::tree_reduce_host<false>(&cterms[0], F); nm.atu2 = pg::tree_reduce_host<false>(&cterms[(size_t)F], F);
    return nm;
  }
  void fetch_x(std::vector<double>* x) const { *x = X; }
  void apply(const std::vector<double>& x) {
    for (int c = 0; c < F; ++c) {
      if (c == start) continue;
      const double xc[3] = {x[(size_t)c], x[(size_t)F + c], x[2 * (size_t)F + c]};
      ra::apply_update(&rot[9 * (size_t)c], xc);
    }
  }
  void apply_x() { apply(X); }
  int irls_solve(const std::vector<double>& xp, std::vector<double>* x) {
    for (int p = 0; p < P; ++p) {
      const double xi[3] = {xp[(size_t)first[p]], xp[(size_t)F + first[p]], xp[2 * (size_t)F + first[p]]}, xj[3] = {xp[(size_t)second[p]], xp[(size_t)F + second[p]], xp[2 * (size_t)F + second[p]]};
      ra::irls_pair(&rot[9 * (size_t)first[p]], &rot[9 * (size_t)second[p]], R21 + 9 * (size_t)p, xi, xj, &rec[(size_t)p], P, &blocks[36 * ((size_t)F + p)]);
    }
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][6];
      for (int l = 0; l < pg::kGroup; ++l) pg::gather_lane<6>(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, ra::kIw, 0x38u, part[l]);
      butterfly<pg::kGroup, 6>(part);
      for (int k = 0; k < 6; ++k) cam[6 * (size_t)c + k] = part[0][k];
      for (int k = 0; k < 3; ++k) blocks[36 * (size_t)c + 7 * k] = 2.0 * part[0][k];
    }
    if (!ra::irls_prepare(&sys, cam.data())) return sys.n + 1;
    const int info = solve_camera_system(&sys, blocks, true);
    if (info != 0) return info;
    if (!pg::finite_all(sys.rhs.data(), sys.rhs.size())) return sys.n + 1;
    ra::irls_expand(sys, x);
    return 0;
  }
};

// pvlm_rotavg_l1 on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int L1Host(int F, int P, const int* first, const int* second, const double* R21, int start, double* rotations, ra::L1Summary* summary) {
  if (!summary || ra::check_args(F, P, first, second, R21, rotations, start, true)) return -1;
  ra::L1Summary s{0, 0, 0, 0};
  if (F > 1) {
    L1HostBackend be(F, P, first, second, R21, start, rotations);
    if (be.info_g != 0) s.info = be.info_g;
    else ra::l1_solve(be, F, P, &s);
    std::memcpy(rotations, be.rot.data(), 9 * (size_t)F * sizeof(double));
  }
  *summary = s;
  return 0;
}

// pvlm_rotavg_l2 on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int L2Host(int F, int P, const int* first, const int* second, const double* R21, double* rotations, double loss_a, int max_num_iterations, pg::Summary* summary) {
  if (!summary || max_num_iterations < 0 || !std::isfinite(loss_a) || ra::check_args(F, P, first, second, R21, rotations, -1, false)) return -1;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P > 0) {
    std::vector<double> aa(3 * (size_t)F);
    for (int c = 0; c < F; ++c) ra::log_rotation(rotations + 9 * (size_t)c, &aa[3 * (size_t)c]);
    pg::Options opt;
    opt.loss_a = loss_a; opt.max_num_iterations = max_num_iterations;
    // the host's LM backend over the device's pair model; finite_pivot = true, as the Cholesky of this twin has always tested (pair-graph layer)
    pairgraph_detail::LmPairHost<ra::L2Model> be(ra::L2Model{R21}, opt, F, P, first, second, aa.data(), nullptr, -1, true);
    pg::lm_solve(be, opt, &s);
    if (pg::finite_all(be.x[be.cur].data(), 3 * (size_t)F)) for (int c = 0; c < F; ++c) ra::exp_rotation(&be.x[be.cur][3 * (size_t)c], rotations + 9 * (size_t)c);
  }
  *summary = s;
  return 0;
}

}  // namespace rotavg_detail
}  // namespace pvlm
