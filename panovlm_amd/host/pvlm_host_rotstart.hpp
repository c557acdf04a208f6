// K45 on the host: the definition of csrc/pvlm_rotstart_core.h (RotationAveragingLeastSquare, the start of the L2 rotation-averaging method) behind a host backend that
// does what the kernels of csrc/pvlm_rotstart.hip do — the per-pair record of M X, the per-camera gather over kGroup lanes and their butterfly, the fixed reduction
// tree — on the host's pair-graph layer (pvlm_host_pairgraph.hpp).  In place of the library's solver stands a dense host Cholesky of M + sigma I, factorised once a
// call (the matrix does not change between the solves).  No device, no dependency on the rest of the host mirror: the equality partner of pvlm_rotavg_least_square
// (tests/cpp/rotstart_core_check.cpp) and the `host` route of RotationAveragingLeastSquare (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_rotstart_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace rotstart_detail {

namespace rs = pvlm_rotstart;
namespace pg = pvlm_pairgraph;

struct HostBackend {
  int F, P, n, info_f = 0;
  const int *first, *second; const double* R21;
  std::vector<double> X, MX, rec, blocks, terms, L;
  std::vector<int> off, ent;
  pg::CameraSystem sys;

  HostBackend(int F_, int P_, const int* fi, const int* se, const double* R21_) : F(F_), P(P_), n(3 * F_), first(fi), second(se), R21(R21_) {
    pg::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, -1);
    X.assign(9 * (size_t)F, 0.0); MX.assign(9 * (size_t)F, 0.0); rec.assign((size_t)rs::kSlots * P, 0.0); blocks.assign(36 * ((size_t)F + P), 0.0);
    terms.assign((size_t)rs::kSym * F, 0.0);
  }
  bool failed() const { return false; }
  void assemble(double sigma) {
    for (int c = 0; c < F; ++c) rs::diag_block((double)(off[(size_t)c + 1] - off[(size_t)c]), sigma, &blocks[36 * (size_t)c]);
    for (int p = 0; p < P; ++p) rs::off_block(R21 + 9 * (size_t)p, &blocks[36 * ((size_t)F + p)]);
    L.assign((size_t)n * n, 0.0);
    for (size_t b = 0; b < (size_t)F + P; ++b)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          const int i = sys.rows[6 * b + r], j = sys.cols[6 * b + c];
          L[(size_t)i * n + j] += blocks[36 * b + 6 * r + c];
          if (sys.mirror[b]) L[(size_t)j * n + i] += blocks[36 * b + 6 * r + c];
        }
    info_f = pairgraph_detail::dense_spd_solve(n, L, 0, nullptr, false);
  }
  int solve() {
    if (info_f) return info_f;
    double* x = sys.rhs.data();
    for (int i = 0; i < n; ++i) { double w = x[i]; for (int k = 0; k < i; ++k) w -= L[(size_t)i * n + k] * x[k]; x[i] = w / L[(size_t)i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { double w = x[i]; for (int k = i + 1; k < n; ++k) w -= L[(size_t)k * n + i] * x[k]; x[i] = w / L[(size_t)i * n + i]; }
    return 0;
  }
  void put(const std::vector<double>& x) { X = x; }
  void fetch(std::vector<double>* x) const { *x = X; }
  void reduce(int cols, double* out) const { for (int k = 0; k < cols; ++k) out[k] = pg::tree_reduce_host<false>(&terms[(size_t)k * F], F); }
  void gram(double* g) {
    for (int c = 0; c < F; ++c) rs::sym_terms(&X[9 * (size_t)c], &X[9 * (size_t)c], &terms[(size_t)c], F);
    reduce(rs::kSym, g);
  }
  void mul(const double* C) { for (int c = 0; c < F; ++c) rs::mul_block(&X[9 * (size_t)c], C); }
  void rayleigh(double* t) {
    for (int p = 0; p < P; ++p) rs::mx_pair(R21 + 9 * (size_t)p, &X[9 * (size_t)first[p]], &X[9 * (size_t)second[p]], &rec[(size_t)p], P);
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][rs::kBlock];
      for (int l = 0; l < pg::kGroup; ++l) rs::gather_lane(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, part[l]);
      pairgraph_detail::butterfly<pg::kGroup, rs::kBlock>(part);
      for (int k = 0; k < rs::kBlock; ++k) MX[9 * (size_t)c + k] = part[0][k];
      rs::sym_terms(&X[9 * (size_t)c], &MX[9 * (size_t)c], &terms[(size_t)c], F);
    }
    reduce(rs::kSym, t);
  }
  void rotate(const double* S, const double* theta, double* r2, std::vector<double>* x) {
    for (int c = 0; c < F; ++c) {
      rs::mul_block(&X[9 * (size_t)c], S); rs::mul_block(&MX[9 * (size_t)c], S);
      rs::residual_terms(&X[9 * (size_t)c], &MX[9 * (size_t)c], theta, &terms[(size_t)c], F);
    }
    reduce(3, r2);
    *x = X;
  }
  double polar(std::vector<double>* out) {
    out->assign(9 * (size_t)F, 0.0);
    for (int c = 0; c < F; ++c) terms[(size_t)c] = rs::final_rotation(&X[9 * (size_t)c], &X[0], &(*out)[9 * (size_t)c]);
    return pg::tree_reduce_host<true>(terms.data(), F);
  }
};

// pvlm_rotavg_least_square on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  rotations is written only when summary->info is 0.
inline int LeastSquareHost(int F, int P, const int* first, const int* second, const double* R21, double* rotations, const rs::Params* prm, rs::Summary* summary) {
  if (!summary || rs::check_args(F, P, first, second, R21, rotations, prm)) return -1;
  HostBackend be(F, P, first, second, R21);
  std::vector<double> out;
  if (rs::run(be, *prm, (double)rs::max_degree(F, P, first, second), rotations, &out, summary) == 0) std::memcpy(rotations, out.data(), out.size() * sizeof(double));
  return 0;
}

}  // namespace rotstart_detail
}  // namespace pvlm
