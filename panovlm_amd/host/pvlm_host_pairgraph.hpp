// The pair-graph layer of csrc/pvlm_pairgraph_core.h on the host: what csrc/pvlm_pairgraph.h does on the device, done by loops — the gather over kGroup lanes and
// their butterfly, the camera step, the LM backend of a pair model — with a dense host Cholesky of the camera system in place of the library's solver.  Under the
// host twins of K40 (pvlm_host_rotavg.hpp), K42 (pvlm_host_transavg.hpp), K44 (pvlm_host_bata.hpp), K45 (pvlm_host_rotstart.hpp), K46 (pvlm_host_transdir.hpp) and
// K47 (pvlm_host_translp.hpp); no device, no dependency on the rest of the host mirror.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_pairgraph_core.h"

namespace pvlm {
namespace pairgraph_detail {

namespace pg = pvlm_pairgraph;

// Cholesky of the row-major SPD matrix M (order n, lower triangle read, overwritten by L) and the solution of M X = B for nrhs right-hand sides stored one after
// the other (B[r * n + i]).  Returns 0, or k > 0 when the leading minor of order k is not positive definite.  finite_pivot: a pivot that has overflowed to +inf is
// rejected too (the library's factorisation only asks for d > 0: see DESIGN.md, K40 / K42).
inline int dense_spd_solve(int n, std::vector<double>& M, int nrhs, double* B, bool finite_pivot) {
  for (int j = 0; j < n; ++j) {
    double v = M[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) v -= M[(size_t)j * n + k] * M[(size_t)j * n + k];
    if (!(v > 0.0) || (finite_pivot && !std::isfinite(v))) return j + 1;
    const double l = std::sqrt(v);
    M[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double w = M[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) w -= M[(size_t)i * n + k] * M[(size_t)j * n + k];
      M[(size_t)i * n + j] = w / l;
    }
  }
  for (int r = 0; r < nrhs; ++r) {
    double* x = B + (size_t)r * n;
    for (int i = 0; i < n; ++i) { double w = x[i]; for (int k = 0; k < i; ++k) w -= M[(size_t)i * n + k] * x[k]; x[i] = w / M[(size_t)i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { double w = x[i]; for (int k = i + 1; k < n; ++k) w -= M[(size_t)k * n + i] * x[k]; x[i] = w / M[(size_t)i * n + i]; }
  }
  return 0;
}

// M = D (sum of the 6 x 6 blocks) D + diag of a CameraSystem, dense row-major; the solution replaces sys->rhs
inline int solve_camera_system(pg::CameraSystem* sys, const std::vector<double>& blocks, bool finite_pivot) {
  const int n = sys->n;
  std::vector<double> M((size_t)n * n, 0.0);
  for (size_t b = 0; b < (size_t)sys->F + sys->P; ++b)
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        const int i = sys->rows[6 * b + r], j = sys->cols[6 * b + c];
        if (i < 0 || j < 0) continue;
        const double v = blocks[36 * b + 6 * r + c] * sys->sigma[(size_t)i] * sys->sigma[(size_t)j];
        M[(size_t)i * n + j] += v;
        if (sys->mirror[b]) M[(size_t)j * n + i] += v;
      }
  for (int i = 0; i < n; ++i) M[(size_t)i * n + i] += sys->diag[(size_t)i];
  return dense_spd_solve(n, M, 1, sys->rhs.data(), finite_pivot);
}

// the xor butterfly of a lane group: lane 0's sum
template <int LANES, int N> inline void butterfly(double (*part)[N]) {
  double nxt[LANES][N];
  for (int m = 1; m < LANES; m <<= 1) {
    for (int l = 0; l < LANES; ++l) for (int k = 0; k < N; ++k) nxt[l][k] = part[l][k] + part[l ^ m][k];
    std::memcpy(part, nxt, sizeof nxt);
  }
}

// What an LM backend (pg::lm_solve) keeps whatever its pair model: the pair list and its CSR, the camera system and its block list ([F diagonal | P off-diagonal]),
// the gather, the step.  finite_pivot: see dense_spd_solve.
struct LmHost {
  pg::Options opt; int F, P; bool finite_pivot;
  const int *first, *second;
  std::vector<double> blocks, cam, step, cterms;
  std::vector<int> off, ent;
  pg::CameraSystem sys;
  int info = 0;                // of the last factorisation

  LmHost(const pg::Options& o, int F_, int P_, const int* fi, const int* se, int origin, bool finite_pivot_)
      : opt(o), F(F_), P(P_), finite_pivot(finite_pivot_), first(fi), second(se) {
    pg::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, origin);
    blocks.assign(36 * ((size_t)F + P), 0.0); cam.assign((size_t)pg::kCam * F, 0.0); cterms.assign(2 * (size_t)F, 0.0);
  }
  bool failed() const { return false; }
  double* off_block(int p) { return &blocks[36 * ((size_t)F + p)]; }
  // the end of a linearisation: per camera the lanes' partial sums over the pair records, their butterfly, the gather and the diagonal block
  void gather(const std::vector<double>& rec) {
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][pg::kCam];
      for (int l = 0; l < pg::kGroup; ++l) pg::gather_lane(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, part[l]);
      butterfly<pg::kGroup, pg::kCam>(part);
      for (int k = 0; k < pg::kCam; ++k) cam[(size_t)pg::kCam * c + k] = part[0][k];
      pg::diagonal_block(part[0], &blocks[36 * (size_t)c]);
    }
  }
  bool solve(double radius, bool damped) {
    sys.prepare(cam.data(), damped, radius, opt);
    info = solve_camera_system(&sys, blocks, finite_pivot);
    if (info != 0) return false;
    sys.expand(&step);
    return true;
  }
  // the camera half of a candidate: xc = x + step and the cameras' terms ([0] = |step|^2, [1] = |x|^2)
  void step_cameras(const std::vector<double>& x, std::vector<double>& xc) {
    for (int c = 0; c < F; ++c) {
      const double* v = &x[3 * (size_t)c]; const double* d = &step[3 * (size_t)c];
      for (int k = 0; k < 3; ++k) xc[3 * (size_t)c + k] = v[k] + d[k];
      cterms[(size_t)c] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]; cterms[(size_t)F + c] = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    }
  }
  double camera_term(int k) const { return pg::tree_reduce_host<false>(&cterms[(size_t)k * F], F); }
};

// The LM backend of a pair model M (csrc/pvlm_pairgraph_core.h, at lm_solve): LmPairDevice of csrc/pvlm_pairgraph.h with a loop over the pairs for every launch.
// The model's pointers are host memory that outlives the backend.  x0: 3 F; s0: P where M::kScale, else unread.  damped = false: see LmPairDevice.
template <class M> struct LmPairHost : LmHost {
  M model;
  bool damped = true;
  std::vector<double> x[2], s[2], sigma, gs, rec, terms;
  int cur = 0;

  LmPairHost(const M& m, const pg::Options& o, int F_, int P_, const int* fi, const int* se, const double* x0, const double* s0, int origin, bool finite_pivot_)
      : LmHost(o, F_, P_, fi, se, origin, finite_pivot_), model(m) {
    x[0].assign(x0, x0 + 3 * (size_t)F); x[1] = x[0];
    if (M::kScale) { s[0].assign(s0, s0 + (size_t)P); s[1] = s[0]; sigma.assign((size_t)P, 0.0); gs.assign((size_t)P, 0.0); }
    rec.assign((size_t)M::kSlots * P, 0.0); terms.assign((size_t)M::kTerms * P, 0.0);
  }
  double initial_cost() {
    for (int p = 0; p < P; ++p)
      terms[(size_t)p] = model.cost(p, &x[cur][3 * (size_t)first[p]], &x[cur][3 * (size_t)second[p]], pg::pair_scale<M>(s[cur].data(), p), opt.loss_a);
    return pg::tree_reduce_host<false>(terms.data(), P);
  }
  double linearise(double radius, bool first_time) {
    for (int p = 0; p < P; ++p) {
      model.linearise(p, &x[cur][3 * (size_t)first[p]], &x[cur][3 * (size_t)second[p]], pg::pair_scale<M>(s[cur].data(), p), opt.loss_a, radius, opt.min_lm_diagonal,
                      opt.max_lm_diagonal, first_time, pg::pair_slot<M>(sigma.data(), p), &rec[(size_t)p], P, off_block(p));
      if constexpr (M::kScale) gs[(size_t)p] = std::fabs(rec[(size_t)M::kGs * P + p]);
    }
    gather(rec);
    if (first_time && damped) sys.set_sigma(cam.data());
    const double g_max = sys.gradient_max(cam.data());
    if constexpr (M::kScale) return std::fmax(pg::tree_reduce_host<true>(gs.data(), P), g_max);
    else return g_max;
  }
  bool solve(double radius) { return LmHost::solve(radius, damped); }
  pg::Scalars candidate() {
    std::vector<double>& xc = x[cur ^ 1];
    step_cameras(x[cur], xc);
    for (int p = 0; p < P; ++p) {
      const size_t i = (size_t)first[p], j = (size_t)second[p];
      model.step(p, &rec[(size_t)p], P, &step[3 * i], &step[3 * j], &xc[3 * i], &xc[3 * j], pg::pair_scale<M>(s[cur].data(), p), opt.loss_a,
                 pg::pair_slot<M>(s[cur ^ 1].data(), p), &terms[(size_t)p], P);
    }
    double pt[4] = {0, 0, 0, 0};
    for (int k = 0; k < M::kTerms; ++k) pt[k] = pg::tree_reduce_host<false>(&terms[(size_t)k * P], P);
    if constexpr (M::kScale) return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], pt[pg::kTermStep2] + camera_term(0), pt[pg::kTermX2] + camera_term(1)};
    else return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], camera_term(0), camera_term(1)};
  }
  void accept() { cur ^= 1; }
};

}  // namespace pairgraph_detail
}  // namespace pvlm
