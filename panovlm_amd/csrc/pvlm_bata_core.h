// K44: the definition of BATA translation averaging (sfm/BATA.cpp:36-237, Zhuang et al.'s bilinear angle-based averaging behind a revised-LUD start) — host and
// device.  Compiled for the device by pvlm_bata.hip and for the host by tests/cpp/bata_core_check.cpp (host/pvlm_host_bata.hpp); both run the SAME loop (run() below)
// over a backend that records the pairs, gathers per camera, solves the camera system and reduces on the fixed tree of pvlm_pairgraph_core.h.
//
// Inputs (:176-219): P pairs (first, second), unit directions tij, start scales.  F = max_id - min_id + 1 cameras, the ids shifted by min_id (:197, :207).  At0 has
// +I3 at `first` and -I3 at `second`, so the pair's difference is d_k = t[first] - t[second]; camera 0 is the gauge (:219, :121-123).
//
// LUD stage (LUDRevised :36-125), init_iteration times:
//   weight w_k: 1 at the first iteration, (|r_k|^2 + delta)^-1/2 afterwards (:116); the double square root of :75 / :118 is followed as written: A = diag(sqrt w) At0,
//     so the Laplacian carries sqrt(w) * sqrt(w) and the right-hand side sqrt(w) * (sqrt(w) * s * tij) (:81-83);
//   solve  min sum w_k |d_k - s_k tij_k|^2  subject to  sum_k tij_k . d_k = P  and  sum t = 0  (:84-104);
//   s_k = d_k . tij_k / |tij_k|^2 (:107-108),  r_k = d_k - s_k tij_k (:112-113).
//   Start (:64-73): Svec *= P / sum(Svec), the sum on the layer's tree.  Which pairs count as unscaled (:192-193) and what they draw (:64) is the caller's business:
//   start_scales() merges a given scale (>= 0) with a caller-supplied positive draw, as :68 does.
// STATED DIVERGENCE — the solve method, not the result.  Upstream factorises the indefinite (3 F + 4) KKT matrix [2 A^T A, Aeq^T; Aeq, 0] with SparseLU (:89-100).
// Here it is two SPD solves of the grounded weighted Laplacian L~ = 2 A~^T A~ (camera 0's columns removed):
//   x1 = L~^-1 (2 A~^T B),   x2 = L~^-1 c~  with  c = At0^T vec(tij) (the first row of Aeq, :51-57),   t = x1 - lambda x2,   lambda = (c~^T x1 - P) / (c~^T x2).
// That is exact: c and A^T B are both orthogonal to the translations of all cameras (At0 maps them to zero), so multiplying the first KKT row by the three
// translation vectors leaves (E^T E) mu = 0: the multiplier of sum t = 0 is zero, L t = b - lambda c holds for every shift of t, and c^T t does not see the shift.
// Upstream moves camera 0 to the origin at :121-123 anyway; s_k and r_k read differences only.  c~^T x is summed per pair: sum_k tij_k . (x[first] - x[second]).
//
// IRLS stage (IRLS :127-174), outer_iteration - 1 outers of inner_iteration inners:
//   outer (:139-149): e_k = |(1 / S_k) d_k - tij_k|; Wvec = 1 below robust_threshold, thr / e above it, 0 at equality or NaN (:144-146 leave it so);
//   inner (:152-167): S_k = |d_k|^2 / (d_k . tij_k), +inf where that is negative (:156: the row drops out); A = diag(sqrt(Wvec) / S) At0, B = sqrt(Wvec) tij, so the
//     Laplacian weight is omega_k = (sqrt(Wvec_k) / S_k)^2 and the right-hand side +-(sqrt(Wvec_k) / S_k) (sqrt(Wvec_k) tij_k); solve with camera 0 fixed.
// STATED DIVERGENCES.  Upstream's SparseQR on A^T A (:161-165) is a Cholesky here: a system that is not positive definite (a graph that is not connected, a camera
// whose pairs have all dropped) returns info > 0 with the output untouched, where upstream returns some basic solution.  A scale that is not a number (0 / 0: two
// cameras on one point) poisons everything upstream; here it returns info = -1 with the output untouched, and so does any solution that is not finite.
// Not built: Svec.txt, LUD.txt, LUD.pcd (:69-71, :223-230).  init_iteration >= 1 is required: upstream reads an empty vector at 0 (:120).
// Sums: per camera over its pairs in list order on kGroup lanes and a fixed butterfly, the scalars on the fixed tree; the system is L (x) I3.
#pragma once
#include <cmath>
#include <vector>

#include "pvlm_pairgraph_core.h"

#if defined(__HIPCC__)
#define PVLM_BT_HD __host__ __device__ __forceinline__
#else
#define PVLM_BT_HD inline
#endif

namespace pvlm_bata {

namespace pg = pvlm_pairgraph;

// per-pair record, component-major (component k of pair p at [k * P + p]): the Laplacian weight, then the pair's right-hand side vector
enum { kW = 0, kQ = 1, kSlots = 4 };
enum { kCam = 4 };                                        // per camera: sum of weights, signed sum of the right-hand side vectors
enum { kInfoNotFinite = -1, kInfoNoPairs = -2, kDeviceError = -1000000 };      // kDeviceError never leaves the library: the entry point returns its status

struct Params { double delta = 1e-6; int init_iteration = 10, inner_iteration = 10, outer_iteration = 10; double robust_threshold = 0.1; };

// :107-108, :112-116 for one pair at d = ti - tj: the scale and the next weight
PVLM_BT_HD void lud_update(const double* tij, const double* ti, const double* tj, double delta, double* s, double* w) {
  const double d0 = ti[0] - tj[0], d1 = ti[1] - tj[1], d2 = ti[2] - tj[2];
  const double sq = (tij[0] * tij[0] + tij[1] * tij[1]) + tij[2] * tij[2];
  const double sc = ((d0 * tij[0] + d1 * tij[1]) + d2 * tij[2]) / sq;
  const double r0 = d0 - sc * tij[0], r1 = d1 - sc * tij[1], r2 = d2 - sc * tij[2];
  *s = sc; *w = pow(((r0 * r0 + r1 * r1) + r2 * r2) + delta, -0.5);
}
// :79-92 for one pair: the record and the off-diagonal block -2 w I3 (a 6 x 6 row-major block whose other entries stay zero)
PVLM_BT_HD void lud_record(const double* tij, double s, double w, double* rec, long long P, double* off) {
  const double sw = sqrt(w), ww = sw * sw;
  rec[kW * P] = ww;
  for (int k = 0; k < 3; ++k) { rec[(kQ + k) * P] = sw * ((sw * s) * tij[k]); off[7 * k] = -2.0 * ww; }
}
// the pair's terms of c~^T x1 and c~^T x2
PVLM_BT_HD void dots_pair(const double* tij, const double* x1i, const double* x1j, const double* x2i, const double* x2j, double* terms, long long stride) {
  terms[0] = (tij[0] * (x1i[0] - x1j[0]) + tij[1] * (x1i[1] - x1j[1])) + tij[2] * (x1i[2] - x1j[2]);
  terms[stride] = (tij[0] * (x2i[0] - x2j[0]) + tij[1] * (x2i[1] - x2j[1])) + tij[2] * (x2i[2] - x2j[2]);
}
// :139-146 for one pair: Wvec
PVLM_BT_HD double outer_weight(const double* tij, const double* ti, const double* tj, double S, double thr) {
  const double inv = 1.0 / S;
  const double u0 = inv * (ti[0] - tj[0]) - tij[0], u1 = inv * (ti[1] - tj[1]) - tij[1], u2 = inv * (ti[2] - tj[2]) - tij[2];
  const double e = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
  double w = 0.0;
  if (e < thr) w = 1.0;
  if (e > thr) w = thr / e;
  return w;
}
// :152-159 for one pair: the scale, the record, the off-diagonal block -omega I3.  Returns 1 when the scale is not a number, else 0.
PVLM_BT_HD double inner_record(const double* tij, const double* ti, const double* tj, double wvec, double* S, double* rec, long long P, double* off) {
  const double d0 = ti[0] - tj[0], d1 = ti[1] - tj[1], d2 = ti[2] - tj[2];
  double sc = ((d0 * d0 + d1 * d1) + d2 * d2) / ((d0 * tij[0] + d1 * tij[1]) + d2 * tij[2]);
  if (sc < 0) sc = INFINITY;
  const double sw = sqrt(wvec), a = sw / sc, om = a * a;
  *S = sc;
  rec[kW * P] = om;
  for (int k = 0; k < 3; ++k) { rec[(kQ + k) * P] = a * (sw * tij[k]); off[7 * k] = -om; }
  return sc != sc ? 1.0 : 0.0;
}

// ---- host side: shared by the device entry point and by the host compile -----------------------------------------------------------------------------------

// :67-68: the given scale where it is >= 0, else the draw
inline void start_scales(int P, const double* given, const double* draw, double* out) { for (int p = 0; p < P; ++p) out[p] = given[p] >= 0 ? given[p] : draw[p]; }

// nullptr, or what is wrong with the arguments; on success min_id and F = max_id - min_id + 1 (:182-197)
inline const char* check_args(int n_cameras, int P, const int* first, const int* second, const double* dir, const double* scales0, const Params* prm, int* min_id, int* F) {
  if (!prm) return "null argument";
  if (n_cameras < 2) return "fewer than two cameras";
  if (P < 0) return "a negative count";
  if (prm->init_iteration < 1 || prm->inner_iteration < 1 || prm->outer_iteration < 1) return "an iteration count below 1";
  if (!std::isfinite(prm->delta) || !std::isfinite(prm->robust_threshold)) return "a parameter is not finite";
  if (P > 0 && (!first || !second || !dir || !scales0)) return "null argument";
  int lo = n_cameras, hi = -1;
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= n_cameras || second[p] < 0 || second[p] >= n_cameras) return "a pair names a camera that is not there";
    if (first[p] == second[p]) return "a pair of a camera with itself";
    const double* d = dir + 3 * (size_t)p;
    if (!pg::finite_all(d, 3) || !std::isfinite(scales0[p])) return "a direction or a scale is not finite";
    if (!(std::fabs(std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0) <= 1e-9)) return "a direction is not of unit length";
    if (!(scales0[p] > 0)) return "a start scale is not positive";
    lo = first[p] < lo ? first[p] : lo; lo = second[p] < lo ? second[p] : lo; hi = first[p] > hi ? first[p] : hi; hi = second[p] > hi ? second[p] : hi;
  }
  *min_id = P > 0 ? lo : 0; *F = P > 0 ? hi - lo + 1 : 0;
  return nullptr;
}

// the camera system's right-hand side from per-camera 3-vectors v (stride numbers per camera, the vector at v[stride * c + at ..]) times `factor`; no scaling, no
// added diagonal
inline void set_rhs(pg::CameraSystem* sys, const double* v, int stride, int at, double factor) {
  for (int c = 0; c < sys->F; ++c) {
    if (sys->index(c) < 0) continue;
    for (int k = 0; k < 3; ++k) { const size_t i = (size_t)sys->index(c) + k; sys->sigma[i] = 1.0; sys->diag[i] = 0.0; sys->rhs[i] = factor * v[(size_t)stride * c + at + k]; }
  }
}
// the solved rhs -> 3 numbers per camera, zero at camera 0
inline void expand(const pg::CameraSystem& sys, std::vector<double>* x) {
  x->assign(3 * (size_t)sys.F, 0.0);
  for (int c = 0; c < sys.F; ++c) if (sys.index(c) >= 0) for (int k = 0; k < 3; ++k) (*x)[3 * (size_t)c + k] = sys.rhs[(size_t)sys.index(c) + k];
}

// The whole of BATA over a backend B:
//   int F, P; pg::CameraSystem sys; std::vector<double> cam (kCam per camera: the last gather);
//   bool failed()                              a device error: the loop stops;
//   double scale_sum()                         the tree's sum of the start scales;
//   void gather_c(std::vector<double>* c)      c = At0^T vec(tij) per camera (3 F): minus the signed gather of the directions;
//   void lud_pairs(bool first, double factor)  per pair: at the first iteration s = factor * start and w = 1, else lud_update at the current t; the record; the gather;
//   void lud_scales()                          lud_update alone: the scales S that the IRLS stage starts from (:107-110 of the last iteration);
//   int solve()                                sys (right-hand side set) -> info of the factorisation, the solution in sys.rhs;
//   void dots(x1, x2, double a[2])             c~^T x1, c~^T x2 on the tree;
//   void set_t(t)                              the cameras' positions for the next per-pair pass;
//   void outer(thr)                            Wvec per pair;
//   double inner_pairs()                       per pair: inner_record; the gather; returns the tree's maximum of the flags.
// lud / centres: 3 F each, written only when 0 is returned.  Returns 0, k > 0 (not positive definite), kInfoNotFinite or kDeviceError.
template <class B> inline int run(B& be, const Params& prm, std::vector<double>* lud, std::vector<double>* centres) {
  const int P = be.P;
  pg::CameraSystem& sys = be.sys;
  const double factor = P / be.scale_sum();                    // :72
  std::vector<double> c, x1, x2, t;
  be.gather_c(&c);
  for (int iter = 0; iter < prm.init_iteration; ++iter) {
    be.lud_pairs(iter == 0, factor);
    if (be.failed()) return kDeviceError;
    if (!pg::finite_all(be.cam.data(), be.cam.size())) return kInfoNotFinite;
    set_rhs(&sys, be.cam.data(), kCam, kQ, -2.0);           // 2 A^T B: the gather's sign is - for first, + for second
    int info = be.solve();
    if (be.failed()) return kDeviceError;
    if (info) return info;
    expand(sys, &x1);
    set_rhs(&sys, c.data(), 3, 0, 1.0);
    info = be.solve();
    if (be.failed()) return kDeviceError;
    if (info) return info;
    expand(sys, &x2);
    if (!pg::finite_all(x1.data(), x1.size()) || !pg::finite_all(x2.data(), x2.size())) return kInfoNotFinite;
    double a[2] = {0, 0};
    be.dots(x1, x2, a);
    if (be.failed()) return kDeviceError;
    const double lambda = (a[0] - P) / a[1];
    t.resize(x1.size());
    for (size_t i = 0; i < t.size(); ++i) t[i] = x1[i] - lambda * x2[i];
    if (!pg::finite_all(t.data(), t.size())) return kInfoNotFinite;
    be.set_t(t);
  }
  be.lud_scales();
  *lud = t;
  for (int o = 0; o + 1 < prm.outer_iteration; ++o) {
    be.outer(prm.robust_threshold);
    for (int j = 0; j < prm.inner_iteration; ++j) {
      const double bad = be.inner_pairs();
      if (be.failed()) return kDeviceError;
      if (bad != 0.0 || !pg::finite_all(be.cam.data(), be.cam.size())) return kInfoNotFinite;
      set_rhs(&sys, be.cam.data(), kCam, kQ, -1.0);
      const int info = be.solve();
      if (be.failed()) return kDeviceError;
      if (info) return info;
      expand(sys, &t);
      if (!pg::finite_all(t.data(), t.size())) return kInfoNotFinite;
      be.set_t(t);
    }
  }
  *centres = t;
  return be.failed() ? (int)kDeviceError : 0;
}

}  // namespace pvlm_bata
