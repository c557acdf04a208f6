// K46: the definition of the two translation-averaging methods on world-frame directions — TranslationAveragingL2Chordal (sfm/TranslationAveraging.cpp:206-274,
// ChrodalResidual base/CostFunction.h:149-173) and one solve of TranslationAveragingLUD's loop (:553-614, LUDResidual and ScaleFactor :89-144) — host and device.
// Compiled for the device by pvlm_transdir.hip and for the host by tests/cpp/transdir_core_check.cpp; both run the SAME Levenberg-Marquardt policy (lm_solve of
// pvlm_pairgraph_core.h, with its camera system, gather and fixed reduction tree) over a backend that evaluates, gathers, solves and steps.
//
// Unknowns: one CENTRE c per camera (upstream's t_wc; the camera origin_idx is constant and zero).  Pair p carries a unit direction dir_p in the world frame.
//   Chordal:  u = c[first] - c[second], n = |u|, r = u / n - dir (three residuals, weight 1) under HuberLoss(a) on |r|^2; rho'' <= 0, so the corrector scales r and J
//             by sqrt(rho').  dr/dc_first = A = (I - uu^T / n^2) / n, dr/dc_second = -A; A^T A = (I - uu^T / n^2) / n^2 is taken in that closed form.  No scale: the
//             reduced block and gradient of the layer's record equal the unreduced ones.  n == 0 makes the cost NaN: at the start that is
//             termination 5, at a candidate a rejected step (lm_solve).  The cost is invariant under c -> lambda c: the overall scale is a gauge that only the LM
//             damping holds, so the result keeps roughly the scale of its start.
//   Lud:      one private scale s_p per pair; e = c[first] - c[second] - s_p dir_p, ONE residual f = w_p |e|^(1/2), no loss.  w_p is an input and is applied (the
//             LUD functor reads its weight, unlike K42's).  q = w_p / 2 |e|^(-3/2) e: df/dc_first = q^T, df/dc_second = -q^T, df/ds = -q . dir.
//             STATED DIVERGENCE: where |e| == 0 at a linearisation point the pair contributes q = 0, a zero row; upstream's Jet gives a non-finite derivative there
//             and Ceres fails the solve.
//             Scale block, by the INCOMING scale s0: s0 != 1 (as written, :563) gives ScaleFactor(upper_ratio s0, lower_ratio s0) and the parameter bounds
//             [0.5 s0, 3 s0]; otherwise ScaleFactor(2, 1) and a parameter LOWER bound of 1 only (:576-578) — K42's unscaled pairs have no parameter bound.
//             K42's scale_factor and clamp_scale are used as they are.
// One LM iteration eliminates every scale (a 1 x 1 pivot), gathers the reduced 3 x 3 blocks per camera, solves the camera system, back-substitutes the scale steps,
// CLAMPS the candidate scales onto their parameter bounds and takes the step quality against the model at the clamped step: K42's stand-in for Ceres' projection
// plus line search, the same divergence.
// Sums: every scalar is the root of the fixed tree over its per-pair or per-camera terms.
// Write-back of Lud (:615-626): weight[p] = (|e_p| + 1e-2)^(-1/2) and sum_e = the tree's sum of |e_p|, both on dir_p.  Upstream normalises R_w2 t_21 in the functor
// and rotates the normalised t_21 in the weight: the two differ by rounding only, one dir_p serves both.
#pragma once
#include <cmath>
#include <vector>

#include "pvlm_pairgraph_core.h"
#include "pvlm_transavg_core.h"

#if defined(__HIPCC__)
#define PVLM_TD_HD __host__ __device__ __forceinline__
#else
#define PVLM_TD_HD inline
#endif

namespace pvlm_transdir {

namespace pg = pvlm_pairgraph;
namespace ta = pvlm_transavg;

// bnd[4] = ScaleFactor upper, lower, parameter lower, parameter upper of a Lud pair that comes in at s0
PVLM_TD_HD void lud_bounds(double s0, double upper_ratio, double lower_ratio, double* bnd) {
  if (s0 != 1) { bnd[0] = s0 * upper_ratio; bnd[1] = s0 * lower_ratio; bnd[2] = s0 * 0.5; bnd[3] = s0 * 3.0; }
  else { bnd[0] = 2.0; bnd[1] = 1.0; bnd[2] = 1.0; bnd[3] = 1.7976931348623157e308; }
}

// Lud: e = ci - cj - s dir and its length
PVLM_TD_HD double lud_error(const double* dir, const double* ci, const double* cj, double s, double* e) {
  for (int k = 0; k < 3; ++k) e[k] = ci[k] - cj[k] - s * dir[k];
  return sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
}
// Chordal: u / n, r = u / n - dir; returns n (0: the outputs are NaN)
PVLM_TD_HD double chordal_residual(const double* dir, const double* ci, const double* cj, double* unit, double* r) {
  const double u[3] = {ci[0] - cj[0], ci[1] - cj[1], ci[2] - cj[2]};
  const double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) { unit[k] = u[k] / n; r[k] = unit[k] - dir[k]; }
  return n;
}

// The pair model of TranslationAveragingL2Chordal (pvlm_pairgraph_core.h, at lm_solve): no scale, so the reduced block and gradient of the layer's record equal the
// unreduced ones.  dir: the unit directions (3 per pair).
struct Chordal {
  // the record after the two sides: u / n (3), n, rho', r (3)
  enum { kUnit = 30, kNorm = 33, kRw = 34, kRes = 35 };
  static constexpr int kSlots = 38, kTerms = 2;
  static constexpr bool kScale = false;
  const double* dir;

  // 0.5 rho(|r|^2), NaN when the two centres coincide
  PVLM_TD_HD double cost(long long p, const double* ci, const double* cj, double, double a) const {
    const double d[3] = {dir[3 * p], dir[3 * p + 1], dir[3 * p + 2]};
    double unit[3], r[3], rho, rho1;
    chordal_residual(d, ci, cj, unit, r);
    pg::huber(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rho1);
    return 0.5 * rho;
  }
  PVLM_TD_HD void linearise(long long p, const double* ci, const double* cj, double, double a, double, double, double, bool, double*, double* rec, long long P,
                            double* off) const {
    const double d[3] = {dir[3 * p], dir[3 * p + 1], dir[3 * p + 2]};
    double* si = rec; double* sj = rec + (long long)pg::kCam * P;
    double unit[3], r[3], rho, rw;
    const double n = chordal_residual(d, ci, cj, unit, r);
    pg::huber(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rw);
    const double ur = unit[0] * r[0] + unit[1] * r[1] + unit[2] * r[2];
    int t = 0;
    for (int x = 0; x < 3; ++x)
      for (int y = x; y < 3; ++y, ++t) {
        const double h = rw * (((x == y ? 1.0 : 0.0) - unit[x] * unit[y]) / (n * n));
        si[t * P] = h; sj[t * P] = h;
        if (x == y) { si[(6 + x) * P] = h; sj[(6 + x) * P] = h; }
      }
    for (int k = 0; k < 3; ++k) {
      const double gi = rw * ((r[k] - unit[k] * ur) / n);
      si[(9 + k) * P] = gi; sj[(9 + k) * P] = -gi; si[(12 + k) * P] = gi; sj[(12 + k) * P] = -gi;
      rec[(kUnit + k) * P] = unit[k]; rec[(kRes + k) * P] = r[k];
      for (int y = 0; y < 3; ++y) off[6 * k + y] = -(rw * (((k == y ? 1.0 : 0.0) - unit[k] * unit[y]) / (n * n)));
    }
    rec[kNorm * P] = n; rec[kRw * P] = rw;
  }
  // dti / dtj: the steps of the pair's two cameras, cti / ctj: their candidates
  PVLM_TD_HD void step(long long p, const double* rec, long long P, const double* dti, const double* dtj, const double* cti, const double* ctj, double, double a, double*,
                       double* terms, long long tstride) const {
    const double d[3] = {dti[0] - dtj[0], dti[1] - dtj[1], dti[2] - dtj[2]};
    const double n = rec[kNorm * P], rw = rec[kRw * P];
    const double ud = rec[kUnit * P] * d[0] + rec[(kUnit + 1) * P] * d[1] + rec[(kUnit + 2) * P] * d[2];
    double rv = 0, vv = 0;
    for (int k = 0; k < 3; ++k) { const double v = (d[k] - rec[(kUnit + k) * P] * ud) / n; rv += rec[(kRes + k) * P] * v; vv += v * v; }
    terms[pg::kTermCost * tstride] = cost(p, cti, ctj, 0.0, a);
    terms[pg::kTermModel * tstride] = -(rw * rv + 0.5 * rw * vv);
  }
};

// The pair model of one LUD solve: the scale of every pair is eliminated by its 1 x 1 pivot.  dir: the unit directions (3 per pair), bnd: lud_bounds() (4), w: the
// weights (1).  The loss parameter a is not read.
struct Lud {
  // the record after the two sides: the scale's pivot and gradient, q (3), df/ds, f, the ScaleFactor's residual and derivative
  enum { kPiv = 30, kQ = 32, kJs = 35, kF = 36, kF2 = 37, kJf = 38 };
  static constexpr int kSlots = 39, kTerms = 4, kGs = 31;
  static constexpr bool kScale = true;
  const double *dir, *bnd, *w;

  // the pair's inputs into the lane's registers
  PVLM_TD_HD void load(long long p, double* dp, double* bp) const {
    for (int k = 0; k < 3; ++k) dp[k] = dir[3 * p + k];
    for (int k = 0; k < 4; ++k) bp[k] = bnd[4 * p + k];
  }
  // 0.5 w^2 |e| + 0.5 f2^2
  PVLM_TD_HD static double cost_of(const double* dp, const double* bp, double wp, const double* ci, const double* cj, double s) {
    double e[3], f2, jf;
    const double f = wp * sqrt(lud_error(dp, ci, cj, s, e));
    ta::scale_factor(s, bp, &f2, &jf);
    return 0.5 * f * f + 0.5 * f2 * f2;
  }
  PVLM_TD_HD double cost(long long p, const double* ci, const double* cj, double s, double) const {
    double dp[3], bp[4];
    load(p, dp, bp);
    return cost_of(dp, bp, w[p], ci, cj, s);
  }
  // first_time: the Jacobi scale of s is taken here (*sigma), else read
  PVLM_TD_HD void linearise(long long p, const double* ci, const double* cj, double s, double, double radius, double min_diag, double max_diag, bool first_time,
                            double* sigma, double* rec, long long P, double* off) const {
    double dp[3], bp[4];
    load(p, dp, bp);
    const double wp = w[p];
    double* si = rec; double* sj = rec + (long long)pg::kCam * P;
    double e[3], q[3], f2, jf;
    const double m = lud_error(dp, ci, cj, s, e), f = wp * sqrt(m), g = m > 0.0 ? wp * 0.5 / (m * sqrt(m)) : 0.0;
    for (int k = 0; k < 3; ++k) q[k] = g * e[k];
    const double js = -(q[0] * dp[0] + q[1] * dp[1] + q[2] * dp[2]);
    ta::scale_factor(s, bp, &f2, &jf);
    const double hss = js * js + jf * jf;
    if (first_time) *sigma = 1.0 / (1.0 + sqrt(hss));
    const double sg = *sigma;
    const double piv = hss + pg::clip(sg * sg * hss, min_diag, max_diag) / radius / (sg * sg), gs = js * f + jf * f2;
    int t = 0;
    for (int x = 0; x < 3; ++x)
      for (int y = x; y < 3; ++y, ++t) {
        // the couplings with the scale are +- q js: their products are the same on both sides
        const double red = q[x] * q[y] - (q[x] * js) * (q[y] * js) / piv;
        si[t * P] = red; sj[t * P] = red;
        if (x == y) { si[(6 + x) * P] = q[x] * q[x]; sj[(6 + x) * P] = q[x] * q[x]; }
      }
    for (int k = 0; k < 3; ++k) {
      const double gi = q[k] * f, c = q[k] * js;
      si[(9 + k) * P] = gi; sj[(9 + k) * P] = -gi;
      si[(12 + k) * P] = gi - c * gs / piv; sj[(12 + k) * P] = -gi + c * gs / piv;
      rec[(kQ + k) * P] = q[k];
      for (int y = 0; y < 3; ++y) off[6 * k + y] = -q[k] * q[y] + c * (q[y] * js) / piv;
    }
    rec[kPiv * P] = piv; rec[kGs * P] = gs; rec[kJs * P] = js; rec[kF * P] = f; rec[kF2 * P] = f2; rec[kJf * P] = jf;
  }
  // the scale step from the camera steps (dti / dtj), the clamp, the candidate scale and the pair's terms at the candidates cti / ctj
  PVLM_TD_HD void step(long long p, const double* rec, long long P, const double* dti, const double* dtj, const double* cti, const double* ctj, double s, double,
                       double* s_cand, double* terms, long long tstride) const {
    double dp[3], bp[4];
    load(p, dp, bp);
    const double d[3] = {dti[0] - dtj[0], dti[1] - dtj[1], dti[2] - dtj[2]};
    const double piv = rec[kPiv * P], gs = rec[kGs * P], js = rec[kJs * P], f = rec[kF * P], f2 = rec[kF2 * P], jf = rec[kJf * P];
    const double qd = rec[kQ * P] * d[0] + rec[(kQ + 1) * P] * d[1] + rec[(kQ + 2) * P] * d[2];
    const double sc = ta::clamp_scale(s + (-gs - js * qd) / piv, bp), ds = sc - s;
    const double v = qd + js * ds, v2 = jf * ds;
    *s_cand = sc;
    terms[pg::kTermCost * tstride] = cost_of(dp, bp, w[p], cti, ctj, sc);
    terms[pg::kTermModel * tstride] = -(f * v + 0.5 * v * v) - (f2 * v2 + 0.5 * v2 * v2);
    terms[pg::kTermStep2 * tstride] = ds * ds;
    terms[pg::kTermX2 * tstride] = s * s;
  }
};

// Lud's write-back: the next weight of the pair, its |e| in *m
PVLM_TD_HD double final_weight(const double* dir, const double* ci, const double* cj, double s, double* m) {
  double e[3];
  *m = lud_error(dir, ci, cj, s, e);
  return pow(*m + 1e-2, -0.5);
}

// nullptr, or what is wrong with the shared arguments of the two entry points
inline const char* check_pairs(int F, int P, const int* first, const int* second, const double* dir) {
  if (F < 0 || P < 0) return "a negative count";
  if (P > 0 && (!first || !second || !dir)) return "null argument";
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= F || second[p] < 0 || second[p] >= F) return "a pair names a camera that is not there";
    if (first[p] == second[p]) return "a pair of a camera with itself";
    const double* d = dir + 3 * (size_t)p;
    if (!pg::finite_all(d, 3)) return "a direction is not finite";
    if (!(std::fabs(std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0) <= 1e-9)) return "a direction is not of unit length";
  }
  return nullptr;
}
// nullptr, or what is wrong with the centres and the origin
inline const char* check_centres(int F, int origin, const double* centres) {
  if (origin < 0 || origin >= F) return "origin_idx names no camera";
  if (!pg::finite_all(centres, 3 * (size_t)F)) return "a centre is not finite";
  for (int k = 0; k < 3; ++k) if (centres[3 * (size_t)origin + k] != 0.0) return "the centre of the origin camera is not zero";
  return nullptr;
}
inline pg::Options chordal_options(double loss_a, int max_num_iterations) {
  pg::Options o;
  o.loss_a = loss_a; o.max_num_iterations = max_num_iterations; o.function_tolerance = 1e-7; o.parameter_tolerance = 1e-8;      // :254-257
  return o;
}

}  // namespace pvlm_transdir
