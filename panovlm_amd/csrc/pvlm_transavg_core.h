// K42: the definition of translation averaging (TranslationAveragingL2 / TranslationAveragingDLT, sfm/TranslationAveraging.cpp:31-169) — host and device.
// Compiled for the device by pvlm_transavg.hip and for the host by tests/cpp/transavg_core_check.cpp; both run the SAME Levenberg-Marquardt policy (lm_solve of
// pvlm_pairgraph_core.h, with its camera system, gather and fixed reduction tree) over a backend that evaluates, gathers, solves and steps.
//
// Unknowns: one translation t_c per camera (the camera origin_idx is constant and zero) and one private scale s_p per pair.  Residual blocks:
//   pair p:   r = t[second] - R_21 t[first] - s_p d_p,  d_p = t_21 / |t_21|  (base/CostFunction.h:51-83), Jacobians -R_21, I, -d_p; the loss acts on |r|^2:
//             SoftLOneLoss(a), rho(s) = 2 b (sqrt(1 + s / b) - 1), b = a^2, or none when a < 0 (:184-185).  rho'' <= 0, so the corrector scales r and J by sqrt(rho').
//             The functor's `weight` member is never applied upstream (operator() does not read it): it is not applied here either.
//             Upstream turns R_21 into an angle-axis vector and rotates with AngleAxisRotatePoint; R_21 is used directly (the divergence K36 documents).
//   scale p:  ScaleFactor(upper, lower, 1) (CostFunction.h:119-144), no loss: f = s - upper above, lower - s below, 0 between, the branch taken by value.
//             scales[p] != 1 (as written, :101): upper / lower = ratio * s0 and the parameter bounds [0.5 s0, 3 s0]; otherwise ScaleFactor(2, 1), no parameter bounds.
// One LM iteration eliminates every scale (a 1 x 1 pivot: rho' d.d + jf^2 + its LM diagonal), gathers the reduced 3 x 3 blocks per camera over a CSR of its incident
// pairs (pair-list order split over kGroup lanes, then an xor butterfly: one order, no floating-point atomics), solves the camera system, back-substitutes the scale
// steps, CLAMPS the candidate scales onto their parameter bounds and evaluates the candidate; the step quality is taken against the model at the clamped step.
// Ceres' own treatment of bounds (projection plus a line search) cannot be pinned down here: clamp-without-line-search is the stand-in.
// Sums: every scalar (cost, model decrease, step and parameter norms) is the root of the fixed tree over its per-pair or per-camera terms.
// Write-back (:160-166): final cost, weight[i] = (|t2 - R t1 - scales[i] * t_21| + 1e-2)^-0.5 — with t_21 NOT normalised, as line 165 is written.
#pragma once
#include <cmath>
#include <vector>

#include "pvlm_pairgraph_core.h"

#if defined(__HIPCC__)
#define PVLM_TA_HD __host__ __device__ __forceinline__
#else
#define PVLM_TA_HD inline
#endif

namespace pvlm_transavg {

namespace pg = pvlm_pairgraph;

// per-pair record, component-major (component k of pair p at [k * P + p]): side 0 (first) and side 1 (second) as pg::kCam numbers each, then
enum { kPiv = 30, kGs = 31, kCi = 32, kCj = 35, kRw = 38, kRes = 39, kF = 42, kJf = 43, kPairSlots = 44 };

// d = t_21 / |t_21| (Eigen's normalize); false: zero length or not finite
PVLM_TA_HD bool direction(const double* t, double* d) {
  const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  if (!(n > 0.0) || !(n < 1.7e308)) return false;
  d[0] = t[0] / n; d[1] = t[1] / n; d[2] = t[2] / n;
  return true;
}

// bnd[4] = ScaleFactor upper, lower, parameter lower, parameter upper of a pair that starts at s0
PVLM_TA_HD void bounds(double s0, double upper_ratio, double lower_ratio, double* bnd) {
  if (s0 != 1) { bnd[0] = s0 * upper_ratio; bnd[1] = s0 * lower_ratio; bnd[2] = s0 * 0.5; bnd[3] = s0 * 3.0; }
  else { bnd[0] = 2.0; bnd[1] = 1.0; bnd[2] = -1.7976931348623157e308; bnd[3] = 1.7976931348623157e308; }
}
PVLM_TA_HD double clamp_scale(double s, const double* bnd) { return fmin(fmax(s, bnd[2]), bnd[3]); }

PVLM_TA_HD void scale_factor(double s, const double* bnd, double* f, double* jf) {
  if (s > bnd[0]) { *f = s - bnd[0]; *jf = 1.0; }
  else if (s < bnd[1]) { *f = bnd[1] - s; *jf = -1.0; }
  else { *f = 0.0; *jf = 0.0; }
}
// R row-major; r = tj - R ti - s d
PVLM_TA_HD void residual(const double* R, const double* d, const double* ti, const double* tj, double s, double* r) {
  for (int k = 0; k < 3; ++k) r[k] = tj[k] - (R[3 * k] * ti[0] + R[3 * k + 1] * ti[1] + R[3 * k + 2] * ti[2]) - s * d[k];
}
// the pair's cost term: 0.5 rho(|r|^2) + 0.5 f^2
PVLM_TA_HD double pair_cost(const double* R, const double* d, const double* bnd, const double* ti, const double* tj, double s, double a) {
  double r[3], rho, rho1, f, jf;
  residual(R, d, ti, tj, s, r);
  pg::loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rho1);
  scale_factor(s, bnd, &f, &jf);
  return 0.5 * rho + 0.5 * f * f;
}

// Kernel a for one pair: the linearisation at (ti, tj, s) with the scale eliminated.  rec: the pair's record (stride P), off: the 3 x 3 block between first (rows)
// and second (columns), written into a 6 x 6 row-major block.  first_time: the Jacobi scale of s is taken here (*sigma), else read.
// dlt: the block of TranslationAveragingDLT instead (r = tj - R ti - d with d = t_21 itself, no scale, no loss).
PVLM_TA_HD void linearise_pair(const double* R, const double* d, const double* bnd, const double* ti, const double* tj, double s, double a, double radius,
                               double min_diag, double max_diag, bool first_time, bool dlt, double* sigma, double* rec, long long P, double* off) {
  double r[3], rho = 0, rw = 1, f = 0, jf = 0, piv = 1, gs = 0, ci[3] = {0, 0, 0}, cj[3] = {0, 0, 0};
  residual(R, d, ti, tj, dlt ? 1.0 : s, r);
  if (!dlt) {
    pg::loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rw);
    scale_factor(s, bnd, &f, &jf);
    const double hss = rw * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + jf * jf;
    if (first_time) *sigma = 1.0 / (1.0 + sqrt(hss));
    const double sg = *sigma;
    piv = hss + pg::clip(sg * sg * hss, min_diag, max_diag) / radius / (sg * sg);
    gs = -rw * (d[0] * r[0] + d[1] * r[1] + d[2] * r[2]) + jf * f;
    for (int k = 0; k < 3; ++k) { ci[k] = rw * (R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]); cj[k] = -rw * d[k]; }
  }
  double* si = rec; double* sj = rec + (long long)pg::kCam * P;
  int q = 0;
  for (int x = 0; x < 3; ++x)
    for (int y = x; y < 3; ++y, ++q) {
      const double rtr = R[x] * R[y] + R[3 + x] * R[3 + y] + R[6 + x] * R[6 + y];
      si[q * P] = rw * rtr - ci[x] * ci[y] / piv;
      sj[q * P] = (x == y ? rw : 0.0) - cj[x] * cj[y] / piv;
      if (x == y) { si[(6 + x) * P] = rw * rtr; sj[(6 + x) * P] = rw; }
    }
  for (int k = 0; k < 3; ++k) {
    const double gi = -rw * (R[k] * r[0] + R[3 + k] * r[1] + R[6 + k] * r[2]), gj = rw * r[k];
    si[(9 + k) * P] = gi; sj[(9 + k) * P] = gj;
    si[(12 + k) * P] = gi - ci[k] * gs / piv; sj[(12 + k) * P] = gj - cj[k] * gs / piv;
    rec[(kCi + k) * P] = ci[k]; rec[(kCj + k) * P] = cj[k]; rec[(kRes + k) * P] = r[k];
    for (int y = 0; y < 3; ++y) off[6 * k + y] = -rw * R[3 * y + k] - ci[k] * cj[y] / piv;
  }
  rec[kPiv * P] = piv; rec[kGs * P] = gs; rec[kRw * P] = rw; rec[kF * P] = f; rec[kJf * P] = jf;
}

// Kernel d for one pair: the scale step from the camera steps, the clamp, the candidate scale and the pair's terms.  dti / dtj: the steps of its two cameras.
PVLM_TA_HD void step_pair(const double* R, const double* d, const double* bnd, const double* rec, long long P, const double* dti, const double* dtj,
                          const double* cti, const double* ctj, double s, double a, double* s_cand, double* terms, long long tstride) {
  const double piv = rec[kPiv * P], gs = rec[kGs * P], rw = rec[kRw * P], f = rec[kF * P], jf = rec[kJf * P];
  double dot = 0;
  for (int k = 0; k < 3; ++k) dot += rec[(kCi + k) * P] * dti[k] + rec[(kCj + k) * P] * dtj[k];
  const double sc = clamp_scale(s + (-gs - dot) / piv, bnd), ds = sc - s;
  double ru = 0, uu = 0;
  for (int k = 0; k < 3; ++k) {
    const double u = dtj[k] - (R[3 * k] * dti[0] + R[3 * k + 1] * dti[1] + R[3 * k + 2] * dti[2]) - ds * d[k];
    ru += rec[(kRes + k) * P] * u; uu += u * u;
  }
  const double v = jf * ds;
  *s_cand = sc;
  terms[pg::kTermCost * tstride] = pair_cost(R, d, bnd, cti, ctj, sc, a);
  terms[pg::kTermModel * tstride] = -(rw * ru + 0.5 * rw * uu) - (f * v + 0.5 * v * v);
  terms[pg::kTermStep2 * tstride] = ds * ds;
  terms[pg::kTermX2 * tstride] = s * s;
}

// The pair model of both entry points (pvlm_pairgraph_core.h, at lm_solve).  R: R_21 (9 per pair), d: the direction, or t_21 itself with dlt (3), bnd: bounds() (4).
struct Model {
  static constexpr int kSlots = kPairSlots, kTerms = 4, kGs = pvlm_transavg::kGs;
  static constexpr bool kScale = true;
  const double *R, *d, *bnd;
  bool dlt;

  // the pair's inputs into the lane's registers
  PVLM_TA_HD void load(long long p, double* Rp, double* dp, double* bp) const {
    for (int k = 0; k < 9; ++k) Rp[k] = R[9 * p + k];
    for (int k = 0; k < 3; ++k) dp[k] = d[3 * p + k];
    for (int k = 0; k < 4; ++k) bp[k] = bnd[4 * p + k];
  }
  PVLM_TA_HD double cost(long long p, const double* ti, const double* tj, double s, double a) const {
    double Rp[9], dp[3], bp[4];
    load(p, Rp, dp, bp);
    return pair_cost(Rp, dp, bp, ti, tj, s, a);
  }
  PVLM_TA_HD void linearise(long long p, const double* ti, const double* tj, double s, double a, double radius, double min_diag, double max_diag, bool first_time,
                            double* sigma, double* rec, long long P, double* off) const {
    double Rp[9], dp[3], bp[4];
    load(p, Rp, dp, bp);
    linearise_pair(Rp, dp, bp, ti, tj, s, a, radius, min_diag, max_diag, first_time, dlt, sigma, rec, P, off);
  }
  PVLM_TA_HD void step(long long p, const double* rec, long long P, const double* dti, const double* dtj, const double* cti, const double* ctj, double s, double a,
                       double* s_cand, double* terms, long long tstride) const {
    double Rp[9], dp[3], bp[4];
    load(p, Rp, dp, bp);
    step_pair(Rp, dp, bp, rec, P, dti, dtj, cti, ctj, s, a, s_cand, terms, tstride);
  }
};

PVLM_TA_HD double final_weight(const double* R, const double* t21, const double* ti, const double* tj, double s) {
  double r[3];
  residual(R, t21, ti, tj, s, r);
  return pow(sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + 1e-2, -0.5);
}

// nullptr, or what is wrong with the shared arguments of the two entry points
inline const char* check_pairs(int F, int P, const int* first, const int* second, const double* R, const double* t21) {
  if (F < 0 || P < 0) return "a negative count";
  if (P > 0 && (!first || !second || !R || !t21)) return "null argument";
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= F || second[p] < 0 || second[p] >= F) return "a pair names a camera that is not there";
    if (first[p] == second[p]) return "a pair of a camera with itself";
    double d[3];
    if (!pg::finite_all(R + 9 * (size_t)p, 9) || !pg::finite_all(t21 + 3 * (size_t)p, 3)) return "a relative pose is not finite";
    if (!direction(t21 + 3 * (size_t)p, d)) return "a relative translation of zero length";
  }
  return nullptr;
}

}  // namespace pvlm_transavg
