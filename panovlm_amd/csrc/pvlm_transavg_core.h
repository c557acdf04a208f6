// K42: the definition of translation averaging (TranslationAveragingL2 / TranslationAveragingDLT, sfm/TranslationAveraging.cpp:31-169) — host and device.
// Compiled for the device by pvlm_transavg.hip and for the host by tests/cpp/transavg_core_check.cpp; both run the SAME Levenberg-Marquardt policy (lm_solve below) over
// a backend that evaluates, gathers, solves and steps.
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
// Trust region: the constants and the policy of ceres_like::Solve (host/pvlm_host.hpp Solver::Options): Jacobi scaling 1 / (1 + sqrt(H_kk)) from the first
// linearisation, radius / max(1/3, 1 - (2 rho - 1)^3) on success, radius / 2, / 4, ... on failure, min_relative_decrease 1e-3 and the three tolerances.
// Sums: every scalar (cost, model decrease, step and parameter norms) is the root of a fixed tree over its per-pair or per-camera terms: leaves in chunks of kChunk,
// a halving tree inside a chunk, the chunk sums reduced the same way.  The tree depends on the count alone.
// Write-back (:160-166): final cost, weight[i] = (|t2 - R t1 - scales[i] * t_21| + 1e-2)^-0.5 — with t_21 NOT normalised, as line 165 is written.
#pragma once
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define PVLM_TA_HD __host__ __device__ __forceinline__
#else
#define PVLM_TA_HD inline
#endif

namespace pvlm_transavg {

constexpr int kGroup = 8;            // lanes that share one camera's gather
constexpr int kChunk = 256;          // leaves under one node of the reduction tree
constexpr int kCam = 15;             // per camera: reduced diagonal block (6, upper triangle by rows), diagonal of the unreduced block (3), gradient (3), reduced gradient (3)
// per-pair record, component-major (component k of pair p at [k * P + p]): side 0 (first) and side 1 (second) as kCam numbers each, then
enum { kPiv = 30, kGs = 31, kCi = 32, kCj = 35, kRw = 38, kRes = 39, kF = 42, kJf = 43, kPairSlots = 44 };
enum { kTermCost = 0, kTermModel = 1, kTermStep2 = 2, kTermX2 = 3, kPairTerms = 4 };
// termination codes on K36's numbering
enum { kMaxIterations = 0, kFunctionTol = 1, kGradientTol = 2, kParameterTol = 3, kRadiusCollapsed = 4, kCostNotFinite = 5, kNoPairs = 6 };

struct Options {
  double loss_a = 0.01;
  int max_num_iterations = 50;
  double initial_radius = 1e4, max_radius = 1e16, min_radius = 1e-32;
  double min_relative_decrease = 1e-3, function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
};
struct Summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; };

PVLM_TA_HD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

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

PVLM_TA_HD void loss(double a, double s2, double* rho, double* rho1) {
  if (a < 0) { *rho = s2; *rho1 = 1.0; return; }
  const double b = a * a, c = 1.0 / b, tmp = sqrt(1.0 + s2 * c);
  *rho = 2.0 * b * (tmp - 1.0); *rho1 = 1.0 / tmp;
}
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
  loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rho1);
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
    loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rw);
    scale_factor(s, bnd, &f, &jf);
    const double hss = rw * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + jf * jf;
    if (first_time) *sigma = 1.0 / (1.0 + sqrt(hss));
    const double sg = *sigma;
    piv = hss + clip(sg * sg * hss, min_diag, max_diag) / radius / (sg * sg);
    gs = -rw * (d[0] * r[0] + d[1] * r[1] + d[2] * r[2]) + jf * f;
    for (int k = 0; k < 3; ++k) { ci[k] = rw * (R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]); cj[k] = -rw * d[k]; }
  }
  double* si = rec; double* sj = rec + (long long)kCam * P;
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

// Kernel b, lane `lane` of the kGroup lanes of one camera: its part of the row ent[e0 .. e1) (entry = 2 * pair + side), in list order.
PVLM_TA_HD void gather_lane(const double* rec, long long P, const int* ent, int e0, int e1, int lane, double* part) {
  for (int k = 0; k < kCam; ++k) part[k] = 0.0;
  for (int e = e0 + lane; e < e1; e += kGroup) {
    const int p = ent[e] >> 1, side = ent[e] & 1;
    const double* s = rec + (long long)side * kCam * P + p;
    for (int k = 0; k < kCam; ++k) part[k] += s[(long long)k * P];
  }
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
  terms[kTermCost * tstride] = pair_cost(R, d, bnd, cti, ctj, sc, a);
  terms[kTermModel * tstride] = -(rw * ru + 0.5 * rw * uu) - (f * v + 0.5 * v * v);
  terms[kTermStep2 * tstride] = ds * ds;
  terms[kTermX2 * tstride] = s * s;
}

// one node of the reduction tree: up to kChunk leaves, zero-padded, halved
template <bool MAX> PVLM_TA_HD double tree_op(double x, double y) { return MAX ? fmax(x, y) : x + y; }

PVLM_TA_HD double final_weight(const double* R, const double* t21, const double* ti, const double* tj, double s) {
  double r[3];
  residual(R, t21, ti, tj, s, r);
  return pow(sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + 1e-2, -0.5);
}

// ---- host side: shared by the device entry points and by the host compile ----------------------------------------------------------------------------------

template <bool MAX> inline double tree_reduce_host(const double* v, long long n) {
  std::vector<double> cur(v, v + n), nxt;
  if (n <= 0) return 0.0;
  for (;;) {
    const long long m = ((long long)cur.size() + kChunk - 1) / kChunk;
    nxt.assign((size_t)m, 0.0);
    for (long long b = 0; b < m; ++b) {
      double buf[kChunk];
      for (int i = 0; i < kChunk; ++i) { const long long j = b * kChunk + i; buf[i] = j < (long long)cur.size() ? cur[(size_t)j] : 0.0; }
      for (int s = kChunk / 2; s > 0; s >>= 1) for (int i = 0; i < s; ++i) buf[i] = tree_op<MAX>(buf[i], buf[i + s]);
      nxt[(size_t)b] = buf[0];
    }
    cur.swap(nxt);
    if (cur.size() == 1) return cur[0];
  }
}

// the CSR of the cameras' incident pairs: entry = 2 * pair + side, in pair-list order
inline void build_csr(int F, int P, const int* first, const int* second, std::vector<int>* off, std::vector<int>* ent) {
  off->assign((size_t)F + 1, 0); ent->assign(2 * (size_t)P, 0);
  for (int p = 0; p < P; ++p) { ++(*off)[(size_t)first[p] + 1]; ++(*off)[(size_t)second[p] + 1]; }
  for (int c = 0; c < F; ++c) (*off)[(size_t)c + 1] += (*off)[(size_t)c];
  std::vector<int> at(off->begin(), off->end() - 1);
  for (int p = 0; p < P; ++p) { (*ent)[(size_t)at[(size_t)first[p]]++] = 2 * p; (*ent)[(size_t)at[(size_t)second[p]]++] = 2 * p + 1; }
}

inline bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// nullptr, or what is wrong with the shared arguments of the two entry points
inline const char* check_pairs(int F, int P, const int* first, const int* second, const double* R, const double* t21) {
  if (F < 0 || P < 0) return "a negative count";
  if (P > 0 && (!first || !second || !R || !t21)) return "null argument";
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= F || second[p] < 0 || second[p] >= F) return "a pair names a camera that is not there";
    if (first[p] == second[p]) return "a pair of a camera with itself";
    double d[3];
    if (!finite_all(R + 9 * (size_t)p, 9) || !finite_all(t21 + 3 * (size_t)p, 3)) return "a relative pose is not finite";
    if (!direction(t21 + 3 * (size_t)p, d)) return "a relative translation of zero length";
  }
  return nullptr;
}

// The camera system of one linearisation on the host's side: the index lists of the reduced blocks ([F diagonal | P off-diagonal], 6 x 6 with the last three
// indices -1), the Jacobi scale of the cameras and, per solve, the LM diagonal and the right-hand side.  cam: the gather (kCam numbers per camera).
struct CameraSystem {
  int F = 0, P = 0, origin = -1, n = 0;
  std::vector<int> rows, cols, mirror;
  std::vector<double> sigma, diag, rhs;
  int index(int c) const { return c == origin ? -1 : 3 * (c < origin || origin < 0 ? c : c - 1); }
  void init(int F_, int P_, const int* first, const int* second, int origin_) {
    F = F_; P = P_; origin = origin_; n = 3 * (origin >= 0 ? F - 1 : F);
    rows.assign(6 * ((size_t)F + P), -1); cols.assign(6 * ((size_t)F + P), -1); mirror.assign((size_t)F + P, 0);
    for (int c = 0; c < F; ++c) for (int k = 0; k < 3; ++k) if (index(c) >= 0) rows[6 * (size_t)c + k] = cols[6 * (size_t)c + k] = index(c) + k;
    for (int p = 0; p < P; ++p) {
      const size_t b = (size_t)F + p;
      mirror[b] = 1;
      for (int k = 0; k < 3; ++k) { if (index(first[p]) >= 0) rows[6 * b + k] = index(first[p]) + k; if (index(second[p]) >= 0) cols[6 * b + k] = index(second[p]) + k; }
    }
    sigma.assign((size_t)n, 1.0); diag.assign((size_t)n, 0.0); rhs.assign((size_t)n, 0.0);
  }
  void set_sigma(const double* cam) {
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) sigma[(size_t)index(c) + k] = 1.0 / (1.0 + std::sqrt(std::fmax(cam[(size_t)kCam * c + 6 + k], 0.0)));
  }
  // damped: the LM diagonal clip(sigma^2 H_kk) / radius; otherwise none (the DLT)
  void prepare(const double* cam, bool damped, double radius, const Options& o) {
    for (int c = 0; c < F; ++c) {
      if (index(c) < 0) continue;
      for (int k = 0; k < 3; ++k) {
        const size_t i = (size_t)index(c) + k; const double sg = sigma[i];
        diag[i] = damped ? clip(sg * sg * cam[(size_t)kCam * c + 6 + k], o.min_lm_diagonal, o.max_lm_diagonal) / radius : 0.0;
        rhs[i] = -sg * cam[(size_t)kCam * c + 12 + k];
      }
    }
  }
  // the solved rhs -> the step of every camera (3 F, zero at the origin)
  void expand(std::vector<double>* step) const {
    step->assign(3 * (size_t)F, 0.0);
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) (*step)[3 * (size_t)c + k] = sigma[(size_t)index(c) + k] * rhs[(size_t)index(c) + k];
  }
  double gradient_max(const double* cam) const {
    double g = 0;
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) g = std::fmax(g, std::fabs(cam[(size_t)kCam * c + 9 + k]));
    return g;
  }
};

struct Scalars { double cost, model, step2, x2; };

// The LM loop.  Backend: double initial_cost(); double linearise(double radius, bool first) -> max |g|; bool solve(double radius) (false: no step);
// Scalars candidate(); void accept(); bool failed() (a device error: the loop stops).
template <class B> inline void lm_solve(B& be, const Options& o, Summary* out) {
  Summary s{0.0, 0.0, 0, 0, -1};
  double cost = be.initial_cost();
  s.initial_cost = cost;
  double radius = o.initial_radius, dec = 2.0;
  int it = 0;
  if (!std::isfinite(cost)) s.termination = kCostNotFinite;
  else if (o.max_num_iterations > 0 && be.linearise(radius, true) <= o.gradient_tolerance) s.termination = kGradientTol;
  while (s.termination < 0 && it < o.max_num_iterations && !be.failed()) {
    ++it;
    bool ok = be.solve(radius), accepted = false;
    Scalars c{0, 0, 0, 0};
    if (ok) { c = be.candidate(); ok = c.model > 0 && std::isfinite(c.model); }
    if (ok) {
      const double rho = (cost - c.cost) / c.model;
      if (std::isfinite(c.cost) && rho > o.min_relative_decrease) {
        accepted = true;
        const double change = cost - c.cost, prev = cost;
        be.accept();
        cost = c.cost;
        radius = std::fmin(o.max_radius, radius / std::fmax(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0)));
        dec = 2.0;
        ++s.successful_steps;
        if (std::fabs(change) <= o.function_tolerance * prev) s.termination = kFunctionTol;
        else if (be.linearise(radius, false) <= o.gradient_tolerance) s.termination = kGradientTol;
        else if (std::sqrt(c.step2) <= o.parameter_tolerance * (std::sqrt(c.x2) + o.parameter_tolerance)) s.termination = kParameterTol;
      }
    }
    if (!accepted) {
      ++s.unsuccessful_steps;
      radius /= dec; dec *= 2.0;
      if (radius < o.min_radius) s.termination = kRadiusCollapsed;
      else if (it < o.max_num_iterations) be.linearise(radius, false);
    }
  }
  if (s.termination < 0) s.termination = kMaxIterations;
  s.final_cost = cost;
  *out = s;
}

}  // namespace pvlm_transavg
