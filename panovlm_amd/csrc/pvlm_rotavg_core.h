// K40: the definition of rotation averaging (RotationAveragingRefineL1 and RotationAveragingL2, sfm/RotationAveraging.cpp:317-374, :428-582) — host and device.
// Compiled for the device by pvlm_rotavg.hip and for the host by tests/cpp/rotavg_core_check.cpp; both run the SAME drivers (l1_solve below, lm_solve of pvlm_pairgraph_core.h)
// over a backend that evaluates, gathers, multiplies, solves and steps.  F cameras, P pairs (first, second, R_21 row-major), rotations R_cw row-major.
//
// Pair error (:476-478): e_p = log((R_2w^T R_21) R_1w), log = RotationMatrixToAngleAxis of host/pvlm_host.cpp with its branches.
// Rows.  Upstream carries every pair twice, (i, j, R_21) and (j, i, R_21^T), 2 P rows of three.  The mirrored row has the negated incidence (-1 at its first camera,
//   +1 at its second) and the error -e_p up to rounding; z = u = 0 at the start and an odd shrinkage keep the mirrored half of every ADMM vector the negative of the
//   first half.  The core carries the P rows of the list and the factors that follow: A^T v over 2 P rows = 2 A_h^T v_h, A^T A = 2 L (x) I_3 (L: the Laplacian of the
//   pair graph with row and column start_idx removed), every two-norm over the rows = sqrt(2) times the norm over the half.  x, y and z decouple.
// L1 stage (:460-503).  Per outer iteration: b = the errors, then the ADMM of least absolute deviations (Boyd et al. 2011, section 6.1) with rho = 1, alpha = 1:
//     x = (A^T A)^-1 A^T (b + z - u);  z+ = S_1(A x - b + u);  u+ = u + (A x - z+ - b)          S_k(v) = max(0, v - k) - max(0, -v - k)
//   stopped when |A x - z+ - b| < sqrt(rows) 1e-4 + 1e-2 max(|A x|, |z+|, |b|) and |A^T (z+ - z)| < sqrt(columns) 1e-4 + 1e-2 |A^T u+|, rows = 6 P, columns = 3 (F - 1),
//   or after 1000 iterations (not converged is not an error, as upstream ignores Solve's return value).  curr_e = |x|; break before the update when last_e < curr_e;
//   R <- R exp(x_r); continue while ++iter < 32 && curr_e > 1e-5 && (last_e - curr_e) / curr_e > 1e-2.
//   (A^T A)^-1 = G = (2 L)^-1 is formed ONCE per call as a dense matrix of order F - 1; the x-update is the dense product X = G (2 A_h^T (b + z - u)), three columns:
//   row i over kTile lanes (lane l takes the columns l, l + kTile, ...) and an xor butterfly.
// IRLS stage (:505-580), weight function 1: errors = A x_prev - b (x_prev: the previous update, zero at first), weights = |errors|^-1.5 per row and component,
//   A^T W A x = A^T W b (F - 1 diagonal 3 x 3 blocks, diagonal off-blocks), the same rotation update, curr_e = |x_prev - x|, the same loop condition.  A system that
//   is not finite or not positive definite ends the call with info > 0 and the rotations of the last completed iteration (upstream returns false, :553-557).
// L2 refinement (:317-374; PairWiseRotationResidual, base/CostFunction.h:17-47): one angle-axis vector per camera, none fixed, r_p = log((R_2w R_1w^T) R_21^T) under
//   SoftLOneLoss(a) on |r|^2; R_21 is used directly instead of through its angle-axis vector (the divergence K36 and K42 document).  Analytic Jacobians in place of
//   the autodiff: with M = R_2w R_1w^T, d r / d aa_2 = J_l^-1(r) J_l(aa_2), d r / d aa_1 = -J_l^-1(r) M J_l(aa_1).  LM: the pair-graph layer's lm_solve, CameraSystem (no
//   origin), Jacobi scaling and LM diagonal.
// Sums: per camera its pairs in list order over kGroup lanes and an xor butterfly; every scalar the root of the fixed tree over pairs or cameras
// (pvlm_pairgraph_core.h).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>
#include <algorithm>
#include <vector>

#include "pvlm_pairgraph_core.h"

#if defined(__HIPCC__)
#define PVLM_RA_HD __host__ __device__ __forceinline__
#else
#define PVLM_RA_HD inline
#endif

namespace pvlm_rotavg {

namespace pg = pvlm_pairgraph;

using pg::kGroup;                     // lanes that share one camera's gather: the layer's (pvlm_rotavg_group_size)
constexpr int kTile = 64;             // lanes across one row of the dense product
constexpr int kAdmmMaxIterations = 1000, kOuterMaxIterations = 32;
// L1 / IRLS per-pair record, component-major (component k of pair p at [k * P + p])
enum { kB = 0, kZ = 3, kW = 6, kDz = 9, kU = 12, kL1Slots = 15 };     // ADMM: b | z | w = b + z - u | z+ - z | u (the last three are what a camera gathers)
enum { kIw = 0, kIwb = 3 };                                            // IRLS (the same storage): weights | weights * b
enum { kTermR2 = 0, kTermAx2 = 1, kTermZ2 = 2, kL1Terms = 3 };
// L2 per-pair record: side 0 (first) and side 1 (second) as pg::kCam numbers each (no elimination: the reduced pieces equal the unreduced), then
enum { kJ1 = 30, kJ2 = 39, kRes = 48, kRw = 51, kL2Slots = 52 };

struct L1Summary { int l1_iterations, admm_iterations, irls_iterations, info; };     // == pvlm_rotavg_l1_summary

PVLM_RA_HD void mul_nn(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
PVLM_RA_HD void mul_tn(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
PVLM_RA_HD void mul_nt(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}

// host/pvlm_host.cpp RotationMatrixToAngleAxis (row-major R)
PVLM_RA_HD void log_rotation(const double* R, double* aa) {
  double q[4];
  const double trace = R[0] + R[4] + R[8];
  if (trace >= 0.0) {
    double t = sqrt(trace + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i + 1] = 0.5 * t; t = 0.5 / t;
    q[0] = (R[3 * k + j] - R[3 * j + k]) * t; q[j + 1] = (R[3 * j + i] + R[3 * i + j]) * t; q[k + 1] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (s2 > 0.0) {
    const double s = sqrt(s2);
    const double two_theta = 2.0 * ((q[0] < 0.0) ? atan2(-s, -q[0]) : atan2(s, q[0]));
    const double k = two_theta / s;
    aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
  } else {
    aa[0] = q[1] * 2.0; aa[1] = q[2] * 2.0; aa[2] = q[3] * 2.0;
  }
}
// host/pvlm_host.cpp AngleAxisToRotationMatrix (row-major R)
PVLM_RA_HD void exp_rotation(const double* a, double* R) {
  const double x = a[0], y = a[1], z = a[2], th2 = x * x + y * y + z * z;
  if (th2 > 2.220446049250313e-16) {
    const double th = sqrt(th2), wx = x / th, wy = y / th, wz = z / th, c = cos(th), s = sin(th), k = 1.0 - c;
    R[0] = c + wx * wx * k;       R[1] = wx * wy * k - wz * s; R[2] = wy * s + wx * wz * k;
    R[3] = wz * s + wx * wy * k;  R[4] = c + wy * wy * k;      R[5] = -wx * s + wy * wz * k;
    R[6] = -wy * s + wx * wz * k; R[7] = wx * s + wy * wz * k; R[8] = c + wz * wz * k;
  } else {
    R[0] = 1; R[1] = -z; R[2] = y; R[3] = z; R[4] = 1; R[5] = -x; R[6] = -y; R[7] = x; R[8] = 1;
  }
}
// I + A [w]x + B [w]x^2
PVLM_RA_HD void hat_series(const double* w, double A, double B, double* J) {
  const double x = w[0], y = w[1], z = w[2], th2 = x * x + y * y + z * z;
  J[0] = 1.0 + B * (x * x - th2); J[1] = -A * z + B * x * y;      J[2] = A * y + B * x * z;
  J[3] = A * z + B * x * y;       J[4] = 1.0 + B * (y * y - th2); J[5] = -A * x + B * y * z;
  J[6] = -A * y + B * x * z;      J[7] = A * x + B * y * z;       J[8] = 1.0 + B * (z * z - th2);
}
// J_l(w): exp(w + d) = exp(J_l d) exp(w) to first order (the coefficients of pvlm_relpose_core.h pose_row)
PVLM_RA_HD void left_jacobian(const double* w, double* J) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (th2 > 1e-6) { const double th = sqrt(th2); A = (1.0 - cos(th)) / th2; B = (th - sin(th)) / (th2 * th); }
  else { A = 0.5 - th2 * (1.0 / 24.0) + th2 * th2 * (1.0 / 720.0); B = (1.0 / 6.0) - th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0); }
  hat_series(w, A, B, J);
}
// J_l^-1(w) = I - [w]x / 2 + C [w]x^2, C = (1 - th sin th / (2 (1 - cos th))) / th^2
PVLM_RA_HD void left_jacobian_inverse(const double* w, double* J) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double C;
  if (th2 > 1e-6) { const double th = sqrt(th2); C = (1.0 - th * sin(th) / (2.0 * (1.0 - cos(th)))) / th2; }
  else C = (1.0 / 12.0) + th2 * (1.0 / 720.0) + th2 * th2 * (1.0 / 30240.0);
  hat_series(w, -0.5, C, J);
}

// e = log((R2^T R21) R1)
PVLM_RA_HD void pair_error(const double* R1, const double* R2, const double* R21, double* e) {
  double T[9], E[9];
  mul_tn(R2, R21, T); mul_nn(T, R1, E);
  log_rotation(E, e);
}
// R <- R exp(x)
PVLM_RA_HD void apply_update(double* R, const double* x) {
  double U[9], N[9];
  exp_rotation(x, U); mul_nn(R, U, N);
  for (int k = 0; k < 9; ++k) R[k] = N[k];
}
PVLM_RA_HD double shrink(double v, double kappa) { return fmax(0.0, v - kappa) - fmax(0.0, -v - kappa); }

// start of an outer L1 iteration for one pair: b, z = u = 0, w = b; *b2 = |b|^2
PVLM_RA_HD void admm_begin_pair(const double* R1, const double* R2, const double* R21, double* rec, long long P, double* b2) {
  double e[3];
  pair_error(R1, R2, R21, e);
  for (int k = 0; k < 3; ++k) { rec[(kB + k) * P] = e[k]; rec[(kZ + k) * P] = 0.0; rec[(kU + k) * P] = 0.0; rec[(kW + k) * P] = e[k]; rec[(kDz + k) * P] = 0.0; }
  *b2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
}
// the z- and u-update of one pair from the new x of its cameras (xi: first, xj: second; zero for start_idx) and its three terms
PVLM_RA_HD void admm_pair(const double* xi, const double* xj, double* rec, long long P, double* terms, long long tstride) {
  double r2 = 0, ax2 = 0, z2 = 0;
  for (int k = 0; k < 3; ++k) {
    const double b = rec[(kB + k) * P], z = rec[(kZ + k) * P], u = rec[(kU + k) * P];
    const double ax = xj[k] - xi[k];
    const double zn = shrink(ax - b + u, 1.0);
    const double res = ax - zn - b;
    const double un = u + res;
    rec[(kZ + k) * P] = zn; rec[(kU + k) * P] = un; rec[(kW + k) * P] = b + zn - un; rec[(kDz + k) * P] = zn - z;
    r2 += res * res; ax2 += ax * ax; z2 += zn * zn;
  }
  terms[kTermR2 * tstride] = r2; terms[kTermAx2 * tstride] = ax2; terms[kTermZ2 * tstride] = z2;
}
// one camera's ADMM gather (w | z+ - z | u, signed) -> its right-hand side g = A^T (b + z - u) and its terms |A^T (z+ - z)|^2, |A^T u|^2 (A over the 2 P rows)
PVLM_RA_HD void admm_camera(const double* v, double* g, double* s2, double* atu2) {
  double s = 0, a = 0;
  for (int k = 0; k < 3; ++k) { g[k] = 2.0 * v[k]; const double d = 2.0 * v[3 + k], u = 2.0 * v[6 + k]; s += d * d; a += u * u; }
  *s2 = s; *atu2 = a;
}
// IRLS for one pair: b, errors = (x_prev[second] - x_prev[first]) - b, weights = |errors|^-1.5; off: the 3 x 3 block between first (rows) and second (columns) of
// A^T W A inside a 6 x 6 row-major block
PVLM_RA_HD void irls_pair(const double* R1, const double* R2, const double* R21, const double* xi, const double* xj, double* rec, long long P, double* off) {
  double e[3];
  pair_error(R1, R2, R21, e);
  for (int k = 0; k < 3; ++k) {
    const double err = (xj[k] - xi[k]) - e[k];
    const double w = pow(fabs(err), -1.5);
    rec[(kIw + k) * P] = w; rec[(kIwb + k) * P] = w * e[k];
    off[7 * k] = -2.0 * w;
  }
}

struct AdmmNorms { double r2, ax2, z2, s2, atu2; };        // r2, ax2, z2 over the P rows; s2, atu2 over the cameras with A over the 2 P rows
inline bool admm_converged(const AdmmNorms& n, double b2, int F, int P) {
  const double abs_tol = 1e-4, rel_tol = 1e-2;
  const double r_norm = std::sqrt(2.0 * n.r2), s_norm = std::sqrt(n.s2);
  const double max_norm = std::fmax(std::sqrt(2.0 * n.ax2), std::fmax(std::sqrt(2.0 * n.z2), std::sqrt(2.0 * b2)));
  const double primal_eps = std::sqrt(6.0 * P) * abs_tol + rel_tol * max_norm;
  const double dual_eps = std::sqrt(3.0 * (F - 1)) * abs_tol + rel_tol * std::sqrt(n.atu2);
  return r_norm < primal_eps && s_norm < dual_eps;
}

// ---- L2 ------------------------------------------------------------------------------------------------------------------------------------------------------
// r = log((R2 R1^T) R21^T), M = R2 R1^T
PVLM_RA_HD void l2_residual(const double* aa1, const double* aa2, const double* R21, double* r, double* M) {
  double R1[9], R2[9], E[9];
  exp_rotation(aa1, R1); exp_rotation(aa2, R2);
  mul_nt(R2, R1, M); mul_nt(M, R21, E);
  log_rotation(E, r);
}
PVLM_RA_HD void l2_jacobians(const double* aa1, const double* aa2, const double* r, const double* M, double* J1, double* J2) {
  double Ji[9], Jl[9], T[9];
  left_jacobian_inverse(r, Ji);
  left_jacobian(aa2, Jl); mul_nn(Ji, Jl, J2);
  left_jacobian(aa1, Jl); mul_nn(M, Jl, T); mul_nn(Ji, T, J1);
  for (int k = 0; k < 9; ++k) J1[k] = -J1[k];
}
PVLM_RA_HD double l2_pair_cost(const double* aa1, const double* aa2, const double* R21, double a) {
  double r[3], M[9], rho, rho1;
  l2_residual(aa1, aa2, R21, r, M);
  pg::loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rho1);
  return 0.5 * rho;
}
// the linearisation of one pair: rec (stride P), off: rho' J1^T J2 between first (rows) and second (columns) inside a 6 x 6 row-major block
PVLM_RA_HD void l2_linearise_pair(const double* aa1, const double* aa2, const double* R21, double a, double* rec, long long P, double* off) {
  double r[3], M[9], J1[9], J2[9], rho, rw;
  l2_residual(aa1, aa2, R21, r, M);
  l2_jacobians(aa1, aa2, r, M, J1, J2);
  pg::loss(a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &rw);
  double* si = rec; double* sj = rec + (long long)pg::kCam * P;
  int q = 0;
  for (int x = 0; x < 3; ++x)
    for (int y = x; y < 3; ++y, ++q) {
      const double hi = rw * (J1[x] * J1[y] + J1[3 + x] * J1[3 + y] + J1[6 + x] * J1[6 + y]), hj = rw * (J2[x] * J2[y] + J2[3 + x] * J2[3 + y] + J2[6 + x] * J2[6 + y]);
      si[q * P] = hi; sj[q * P] = hj;
      if (x == y) { si[(6 + x) * P] = hi; sj[(6 + x) * P] = hj; }
    }
  for (int k = 0; k < 3; ++k) {
    const double gi = rw * (J1[k] * r[0] + J1[3 + k] * r[1] + J1[6 + k] * r[2]), gj = rw * (J2[k] * r[0] + J2[3 + k] * r[1] + J2[6 + k] * r[2]);
    si[(9 + k) * P] = gi; sj[(9 + k) * P] = gj; si[(12 + k) * P] = gi; sj[(12 + k) * P] = gj;
    rec[(kRes + k) * P] = r[k];
    for (int y = 0; y < 3; ++y) off[6 * k + y] = rw * (J1[k] * J2[y] + J1[3 + k] * J2[3 + y] + J1[6 + k] * J2[6 + y]);
  }
  for (int k = 0; k < 9; ++k) { rec[(kJ1 + k) * P] = J1[k]; rec[(kJ2 + k) * P] = J2[k]; }
  rec[kRw * P] = rw;
}
// one pair's terms of a candidate: its cost at the candidate vectors (c1, c2) and the model decrease of the steps (d1, d2)
PVLM_RA_HD void l2_step_pair(const double* R21, const double* rec, long long P, const double* d1, const double* d2, const double* c1, const double* c2, double a,
                             double* terms, long long tstride) {
  const double rw = rec[kRw * P];
  double ru = 0, uu = 0;
  for (int k = 0; k < 3; ++k) {
    double u = 0;
    for (int y = 0; y < 3; ++y) u += rec[(kJ1 + 3 * k + y) * P] * d1[y] + rec[(kJ2 + 3 * k + y) * P] * d2[y];
    ru += rec[(kRes + k) * P] * u; uu += u * u;
  }
  terms[pg::kTermCost * tstride] = l2_pair_cost(c1, c2, R21, a);
  terms[pg::kTermModel * tstride] = -(rw * ru + 0.5 * rw * uu);
}

// The pair model of the L2 stage (pvlm_pairgraph_core.h, at lm_solve): the cameras' vectors are their angle-axis vectors, no scale.  R21: 9 per pair.
struct L2Model {
  static constexpr int kSlots = kL2Slots, kTerms = 2;
  static constexpr bool kScale = false;
  const double* R21;

  PVLM_RA_HD void load(long long p, double* Rp) const { for (int k = 0; k < 9; ++k) Rp[k] = R21[9 * p + k]; }
  PVLM_RA_HD double cost(long long p, const double* aa1, const double* aa2, double, double a) const {
    double Rp[9];
    load(p, Rp);
    return l2_pair_cost(aa1, aa2, Rp, a);
  }
  PVLM_RA_HD void linearise(long long p, const double* aa1, const double* aa2, double, double a, double, double, double, bool, double*, double* rec, long long P,
                            double* off) const {
    double Rp[9];
    load(p, Rp);
    l2_linearise_pair(aa1, aa2, Rp, a, rec, P, off);
  }
  PVLM_RA_HD void step(long long p, const double* rec, long long P, const double* d1, const double* d2, const double* c1, const double* c2, double, double a, double*,
                       double* terms, long long tstride) const {
    double Rp[9];
    load(p, Rp);
    l2_step_pair(Rp, rec, P, d1, d2, c1, c2, a, terms, tstride);
  }
};

// ---- host side: shared by the device entry points and by the host compile ----------------------------------------------------------------------------------

inline bool is_identity(const double* R) { for (int k = 0; k < 9; ++k) if (R[k] != (k % 4 == 0 ? 1.0 : 0.0)) return false; return true; }

// nullptr, or what is wrong with the arguments of the two entry points (has_start false: pvlm_rotavg_l2, which fixes no camera)
inline const char* check_args(int F, int P, const int* first, const int* second, const double* R21, const double* rotations, int start, bool has_start) {
  if (F < 1 || P < 0) return "a count out of range";
  if (!rotations || (P > 0 && (!first || !second || !R21))) return "null argument";
  if (has_start && (start < 0 || start >= F)) return "start_idx names no camera";
  std::vector<int> root((size_t)F);
  for (int c = 0; c < F; ++c) root[(size_t)c] = c;
  auto find = [&](int c) { while (root[(size_t)c] != c) { root[(size_t)c] = root[(size_t)root[(size_t)c]]; c = root[(size_t)c]; } return c; };
  std::vector<std::pair<int, int>> keys((size_t)P);
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= F || second[p] < 0 || second[p] >= F) return "a pair names a camera that is not there";
    if (first[p] == second[p]) return "a pair of a camera with itself";
    if (!pg::finite_all(R21 + 9 * (size_t)p, 9)) return "a relative rotation is not finite";
    keys[(size_t)p] = std::make_pair(std::min(first[p], second[p]), std::max(first[p], second[p]));
    root[(size_t)find(first[p])] = find(second[p]);
  }
  std::sort(keys.begin(), keys.end());
  for (int p = 1; p < P; ++p) if (keys[(size_t)p] == keys[(size_t)p - 1]) return "a camera pair is named twice";
  if (!pg::finite_all(rotations, 9 * (size_t)F)) return "a rotation is not finite";
  if (has_start && !is_identity(rotations + 9 * (size_t)start)) return "the rotation of start_idx is not the identity";
  for (int c = 1; c < F; ++c) if (find(c) != find(0)) return "the pair graph is not connected";
  return nullptr;
}

// 2 L, dense, order F - 1 (row and column start removed), row-major
inline void laplacian2(int F, int P, const int* first, const int* second, int start, std::vector<double>* A) {
  const size_t n = (size_t)F - 1;
  A->assign(n * n, 0.0);
  auto idx = [&](int c) { return c == start ? -1 : c - (c > start); };
  for (int p = 0; p < P; ++p) {
    const int i = idx(first[p]), j = idx(second[p]);
    if (i >= 0) (*A)[(size_t)i * n + i] += 2.0;
    if (j >= 0) (*A)[(size_t)j * n + j] += 2.0;
    if (i >= 0 && j >= 0) { (*A)[(size_t)i * n + j] -= 2.0; (*A)[(size_t)j * n + i] -= 2.0; }
  }
}

// |v|^2 per camera of a component-major 3 x F table (or of the difference of two) through the fixed tree
inline double table_norm(const std::vector<double>& x, const std::vector<double>* y, int F) {
  std::vector<double> t((size_t)F);
  for (int c = 0; c < F; ++c) {
    double s = 0;
    for (int k = 0; k < 3; ++k) { const double d = x[(size_t)k * F + c] - (y ? (*y)[(size_t)k * F + c] : 0.0); s += d * d; }
    t[(size_t)c] = s;
  }
  return std::sqrt(pg::tree_reduce_host<false>(t.data(), F));
}

// The two stages of RotationAveragingRefineL1.  Backend: bool failed(); double admm_begin() -> |b|^2 over the P rows; AdmmNorms admm_iterate();
// void fetch_x(std::vector<double>*) (3 x F component-major, zero at start_idx); void apply_x() (R <- R exp(x) with the x of the last ADMM iteration); int irls_solve(const std::vector<double>& x_prev,
// std::vector<double>* x) -> info (0: x holds the solution); void apply(const std::vector<double>& x).
template <class B> inline void l1_solve(B& be, int F, int P, L1Summary* out) {
  L1Summary s{0, 0, 0, 0};
  std::vector<double> x, x_prev;
  double curr_e = DBL_MAX, last_e;
  int iter = 0;
  do {
    const double b2 = be.admm_begin();
    for (int i = 0; i < kAdmmMaxIterations && !be.failed(); ++i) {
      const AdmmNorms n = be.admm_iterate();
      ++s.admm_iterations;
      if (admm_converged(n, b2, F, P)) break;
    }
    be.fetch_x(&x);
    if (be.failed()) { *out = s; return; }
    last_e = curr_e;
    curr_e = table_norm(x, nullptr, F);
    if (last_e < curr_e) break;
    be.apply_x();
  } while (++iter < kOuterMaxIterations && curr_e > 1e-5 && (last_e - curr_e) / curr_e > 1e-2);
  s.l1_iterations = iter;
  x_prev.assign(3 * (size_t)F, 0.0);
  curr_e = DBL_MAX; last_e = -1;
  iter = 0;
  do {
    const int info = be.irls_solve(x_prev, &x);
    if (be.failed()) break;
    if (info != 0) { s.info = info; break; }
    be.apply(x);
    last_e = curr_e;
    curr_e = table_norm(x_prev, &x, F);
    x_prev = x;
  } while (++iter < kOuterMaxIterations && curr_e > 1e-5 && (last_e - curr_e) / curr_e > 1e-2);
  s.irls_iterations = iter;
  *out = s;
}

// the IRLS system on the host's side: the pair-graph layer's CameraSystem with start_idx as its origin, no scaling, no LM diagonal.  cam: 6 per camera (sum of weights 3,
// signed sum of weights * b 3).  false: the gather is not finite
inline bool irls_prepare(pg::CameraSystem* sys, const double* cam) {
  if (!pg::finite_all(cam, 6 * (size_t)sys->F)) return false;
  for (int c = 0; c < sys->F; ++c) {
    if (sys->index(c) < 0) continue;
    for (int k = 0; k < 3; ++k) { const size_t i = (size_t)sys->index(c) + k; sys->sigma[i] = 1.0; sys->diag[i] = 0.0; sys->rhs[i] = 2.0 * cam[6 * (size_t)c + 3 + k]; }
  }
  return true;
}
// the solved rhs -> a component-major 3 x F table, zero at the origin
inline void irls_expand(const pg::CameraSystem& sys, std::vector<double>* x) {
  x->assign(3 * (size_t)sys.F, 0.0);
  for (int c = 0; c < sys.F; ++c) if (sys.index(c) >= 0) for (int k = 0; k < 3; ++k) (*x)[(size_t)k * sys.F + c] = sys.rhs[(size_t)sys.index(c) + k];
}

}  // namespace pvlm_rotavg
