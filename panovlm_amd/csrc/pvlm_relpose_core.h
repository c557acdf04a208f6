// Statement of K36: one pair's SfMLocalBA (util/Optimization.cpp:84-170) as SfM::RefineRelativePose calls it (sfm/SfM.cpp:482-485): a two-view bundle
// adjustment with camera 1 the identity and constant, camera 2's (aa_2w, t_2w) free and started from R_21, t_21, the N triangulated points free, two residual
// blocks per point (the keypoint of frame 1, the keypoint of frame 2).  Host / device: csrc/pvlm_relpose.hip runs refine_pair with one workgroup of kLanes
// lanes per pair; the host mirror (host/pvlm_host_relpose.hpp) and tests/cpp/relpose_core_check.cpp run the same function with the lanes taken one after
// the other.  Everything that is summed over the points is summed in ONE order (below), so a pair's result does not depend on who runs it.
//
// Residual kinds (pvlm_ba_kind): PVLM_BA_PIXEL = PanoramaReprojResidual_Pixel on the float keypoint widened to double with HuberLoss(4.0), the one upstream
// calls; PVLM_BA_ANGLE2 = PanoramaReprojResidual_2Angle on eq.ImageToSphere of the keypoint widened to double (the Eigen::Vector2d overload SfMLocalBA calls,
// util/Optimization.cpp:130-142; longitude wrapped into [0, 2 pi) as the functor's constructor does) with HuberLoss(4 pi / 180).  Both through pvlm_reproj::eval_obs2 unchanged: no seam wrap of the residual, zero
// derivatives at the poles; the loss acts on the block's squared norm, the corrector scales by sqrt(rho') (pvlm_reproj::loss_eval, as K31).  rows / cols are
// those of frame 1 for block 1 and of frame 2 for block 2.  PVLM_BA_ANGLE1 is NOT implemented here: the entry points answer PVLM_ERR_ARG.
//
// Trust region: ceres_like::Solve (host/pvlm_host_solver.cpp) with the defaults of Solver::Options, for a problem whose only blocks are these.  Statement
// by statement:
//   linearise()      = bundle_reduce (pvlm_ba_core.h point_pass2 + couple_pass2 with the constant camera's columns dropped): per point V, g_p, the Jacobi
//                      scale of the point columns at the first call, damp3 + spd3_inverse (a block that is not SPD is not eliminated: Vinv = 0); summed
//                      over the points: the reduced 6 x 6 S (21 entries), g_red, Udiag = diag(J_c^T J_c), g_cam, the cost, max |g_p|.
//   scale            = 1 / (1 + sqrt(max(0, Udiag)))                      ("Jacobi scaling from the initial Jacobian", fixed for the whole solve)
//   damp             = clamp(Udiag scale^2, min_lm_diagonal, max_lm_diagonal) / radius;  (D S D + diag(damp)) dy = -D g_red by Cholesky  (the `while` body)
//   back_substitute()= bundle_step (step_point2): dp = -Vinv (g_p + W^T dc), the candidate points, the model decrease of the blocks, |dp|^2, |X|^2;
//                      step_ok = model > 0 and finite; |step|^2 and |x|^2 of the six pose parameters are added to them
//   candidate_cost() = bundle_cost at the candidate;  rho = (cost - candidate) / model;  accepted when the candidate is finite and rho > min_relative_decrease
//   accepted:          radius = min(max_radius, radius / max(1/3, 1 - (2 rho - 1)^3)), decrease factor 2, linearise() at the new point, then in this order
//                      |cost change| <= function_tolerance * previous cost, max |g| <= gradient_tolerance, |step| <= parameter_tolerance (|x| + parameter_tolerance)
//   rejected:          radius /= decrease factor, decrease factor *= 2, linearise() again at the next iteration (the damping changed), radius < min_radius ends
//   before the loop:   a cost that is not finite ends the solve, max |g| <= gradient_tolerance ends it.
// Summary: successful_steps counts ACCEPTED steps (Ceres' own summary counts iteration 0 as well: its number is successful_steps + 1).
//
// Reduction order.  Point i belongs to lane i mod kLanes; a lane adds its points in ascending i, starting from 0.0.  The kLanes partial sums are combined by
// the pairwise tree of strides 1, 2, 4, .., kLanes / 2: level m replaces lane l (l a multiple of 2m) by lane l + lane (l + m).  On the device this is the
// xor butterfly of one wave (addition commutes, so every lane holds lane 0's bits).  max |g_p| takes the same tree with fmax.  The order is a function of N
// alone: not of the batch, the other pairs or the schedule.
//
// Write-back (:158-168): R_21 from the angle-axis, scale = |t_2w|, t_21 = t_2w / scale, triangulated[i] = X_i / scale, ok = isfinite(final cost).
// Deliberate divergences: for PVLM_BA_ANGLE2 upstream converts BOTH keypoints with the one Equirectangular of frame 1 (:112); here block 2 uses frame 2's own image
// size, as the pixel kind does (the same thing wherever the two frames are as large); a pair with no inlier comes back unchanged with ok = 1 and zero steps (upstream: an empty Ceres problem); a pair whose scale is
// zero or not finite comes back with its input pose and points and ok = 0 (upstream: a division by zero); the rotation goes through the host mirror's own
// matrix / angle-axis pair (host/pvlm_host.cpp RotationMatrixToAngleAxis, AngleAxisToRotationMatrix restated below), as K31 does.
#pragma once
#include <cmath>

#include "pvlm_reproj.h"

namespace pvlm_relpose {

constexpr int kLanes = 64;            // W: the workgroup of csrc/pvlm_relpose.hip is one wave
constexpr int kKindAngle2 = 1, kKindPixel = 2;   // == PVLM_BA_ANGLE2, PVLM_BA_PIXEL
constexpr int kScratchPerPoint = 18;  // doubles: X 3 | candidate 3 | scale 3 | Vinv 6 | g_p 3, component-major (component k of point i at scr[k * n + i])
constexpr int kSharedDoubles = 63;    // pose tables: camera 1 (identity) | camera 2 | candidate
constexpr int kLinSums = 40, kLinAll = 41;

enum Termination { kMaxIterations = 0, kFunctionTolerance = 1, kGradientTolerance = 2, kParameterTolerance = 3, kRadiusCollapsed = 4, kCostNotFinite = 5, kNoInliers = 6 };

struct Options {                       // Solver::Options of host/pvlm_host.hpp
  int max_num_iterations = 50;
  double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32;
  double min_relative_decrease = 1e-3, function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
};

struct Summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; };   // == pvlm_relpose_summary

struct Pair {
  int n, kind;                         // inliers; kKindAngle2 / kKindPixel
  double rows1, cols1, rows2, cols2;
  const double* obs;                   // n x 4: the observation of block 1 (2), of block 2 (2), made by make_obs
  double* scr;                         // kScratchPerPoint * n
};

PVLM_HD inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN
PVLM_HD inline double huber_a(int kind) { return kind == kKindPixel ? 4.0 : 4.0 * 3.14159265358979323846 / 180.0; }

// the observation a block is created with from the frame's float keypoint
PVLM_HD inline void make_obs(int kind, float x, float y, int rows, int cols, double* o) {
  if (kind == kKindPixel) { o[0] = (double)x; o[1] = (double)y; return; }
  o[0] = (2 * (double)x / cols - 1) * 3.14159265358979323846;                       // eq.ImageToSphere(Eigen::Vector2d(pt.x, pt.y)): the double overload (:130-142)
  o[1] = (0.5 - (double)y / rows) * 3.14159265358979323846;
  if (o[0] < 0.0) o[0] += 2.0 * 3.14159265358979323846;                            // base/CostFunction.h:178-214, the constructor
}

// host/pvlm_host.cpp RotationMatrixToAngleAxis (row-major R)
PVLM_HD inline void rotation_to_angle_axis(const double* R, double* aa) {
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

// row of the pose table eval_obs2 reads: R = exp([aa]x) (AngleAxisToRotationMatrix, small-angle branch included) | J_l(aa) | t   (k_pose_table of pvlm_eval.hip)
PVLM_HD inline void pose_row(const double* aa, const double* t, double* o) {
  const double x = aa[0], y = aa[1], z = aa[2];
  const double th2 = x * x + y * y + z * z;
  if (th2 > 2.220446049250313e-16) {
    const double th = sqrt(th2);
    const double wx = x / th, wy = y / th, wz = z / th;
    const double c = cos(th), s = sin(th), k = 1.0 - c;
    o[0] = c + wx * wx * k;       o[1] = wx * wy * k - wz * s; o[2] = wy * s + wx * wz * k;
    o[3] = wz * s + wx * wy * k;  o[4] = c + wy * wy * k;      o[5] = -wx * s + wy * wz * k;
    o[6] = -wy * s + wx * wz * k; o[7] = wx * s + wy * wz * k; o[8] = c + wz * wz * k;
  } else {
    o[0] = 1; o[1] = -z; o[2] = y; o[3] = z; o[4] = 1; o[5] = -x; o[6] = -y; o[7] = x; o[8] = 1;
  }
  double A, B;  // J_l = I + A [w]x + B [w]x^2
  if (th2 > 1e-6) {
    const double th = sqrt(th2);
    A = (1.0 - cos(th)) / th2;
    B = (th - sin(th)) / (th2 * th);
  } else {
    A = 0.5 - th2 * (1.0 / 24.0) + th2 * th2 * (1.0 / 720.0);
    B = (1.0 / 6.0) - th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0);
  }
  o[9] = 1.0 + B * (x * x - th2); o[10] = -A * z + B * x * y;      o[11] = A * y + B * x * z;
  o[12] = A * z + B * x * y;      o[13] = 1.0 + B * (y * y - th2); o[14] = -A * x + B * y * z;
  o[15] = -A * y + B * x * z;     o[16] = A * x + B * y * z;       o[17] = 1.0 + B * (z * z - th2);
  o[18] = t[0]; o[19] = t[1]; o[20] = t[2];
}

struct Lin2 { double r[2], rho, rho1, Jc[12], Jp[6]; };

template <int KIND>
PVLM_HD inline void linearise2(const double* tab, const double* X, const double* o, double rows, double cols, double a, Lin2* l) {
  pvlm_reproj::eval_obs2<KIND>(tab, X, o, 1.0, rows, cols, l->r, l->Jc, l->Jp);
  pvlm_reproj::loss_eval(1, a, l->r[0] * l->r[0] + l->r[1] * l->r[1], &l->rho, &l->rho1);
}

PVLM_HD inline void load3(const double* scr, int n, int comp, int i, double* v) {
  v[0] = scr[(size_t)comp * n + i]; v[1] = scr[(size_t)(comp + 1) * n + i]; v[2] = scr[(size_t)(comp + 2) * n + i];
}
PVLM_HD inline void store3(double* scr, int n, int comp, int i, const double* v) {
  scr[(size_t)comp * n + i] = v[0]; scr[(size_t)(comp + 1) * n + i] = v[1]; scr[(size_t)(comp + 2) * n + i] = v[2];
}

// one point of linearise(): part = S (21, i <= j row by row) | g_red 6 | Udiag 6 | g_cam 6 | cost | max |g_p|
template <int KIND>
PVLM_HD inline void lin_point(const Pair& P, const double* tabs, int i, int init, double radius, double min_diag, double max_diag, double* part) {
  const double a = huber_a(KIND);
  double X[3]; load3(P.scr, P.n, 0, i, X);
  Lin2 l1, l2;
  linearise2<KIND>(tabs, X, P.obs + 4 * (size_t)i, P.rows1, P.cols1, a, &l1);
  linearise2<KIND>(tabs + 21, X, P.obs + 4 * (size_t)i + 2, P.rows2, P.cols2, a, &l2);
  double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int b = 0; b < 2; ++b) {
    const Lin2& l = b ? l2 : l1;
    for (int k = 0; k < 2; ++k) {
      const double* jp = l.Jp + 3 * k;
      const double a0 = l.rho1 * jp[0], a1 = l.rho1 * jp[1], a2 = l.rho1 * jp[2];
      V[0] += a0 * jp[0]; V[1] += a0 * jp[1]; V[2] += a0 * jp[2];
      V[3] += a1 * jp[1]; V[4] += a1 * jp[2]; V[5] += a2 * jp[2];
      g[0] += a0 * l.r[k]; g[1] += a1 * l.r[k]; g[2] += a2 * l.r[k];
    }
  }
  double sc[3];
  if (init) { sc[0] = 1.0 / (1.0 + sqrt(V[0])); sc[1] = 1.0 / (1.0 + sqrt(V[3])); sc[2] = 1.0 / (1.0 + sqrt(V[5])); store3(P.scr, P.n, 6, i, sc); }
  else load3(P.scr, P.n, 6, i, sc);
  double Vd[6], inv[6];
  pvlm_reproj::damp3(V, sc, radius, min_diag, max_diag, Vd);
  if (!pvlm_reproj::spd3_inverse(Vd, inv)) { for (int k = 0; k < 6; ++k) inv[k] = 0.0; }
  for (int k = 0; k < 6; ++k) P.scr[(size_t)(9 + k) * P.n + i] = inv[k];
  store3(P.scr, P.n, 15, i, g);
  part[40] = fmax(part[40], fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))));
  // camera 2's rows of the reduced system (couple_pass2 with j == i)
  double y[2][3];
  pvlm_reproj::sym3_mul(inv, l2.Jp, y[0]); pvlm_reproj::sym3_mul(inv, l2.Jp + 3, y[1]);
  double M[2][2];
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) {
      const double* jp = l2.Jp + 3 * c;
      M[r][c] = -l2.rho1 * l2.rho1 * (y[r][0] * jp[0] + y[r][1] * jp[1] + y[r][2] * jp[2]);
    }
  M[0][0] += l2.rho1; M[1][1] += l2.rho1;
  double T[2][6];
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 6; ++c) T[r][c] = M[r][0] * l2.Jc[c] + M[r][1] * l2.Jc[6 + c];
  int at = 0;
  for (int r = 0; r < 6; ++r) {
    const double c0 = l2.Jc[r], c1 = l2.Jc[6 + r];
    for (int c = r; c < 6; ++c) part[at++] += c0 * T[0][c] + c1 * T[1][c];
  }
  const double e0 = l2.r[0] - (y[0][0] * g[0] + y[0][1] * g[1] + y[0][2] * g[2]);
  const double e1 = l2.r[1] - (y[1][0] * g[0] + y[1][1] * g[1] + y[1][2] * g[2]);
  for (int k = 0; k < 6; ++k) {
    const double c0 = l2.Jc[k], c1 = l2.Jc[6 + k];
    part[21 + k] += l2.rho1 * (c0 * e0 + c1 * e1);
    part[27 + k] += l2.rho1 * (c0 * c0 + c1 * c1);
    part[33 + k] += l2.rho1 * (c0 * l2.r[0] + c1 * l2.r[1]);
  }
  part[39] += 0.5 * l1.rho + 0.5 * l2.rho;
}

// one point of back_substitute(): part = model decrease | |dp|^2 | |X|^2
template <int KIND>
PVLM_HD inline void step_point(const Pair& P, const double* tabs, int i, const double* dc, double* part) {
  const double a = huber_a(KIND);
  double X[3], b[3], inv[6];
  load3(P.scr, P.n, 0, i, X); load3(P.scr, P.n, 15, i, b);
  for (int k = 0; k < 6; ++k) inv[k] = P.scr[(size_t)(9 + k) * P.n + i];
  Lin2 l1, l2;
  linearise2<KIND>(tabs, X, P.obs + 4 * (size_t)i, P.rows1, P.cols1, a, &l1);
  linearise2<KIND>(tabs + 21, X, P.obs + 4 * (size_t)i + 2, P.rows2, P.cols2, a, &l2);
  double jd[2];                                            // Jc dc of camera 2's rows
  for (int r = 0; r < 2; ++r) {
    double e = 0.0;
    for (int k = 0; k < 6; ++k) e += l2.Jc[6 * r + k] * dc[k];
    jd[r] = e;
    e *= l2.rho1;
    b[0] += e * l2.Jp[3 * r]; b[1] += e * l2.Jp[3 * r + 1]; b[2] += e * l2.Jp[3 * r + 2];
  }
  double dp[3]; pvlm_reproj::sym3_mul(inv, b, dp);
  dp[0] = -dp[0]; dp[1] = -dp[1]; dp[2] = -dp[2];
  double model = 0.0;
  for (int c = 0; c < 2; ++c) {
    const Lin2& l = c ? l2 : l1;
    double rd = 0.0, dd = 0.0;
    for (int r = 0; r < 2; ++r) {
      double d = l.Jp[3 * r] * dp[0] + l.Jp[3 * r + 1] * dp[1] + l.Jp[3 * r + 2] * dp[2];
      if (c) d += jd[r];
      rd += l.r[r] * d; dd += d * d;
    }
    model -= l.rho1 * (rd + 0.5 * dd);
  }
  const double Xc[3] = {X[0] + dp[0], X[1] + dp[1], X[2] + dp[2]};
  store3(P.scr, P.n, 3, i, Xc);
  part[0] += model;
  part[1] += dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2];
  part[2] += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
}

// one point of candidate_cost(): the two blocks at the candidate point under the candidate pose (tabs + 42)
template <int KIND>
PVLM_HD inline double cost_point(const Pair& P, const double* tabs, int i) {
  const double a = huber_a(KIND);
  double X[3]; load3(P.scr, P.n, 3, i, X);
  double r[2], rho_a, rho_b, rho1;
  pvlm_reproj::eval_obs2<KIND>(tabs, X, P.obs + 4 * (size_t)i, 1.0, P.rows1, P.cols1, r, nullptr, nullptr);
  pvlm_reproj::loss_eval(1, a, r[0] * r[0] + r[1] * r[1], &rho_a, &rho1);
  pvlm_reproj::eval_obs2<KIND>(tabs + 42, X, P.obs + 4 * (size_t)i + 2, 1.0, P.rows2, P.cols2, r, nullptr, nullptr);
  pvlm_reproj::loss_eval(1, a, r[0] * r[0] + r[1] * r[1], &rho_b, &rho1);
  return 0.5 * rho_a + 0.5 * rho_b;
}

// (D S D + diag(damp)) dy = rhs, S as its 21 upper entries; false when the matrix is not positive definite
PVLM_HD inline bool solve6(const double* S, const double* scale, const double* damp, const double* rhs, double* dy) {
  double L[21];                                            // lower triangle row by row: (r, c) at r (r + 1) / 2 + c
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c) {
      const int up = c * 6 - c * (c - 1) / 2 + (r - c);    // entry (c, r) of the upper triangle
      double s = S[up] * scale[r] * scale[c];
      if (r == c) s += damp[r];
      for (int k = 0; k < c; ++k) s -= L[r * (r + 1) / 2 + k] * L[c * (c + 1) / 2 + k];
      if (c < r) L[r * (r + 1) / 2 + c] = s / L[c * (c + 1) / 2 + c];
      else { if (!(s > 0.0)) return false; L[r * (r + 1) / 2 + r] = sqrt(s); }
    }
  for (int r = 0; r < 6; ++r) { double s = rhs[r]; for (int k = 0; k < r; ++k) s -= L[r * (r + 1) / 2 + k] * dy[k]; dy[r] = s / L[r * (r + 1) / 2 + r]; }
  for (int r = 5; r >= 0; --r) { double s = dy[r]; for (int k = r + 1; k < 6; ++k) s -= L[k * (k + 1) / 2 + r] * dy[k]; dy[r] = s / L[r * (r + 1) / 2 + r]; }
  return true;
}

// A Team runs the lanes and combines their partial results in the order stated at the top.
//   template <class F> void lanes(int n_sum, int n_max, double* out, F&& f)
//     calls f(lane, part) for every lane with part[0 .. n_sum + n_max) zeroed, then leaves in out the tree sum of part[0 .. n_sum) and the tree fmax of the rest
//   double* shared()    kSharedDoubles doubles every lane sees
//   bool leader()       true for the one lane that writes the pair's results
// HostTeam: the lanes one after the other.  The device's team is in csrc/pvlm_relpose.hip.
struct HostTeam {
  double part[kLanes][kLinAll];
  double mem[kSharedDoubles];
  template <class F> void lanes(int n_sum, int n_max, double* out, F&& f) {
    const int nv = n_sum + n_max;
    for (int l = 0; l < kLanes; ++l) { for (int k = 0; k < nv; ++k) part[l][k] = 0.0; f(l, part[l]); }
    for (int m = 1; m < kLanes; m <<= 1)
      for (int l = 0; l < kLanes; l += 2 * m)
        for (int k = 0; k < nv; ++k) part[l][k] = k < n_sum ? part[l][k] + part[l + m][k] : fmax(part[l][k], part[l + m][k]);
    for (int k = 0; k < nv; ++k) out[k] = part[0][k];
  }
  double* shared() { return mem; }
  bool leader() const { return true; }
};

// One pair.  R (9, row-major), t (3), tri (3 n) are read and, by the write-back, replaced; a pair with n == 0 is left as it is.  accept_mask (or null): bit k - 1 is
// set when iteration k <= 64 was accepted (the accept / reject sequence the tests compare between builds).
template <int KIND, class Team>
PVLM_HD inline void refine_pair_kind(Team& team, const Pair& P, const Options& opt, double* R, double* t, double* tri, unsigned char* ok, Summary* sum,
                                      unsigned long long* accept_mask) {
  const int n = P.n;
  Summary s = {0.0, 0.0, 0, 0, kNoInliers};
  unsigned long long mask = 0;
  if (n <= 0) { if (team.leader()) { *ok = 1; if (sum) *sum = s; if (accept_mask) *accept_mask = 0; } return; }
  double* tabs = team.shared();
  double x[6];
  rotation_to_angle_axis(R, x);
  x[3] = t[0]; x[4] = t[1]; x[5] = t[2];
  {
    const double zero[3] = {0.0, 0.0, 0.0};
    pose_row(zero, zero, tabs);
    pose_row(x, x + 3, tabs + 21);
  }
  double red[kLinAll];
  team.lanes(0, 0, red, [&](int lane, double*) {
    for (int i = lane; i < n; i += kLanes) { const double X[3] = {tri[3 * (size_t)i], tri[3 * (size_t)i + 1], tri[3 * (size_t)i + 2]}; store3(P.scr, n, 0, i, X); }
  });
  double radius = opt.initial_trust_region_radius, decrease_factor = 2.0;
  auto linearise = [&](int init) {
    team.lanes(kLinSums, 1, red, [&](int lane, double* part) {
      for (int i = lane; i < n; i += kLanes) lin_point<KIND>(P, tabs, i, init, radius, opt.min_lm_diagonal, opt.max_lm_diagonal, part);
    });
  };
  auto gmax = [&]() { double m = red[40]; for (int k = 0; k < 6; ++k) m = fmax(m, fabs(red[33 + k])); return m; };
  linearise(1);
  double cost = red[39];
  s.initial_cost = s.final_cost = cost;
  s.termination = -1;
  double scale[6];
  for (int k = 0; k < 6; ++k) scale[k] = 1.0 / (1.0 + sqrt(fmax(0.0, red[27 + k])));
  if (!finite_d(cost)) s.termination = kCostNotFinite;
  else if (gmax() <= opt.gradient_tolerance) s.termination = kGradientTolerance;
  bool valid = true;
  int iter = 0;
  while (s.termination < 0 && iter < opt.max_num_iterations) {
    ++iter;
    if (!valid) { linearise(0); valid = true; }
    double rhs[6], damp[6], dy[6], step[6];
    for (int k = 0; k < 6; ++k) {
      rhs[k] = -red[21 + k] * scale[k];
      const double hs = red[27 + k] * scale[k] * scale[k];
      damp[k] = fmin(fmax(hs, opt.min_lm_diagonal), opt.max_lm_diagonal) / radius;
    }
    bool step_ok = solve6(red, scale, damp, rhs, dy);
    double model = 0.0, dn = 0.0, xn = 0.0;
    if (step_ok) {
      for (int k = 0; k < 6; ++k) step[k] = dy[k] * scale[k];
      double o3[3];
      team.lanes(3, 0, o3, [&](int lane, double* part) {
        for (int i = lane; i < n; i += kLanes) step_point<KIND>(P, tabs, i, step, part);
      });
      model = o3[0]; dn = o3[1]; xn = o3[2];
      step_ok = model > 0.0 && finite_d(model);
    }
    bool accepted = false;
    if (step_ok) {
      double cand[6];
      for (int k = 0; k < 6; ++k) { cand[k] = x[k] + step[k]; dn += step[k] * step[k]; xn += x[k] * x[k]; }
      pose_row(cand, cand + 3, tabs + 42);
      double ccost;
      team.lanes(1, 0, &ccost, [&](int lane, double* part) {
        for (int i = lane; i < n; i += kLanes) part[0] += cost_point<KIND>(P, tabs, i);
      });
      const double rho = (cost - ccost) / model;
      if (finite_d(ccost) && rho > opt.min_relative_decrease) {
        accepted = true;
        if (iter <= 64) mask |= 1ull << (iter - 1);
        const double cost_change = cost - ccost;
        for (int k = 0; k < 6; ++k) x[k] = cand[k];
        for (int k = 0; k < 21; ++k) tabs[21 + k] = tabs[42 + k];
        team.lanes(0, 0, red, [&](int lane, double*) {
          for (int i = lane; i < n; i += kLanes) { double X[3]; load3(P.scr, n, 3, i, X); store3(P.scr, n, 0, i, X); }
        });
        const double w = 2.0 * rho - 1.0;
        radius = fmin(opt.max_trust_region_radius, radius / fmax(1.0 / 3.0, 1.0 - w * w * w));
        decrease_factor = 2.0;
        linearise(0);
        s.successful_steps++;
        const double prev = cost;
        cost = ccost;
        if (fabs(cost_change) <= opt.function_tolerance * prev) s.termination = kFunctionTolerance;
        else if (gmax() <= opt.gradient_tolerance) s.termination = kGradientTolerance;
        else if (sqrt(dn) <= opt.parameter_tolerance * (sqrt(xn) + opt.parameter_tolerance)) s.termination = kParameterTolerance;
      }
    }
    if (!accepted) {
      s.unsuccessful_steps++;
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      valid = false;
      if (radius < opt.min_trust_region_radius) s.termination = kRadiusCollapsed;
    }
  }
  if (s.termination < 0) s.termination = kMaxIterations;
  s.final_cost = cost;
  // write-back
  const double scale_t = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
  const bool good = scale_t > 0.0 && finite_d(scale_t);
  if (good) {
    team.lanes(0, 0, red, [&](int lane, double*) {
      for (int i = lane; i < n; i += kLanes) {
        double X[3]; load3(P.scr, n, 0, i, X);
        tri[3 * (size_t)i] = X[0] / scale_t; tri[3 * (size_t)i + 1] = X[1] / scale_t; tri[3 * (size_t)i + 2] = X[2] / scale_t;
      }
    });
  }
  if (team.leader()) {
    if (good) {
      for (int k = 0; k < 9; ++k) R[k] = tabs[21 + k];
      t[0] = x[3] / scale_t; t[1] = x[4] / scale_t; t[2] = x[5] / scale_t;
    }
    *ok = (good && finite_d(s.final_cost)) ? 1 : 0;
    if (sum) *sum = s;
    if (accept_mask) *accept_mask = mask;
  }
}

template <class Team>
PVLM_HD inline void refine_pair(Team& team, const Pair& P, const Options& opt, double* R, double* t, double* tri, unsigned char* ok, Summary* sum,
                                 unsigned long long* accept_mask = nullptr) {
  if (P.kind == kKindPixel) refine_pair_kind<kKindPixel>(team, P, opt, R, t, tri, ok, sum, accept_mask);
  else refine_pair_kind<kKindAngle2>(team, P, opt, R, t, tri, ok, sum, accept_mask);
}

}  // namespace pvlm_relpose
