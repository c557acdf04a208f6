// K45: the definition of RotationAveragingLeastSquare (sfm/RotationAveraging.cpp:185-275), the start of the L2 rotation-averaging method — host and device.  Compiled
// for the device by pvlm_rotstart.hip and for the host by tests/cpp/rotstart_core_check.cpp (host/pvlm_host_rotstart.hpp); both run the SAME loop (run() below) over a
// backend that records the pairs, gathers per camera, solves the camera system and reduces on the fixed tree of pvlm_pairgraph_core.h.
//
// Inputs: F cameras, P pairs (first, second, R_21 row-major) in either orientation.  The unknown is a 3 F x 3 matrix X whose 3 x 3 block of camera c is R_cw times
// one common orthogonal matrix; the pair's equation is X_second = R_21 X_first (:201).  M = A^T A has the blocks (:203-217, i = first, j = second)
//   M(i,i) += R_21^T R_21, taken as I;   M(j,j) += I;   M(j,i) -= R_21;   M(i,j) -= R_21^T.
// M is positive semi-definite; on noise-free input or a tree its three smallest eigenvalues are zero.  Upstream takes the three eigenvectors of smallest |lambda|
// from a dense SelfAdjointEigenSolver (:229-244), per camera the polar factor U V^T of its block (:252-262), the sign rule det < 0 -> -rot (:264-265) and the
// product with R_0^T (:270-272).
//
// STATED DIVERGENCE — the method, not the result.  The output depends only on the invariant subspace of the three smallest eigenvalues: replacing the basis V by V Q
// with Q orthogonal multiplies every camera's polar factor by the same Q, the sign rule then makes every rot_c into rot_c (det(Q) Q), and det(Q) Q is a proper
// rotation that the product with R_0^T removes.  So any method that finds the subspace is exact.  Here it is shift-and-invert subspace iteration of width 3 with
// Rayleigh-Ritz, O(F) memory where upstream's dense decomposition takes 72 F^2 bytes and 27 F^3 operations:
//   1. factorise M + sigma I, sigma = shift_rel * d_max (d_max: the largest camera degree), with the library's block-sparse solver; no camera is grounded;
//   2. per iteration: three solves Y = (M + sigma I)^-1 X; Y = Q L^T through the Cholesky of its 3 x 3 Gram matrix; T = Q^T M Q and its eigen-decomposition
//      T = S diag(theta) S^T (Jacobi, theta ordered by |theta| as upstream orders lambda); X = Q S;
//   3. stop when max_k |M x_k - theta_k x_k|_2 <= tol * d_max;
//   4. per camera the polar factor of its block of X, the sign rule, the product with rot_0^T.
// The start X_0 is the `rotations` array as it comes in (the host mirror passes RotationAveragingSpanningTree's result: exact null vectors on noise-free input,
// X_0^T X_0 = F I); it is orthonormalised through its own Gram matrix first.  The eigenvalues come in well-separated triples (lambda_2 of the order of the squared
// noise, lambda_3 the next eigenvalue of the graph's Laplacian, three times), which is why width 3 suffices.
// The polar factor: Newton's iteration X <- (g X + X^-T / g) / 2 on the block scaled to Frobenius norm sqrt(3), g = |det X|^-1/3 while the determinant is away from
// one; it converges to U V^T of any non-singular block, the improper one included.  A block is singular when it is not finite, zero, or its scaled determinant is
// at most kSingularDet in magnitude; a 3 x 3 Gram matrix is singular when a Cholesky pivot is at most kSingularPivot times its diagonal entry.
// info: 0; k > 0: the shifted matrix is not positive definite (R_21 far from a rotation); -1: something is not finite; -2: max_iterations reached; -3: a camera's
// block or a Gram matrix is singular.  Unless info is 0 nothing is written.
// Sums: per camera over its pairs in list order on kGroup lanes and a fixed butterfly, the scalars on the fixed tree over the cameras.
#pragma once
#include <cmath>
#include <vector>

#include "pvlm_pairgraph_core.h"
#include "pvlm_rotavg_core.h"

#if defined(__HIPCC__)
#define PVLM_RS_HD __host__ __device__ __forceinline__
#else
#define PVLM_RS_HD inline
#endif

namespace pvlm_rotstart {

namespace pg = pvlm_pairgraph;
namespace ra = pvlm_rotavg;

// the two-sided per-pair record, component-major: side s (0 = first, 1 = second), entry 3 r + k of the side's 3 x 3 term at [(9 s + 3 r + k) * P + p]
enum { kBlock = 9, kSlots = 18 };
enum { kSym = 6 };                                        // a symmetric 3 x 3 matrix: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
enum { kInfoNotFinite = -1, kInfoMaxIterations = -2, kInfoSingular = -3, kDeviceError = -1000000 };      // kDeviceError never leaves the library
constexpr double kSingularDet = 1e-12, kSingularPivot = 1e-12;
constexpr int kPolarIterations = 40;

struct Params { double shift_rel = 1e-9, tol = 1e-12; int max_iterations = 100; };
struct Summary { int iterations, solves, info; double residual, theta[3]; };

// the pair's terms of Y = M X for the three columns: first gets X_i - R^T X_j, second X_j - R X_i (a camera's block is row-major: entry 3 r + k = row r, column k)
PVLM_RS_HD void mx_pair(const double* R, const double* xi, const double* xj, double* rec, long long P) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {
      const double a = (R[r] * xj[k] + R[3 + r] * xj[3 + k]) + R[6 + r] * xj[6 + k];
      const double b = (R[3 * r] * xi[k] + R[3 * r + 1] * xi[3 + k]) + R[3 * r + 2] * xi[6 + k];
      rec[(long long)(3 * r + k) * P] = xi[3 * r + k] - a;
      rec[(long long)(kBlock + 3 * r + k) * P] = xj[3 * r + k] - b;
    }
}
// lane `lane` of the kGroup lanes of one camera over the two-sided record: its part of the row ent[e0 .. e1) (entry = 2 * pair + side), in list order (the layer's
// two-sided gather_lane is that of an LM record, pg::kCam numbers a side; this is the same walk over kBlock)
PVLM_RS_HD void gather_lane(const double* rec, long long P, const int* ent, int e0, int e1, int lane, double* part) {
  for (int k = 0; k < kBlock; ++k) part[k] = 0.0;
  for (int e = e0 + lane; e < e1; e += pg::kGroup) {
    const int p = ent[e] >> 1, side = ent[e] & 1;
    const double* s = rec + (long long)side * kBlock * P + p;
    for (int k = 0; k < kBlock; ++k) part[k] += s[(long long)k * P];
  }
}
// the solver's blocks (6 x 6 row-major, the other entries stay zero): the pair's M(first, second) = -R_21^T, the layout of K42's pairs; the camera's (deg + sigma) I3
PVLM_RS_HD void off_block(const double* R, double* B) { for (int k = 0; k < 3; ++k) for (int y = 0; y < 3; ++y) B[6 * k + y] = -R[3 * y + k]; }
PVLM_RS_HD void diag_block(double deg, double sigma, double* B) { for (int k = 0; k < 3; ++k) B[7 * k] = deg + sigma; }

// a camera's terms of the symmetric 3 x 3 matrix A^T B (A, B: blocks of two 3 F x 3 matrices), the upper triangle
PVLM_RS_HD void sym_terms(const double* A, const double* B, double* terms, long long stride) {
  int n = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b, ++n) terms[(long long)n * stride] = (A[a] * B[b] + A[3 + a] * B[3 + b]) + A[6 + a] * B[6 + b];
}
// X <- X C for one camera's block
PVLM_RS_HD void mul_block(double* X, const double* C) {
  double Y[9];
  ra::mul_nn(X, C, Y);
  for (int k = 0; k < 9; ++k) X[k] = Y[k];
}
// a camera's terms of |M x_k - theta_k x_k|^2 for the three columns
PVLM_RS_HD void residual_terms(const double* X, const double* MX, const double* theta, double* terms, long long stride) {
  for (int k = 0; k < 3; ++k) {
    const double u = MX[k] - theta[k] * X[k], v = MX[3 + k] - theta[k] * X[3 + k], w = MX[6 + k] - theta[k] * X[6 + k];
    terms[(long long)k * stride] = (u * u + v * v) + w * w;
  }
}

PVLM_RS_HD double det3(const double* A) {
  return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
// the polar factor U V^T of A with the sign rule (:259-265): false when the block is singular (nothing written)
PVLM_RS_HD bool polar_rotation(const double* A, double* rot) {
  double n2 = 0;
  for (int k = 0; k < 9; ++k) n2 += A[k] * A[k];
  if (!(n2 > 0) || !(n2 < INFINITY)) return false;
  const double s = sqrt(3.0 / n2);
  double X[9];
  for (int k = 0; k < 9; ++k) X[k] = A[k] * s;
  double d = det3(X);
  if (!(fabs(d) > kSingularDet)) return false;
  for (int it = 0; it < kPolarIterations; ++it) {
    const double C[9] = {X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],      // the cofactors: X^-T = C / det
                         X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                         X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
    const double g = fabs(fabs(d) - 1.0) > 0.1 ? 1.0 / cbrt(fabs(d)) : 1.0, h = 1.0 / (g * d);
    double change = 0;
    for (int k = 0; k < 9; ++k) { const double v = 0.5 * (g * X[k] + h * C[k]), e = v - X[k]; change += e * e; X[k] = v; }
    d = det3(X);
    if (change <= 1e-30) break;
  }
  const double sign = d < 0 ? -1.0 : 1.0;
  for (int k = 0; k < 9; ++k) rot[k] = sign * X[k];
  return true;
}
// :252-272 for one camera: its rotation times rot_0^T.  Returns 1 when the camera's block or camera 0's is singular (nothing written), else 0
PVLM_RS_HD double final_rotation(const double* Xc, const double* X0, double* out) {
  double rc[9], r0[9];
  if (!polar_rotation(Xc, rc) || !polar_rotation(X0, r0)) return 1.0;
  ra::mul_nt(rc, r0, out);
  return 0.0;
}

// ---- host side: shared by the device entry point and by the host compile -----------------------------------------------------------------------------------

// nullptr, or what is wrong with the arguments
inline const char* check_args(int F, int P, const int* first, const int* second, const double* R21, const double* rotations, const Params* prm) {
  if (!prm) return "null argument";
  if (F < 2 || P < 1) return "fewer than two cameras or no pair";
  if (!(prm->shift_rel > 0) || !(prm->tol > 0) || !std::isfinite(prm->shift_rel) || !std::isfinite(prm->tol) || prm->max_iterations < 1)
    return "shift_rel <= 0, tol <= 0 or max_iterations < 1";
  return ra::check_args(F, P, first, second, R21, rotations, -1, false);
}

// G = L L^T of a symmetric 3 x 3 matrix (kSym numbers) and C = L^-T, row-major (upper triangular): Y C has orthonormal columns when G = Y^T Y.  false: singular
inline bool gram_factor(const double* g, double* C) {
  const double G[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}};
  double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int j = 0; j < 3; ++j) {
    double v = G[j][j];
    for (int k = 0; k < j; ++k) v -= L[j][k] * L[j][k];
    if (!(v > kSingularPivot * G[j][j])) return false;
    L[j][j] = std::sqrt(v);
    for (int i = j + 1; i < 3; ++i) { double w = G[i][j]; for (int k = 0; k < j; ++k) w -= L[i][k] * L[j][k]; L[i][j] = w / L[j][j]; }
  }
  // W = L^-1 (lower), C = W^T
  double W[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int j = 0; j < 3; ++j) {
    W[j][j] = 1.0 / L[j][j];
    for (int i = j + 1; i < 3; ++i) { double w = 0; for (int k = j; k < i; ++k) w -= L[i][k] * W[k][j]; W[i][j] = w / L[i][i]; }
  }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[3 * r + c] = W[c][r];
  return true;
}

// T = S diag(theta) S^T of a symmetric 3 x 3 matrix (kSym numbers) by cyclic Jacobi; the columns of S (row-major) ordered by |theta|, equal ones in the order found
inline void eig3(const double* t, double* theta, double* S) {
  double A[3][3] = {{t[0], t[1], t[2]}, {t[1], t[3], t[4]}, {t[2], t[4], t[5]}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 60; ++sweep) {
    const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double tt = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau)), cs = 1.0 / std::sqrt(1.0 + tt * tt), sn = tt * cs;
        for (int k = 0; k < 3; ++k) { const double u = A[k][p], v = A[k][q]; A[k][p] = cs * u - sn * v; A[k][q] = sn * u + cs * v; }
        for (int k = 0; k < 3; ++k) { const double u = A[p][k], v = A[q][k]; A[p][k] = cs * u - sn * v; A[q][k] = sn * u + cs * v; }
        for (int k = 0; k < 3; ++k) { const double u = V[k][p], v = V[k][q]; V[k][p] = cs * u - sn * v; V[k][q] = sn * u + cs * v; }
        A[p][q] = A[q][p] = 0.0;
      }
  }
  int order[3] = {0, 1, 2};
  for (int a = 1; a < 3; ++a) for (int b = a; b > 0 && std::fabs(A[order[b]][order[b]]) < std::fabs(A[order[b - 1]][order[b - 1]]); --b) { const int o = order[b]; order[b] = order[b - 1]; order[b - 1] = o; }
  for (int k = 0; k < 3; ++k) { theta[k] = A[order[k]][order[k]]; for (int r = 0; r < 3; ++r) S[3 * r + k] = V[r][order[k]]; }
}

inline int max_degree(int F, int P, const int* first, const int* second) {
  std::vector<int> deg((size_t)F, 0);
  int d = 0;
  for (int p = 0; p < P; ++p) { ++deg[(size_t)first[p]]; ++deg[(size_t)second[p]]; }
  for (int c = 0; c < F; ++c) d = deg[(size_t)c] > d ? deg[(size_t)c] : d;
  return d;
}

// The whole of the least-square start over a backend B:
//   int F; pg::CameraSystem sys (no origin; its scale 1 and added diagonal 0 as init leaves them);
//   bool failed()                            a device error: the loop stops;
//   void assemble(double sigma)              the solver's block list of M + sigma I;
//   int solve()                              sys.rhs -> info of the factorisation, the solution in sys.rhs;
//   void put(const std::vector<double>& x)   the 3 F x 3 matrix (9 per camera) the next three calls work on;
//   void gram(double g[kSym])                X^T X on the tree;
//   void mul(const double C[9])              X <- X C;
//   void fetch(std::vector<double>* x)       X as it stands;
//   void rayleigh(double t[kSym])            per pair mx_pair, the gather M X per camera, X^T (M X) on the tree;
//   void rotate(S, theta, double r2[3], std::vector<double>* x)     X <- X S, M X <- (M X) S, |M x_k - theta_k x_k|^2 on the tree, X fetched;
//   double polar(std::vector<double>* out)   final_rotation per camera into out (9 F); returns the tree's maximum of the flags.
// x0: the start (9 F); out: written only when 0 is returned.  Returns the info (also in sum->info) or kDeviceError.
template <class B> inline int run(B& be, const Params& prm, double d_max, const double* x0, std::vector<double>* out, Summary* sum) {
  const int F = be.F;
  pg::CameraSystem& sys = be.sys;
  *sum = Summary{0, 0, 0, 0.0, {0.0, 0.0, 0.0}};
  auto done = [&](int info) { sum->info = info == kDeviceError ? 0 : info; return info; };
  std::vector<double> X(x0, x0 + 9 * (size_t)F), Y(9 * (size_t)F), rot;
  double g[kSym], C[9], theta[3] = {0, 0, 0}, r2[3];
  be.assemble(prm.shift_rel * d_max);
  // the start, orthonormalised
  be.put(X); be.gram(g);
  if (be.failed()) return done(kDeviceError);
  if (!pg::finite_all(g, kSym)) return done(kInfoNotFinite);
  if (!gram_factor(g, C)) return done(kInfoSingular);
  be.mul(C); be.fetch(&X);
  if (be.failed()) return done(kDeviceError);
  bool converged = false;
  while (!converged && sum->iterations < prm.max_iterations) {
    ++sum->iterations;
    for (int k = 0; k < 3; ++k) {
      for (int c = 0; c < F; ++c) for (int r = 0; r < 3; ++r) sys.rhs[3 * (size_t)c + r] = X[9 * (size_t)c + 3 * r + k];
      const int info = be.solve();
      ++sum->solves;
      if (be.failed()) return done(kDeviceError);
      if (info) return done(info);
      for (int c = 0; c < F; ++c) for (int r = 0; r < 3; ++r) Y[9 * (size_t)c + 3 * r + k] = sys.rhs[3 * (size_t)c + r];
    }
    if (!pg::finite_all(Y.data(), Y.size())) return done(kInfoNotFinite);
    be.put(Y); be.gram(g);
    if (be.failed()) return done(kDeviceError);
    if (!pg::finite_all(g, kSym)) return done(kInfoNotFinite);
    if (!gram_factor(g, C)) return done(kInfoSingular);
    be.mul(C); be.rayleigh(g);
    if (be.failed()) return done(kDeviceError);
    if (!pg::finite_all(g, kSym)) return done(kInfoNotFinite);
    double S[9];
    eig3(g, theta, S);
    be.rotate(S, theta, r2, &X);
    if (be.failed()) return done(kDeviceError);
    if (!pg::finite_all(r2, 3) || !pg::finite_all(X.data(), X.size())) return done(kInfoNotFinite);
    const double worst = std::sqrt(std::fmax(r2[0], std::fmax(r2[1], r2[2])));
    sum->residual = worst / d_max;
    for (int k = 0; k < 3; ++k) sum->theta[k] = theta[k];
    converged = worst <= prm.tol * d_max;
  }
  if (!converged) return done(kInfoMaxIterations);
  const double bad = be.polar(&rot);
  if (be.failed()) return done(kDeviceError);
  if (bad != 0.0) return done(kInfoSingular);
  if (!pg::finite_all(rot.data(), rot.size())) return done(kInfoNotFinite);
  *out = rot;
  return done(0);
}

}  // namespace pvlm_rotstart
