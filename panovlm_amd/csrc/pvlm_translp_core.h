// K47: the definition of TranslationAveragingL1 (sfm/TranslationAveraging.cpp:277-417) — host and device.  Compiled for the device by pvlm_translp.hip and for the
// host by tests/cpp/translp_core_check.cpp (host/pvlm_host_translp.hpp); both run the SAME interior-point loop (run(), below) over a backend that does the
// per-triplet work, the gathers, the reductions and the camera solves.
//
// The programme, as upstream writes it: unknowns t_cw of every camera (3 F), one lambda per TRIPLET and one gamma; for triplet (i, j, k) the pairs (i,j), (j,k), (i,k)
// in that order, for each pair and component c two rows  e_c - gamma <= 0  and  e_c + gamma >= 0  with e = t[second] - R_21 t[first] - lambda_T t_21 (18 rows per
// triplet); lambda_T >= 0.9 x the mean of |t_21| over the triplet's three pairs (t_21 as it comes, not normalised); the origin camera fixed at zero; cost gamma.
// Written as  min c^T x  s.t.  G x + s = h, s >= 0  with multipliers z >= 0: the 18 rows (h = 0) and one bound row  -lambda_T <= -lo_T  per triplet, 19 in all, row
// r = 6 q + 2 c + sign of pair slot q, the bound row last.  gamma >= 0 is implied by the row pairs.
//
// The method: a primal-dual interior-point iteration with Mehrotra's predictor and corrector on the normal equations.  With w = z / s, G^T W G has
//   a 1 x 1 block per triplet for its lambda (private to the triplet: eliminated by its pivot D_T = sum w t_21,c^2 + w_bound),
//   3 x 3 blocks on the cameras — three diagonal and three off-diagonal per triplet, the latter on the triplet's own pairs, so the fill is the pair graph's —
//   and one dense border column for gamma, taken by a 1 x 1 Schur complement after two camera solves.
// Per iteration three camera systems are solved (the gamma column, the predictor, the corrector) through the pair-graph layer's block list [F diagonal | P
// off-diagonal], Jacobi-scaled by 1 / sqrt(diag) with diag_add = 1e-12 on the scaled diagonal; a factorisation that fails multiplies diag_add by 100 and is retried,
// at most three times in a call.  Without the scaling the factorisation is lost between iterations 9 and 16: it is part of the method.
// Start: t = 0, lambda = lo + 1, gamma = max |e| + 1, s = h - G x, z = 1 / rows.  Step: 0.99 of the way to the boundary, capped at 1, primal and dual apart (the
// predictor goes the whole way).  Stop: s^T z <= gap_tol max(1, |gamma|), |G x + s - h|_inf <= feas_tol, |c + G^T z|_inf <= feas_tol.
// Gauge: cameras joined by a triplet form components; origin_idx pins its own, every other component has its lowest-numbered camera pinned at zero (its translation
// is free in upstream's programme too, so no optimum changes); a camera in no triplet stays zero.
// Sums: per camera and per pair over a CSR of (triplet, slot) entries in triplet order, kGroup lanes and a fixed butterfly; every scalar is the root of the fixed
// tree over its per-triplet terms.  No atomics, one order per sum.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <utility>
#include <vector>

#include "pvlm_pairgraph_core.h"

#if defined(__HIPCC__)
#define PVLM_LP_HD __host__ __device__ __forceinline__
#else
#define PVLM_LP_HD inline
#endif

namespace pvlm_translp {

namespace pg = pvlm_pairgraph;

constexpr int kRows = 19;                  // rows of one triplet: 18 and its bound row
constexpr int kBound = 18;
// the triplet's record, component-major (component k of triplet t at [k * T + t]): per camera slot the reduced diagonal block (6, upper triangle by rows), its
// part of the gamma column (3) and of G^T z (3); per pair slot the reduced off-diagonal block (9, rows = first); the couplings u of the cameras with lambda (9), the
// pivot, the lambda-gamma coupling; then what a right-hand side adds: its lambda entry and the reduced camera entries (3 per slot)
enum { kCamRec = 12, kRecOff = 36, kRecU = 63, kRecPiv = 72, kRecHlg = 73, kRecRl = 74, kRecRhs = 75, kRecSlots = 84 };
// per-triplet terms of an evaluation: sums (s^T z, the gamma entry of G^T z, the gamma-gamma share), then maxima (|primal residual|, |lambda entry of G^T z|)
enum { kTermSz = 0, kTermGzg = 1, kTermKappa = 2, kTermRp = 3, kTermRdl = 4, kTerms = 5 };
enum { kPredictor = 0, kCorrector = 1 };
enum { kConverged = 0, kIterationLimit = 1, kFactorisationLost = 2, kNotFinite = 3, kNoTriplets = 6 };

struct Params { int max_iterations = 60; double gap_tol = 1e-9, feas_tol = 1e-9; };
struct Summary { double gamma, dual_objective, gap, primal_residual, dual_residual; int iterations, bumps, n_components, n_loose, termination; };

PVLM_LP_HD int slot_first(int q) { return q == 1 ? 1 : 0; }          // (i,j), (j,k), (i,k) over the cameras (i, j, k)
PVLM_LP_HD int slot_second(int q) { return q == 0 ? 1 : 2; }

struct Trip { double R[3][9], t[3][3], lo; };

PVLM_LP_HD void load_trip(long long t, const int* trip_pair, const double* R21, const double* t21, const double* lo, Trip* o) {
  for (int q = 0; q < 3; ++q) {
    const long long p = trip_pair[3 * t + q];
    for (int k = 0; k < 9; ++k) o->R[q][k] = R21[9 * p + k];
    for (int k = 0; k < 3; ++k) o->t[q][k] = t21[3 * p + k];
  }
  o->lo = lo[t];
}
PVLM_LP_HD void load_rows(const double* v, long long T, long long t, double* out) { for (int r = 0; r < kRows; ++r) out[r] = v[r * T + t]; }
PVLM_LP_HD void store_rows(double* v, long long T, long long t, const double* in) { for (int r = 0; r < kRows; ++r) v[r * T + t] = in[r]; }
PVLM_LP_HD void load_cams(const double* x, const int* trip_cam, long long t, double (*out)[3]) {
  for (int m = 0; m < 3; ++m) { const long long c = trip_cam[3 * t + m]; for (int k = 0; k < 3; ++k) out[m][k] = x[3 * c + k]; }
}

// 0.9 x the mean of |t_21| over the three pairs (:381-385)
inline double lambda_bound(const double* a, const double* b, const double* c) {
  double sum = 0;
  for (const double* v : {a, b, c}) sum += std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  sum /= 3.0;
  return sum * 0.9;
}

// e of pair slot q at the cameras x and lambda
PVLM_LP_HD void pair_e(const Trip& tr, int q, const double (*x)[3], double lam, double* e) {
  const double* R = tr.R[q]; const double* a = x[slot_first(q)]; const double* b = x[slot_second(q)];
  for (int c = 0; c < 3; ++c) e[c] = b[c] - ((R[3 * c] * a[0] + R[3 * c + 1] * a[1]) + R[3 * c + 2] * a[2]) - lam * tr.t[q][c];
}
// the triplet's 19 entries of G x
PVLM_LP_HD void rows_G(const Trip& tr, const double (*x)[3], double lam, double gam, double* out) {
  for (int q = 0; q < 3; ++q) {
    double e[3];
    pair_e(tr, q, x, lam, e);
    for (int c = 0; c < 3; ++c) { out[6 * q + 2 * c] = e[c] - gam; out[6 * q + 2 * c + 1] = -e[c] - gam; }
  }
  out[kBound] = -lam;
}
// the triplet's entries of G x + s - h
PVLM_LP_HD void primal_residual(const Trip& tr, const double (*x)[3], double lam, double gam, const double* s, double* rp) {
  rows_G(tr, x, lam, gam, rp);
  for (int r = 0; r < kRows; ++r) rp[r] += s[r];
  rp[kBound] += tr.lo;
}
// the start of one triplet's rows at t = 0, its lambda and gamma: s = h - G x, z = zval
PVLM_LP_HD void start_rows(const Trip& tr, double lam, double gam, double zval, double* s, double* z) {
  const double zero[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double g[kRows];
  rows_G(tr, zero, lam, gam, g);
  for (int r = 0; r < kRows; ++r) { s[r] = (r == kBound ? -tr.lo : 0.0) - g[r]; z[r] = zval; }
}
// the triplet's part of G^T v: on its cameras, its lambda and gamma
PVLM_LP_HD void gt_apply(const Trip& tr, const double* v, double (*cam)[3], double* lam, double* gam) {
  for (int m = 0; m < 3; ++m) for (int k = 0; k < 3; ++k) cam[m][k] = 0.0;
  double l = 0.0, g = 0.0;
  for (int q = 0; q < 3; ++q) {
    const double* R = tr.R[q]; const int a = slot_first(q), b = slot_second(q);
    for (int c = 0; c < 3; ++c) {
      const double d = v[6 * q + 2 * c] - v[6 * q + 2 * c + 1], sm = v[6 * q + 2 * c] + v[6 * q + 2 * c + 1];
      cam[b][c] += d;
      for (int x = 0; x < 3; ++x) cam[a][x] -= R[3 * c + x] * d;
      l -= d * tr.t[q][c]; g -= sm;
    }
  }
  *lam = l - v[kBound]; *gam = g;
}

// The evaluation of one triplet at (x, lam, gam, s, z): its record with lambda eliminated (rec, stride T) and its terms (terms, stride tstride).
PVLM_LP_HD void assemble_triplet(const Trip& tr, const double (*x)[3], double lam, double gam, const double* s, const double* z, double* rec, long long T, double* terms,
                                 long long tstride) {
  double D[3][6], O[3][9], u[3][3], bg[3][3], gz[3][3], hll = 0.0, hlg = 0.0, hgg = 0.0, gzl, gzg, sz = 0.0, rp[kRows], rpm = 0.0;
  for (int m = 0; m < 3; ++m) { for (int k = 0; k < 6; ++k) D[m][k] = 0.0; for (int k = 0; k < 3; ++k) { u[m][k] = 0.0; bg[m][k] = 0.0; } }
  for (int q = 0; q < 3; ++q) {
    const double* R = tr.R[q]; const int a = slot_first(q), b = slot_second(q);
    double sg[3], dl[3];
    for (int c = 0; c < 3; ++c) {
      const double wp = z[6 * q + 2 * c] / s[6 * q + 2 * c], wm = z[6 * q + 2 * c + 1] / s[6 * q + 2 * c + 1];
      sg[c] = wp + wm; dl[c] = wp - wm;
      const double tc = tr.t[q][c];
      hll += sg[c] * tc * tc; hlg += dl[c] * tc; hgg += sg[c];
      u[b][c] -= sg[c] * tc; bg[b][c] -= dl[c];
    }
    D[b][0] += sg[0]; D[b][3] += sg[1]; D[b][5] += sg[2];
    int k = 0;
    for (int xx = 0; xx < 3; ++xx) {
      for (int y = xx; y < 3; ++y, ++k) D[a][k] += (sg[0] * R[xx] * R[y] + sg[1] * R[3 + xx] * R[3 + y]) + sg[2] * R[6 + xx] * R[6 + y];
      u[a][xx] += (R[xx] * (sg[0] * tr.t[q][0]) + R[3 + xx] * (sg[1] * tr.t[q][1])) + R[6 + xx] * (sg[2] * tr.t[q][2]);
      bg[a][xx] += (R[xx] * dl[0] + R[3 + xx] * dl[1]) + R[6 + xx] * dl[2];
      for (int c = 0; c < 3; ++c) O[q][3 * xx + c] = -R[3 * c + xx] * sg[c];
    }
  }
  hll += z[kBound] / s[kBound];
  gt_apply(tr, z, gz, &gzl, &gzg);
  primal_residual(tr, x, lam, gam, s, rp);
  for (int r = 0; r < kRows; ++r) { sz += s[r] * z[r]; rpm = fmax(rpm, fabs(rp[r])); }
  // lambda leaves by its pivot
  for (int m = 0; m < 3; ++m) {
    int k = 0;
    for (int xx = 0; xx < 3; ++xx) for (int y = xx; y < 3; ++y, ++k) D[m][k] -= u[m][xx] * u[m][y] / hll;
    for (int k2 = 0; k2 < 3; ++k2) bg[m][k2] -= u[m][k2] * hlg / hll;
  }
  for (int q = 0; q < 3; ++q) {
    const int a = slot_first(q), b = slot_second(q);
    for (int xx = 0; xx < 3; ++xx) for (int y = 0; y < 3; ++y) O[q][3 * xx + y] -= u[a][xx] * u[b][y] / hll;
  }
  for (int m = 0; m < 3; ++m) {
    double* o = rec + (long long)(kCamRec * m) * T;
    for (int k = 0; k < 6; ++k) o[k * T] = D[m][k];
    for (int k = 0; k < 3; ++k) { o[(6 + k) * T] = bg[m][k]; o[(9 + k) * T] = gz[m][k]; rec[(kRecU + 3 * m + k) * T] = u[m][k]; }
  }
  for (int q = 0; q < 3; ++q) for (int k = 0; k < 9; ++k) rec[(kRecOff + 9 * q + k) * T] = O[q][k];
  rec[kRecPiv * T] = hll; rec[kRecHlg * T] = hlg;
  terms[kTermSz * tstride] = sz; terms[kTermGzg * tstride] = gzg; terms[kTermKappa * tstride] = hgg - hlg * hlg / hll;
  terms[kTermRp * tstride] = rpm; terms[kTermRdl * tstride] = fabs(gzl);
}

// the complementarity right-hand side of row r in a mode: s z, and for the corrector - sigma mu + ds_aff dz_aff on top
PVLM_LP_HD double comp_rhs(int mode, double s, double z, double sigma_mu, double ds_aff, double dz_aff) {
  return mode == kCorrector ? s * z - sigma_mu + ds_aff * dz_aff : s * z;
}

// The right-hand side of a mode for one triplet: G^T q with q = (r_c - s z) / s - w r_p, lambda eliminated; the lambda entry and the reduced camera entries go into
// the record, the reduced gamma share comes back.  ds / dz: the predictor's direction (read by the corrector only).
PVLM_LP_HD double rhs_triplet(int mode, const Trip& tr, const double (*x)[3], double lam, double gam, const double* s, const double* z, const double* ds, const double* dz,
                              double sigma_mu, double* rec, long long T) {
  double rp[kRows], qv[kRows], cam[3][3], rl, rg;
  primal_residual(tr, x, lam, gam, s, rp);
  for (int r = 0; r < kRows; ++r) qv[r] = (comp_rhs(mode, s[r], z[r], sigma_mu, ds[r], dz[r]) - s[r] * z[r]) / s[r] - z[r] / s[r] * rp[r];
  gt_apply(tr, qv, cam, &rl, &rg);
  const double piv = rec[kRecPiv * T], hlg = rec[kRecHlg * T];
  rec[kRecRl * T] = rl;
  for (int m = 0; m < 3; ++m) for (int k = 0; k < 3; ++k) rec[(kRecRhs + 3 * m + k) * T] = cam[m][k] - rec[(kRecU + 3 * m + k) * T] * rl / piv;
  return rg - hlg * rl / piv;
}

// The direction of a mode for one triplet from the camera steps dx and dgam: dlam by back-substitution, ds and dz per row (ds / dz hold the predictor's on entry of
// the corrector and the new direction on exit); ratio[0] = max -ds / s, ratio[1] = max -dz / z over its rows (0 when none is negative).
PVLM_LP_HD void direction_triplet(int mode, const Trip& tr, const double (*x)[3], double lam, double gam, const double* s, const double* z, const double (*dx)[3], double dgam,
                                  double sigma_mu, const double* rec, long long T, double* ds, double* dz, double* dlam, double* ratio) {
  double rp[kRows], gdx[kRows], ud = 0.0;
  for (int m = 0; m < 3; ++m) for (int k = 0; k < 3; ++k) ud += rec[(kRecU + 3 * m + k) * T] * dx[m][k];
  const double dl = (rec[kRecRl * T] - ud - rec[kRecHlg * T] * dgam) / rec[kRecPiv * T];
  primal_residual(tr, x, lam, gam, s, rp);
  rows_G(tr, dx, dl, dgam, gdx);
  double rs = 0.0, rz = 0.0;
  for (int r = 0; r < kRows; ++r) {
    const double rc = comp_rhs(mode, s[r], z[r], sigma_mu, ds[r], dz[r]);
    const double d_s = -rp[r] - gdx[r], d_z = (-rc - z[r] * d_s) / s[r];
    ds[r] = d_s; dz[r] = d_z;
    rs = fmax(rs, -d_s / s[r]); rz = fmax(rz, -d_z / z[r]);
  }
  *dlam = dl; ratio[0] = rs; ratio[1] = rz;
}

// the triplet's term of the predictor's complementarity at its step lengths
PVLM_LP_HD double mu_aff_triplet(const double* s, const double* z, const double* ds, const double* dz, double ap, double ad) {
  double sum = 0.0;
  for (int r = 0; r < kRows; ++r) sum += (s[r] + ap * ds[r]) * (z[r] + ad * dz[r]);
  return sum;
}

// lane `lane` of the kGroup lanes of one row of a CSR of (triplet, slot) entries (entry = 3 * triplet + slot): N consecutive components from slot0 + slot * per_slot
template <int N> PVLM_LP_HD void gather_lane(const double* rec, long long T, const int* ent, int e0, int e1, int lane, int slot0, int per_slot, double* part) {
  for (int k = 0; k < N; ++k) part[k] = 0.0;
  for (int e = e0 + lane; e < e1; e += pg::kGroup) {
    const int t = ent[e] / 3, m = ent[e] % 3;
    const double* s = rec + (long long)(slot0 + m * per_slot) * T + t;
    for (int k = 0; k < N; ++k) part[k] += s[(long long)k * T];
  }
}
// a pair's gathered 3 x 3 into its 6 x 6 row-major block of the solver's list
PVLM_LP_HD void off_block(const double* v, double* B) { for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) B[6 * x + y] = v[3 * x + y]; }

// ---- host side: shared by the device entry point and by the host compile -------------------------------------------------------------------------------------

// nullptr, or what is wrong with the arguments
inline const char* check_args(int F, int P, const int* first, const int* second, const double* R21, const double* t21, int T, const int* trip_pairs, int origin,
                              const double* translations, const Params* prm) {
  if (F < 0 || P < 0 || T < 0) return "a negative count";
  if (!prm || !translations || (P > 0 && (!first || !second || !R21 || !t21)) || (T > 0 && !trip_pairs)) return "null argument";
  if (origin < 0 || origin >= F) return "origin_idx names no camera";
  if (prm->max_iterations < 1) return "max_iterations < 1";
  if (!(prm->gap_tol > 0.0) || !(prm->feas_tol > 0.0) || !std::isfinite(prm->gap_tol) || !std::isfinite(prm->feas_tol)) return "a tolerance is not positive and finite";
  std::vector<std::pair<int, int>> seen((size_t)P);
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || first[p] >= F || second[p] < 0 || second[p] >= F) return "a pair names a camera that is not there";
    if (first[p] >= second[p]) return "a pair with first >= second";
    seen[(size_t)p] = {first[p], second[p]};
  }
  std::sort(seen.begin(), seen.end());
  for (int p = 1; p < P; ++p) if (seen[(size_t)p] == seen[(size_t)p - 1]) return "a repeated pair";
  if (!pg::finite_all(R21, 9 * (size_t)P) || !pg::finite_all(t21, 3 * (size_t)P) || !pg::finite_all(translations, 3 * (size_t)F)) return "an input is not finite";
  for (int k = 0; k < 3; ++k) if (translations[3 * (size_t)origin + k] != 0.0) return "the translation of the origin camera is not zero";
  for (int t = 0; t < T; ++t) {
    const int* q = trip_pairs + 3 * (size_t)t;
    for (int k = 0; k < 3; ++k) if (q[k] < 0 || q[k] >= P) return "a triplet names a pair that is not there";
    const int i = first[q[0]], j = second[q[0]], k = second[q[1]];
    if (first[q[1]] != j || first[q[2]] != i || second[q[2]] != k) return "a triplet whose pairs are not (i,j), (j,k), (i,k)";      // i < j < k follows from first < second
  }
  return nullptr;
}

// What a call fixes before its first iteration: the triplets' cameras and bounds, the components and pins, both CSRs, the index lists of the camera system
// ([F diagonal | P off-diagonal] as pg::CameraSystem has them, a pinned or loose camera and a pair in no triplet dropped) and the start.
struct Problem {
  int F = 0, P = 0, T = 0, n_components = 0, n_loose = 0;
  std::vector<int> trip_cam, cam_off, cam_ent, pair_off, pair_ent, index;      // index: 3 x the camera's place among the free ones, or -1
  std::vector<double> lo, lam0;
  double gamma0 = 0, z0 = 0;                                                     // the start: lambda = lo + 1, gamma, every multiplier (the rows start by start_rows)
  pg::CameraSystem sys;

  void init(int F_, int P_, const int* first, const int* second, const double* R21, const double* t21, int T_, const int* trip_pairs, int origin) {
    F = F_; P = P_; T = T_;
    trip_cam.resize(3 * (size_t)T); lo.resize((size_t)T); lam0.resize((size_t)T);
    std::vector<int> root((size_t)F), in_trip((size_t)F, 0), in_pair((size_t)P, 0);
    std::iota(root.begin(), root.end(), 0);
    auto find = [&](int c) { while (root[(size_t)c] != c) { root[(size_t)c] = root[(size_t)root[(size_t)c]]; c = root[(size_t)c]; } return c; };
    cam_off.assign((size_t)F + 1, 0); pair_off.assign((size_t)P + 1, 0);
    for (int t = 0; t < T; ++t) {
      const int* q = trip_pairs + 3 * (size_t)t;
      int* c = &trip_cam[3 * (size_t)t];
      c[0] = first[q[0]]; c[1] = second[q[0]]; c[2] = second[q[1]];
      lo[(size_t)t] = lambda_bound(t21 + 3 * (size_t)q[0], t21 + 3 * (size_t)q[1], t21 + 3 * (size_t)q[2]);
      lam0[(size_t)t] = lo[(size_t)t] + 1.0;
      for (int m = 0; m < 3; ++m) { in_trip[(size_t)c[m]] = 1; in_pair[(size_t)q[m]] = 1; ++cam_off[(size_t)c[m] + 1]; ++pair_off[(size_t)q[m] + 1]; }
      for (int m = 1; m < 3; ++m) { const int a = find(c[0]), b = find(c[m]); if (a != b) root[(size_t)(a > b ? a : b)] = a < b ? a : b; }
    }
    for (int c = 0; c < F; ++c) cam_off[(size_t)c + 1] += cam_off[(size_t)c];
    for (int p = 0; p < P; ++p) pair_off[(size_t)p + 1] += pair_off[(size_t)p];
    cam_ent.assign(3 * (size_t)T, 0); pair_ent.assign(3 * (size_t)T, 0);
    std::vector<int> cat(cam_off.begin(), cam_off.end() - 1), pat(pair_off.begin(), pair_off.end() - 1);
    for (int t = 0; t < T; ++t)
      for (int m = 0; m < 3; ++m) { cam_ent[(size_t)cat[(size_t)trip_cam[3 * (size_t)t + m]]++] = 3 * t + m; pair_ent[(size_t)pat[(size_t)trip_pairs[3 * (size_t)t + m]]++] = 3 * t + m; }
    // the union keeps the lowest camera as the root: it is the pin unless the component is the origin's
    const int origin_root = in_trip[(size_t)origin] ? find(origin) : -1;
    index.assign((size_t)F, -1);
    int n_free = 0;
    n_components = 0; n_loose = 0;
    for (int c = 0; c < F; ++c) {
      if (!in_trip[(size_t)c]) { ++n_loose; continue; }
      const int r = find(c);
      if (r == c) ++n_components;
      const int pin = r == origin_root ? origin : r;
      if (c != pin) index[(size_t)c] = 3 * n_free++;
    }
    sys.F = F; sys.P = P; sys.origin = -1; sys.n = 3 * n_free;
    sys.rows.assign(6 * ((size_t)F + P), -1); sys.cols.assign(6 * ((size_t)F + P), -1); sys.mirror.assign((size_t)F + P, 0);
    for (int c = 0; c < F; ++c) for (int k = 0; k < 3; ++k) if (index[(size_t)c] >= 0) sys.rows[6 * (size_t)c + k] = sys.cols[6 * (size_t)c + k] = index[(size_t)c] + k;
    for (int p = 0; p < P; ++p) {
      const size_t b = (size_t)F + p;
      sys.mirror[b] = 1;
      if (!in_pair[(size_t)p]) continue;
      for (int k = 0; k < 3; ++k) {
        if (index[(size_t)first[p]] >= 0) sys.rows[6 * b + k] = index[(size_t)first[p]] + k;
        if (index[(size_t)second[p]] >= 0) sys.cols[6 * b + k] = index[(size_t)second[p]] + k;
      }
    }
    sys.sigma.assign((size_t)sys.n, 1.0); sys.diag.assign((size_t)sys.n, 0.0); sys.rhs.assign((size_t)sys.n, 0.0);
    // the start: t = 0, so e = -lambda t_21
    std::vector<double> emax((size_t)T);
    for (int t = 0; t < T; ++t) {
      double m = 0;
      for (int q = 0; q < 3; ++q) for (int k = 0; k < 3; ++k) m = std::fmax(m, std::fabs(lam0[(size_t)t] * t21[3 * (size_t)trip_pairs[3 * (size_t)t + q] + k]));
      emax[(size_t)t] = m;
    }
    gamma0 = pg::tree_reduce_host<true>(emax.data(), T) + 1.0;
    z0 = 1.0 / ((double)kRows * T);
  }
  // the Jacobi scale of the free cameras from the gather (kCamRec numbers per camera) and the regularisation
  void prepare(const double* cam, double diag_add) {
    static const int at[3] = {0, 3, 5};
    for (int c = 0; c < F; ++c) {
      if (index[(size_t)c] < 0) continue;
      for (int k = 0; k < 3; ++k) { sys.sigma[(size_t)index[(size_t)c] + k] = 1.0 / std::sqrt(cam[(size_t)kCamRec * c + at[k]]); sys.diag[(size_t)index[(size_t)c] + k] = diag_add; }
    }
  }
  // a 3-per-camera vector into the system's scaled right-hand side, and the solution back (zero where the camera is not free)
  void set_rhs(const double* v, int stride, int at) {
    for (int c = 0; c < F; ++c) if (index[(size_t)c] >= 0) for (int k = 0; k < 3; ++k) sys.rhs[(size_t)index[(size_t)c] + k] = sys.sigma[(size_t)index[(size_t)c] + k] * v[(size_t)stride * c + at + k];
  }
  void get_solution(std::vector<double>* out) const {
    out->assign(3 * (size_t)F, 0.0);
    for (int c = 0; c < F; ++c) if (index[(size_t)c] >= 0) for (int k = 0; k < 3; ++k) (*out)[3 * (size_t)c + k] = sys.sigma[(size_t)index[(size_t)c] + k] * sys.rhs[(size_t)index[(size_t)c] + k];
  }
  // the dot product of two 3-per-camera vectors over the free cameras, in camera order
  double dot(const double* a, int stride, int at, const std::vector<double>& b) const {
    double sum = 0;
    for (int c = 0; c < F; ++c) if (index[(size_t)c] >= 0) for (int k = 0; k < 3; ++k) sum += a[(size_t)stride * c + at + k] * b[3 * (size_t)c + k];
    return sum;
  }
  double max_abs(const double* a, int stride, int at) const {
    double m = 0;
    for (int c = 0; c < F; ++c) if (index[(size_t)c] >= 0) for (int k = 0; k < 3; ++k) m = std::fmax(m, std::fabs(a[(size_t)stride * c + at + k]));
    return m;
  }
};

// The interior-point loop.  Backend (B), every call false on a device error:
//   bool evaluate(double gam, double* terms)             the evaluation at the state: the record, both gathers (cam(): kCamRec per camera), the kTerms roots;
//   bool rhs(int mode, double gam, double sigma_mu, double* gamma_share)   the right-hand side of a mode: cam_rhs() (3 per camera) and the root of the gamma shares;
//   bool solve(int* info)                                the camera system of prob.sys, the solution in prob.sys.rhs;
//   bool direction(int mode, double gam, const std::vector<double>& dx, double dgam, double sigma_mu, double* ratio)   the two maxima;
//   bool mu_aff(double ap, double ad, double* sum);  bool update(double ap, double ad, const std::vector<double>& dx).
// gaps: when given, s^T z at every evaluation (the tests' admission rule reads it).
template <class B> inline void run(B& be, Problem& prob, const Params& prm, Summary* out, std::vector<double>* gaps = nullptr) {
  Summary s{0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, prob.n_components, prob.n_loose, -1};
  const double rows = (double)kRows * prob.T;
  double gam = prob.gamma0, diag_add = 1e-12, terms[kTerms];
  std::vector<double> y1, y2, dx;
  // one camera solve with the retries; the solution (3 per camera) in *sol
  auto solve = [&](const double* v, int stride, int at, std::vector<double>* sol) {
    for (;;) {
      int info = 0;
      prob.prepare(be.cam(), diag_add);
      prob.set_rhs(v, stride, at);
      if (!be.solve(&info)) return false;
      if (info == 0) { prob.get_solution(sol); return true; }
      if (info < 0 || s.bumps == 3) { s.termination = kFactorisationLost; return false; }
      ++s.bumps; diag_add *= 100.0;
    }
  };
  // the step of a mode from its right-hand side: dx and dgam through the 1 x 1 border
  auto border = [&](double gamma_share, double kappa, double* dgam) {
    const double* cam = be.cam();
    if (!solve(be.cam_rhs(), 3, 0, &y2)) return false;
    const double rho = -1.0 + gamma_share;
    *dgam = (rho - prob.dot(cam, kCamRec, 6, y2)) / (kappa - prob.dot(cam, kCamRec, 6, y1));
    dx.resize(y2.size());
    for (size_t i = 0; i < y2.size(); ++i) dx[i] = y2[i] - *dgam * y1[i];
    return true;
  };
  for (int it = 0;; ++it) {
    if (!be.evaluate(gam, terms)) break;
    const double* cam = be.cam();
    s.gamma = gam; s.gap = terms[kTermSz]; s.primal_residual = terms[kTermRp]; s.iterations = it;
    s.dual_residual = std::fmax(std::fmax(prob.max_abs(cam, kCamRec, 9), terms[kTermRdl]), std::fabs(1.0 + terms[kTermGzg]));
    if (gaps) gaps->push_back(s.gap);
    if (!std::isfinite(gam) || !std::isfinite(s.gap) || !std::isfinite(s.primal_residual) || !std::isfinite(s.dual_residual) || !std::isfinite(terms[kTermKappa])) {
      s.termination = kNotFinite; break;
    }
    if (s.gap <= prm.gap_tol * std::fmax(1.0, std::fabs(gam)) && s.primal_residual <= prm.feas_tol && s.dual_residual <= prm.feas_tol) { s.termination = kConverged; break; }
    if (it == prm.max_iterations) { s.termination = kIterationLimit; break; }
    const double mu = s.gap / rows, kappa = terms[kTermKappa];
    double share = 0, dgam = 0, ratio[2], sum = 0;
    if (!solve(cam, kCamRec, 6, &y1)) break;                              // the gamma column
    if (!be.rhs(kPredictor, gam, 0.0, &share) || !border(share, kappa, &dgam)) break;
    if (!be.direction(kPredictor, gam, dx, dgam, 0.0, ratio)) break;
    const double ap_aff = ratio[0] > 1.0 ? 1.0 / ratio[0] : 1.0, ad_aff = ratio[1] > 1.0 ? 1.0 / ratio[1] : 1.0;
    if (!be.mu_aff(ap_aff, ad_aff, &sum)) break;
    const double frac = (sum / rows) / mu, sigma_mu = frac * frac * frac * mu;
    if (!std::isfinite(sigma_mu) || !std::isfinite(dgam)) { s.termination = kNotFinite; break; }
    if (!be.rhs(kCorrector, gam, sigma_mu, &share) || !border(share, kappa, &dgam)) break;
    if (!be.direction(kCorrector, gam, dx, dgam, sigma_mu, ratio)) break;
    if (!std::isfinite(dgam) || !std::isfinite(ratio[0]) || !std::isfinite(ratio[1])) { s.termination = kNotFinite; break; }
    const double ap = std::fmin(1.0, ratio[0] > 0.0 ? 0.99 / ratio[0] : 1.0), ad = std::fmin(1.0, ratio[1] > 0.0 ? 0.99 / ratio[1] : 1.0);
    if (!be.update(ap, ad, dx)) break;
    gam += ap * dgam;
  }
  *out = s;
}

// the dual objective -h^T z = sum lo_T z_bound of the bound rows' multipliers (one per triplet), by the fixed tree
inline double dual_objective(const Problem& prob, const double* z_bound) {
  std::vector<double> v((size_t)prob.T);
  for (int t = 0; t < prob.T; ++t) v[(size_t)t] = prob.lo[(size_t)t] * z_bound[t];
  return pg::tree_reduce_host<false>(v.data(), prob.T);
}

}  // namespace pvlm_translp
