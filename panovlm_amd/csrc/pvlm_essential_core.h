// Statement of K34: the loop body of SfM::FilterImagePairs (sfm/SfM.cpp:298-480) up to, and not including, RefineRelativePose: ComputeEssential
// (base/EssentialMatrix.cpp:10-40), the AC-RANSAC loop of FindEssentialACRANSAC (:180-288), ACRansac_NFA::ComputeNFA in its non-quantified branch
// (base/ACRansac_NFA.cpp:103-137) with the constructor's tables (:23-36), DecomposeEssential (:151-178), SfM::CheckRT (sfm/SfM.cpp:1478-1547) and the selection
// over the runs (:361-391, :413-416).  Host / device: csrc/pvlm_essential.hip runs one (pair, run) chain per workgroup on these functions, the host mirror
// (host/pvlm_host_essential.hpp) runs the serial chain at the end of this file, and a host compile (tests/cpp/essential_core_check.cpp) is what the CPU
// tests compare with numpy and the GPU tests compare with bit for bit.  Compile with -ffp-contract=off.  Nothing here calls libm on a path that feeds a
// decision: only + - * / sqrt and integer operations on the bit pattern of a double (exact on both sides).  The two libm values the stage needs, the
// log10 tables of the NFA and the cosine of 3 degrees, are INPUTS made once on the host (nfa_tables, angle_threshold).
//
// ComputeEssential.  Row i of A is p2 (x) p1 = (p2x p1x, p2x p1y, p2x p1z, p2y p1x, ...), float bearings promoted to double.  AtA is kept as its 45 distinct
// entries (r <= c, row by row), every entry the sum of its products in row order.  The eigenvector of the smallest eigenvalue (first index among equal
// ones) reshaped row-major is E0.  Upstream's tridiagonal QL and JacobiSVD are both replaced by the cyclic Jacobi below (parity with Eigen by tolerance,
// host against device in bits): rotations (p, q) in the order (0,1) (0,2) .. (0,n-1) (1,2) .. (n-2,n-1), at most kSweeps sweeps, a sweep that finds every
// off-diagonal entry exactly zero ends it.  A rotation is skipped, and the entry set to zero, when 100 |a_pq| added to |a_pp| and to |a_qq| changes
// neither.  The 3 x 3 SVD goes through the Jacobi eigen-decomposition of E0^T E0 = V diag(w) V^T, w sorted descending (first index among equal ones):
// the singular values are sqrt(max(w_i, 0)), U diag(s0, s1, 0) V^T = E0 (v0 v0^T + v1 v1^T): no division, and the third singular value is 0 exactly.
// DecomposeEssential: V as above, u0 = E v0 / |E v0|, u1 = E v1 / |E v1|, u2 = u0 x u1 (the sign of u2 is free in an SVD: Eigen may order the same four
// candidates differently).
//
// The AC-RANSAC loop is upstream's with ac_ransac_mode = true as upstream forces it (:207), so `precision` is unused: max_threshold = +inf.  min_point_set1/2
// are declared outside the loop and never cleared (:194, :212-216): hypothesis k of a run is fitted to all 8 (k + 1) points sampled so far.  That is the
// default here: AtA is carried and 8 outer products are added.  PVLM_FLAG_ESSENTIAL_FRESH_SAMPLE (kFreshSample) resets AtA every iteration, the textbook
// 8-point hypothesis: a deviation.  iter_limit / iter_reserved, the switch of the sampling set to curr_inlier_idx and the final minNFA >= 0 -> zero matrix
// are restated literally.  The residual is Square(asin(p2 . (E p1).normalized())); the sort key is (residual, match index), a strict total order, so any
// correct sort gives std::sort's result; a NaN residual (|p2 . n| > 1 by rounding) is sorted as +inf and, like upstream's `NaN <= max_threshold`, ends the
// scan.  The scan keeps the lowest k among equal NFA values (strict <).
//
// Deviations.  (1) Sampling: upstream seeds an mt19937 from std::random_device on every draw, so there is nothing to be equal to.  Here: Philox-4x32-10.
// chain key = words 0, 1 of philox(counter = (src frame, tgt frame, run, 0), key = (seed lo, seed hi)); hypothesis k draws the words of
// philox(counter = (k, j, 0, 0), key = chain key), j = 0, 1, ..; an index is mulhi(word, m); a duplicate is rejected and the next word taken until 8
// distinct indices are held; m == 8 uses the set as it stands (base/Random.hpp:70-71).  Nothing depends on batch composition or launch geometry.
// (2) Pairs with fewer than 9 matches are dropped: upstream returns zero below 8 and reads sorted_residuals[-1] at exactly 8.  (3) The runs are ranked
// upstream by an unstable std::sort on the count alone; here the lowest run index among equal counts wins.  (4) parallax is not produced: its only reader
// upstream is commented out (sfm/SfM.cpp:369-373).  (5) FRESH_SAMPLE, above.
// Recalled from Eigen and not pinned against a build of it: fixed-size products sum their three terms in index order; normalized() divides by
// sqrt(squaredNorm) when that is > 0 and returns the vector unchanged otherwise; determinant() of a 3 x 3 is the cofactor expansion along the first row.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "pvlm_triangulate_core.h"

namespace pvlm_essential {

constexpr int kMinSample = 8;          // minimum_sample of ACRansac_NFA
constexpr int kSweeps = 30;
constexpr int kNLds = 1024;           // N_LDS: the largest match count a workgroup of csrc/pvlm_essential.hip handles in LDS (the results do not depend on it)
constexpr long long kMaxMatches = 1ll << 29;    // per pair: the sort pads to the next power of two and its loop doubles once more, in int
constexpr unsigned kFreshSample = 0x800u;     // PVLM_FLAG_ESSENTIAL_FRESH_SAMPLE

PVLM_EQ_UD double inf_d() { return __builtin_huge_val(); }
PVLM_EQ_UD double nan_d() { return __builtin_nan(""); }
PVLM_EQ_UD uint64_t bits_of(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
PVLM_EQ_UD double from_bits(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }
PVLM_EQ_UD double high_part(double x) { return from_bits(bits_of(x) & 0xffffffff00000000ull); }     // the low 32 bits of the significand cleared

// ---- asin and log10 without libm (the fdlibm evaluations: a rational / polynomial after an argument reduction; < 1 ulp on paper, <= 2 ulp tested) ----
PVLM_EQ_UD double asin_r(double z) {
  const double p = z * (0x1.5555555555555p-3 + z * (-0x1.4d61203eb6f7dp-2 + z * (0x1.9c1550e884455p-3 + z * (-0x1.48228b5688f3bp-5 + z * (0x1.9efe07501b288p-11 + z * 0x1.23de10dfdf709p-15)))));
  const double q = 1.0 + z * (-0x1.33a271c8a2d4bp+1 + z * (0x1.02ae59c598ac8p+1 + z * (-0x1.6066c1b8d0159p-1 + z * 0x1.3b8c5b12e9282p-4)));
  return p / q;
}
PVLM_EQ_UD double asin_d(double x) {
  const double pio2_hi = 0x1.921fb54442d18p+0, pio2_lo = 0x1.1a62633145c07p-54;
  const double ax = x < 0.0 ? -x : x;
  if (!(ax <= 1.0)) return nan_d();                        // |x| > 1 and NaN
  if (ax == 1.0) return x * pio2_hi;
  if (ax < 0.5) {
    if (ax < 0x1p-26) return x;
    return x + x * asin_r(x * x);
  }
  const double z = (1.0 - ax) * 0.5, s = sqrt(z), r = asin_r(z);
  double y;
  if (ax >= 0.975) {
    y = pio2_hi - (2.0 * (s + s * r) - pio2_lo);
  } else {
    const double f = high_part(s), c = (z - f * f) / (s + f);
    y = 0.5 * pio2_hi - (2.0 * s * r - (pio2_lo - 2.0 * c) - (0.5 * pio2_hi - 2.0 * f));
  }
  return x < 0.0 ? -y : y;
}
PVLM_EQ_UD double log10_d(double x) {
  const double ivln10hi = 0x1.bcb7b152p-2, ivln10lo = 0x1.b9438ca9aadd5p-36, log10_2hi = 0x1.34413509f6p-2, log10_2lo = 0x1.9fef311f12b36p-42;
  if (x != x || x < 0.0) return nan_d();
  if (x == 0.0) return -inf_d();
  if (x == inf_d()) return x;
  int k = 0;
  if (x < 0x1p-1022) { x = x * 0x1p54; k = -54; }
  uint64_t u = bits_of(x);
  uint32_t hx = (uint32_t)(u >> 32);
  hx += 0x3ff00000u - 0x3fe6a09eu;
  k += (int)(hx >> 20) - 0x3ff;
  hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
  x = from_bits(((uint64_t)hx << 32) | (u & 0xffffffffull));           // in [sqrt(2) / 2, sqrt(2))
  const double f = x - 1.0, hfsq = 0.5 * f * f, s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (0x1.999999997fa04p-2 + w * (0x1.c71c51d8e78afp-3 + w * 0x1.39a09d078c69fp-3));
  const double t2 = z * (0x1.5555555555593p-1 + w * (0x1.2492494229359p-2 + w * (0x1.7466496cb03dep-3 + w * 0x1.2f112df3e5244p-3)));
  const double R = t2 + t1;
  const double hi = high_part(f - hfsq), lo = (f - hi) - hfsq + s * (hfsq + R);
  double val_hi = hi * ivln10hi;
  const double dk = (double)k, y = dk * log10_2hi;
  double val_lo = dk * log10_2lo + (lo + hi) * ivln10lo + lo * ivln10hi;
  const double w2 = y + val_hi;
  val_lo = val_lo + ((y - w2) + val_hi);
  val_hi = w2;
  return val_lo + val_hi;
}

// ---- Philox-4x32-10 ----
struct U4 { uint32_t v[4]; };
PVLM_EQ_UD U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n1 = (uint32_t)b, n2 = (uint32_t)(a >> 32) ^ c3 ^ k1, n3 = (uint32_t)a;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  U4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}
struct ChainKey { uint32_t k0, k1; };
PVLM_EQ_UD ChainKey chain_key(unsigned long long seed, int src, int tgt, int run) {
  const U4 o = philox((uint32_t)src, (uint32_t)tgt, (uint32_t)run, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  ChainKey k; k.k0 = o.v[0]; k.k1 = o.v[1];
  return k;
}
// the 8 positions hypothesis k of a chain draws from a sampling set of m entries (m >= 8)
PVLM_EQ_UD void sample8(ChainKey key, int k, int m, int* out) {
  if (m == 8) { for (int i = 0; i < 8; ++i) out[i] = i; return; }
  int have = 0;
  for (uint32_t j = 0; have < 8; ++j) {
    const U4 o = philox((uint32_t)k, j, 0u, 0u, key.k0, key.k1);
    for (int w = 0; w < 4 && have < 8; ++w) {
      const int idx = (int)(((uint64_t)o.v[w] * (uint64_t)(uint32_t)m) >> 32);
      bool dup = false;
      for (int i = 0; i < have; ++i) dup = dup || out[i] == idx;
      if (!dup) out[have++] = idx;
    }
  }
}

// ---- AtA ----
// entry e of the 45 <-> (r, c), r <= c, row by row
PVLM_EQ_UD void ata_rc(int e, int* r, int* c) {
  int a = 0, left = e;
  while (left >= 9 - a) { left -= 9 - a; ++a; }
  *r = a; *c = a + left;
}
PVLM_EQ_UD int ata_index(int r, int c) { if (r > c) { const int t = r; r = c; c = t; } return r * 9 - (r * (r - 1)) / 2 + (c - r); }
// entry (r, c) += row[r] * row[c] of the correspondence (p1, p2)
PVLM_EQ_UD double ata_term(const float* p1, const float* p2, int r, int c) {
  const double ar = (double)p2[r / 3] * (double)p1[r % 3], ac = (double)p2[c / 3] * (double)p1[c % 3];
  return ar * ac;
}

// ---- cyclic Jacobi on an n x n symmetric matrix a (row-major, both triangles kept) with the rotations accumulated in v ----
struct Rot { double t, c, s; int what; };     // what: 0 = nothing to do (a_pq == 0), 1 = negligible (set a_pq to 0), 2 = rotate
PVLM_EQ_UD Rot jacobi_coeffs(double app, double aqq, double apq) {
  Rot R; R.t = 0.0; R.c = 1.0; R.s = 0.0; R.what = 0;
  if (apq == 0.0) return R;
  const double g = 100.0 * fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { R.what = 1; return R; }
  const double theta = (aqq - app) / (2.0 * apq);
  R.t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  R.c = 1.0 / sqrt(R.t * R.t + 1.0); R.s = R.t * R.c; R.what = 2;
  return R;
}
// the part of rotation (p, q) that belongs to row r: rows are independent of each other, so a device may give every row to a lane
PVLM_EQ_UD void jacobi_row(double* a, double* v, int n, int p, int q, int r, const Rot& R) {
  if (r != p && r != q) {
    const double arp = a[r * n + p], arq = a[r * n + q];
    const double np_ = R.c * arp - R.s * arq, nq_ = R.s * arp + R.c * arq;
    a[r * n + p] = np_; a[p * n + r] = np_; a[r * n + q] = nq_; a[q * n + r] = nq_;
  }
  const double vrp = v[r * n + p], vrq = v[r * n + q];
  v[r * n + p] = R.c * vrp - R.s * vrq; v[r * n + q] = R.s * vrp + R.c * vrq;
}
PVLM_EQ_UD void jacobi_diag(double* a, int n, int p, int q, double app, double aqq, double apq, const Rot& R) {
  if (R.what == 2) { a[p * n + p] = app - R.t * apq; a[q * n + q] = aqq + R.t * apq; }
  a[p * n + q] = 0.0; a[q * n + p] = 0.0;
}
PVLM_EQ_UD void jacobi_serial(double* a, double* v, int n) {
  for (int i = 0; i < n * n; ++i) v[i] = (i / n == i % n) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    bool done = true;
    for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) done = done && a[p * n + q] == 0.0;
    if (done) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double app = a[p * n + p], aqq = a[q * n + q], apq = a[p * n + q];
        const Rot R = jacobi_coeffs(app, aqq, apq);
        if (R.what == 0) continue;
        if (R.what == 2) for (int r = 0; r < n; ++r) jacobi_row(a, v, n, p, q, r, R);
        jacobi_diag(a, n, p, q, app, aqq, apq, R);
      }
  }
}
// the 9 x 9 from the 45 entries
PVLM_EQ_UD void ata_expand(const double* ata, double* a) {
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) a[r * 9 + c] = ata[ata_index(r, c)];
}
// after the Jacobi of the 9 x 9 (a diagonal, v the eigenvectors in columns): E0, then the rank-2 projection.  sv (optional): the singular values (s0, s1, 0)
PVLM_EQ_UD void essential_from_eig9(const double* a, const double* v, double* E, double* sv) {
  int best = 0;
  for (int i = 1; i < 9; ++i) if (a[i * 9 + i] < a[best * 9 + best]) best = i;
  double E0[9], m[9], V[9];
  for (int i = 0; i < 9; ++i) E0[i] = v[i * 9 + best];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[3 * i + j] = (E0[i] * E0[j] + E0[3 + i] * E0[3 + j]) + E0[6 + i] * E0[6 + j];        // E0^T E0
  jacobi_serial(m, V, 3);
  int o0 = 0;
  for (int i = 1; i < 3; ++i) if (m[4 * i] > m[4 * o0]) o0 = i;
  int o1 = o0 == 0 ? 1 : 0;
  for (int i = 0; i < 3; ++i) if (i != o0 && m[4 * i] > m[4 * o1]) o1 = i;
  double Pm[9];                                                                                                     // v0 v0^T + v1 v1^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Pm[3 * i + j] = V[3 * i + o0] * V[3 * j + o0] + V[3 * i + o1] * V[3 * j + o1];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[3 * i + j] = (E0[3 * i] * Pm[j] + E0[3 * i + 1] * Pm[3 + j]) + E0[3 * i + 2] * Pm[6 + j];
  if (sv) { sv[0] = sqrt(m[4 * o0] > 0.0 ? m[4 * o0] : 0.0); sv[1] = sqrt(m[4 * o1] > 0.0 ? m[4 * o1] : 0.0); sv[2] = 0.0; }
}

// ---- residual and NFA ----
PVLM_EQ_UD double residual(const double* E, const float* p1f, const float* p2f) {
  const double p1[3] = {(double)p1f[0], (double)p1f[1], (double)p1f[2]}, p2[3] = {(double)p2f[0], (double)p2f[1], (double)p2f[2]};
  double q[3];
  for (int i = 0; i < 3; ++i) q[i] = (E[3 * i] * p1[0] + E[3 * i + 1] * p1[1]) + E[3 * i + 2] * p1[2];
  const double z = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
  if (z > 0.0) { const double s = sqrt(z); q[0] = q[0] / s; q[1] = q[1] / s; q[2] = q[2] / s; }
  const double angle = (p2[0] * q[0] + p2[1] * q[1]) + p2[2] * q[2];
  const double a = asin_d(angle);
  return a * a;
}
PVLM_EQ_UD double sort_key(double res) { return res != res ? inf_d() : res; }
PVLM_EQ_UD bool key_less(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }
// tab: [log_e0, log_alpha0, log_c_n[0..n], log_c_k[0..n]] of nfa_tables(n).  The NFA of taking the k smallest residuals, key = the k-th smallest (finite).
PVLM_EQ_UD double nfa_value(const double* tab, int n, int k, double key) {
  const double log_alpha = tab[1] + 0.25 * log10_d(key + 0x1p-23);            // numeric_limits<float>::epsilon()
  return ((tab[0] + log_alpha * (double)(k - kMinSample)) + tab[2 + k]) + tab[2 + (n + 1) + k];
}

// ---- the bookkeeping of one chain (:189-193, :241-285), the same object on the host and in every lane of a workgroup ----
struct ChainState {
  double minNFA; int iter, iter_limit, iter_reserved, max_iterations;
};
PVLM_EQ_UD ChainState chain_begin(int max_iterations) {
  ChainState s; s.minNFA = inf_d(); s.iter = 0; s.max_iterations = max_iterations; s.iter_reserved = max_iterations / 10; s.iter_limit = max_iterations - s.iter_reserved;
  return s;
}
PVLM_EQ_UD bool chain_running(const ChainState& s) { return s.iter < s.iter_limit && s.iter < s.max_iterations; }
// after hypothesis s.iter with ComputeNFA's (best_nfa, best_k): *better = the model is the best so far, *swap = the sampling set becomes the first best_k of
// the sorted list.  Advances s.iter.
PVLM_EQ_UD void chain_step(ChainState& s, double best_nfa, int best_k, bool* better, bool* swap) {
  const bool good = best_k > kMinSample;
  *better = good && best_nfa < s.minNFA;
  *swap = false;
  if (*better) s.minNFA = best_nfa;
  if ((*better && s.minNFA < 0.0) || (s.iter + 1 == s.iter_limit && s.iter_reserved > 0)) {
    if (best_k == 0) { s.iter_limit++; s.iter_reserved--; }
    else {
      *swap = true;
      if (s.iter_reserved > 0) { s.iter_limit = s.iter + 1 + s.iter_reserved; s.iter_reserved = 0; }
    }
  }
  s.iter++;
}
PVLM_EQ_UD bool chain_has_model(const ChainState& s) { return !(s.minNFA >= 0.0); }

// ---- DecomposeEssential and CheckRT ----
PVLM_EQ_UD double det3(const double* m) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// R: 4 x 9 (rot_1, rot_1, rot_2, rot_2), t: 4 x 3 (trans, -trans, trans, -trans)
PVLM_EQ_UD void decompose(const double* E, double* R, double* t) {
  double m[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[3 * i + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
  jacobi_serial(m, V, 3);
  int o[3]; o[0] = 0;
  for (int i = 1; i < 3; ++i) if (m[4 * i] > m[4 * o[0]]) o[0] = i;
  o[1] = o[0] == 0 ? 1 : 0;
  for (int i = 0; i < 3; ++i) if (i != o[0] && m[4 * i] > m[4 * o[1]]) o[1] = i;
  o[2] = 3 - o[0] - o[1];
  double U[9], Vs[9];                                      // columns in singular-value order
  for (int c = 0; c < 3; ++c) for (int i = 0; i < 3; ++i) Vs[3 * i + c] = V[3 * i + o[c]];
  for (int c = 0; c < 2; ++c) {
    double u[3];
    for (int i = 0; i < 3; ++i) u[i] = (E[3 * i] * Vs[c] + E[3 * i + 1] * Vs[3 + c]) + E[3 * i + 2] * Vs[6 + c];
    const double z = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    if (z > 0.0) { const double s = sqrt(z); u[0] = u[0] / s; u[1] = u[1] / s; u[2] = u[2] / s; }
    for (int i = 0; i < 3; ++i) U[3 * i + c] = u[i];
  }
  U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];      // u0 x u1
  double tr[3] = {U[2], U[5], U[8]};
  const double z = (tr[0] * tr[0] + tr[1] * tr[1]) + tr[2] * tr[2];
  if (z > 0.0) { const double s = sqrt(z); tr[0] = tr[0] / s; tr[1] = tr[1] / s; tr[2] = tr[2] / s; }
  // U W = [u1, -u0, u2], U W^T = [-u1, u0, u2]
  double r1[9], r2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      r1[3 * i + j] = (U[3 * i + 1] * Vs[3 * j] + (-U[3 * i]) * Vs[3 * j + 1]) + U[3 * i + 2] * Vs[3 * j + 2];
      r2[3 * i + j] = ((-U[3 * i + 1]) * Vs[3 * j] + U[3 * i] * Vs[3 * j + 1]) + U[3 * i + 2] * Vs[3 * j + 2];
    }
  if (det3(r1) < 0.0) for (int i = 0; i < 9; ++i) r1[i] = -r1[i];
  if (det3(r2) < 0.0) for (int i = 0; i < 9; ++i) r2[i] = -r2[i];
  for (int i = 0; i < 9; ++i) { R[i] = r1[i]; R[9 + i] = r1[i]; R[18 + i] = r2[i]; R[27 + i] = r2[i]; }
  for (int i = 0; i < 3; ++i) { t[i] = tr[i]; t[3 + i] = -tr[i]; t[6 + i] = tr[i]; t[9 + i] = -tr[i]; }
}
// VectorAngle3D(a, b) * 180 / M_PI > 3, restated on the cosine: cos_reject = the largest cosine whose angle the host's acos still puts above 3 degrees
PVLM_EQ_UD bool angle_above(const double* a, const double* b, double cos_reject) {
  double c = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
  const double n1 = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), n2 = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  c = c / (n1 * n2);
  return c <= cos_reject;                                    // false for NaN, as acos(NaN) * 180 / M_PI > 3 is
}
// one match of CheckRT (:1501-1534): the triangulated point and whether it counts
PVLM_EQ_UD bool check_point(const double* R, const double* t, const float* p1, const float* p2, double cos_reject, double* P) {
  pvlm_triangulate::triangulate_2view(R, t, p1, p2, P);
  const double big = inf_d();
  if (!(P[0] == P[0] && P[0] != big && P[0] != -big) || !(P[1] == P[1] && P[1] != big && P[1] != -big) || !(P[2] == P[2] && P[2] != big && P[2] != -big)) return false;
  double n1[3] = {P[0], P[1], P[2]};
  const double z = (n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2];
  if (z > 0.0) { const double s = sqrt(z); n1[0] = n1[0] / s; n1[1] = n1[1] / s; n1[2] = n1[2] / s; }
  const double p1d[3] = {(double)p1[0], (double)p1[1], (double)p1[2]}, p2d[3] = {(double)p2[0], (double)p2[1], (double)p2[2]};
  if (angle_above(n1, p1d, cos_reject)) return false;
  double in2[3];
  for (int i = 0; i < 3; ++i) in2[i] = ((R[3 * i] * P[0] + R[3 * i + 1] * P[1]) + R[3 * i + 2] * P[2]) + t[i];
  if (angle_above(in2, p2d, cos_reject)) return false;
  return true;
}
// the selection inside one run (:361-380) on the four CheckRT counts: the candidate, or -1 when the run is dropped
PVLM_EQ_UD int select_candidate(const int* num_pts, int triangulation_num_threshold) {
  int best = 0;
  for (int j = 1; j < 4; ++j) if (num_pts[j] > num_pts[best]) best = j;
  if (num_pts[best] < triangulation_num_threshold) return -1;
  int similar = 0;
  for (int j = 0; j < 4; ++j) similar += ((double)(unsigned)num_pts[j] > 0.8 * (double)num_pts[best]) ? 1 : 0;
  if (similar > 1) return -1;
  return best;
}

// ---- host only: the libm inputs ----
// [log_e0, log_alpha0, log_c_n[0..n], log_c_k[0..n]] (base/ACRansac_NFA.cpp:16-36); n >= 9; tab holds 2 + 2 (n + 1) doubles
inline void nfa_tables(int n, double* tab) {
  tab[0] = std::log10(1.0 * (double)(n - kMinSample));
  tab[1] = std::log10(0.5);
  double* cn = tab + 2; double* ck = tab + 2 + (n + 1);
  auto lg = [](int i) { return i == 0 ? 0.0 : std::log10((double)i); };
  for (int k = 0; k < kMinSample + 1; ++k) ck[k] = 0.0;
  for (int k = kMinSample + 1; k <= n; ++k) ck[k] = ck[k - 1] + lg(k) - lg(k - kMinSample);
  cn[0] = 0.0; cn[1] = lg(n);
  for (int k = 2; k <= n; ++k) cn[k] = cn[k - 1] + lg(n - k + 1) - lg(k);
}
// the largest cosine c with acos(c) * 180.0 / M_PI > 3 by THIS process's acos (bisection, then a monotonicity check over 4096 neighbouring doubles on
// either side, as turn_thresholds of pvlm_linegrow_core.h does for 1 degree).  *monotone = false when the libm is not monotone there: the callers refuse.
inline double angle_threshold(bool* monotone) {
  auto above = [](double c) { volatile double a = std::acos(c); return a * 180.0 / M_PI > 3; };
  double lo = 0.9, hi = 1.0;
  for (int it = 0; it < 200; ++it) {
    const double mid = lo + (hi - lo) / 2;
    if (mid <= lo || mid >= hi) break;
    if (above(mid)) lo = mid; else hi = mid;
  }
  double last_true = lo, first_false = hi, c = lo;
  for (int k = 0; k < 4096; ++k) c = std::nextafter(c, 0.0);
  for (int k = 0; k < 8192; ++k, c = std::nextafter(c, 2.0)) {
    if (above(c)) { if (c > last_true) last_true = c; }
    else if (c < first_false) first_false = c;
  }
  *monotone = first_false > last_true;
  return last_true;
}

}  // namespace pvlm_essential

#if !defined(__HIPCC__)
// ---- host loops: the serial chain, CheckRT over a pair, the selection over the runs ----
#include <algorithm>
#include <utility>
#include <vector>

namespace pvlm_essential {

struct Match { int query, train; float distance; };

// ComputeEssential on n correspondences (3 floats each)
inline void compute_essential(const float* p1, const float* p2, int n, double* E, double* sv = nullptr) {
  double ata[45], a[81], v[81];
  for (int e = 0; e < 45; ++e) {
    int r, c; ata_rc(e, &r, &c);
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + ata_term(p1 + 3 * i, p2 + 3 * i, r, c);
    ata[e] = s;
  }
  ata_expand(ata, a);
  jacobi_serial(a, v, 9);
  essential_from_eig9(a, v, E, sv);
}

struct ChainResult {
  double E[9]; double nfa; int iterations; std::vector<int> inliers;       // inliers in the order of the sorted residuals; empty without a model
  std::vector<std::pair<int, double>> betters;                               // (iteration, NFA) of every hypothesis that became the best (tests)
};
// FindEssentialACRANSAC on the n >= 9 matches m of frames (b1, b2)
inline void run_chain(const float* b1, const float* b2, const Match* m, int n, const double* tab, unsigned long long seed, int src, int tgt, int run,
                      int max_iterations, unsigned flags, ChainResult& out) {
  const ChainKey key = chain_key(seed, src, tgt, run);
  ChainState st = chain_begin(max_iterations);
  std::vector<int> set((size_t)n); for (int i = 0; i < n; ++i) set[(size_t)i] = i;
  int msize = n;
  double ata[45], a[81], v[81], E[9], bestE[9];
  for (int e = 0; e < 45; ++e) ata[e] = 0.0;
  for (int i = 0; i < 9; ++i) bestE[i] = 0.0;
  std::vector<std::pair<double, int>> sorted((size_t)n);
  out.betters.clear();
  while (chain_running(st)) {
    int pos[8];
    sample8(key, st.iter, msize, pos);
    if (flags & kFreshSample) for (int e = 0; e < 45; ++e) ata[e] = 0.0;
    for (int e = 0; e < 45; ++e) {
      int r, c; ata_rc(e, &r, &c);
      for (int s = 0; s < 8; ++s) { const Match& mm = m[set[(size_t)pos[s]]]; ata[e] = ata[e] + ata_term(b1 + 3 * (size_t)mm.query, b2 + 3 * (size_t)mm.train, r, c); }
    }
    ata_expand(ata, a);
    jacobi_serial(a, v, 9);
    essential_from_eig9(a, v, E, nullptr);
    for (int i = 0; i < n; ++i) sorted[(size_t)i] = {sort_key(residual(E, b1 + 3 * (size_t)m[i].query, b2 + 3 * (size_t)m[i].train)), i};
    std::sort(sorted.begin(), sorted.end());
    double best_nfa = inf_d(); int best_k = 0;
    for (int k = kMinSample + 1; k <= n && sorted[(size_t)k - 1].first < inf_d(); ++k) {
      const double x = nfa_value(tab, n, k, sorted[(size_t)k - 1].first);
      if (x < best_nfa) { best_nfa = x; best_k = k; }
    }
    bool better, swap;
    const int it = st.iter;
    chain_step(st, best_nfa, best_k, &better, &swap);
    if (better) { for (int i = 0; i < 9; ++i) bestE[i] = E[i]; out.betters.push_back({it, best_nfa}); }
    if (swap) { for (int i = 0; i < best_k; ++i) set[(size_t)i] = sorted[(size_t)i].second; msize = best_k; }
  }
  out.iterations = st.iter; out.nfa = st.minNFA;
  const bool model = chain_has_model(st);
  for (int i = 0; i < 9; ++i) out.E[i] = model ? bestE[i] : 0.0;
  out.inliers.assign(set.begin(), set.begin() + (model ? msize : 0));
}

struct RunPose { int candidate; int count; double R[9], t[3]; };      // candidate -1: the run is dropped
// DecomposeEssential + CheckRT x 4 + the selection inside the run, on the chain's inliers
inline RunPose run_pose(const float* b1, const float* b2, const Match* m, int n, const ChainResult& ch, double cos_reject, int triangulation_num_threshold) {
  RunPose rp; rp.candidate = -1; rp.count = 0;
  if (ch.inliers.empty()) return rp;
  std::vector<unsigned char> mask((size_t)n, 0);
  for (int i : ch.inliers) mask[(size_t)i] = 1;
  double R[36], t[12], P[3];
  decompose(ch.E, R, t);
  int num[4] = {0, 0, 0, 0};
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < n; ++i)
      if (mask[(size_t)i] && check_point(R + 9 * j, t + 3 * j, b1 + 3 * (size_t)m[i].query, b2 + 3 * (size_t)m[i].train, cos_reject, P)) ++num[j];
  rp.candidate = select_candidate(num, triangulation_num_threshold);
  if (rp.candidate >= 0) { rp.count = num[rp.candidate]; std::memcpy(rp.R, R + 9 * rp.candidate, sizeof rp.R); std::memcpy(rp.t, t + 3 * rp.candidate, sizeof rp.t); }
  return rp;
}

struct PairResult { unsigned char keep = 0; double R[9] = {0}, t[3] = {0}; std::vector<int> inlier_idx; std::vector<double> triangulated; long long hypotheses = 0; int chains = 0; };
// the loop body of FilterImagePairs for one pair
inline void filter_pair(const float* b1, const float* b2, const Match* m, int n, int src, int tgt, int n_runs, int max_iterations, int triangulation_num_threshold,
                        unsigned long long seed, unsigned flags, double cos_reject, PairResult& out) {
  out = PairResult();
  if (n <= kMinSample) return;
  std::vector<double> tab(2 + 2 * ((size_t)n + 1));
  nfa_tables(n, tab.data());
  ChainResult ch, best_ch; RunPose best; best.candidate = -1; best.count = -1;
  for (int run = 0; run < n_runs; ++run) {
    run_chain(b1, b2, m, n, tab.data(), seed, src, tgt, run, max_iterations, flags, ch);
    out.hypotheses += ch.iterations; out.chains += 1;
    const RunPose rp = run_pose(b1, b2, m, n, ch, cos_reject, triangulation_num_threshold);
    if (rp.candidate >= 0 && rp.count > best.count) { best = rp; best_ch = ch; }
  }
  if (best.candidate < 0) return;
  out.keep = 1; std::memcpy(out.R, best.R, sizeof out.R); std::memcpy(out.t, best.t, sizeof out.t);
  std::vector<unsigned char> mask((size_t)n, 0);
  for (int i : best_ch.inliers) mask[(size_t)i] = 1;
  double P[3];
  for (int i = 0; i < n; ++i)
    if (mask[(size_t)i] && check_point(best.R, best.t, b1 + 3 * (size_t)m[i].query, b2 + 3 * (size_t)m[i].train, cos_reject, P)) {
      out.inlier_idx.push_back(i); out.triangulated.insert(out.triangulated.end(), P, P + 3);
    }
}

}  // namespace pvlm_essential
#endif
