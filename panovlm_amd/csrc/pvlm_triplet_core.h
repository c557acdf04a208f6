// K48: the definition of the pair graph's triplets (PoseGraph::FindTriplet, sfm/PoseGraph.cpp:195-226) and of the triplet test of SfM::FilterByTriplet
// (sfm/SfM.cpp:705-778) — host and device.  Compiled for the device by pvlm_triplet.hip and for the host by tests/cpp/triplet_core_check.cpp and the host mirror
// (host/pvlm_host_sfm.cpp); find_host / filter_host below do with loops what the kernels do with lanes.
//
// Input: F cameras, P pairs (first, second) with first < second < F, no pair named twice, in any list order.
//   rank     the position of a pair in ascending order of the 64-bit key first * F + second;
//   forward row of camera v: its partners w > v, ascending.  With the pairs in rank order this is a CSR over the sorted list (row_off[F + 1], nbr[P] = second by rank),
//            and a row position IS a pair rank; idx[rank] is the caller's list index of that pair;
//   triplets all (i, j, k), i < j < k, whose three pairs are in the list, in lexicographic order.  Under the conditions above this is upstream's order: its walk over
//            the std::set of edges emits a triangle at its smallest edge (i, j), and every edge that could bring a third node below j has left the adjacency by
//            then.  A triangle is found at pair (i, j) by taking the part of row i behind j (the candidates k, ascending) and looking each one up in row j by binary
//            search; its position is the pair's base (the exclusive scan of the per-pair counts in rank order, 64-bit) plus its rank among that pair's hits;
//   triplet_pairs  the caller's list indices of (i, j), (j, k), (i, k): K47's layout.
// The loop measure of a triplet is upstream's as written (:739-742): c = trace((R_31^T R_32) R_21) / 3 with the operation order of pvlm_rotavg_core.h's mul_tn and
// mul_nn, clamped by min(1.0, max(c, -1.0)); the triplet is kept when acos(c) * 180 / M_PI < angle_threshold; a pair is kept when it lies in a kept triplet.
//
// The device decides against cut = cos(angle_threshold * pi / 180), computed once on the host: clamp(c) > cut keeps.  acos is decreasing, so this is the literal
// test everywhere but next to the cut, and there the device does not decide: a triplet with |clamp(c) - cut| <= kBand goes to an uncertain list, which the host
// decides with the literal std::acos chain.  kBand = 1e-12, absolute in c, is derived, not tuned:
//   - the literal decision flips within one ulp of cut (walked on the CPU at 0.1 and 5 degrees over +-2000 doubles around the cut: one flip, monotone); cut itself
//     carries the rounding of the degree-to-radian product and of cos, below 2e-16 absolute for any threshold;
//   - the 27-product trace differs between a host and a device evaluation by rounding of order 1e-15 at most (none at all when neither contracts);
//   - 1e-12 leaves three orders of margin above that, and at 0.1 degrees (1 - cut = 1.5e-6) the band is a 3e-7 part of the distance to c = 1.
// A threshold <= 0 keeps nothing (acos >= 0) and one above 180 keeps everything (acos * 180 / M_PI <= 180): cut_for gives them cuts that no clamped c comes near.
// A c that is not finite goes where the written clamp sends it: NaN and +inf to 1.0 (kept under any positive threshold), -inf to -1.0.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "pvlm_rotavg_core.h"

#if defined(__HIPCC__)
#define PVLM_TR_HD __host__ __device__ __forceinline__
#else
#define PVLM_TR_HD inline
#endif

namespace pvlm_triplet {

constexpr int kGroup = 16;                 // lanes that share one pair's candidates (pvlm_triplet_group_size)
constexpr double kBand = 1e-12;            // see above
constexpr int kSearchSteps = 32;           // a binary search over a row of fewer than 2^31 entries ends within 31 halvings
enum { kDrop = 0, kKeep = 1, kUncertain = 2 };

struct Stats { long long n_triplets, n_kept_triplets, n_uncertain, n_kept_pairs; };     // == pvlm_triplet_stats

// the position of k in the ascending nbr[lo .. hi), or -1
PVLM_TR_HD int find_in_row(const int* nbr, int lo, int hi, int k) {
  for (int s = 0; s < kSearchSteps && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1), v = nbr[mid];
    if (v == k) return mid;
    if (v < k) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// std::min(1.0, std::max(c, -1.0)) spelled out, so that host and device send a NaN the same way (to 1.0)
PVLM_TR_HD double clamp_cos(double c) {
  const double m = c < -1.0 ? -1.0 : c;
  return m < 1.0 ? m : 1.0;
}

// trace((R_31^T R_32) R_21) / 3, row-major 3 x 3
PVLM_TR_HD double loop_cos(const double* R_21, const double* R_32, const double* R_31) {
  double a[9], rot[9];
  pvlm_rotavg::mul_tn(R_31, R_32, a);
  pvlm_rotavg::mul_nn(a, R_21, rot);
  return (rot[0] + rot[4] + rot[8]) / 3.0;
}

PVLM_TR_HD int classify(double c, double cut) {
  const double cc = clamp_cos(c), d = cc - cut;
  if ((d < 0 ? -d : d) > kBand) return cc > cut ? kKeep : kDrop;
  return kUncertain;
}

// the literal test (host only: the uncertain list and the references)
inline bool keep_literal(double c, double angle_threshold) {
  const double cos_theta = std::min(1.0, std::max(c, -1.0));
  return std::acos(cos_theta) * 180.0 / M_PI < angle_threshold;
}

inline double cut_for(double angle_threshold) {
  if (!(angle_threshold > 0.0)) return 2.0;
  if (angle_threshold > 180.0) return -2.0;
  return std::cos(angle_threshold * M_PI / 180.0);
}

// what every entry refuses before it writes anything; null: the arguments are fine so far (a repeated pair is found by Rows::build)
inline const char* check_args(int F, int P, const int* first, const int* second) {
  if (F < 0 || P < 0) return "a negative size";
  if (P > (1 << 30)) return "more than 2^30 pairs";          // a row position plus a round's lanes stays an int
  if (P > 0 && (!first || !second)) return "null argument";
  for (int p = 0; p < P; ++p) {
    if (first[p] < 0 || second[p] < 0 || first[p] >= F || second[p] >= F) return "a camera index out of range";
    if (first[p] >= second[p]) return "a pair with first >= second";
  }
  return nullptr;
}

// rank and rows
struct Rows {
  int F = 0, P = 0, max_row = 0;
  std::vector<int> row_off, first_r, nbr, idx;     // F + 1 | P: first by rank | P: second by rank | P: rank -> caller's index
  // false: a pair named twice
  bool build(int F_, int P_, const int* first, const int* second) {
    F = F_; P = P_; max_row = 0;
    std::vector<std::pair<uint64_t, int>> keys((size_t)P);
    for (int p = 0; p < P; ++p) keys[(size_t)p] = {(uint64_t)first[p] * (uint64_t)F + (uint64_t)second[p], p};
    std::sort(keys.begin(), keys.end());
    for (int r = 1; r < P; ++r) if (keys[(size_t)r].first == keys[(size_t)r - 1].first) return false;
    row_off.assign((size_t)F + 1, 0); first_r.resize((size_t)P); nbr.resize((size_t)P); idx.resize((size_t)P);
    for (int r = 0; r < P; ++r) {
      const int p = keys[(size_t)r].second;
      idx[(size_t)r] = p; first_r[(size_t)r] = first[p]; nbr[(size_t)r] = second[p];
      ++row_off[(size_t)first[p] + 1];
    }
    for (int v = 0; v < F; ++v) { max_row = std::max(max_row, row_off[(size_t)v + 1]); row_off[(size_t)v + 1] += row_off[(size_t)v]; }
    return true;
  }
  // the rounds a group needs for the longest row: the launch-time bound of the kernels' candidate loop
  int max_rounds() const { return (max_row + kGroup - 1) / kGroup; }
};

// ---- the host compile: the kernels' work by loops ---------------------------------------------------------------------------------------------------------------
// visit(r, q, s, i, j, k): the triangle (i, j, k) found at pair rank r, with (j, k) at rank q and (i, k) at rank s, in lexicographic order
template <class Visit> inline void for_each_triplet(const Rows& g, Visit visit) {
  for (int r = 0; r < g.P; ++r) {
    const int i = g.first_r[(size_t)r], j = g.nbr[(size_t)r];
    for (int s = r + 1; s < g.row_off[(size_t)i + 1]; ++s) {
      const int k = g.nbr[(size_t)s], q = find_in_row(g.nbr.data(), g.row_off[(size_t)j], g.row_off[(size_t)j + 1], k);
      if (q >= 0) visit(r, q, s, i, j, k);
    }
  }
}

// pvlm_triplets_find on the host.  0; -1 (PVLM_ERR_ARG) with nothing written; -5 (PVLM_ERR_CAPACITY) with *needed and pair_counts set and nothing past capacity
// written.  capacity counts only when triplets or triplet_pairs is wanted.
inline int find_host(int F, int P, const int* first, const int* second, int* triplets, int* triplet_pairs, long long capacity, long long* needed, long long* pair_counts) {
  if (!needed || capacity < 0 || check_args(F, P, first, second)) return -1;
  Rows g;
  if (!g.build(F, P, first, second)) return -1;
  for (int p = 0; p < P && pair_counts; ++p) pair_counts[p] = 0;
  long long n = 0;
  for_each_triplet(g, [&](int r, int q, int s, int i, int j, int k) {
    if (n < capacity) {
      if (triplets) { triplets[3 * n] = i; triplets[3 * n + 1] = j; triplets[3 * n + 2] = k; }
      if (triplet_pairs) { triplet_pairs[3 * n] = g.idx[(size_t)r]; triplet_pairs[3 * n + 1] = g.idx[(size_t)q]; triplet_pairs[3 * n + 2] = g.idx[(size_t)s]; }
    }
    if (pair_counts) ++pair_counts[g.idx[(size_t)r]];
    ++n;
  });
  *needed = n;
  return (triplets || triplet_pairs) && n > capacity ? -5 : 0;
}

// one uncertain triplet decided by the literal chain: its pairs' keep bytes and the count
inline void decide_uncertain(const int* pairs3, const double* R_21, double angle_threshold, unsigned char* keep, long long* n_kept) {
  const double c = loop_cos(R_21 + 9 * (size_t)pairs3[0], R_21 + 9 * (size_t)pairs3[1], R_21 + 9 * (size_t)pairs3[2]);
  if (keep_literal(c, angle_threshold)) { keep[pairs3[0]] = keep[pairs3[1]] = keep[pairs3[2]] = 1; ++*n_kept; }
}

// pvlm_triplets_filter on the host, the uncertain list included.  0, or -1 (PVLM_ERR_ARG) with nothing written
inline int filter_host(int F, int P, const int* first, const int* second, const double* R_21, double angle_threshold, unsigned char* keep, Stats* stats) {
  if (!stats || !std::isfinite(angle_threshold) || (P > 0 && (!R_21 || !keep)) || check_args(F, P, first, second)) return -1;
  Rows g;
  if (!g.build(F, P, first, second)) return -1;
  const double cut = cut_for(angle_threshold);
  Stats st{0, 0, 0, 0};
  std::vector<int> uncertain;
  for (int p = 0; p < P; ++p) keep[p] = 0;
  for_each_triplet(g, [&](int r, int q, int s, int, int, int) {
    const int a = g.idx[(size_t)r], b = g.idx[(size_t)q], c3 = g.idx[(size_t)s];
    const int verdict = classify(loop_cos(R_21 + 9 * (size_t)a, R_21 + 9 * (size_t)b, R_21 + 9 * (size_t)c3), cut);
    ++st.n_triplets;
    if (verdict == kKeep) { keep[a] = keep[b] = keep[c3] = 1; ++st.n_kept_triplets; }
    else if (verdict == kUncertain) { uncertain.push_back(a); uncertain.push_back(b); uncertain.push_back(c3); }
  });
  st.n_uncertain = (long long)(uncertain.size() / 3);
  for (size_t u = 0; u < uncertain.size(); u += 3) decide_uncertain(&uncertain[u], R_21, angle_threshold, keep, &st.n_kept_triplets);
  for (int p = 0; p < P; ++p) st.n_kept_pairs += keep[p];
  *stats = st;
  return 0;
}

}  // namespace pvlm_triplet
