// Host-compiled check of K36: the definition of panovlm_amd/csrc/pvlm_relpose_core.h (one pair's two-view bundle adjustment) behind the host loop of
// panovlm_amd/host/pvlm_host_relpose.hpp.  tests/test_relpose_cpu.py compares it with the numpy twin of tests/relpose_ref.py without a GPU;
// tests/test_relpose_gpu.py compares pvlm_refine_relative_poses with it.  Built twice, with -ffp-contract=off and with -ffp-contract=fast: a scene is used only
// when both builds take the same accept / reject sequence.  With -DRELPOSE_CHECK_MAIN it is a stand-alone program (the sanitizer build: 0, 1, 65 and 300 points).
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_relpose.hpp"

struct Match { int query, train; float distance; };
using namespace pvlm::relpose_detail;

extern "C" {

int chk_relpose_lanes() { return pvlm_relpose::kLanes; }

// keypoints: the frames' rows one frame after the other (2 floats each).  summaries: n_pairs x {initial, final, successful, unsuccessful, termination} as 5 doubles.
// Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
int chk_relpose_refine(int n_frames, const int* rows_kp, const float* keypoints, const int* img_rows, const int* img_cols, int n_pairs, const int* src, const int* tgt,
                       const long long* match_offsets, const Match* matches, const long long* inlier_offsets, const int* inlier_idx, double* R, double* t, double* tri, int kind,
                       int max_num_iterations, int n_threads, unsigned char* ok, double* summaries, unsigned long long* accept_masks) {
  std::vector<const float*> ptr((size_t)n_frames);
  size_t at = 0;
  for (int f = 0; f < n_frames; ++f) { ptr[(size_t)f] = keypoints + 2 * at; at += (size_t)rows_kp[f]; }
  std::vector<pvlm_relpose::Summary> s((size_t)n_pairs);
  const int rc = pvlm::relpose_detail::RefinePosesHost(n_frames, ptr.data(), rows_kp, img_rows, img_cols, n_pairs, src, tgt, match_offsets, matches, inlier_offsets, inlier_idx,
                                                       R, t, tri, kind, max_num_iterations, (size_t)n_threads, ok, s.data(), accept_masks);
  if (rc) return rc;
  for (int p = 0; p < n_pairs; ++p) {
    double* o = summaries + 5 * (size_t)p;
    o[0] = s[(size_t)p].initial_cost; o[1] = s[(size_t)p].final_cost; o[2] = s[(size_t)p].successful_steps; o[3] = s[(size_t)p].unsuccessful_steps; o[4] = s[(size_t)p].termination;
  }
  return 0;
}

// SetTranslationScaleDepthMap for one pair.  d1 / d2: the two depth maps (rows 0 = none).  t (3) and tri (3 n) are scaled in place.  out3: points_with_depth, upper_scale,
// lower_scale.  Returns 1 when the pair got a scale.
int chk_relpose_scale(int eq_rows, int eq_cols, int rows1, const uint16_t* d1, int d1_rows, int d1_cols, const uint16_t* d2, int d2_rows, int d2_cols, const double* R, double* t,
                      double* tri, int n, double* out3) {
  TailPair p;
  std::memcpy(p.R, R, sizeof p.R); std::memcpy(p.t, t, sizeof p.t); p.tri.assign(tri, tri + 3 * (size_t)n);
  DepthView a, b;
  a.data = d1; a.rows = d1_rows; a.cols = d1_cols; b.data = d2; b.rows = d2_rows; b.cols = d2_cols;
  const bool ok = SetScaleOne(eq_rows, eq_cols, rows1, a, b, p);
  std::memcpy(t, p.t, sizeof p.t);
  for (size_t i = 0; i < 3 * (size_t)n; ++i) tri[i] = p.tri[i];
  out3[0] = p.points_with_depth; out3[1] = p.upper_scale; out3[2] = p.lower_scale;
  return ok ? 1 : 0;
}

// LargestBiconnectedGraph on a pair list: keep[p] = 1 for the surviving pairs, nodes (capacity 2 n_pairs) the surviving frames ascending.  Returns the node count.
int chk_relpose_graph(int n_pairs, const long long* first, const long long* second, unsigned char* keep, long long* nodes) {
  std::vector<TailPair> pairs((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) { pairs[(size_t)p].image_pair = {(size_t)first[p], (size_t)second[p]}; pairs[(size_t)p].tag = (size_t)p; keep[p] = 0; }
  std::set<size_t> covered;
  for (const TailPair& p : LargestBiconnected(pairs, covered)) keep[p.tag] = 1;
  int k = 0;
  for (size_t v : covered) nodes[k++] = (long long)v;
  return k;
}

// the final sort with upstream's comparator as written: order[k] = the input index of the k-th pair
void chk_relpose_sort(int n, const long long* first, const long long* second, int* order) {
  std::vector<int> v((size_t)n);
  for (int i = 0; i < n; ++i) v[(size_t)i] = i;
  SortAsWritten(v, [&](int a, int b) { return PairLessAsWritten({(size_t)first[a], (size_t)second[a]}, {(size_t)first[b], (size_t)second[b]}); });
  for (int i = 0; i < n; ++i) order[i] = v[(size_t)i];
}

}  // extern "C"

#ifdef RELPOSE_CHECK_MAIN
#include <cmath>
// a two-view scene of n points seen in a 720 x 1440 panorama, camera 2 started a little off; prints the costs and the step counts
static int scene(int n, int kind) {
  const int rows = 720, cols = 1440;
  const double kPi = 3.14159265358979323846;
  std::vector<float> k1((size_t)2 * n + 2), k2((size_t)2 * n + 2);
  std::vector<Match> m((size_t)n + 1);
  std::vector<int> idx((size_t)n + 1);
  std::vector<double> tri((size_t)3 * n + 3);
  uint32_t s = 777u + (uint32_t)n;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; };
  const double ang = 0.2, c = std::cos(ang), sn = std::sin(ang), tt[3] = {1.0, 0.1, 0.05};
  auto px = [&](const double* p, float* o) {
    const double lon = std::atan2(p[0], p[2]), lat = -std::asin(p[1] / std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
    o[0] = (float)(cols * (0.5 + lon / (2 * kPi))); o[1] = (float)(rows * (0.5 - lat / kPi));
  };
  for (int i = 0; i < n; ++i) {
    const double X[3] = {8 * rnd() - 4, 8 * rnd() - 4, 2 + 4 * rnd()};
    const double Y[3] = {c * X[0] - sn * X[1] + tt[0], sn * X[0] + c * X[1] + tt[1], X[2] + tt[2]};
    px(X, &k1[(size_t)2 * i]); px(Y, &k2[(size_t)2 * i]);
    m[(size_t)i] = Match{i, i, 0.0f}; idx[(size_t)i] = i;
    for (int k = 0; k < 3; ++k) tri[(size_t)3 * i + k] = X[k] * (1.0 + 0.01 * (rnd() - 0.5));
  }
  const double a2 = ang + 0.01, c2 = std::cos(a2), s2 = std::sin(a2);
  double R[9] = {c2, -s2, 0, s2, c2, 0, 0, 0, 1}, t[3] = {1.0, 0.13, 0.02};
  const int rk[2] = {n, n}, ir[2] = {rows, rows}, ic[2] = {cols, cols}, src = 0, tgt = 1;
  const float* ptr[2] = {k1.data(), k2.data()};
  const long long off[2] = {0, n};
  unsigned char ok = 9; pvlm_relpose::Summary sum; unsigned long long mask = 0;
  const int rc = pvlm::relpose_detail::RefinePosesHost(2, ptr, rk, ir, ic, 1, &src, &tgt, off, m.data(), off, idx.data(), R, t, tri.data(), kind, 50, 2, &ok, &sum, &mask);
  std::printf("n = %d kind %d: rc %d ok %d cost %.6e -> %.6e steps %d + %d termination %d\n", n, kind, rc, (int)ok, sum.initial_cost, sum.final_cost, sum.successful_steps,
              sum.unsuccessful_steps, sum.termination);
  return rc || !(sum.final_cost <= sum.initial_cost);
}
int main() {
  int rc = 0;
  for (int kind = 1; kind <= 2; ++kind) { rc |= scene(0, kind); rc |= scene(1, kind); rc |= scene(65, kind); rc |= scene(300, kind); }
  return rc;
}
#endif
