// pvlm_host_relpose.hpp — K36 on the host: SfM::RefineRelativePose (sfm/SfM.cpp:482-485, SfMLocalBA util/Optimization.cpp:84-170) over a pair list, on the host
// compile of csrc/pvlm_relpose_core.h (the lanes of a pair taken one after the other, the same sums in the same order), the pairs spread over the worker pool.
// It serves pvlm::SfMLocalBA / RefineRelativePosesHost (the baseline tools/relpose_bench.py times and the equality partner of pvlm_refine_relative_poses) and the
// tests' reference (tests/cpp/relpose_core_check.cpp).  Behind it the host tail of SfM::FilterImagePairs (sfm/SfM.cpp:449-476) on plain arrays:
// SetTranslationScaleDepthMap (:487-679), LargestBiconnectedGraph (:780-799 with sfm/PoseGraph.cpp:63-133, no lemon) and the final sort.  Not installed; not part of
// the interface.
#pragma once
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <map>
#include <set>
#include <utility>
#include <vector>

#ifndef PVLM_HD
#define PVLM_HD
#endif
#include "../csrc/pvlm_relpose_core.h"
#include "../csrc/pvlm_workers.h"

namespace pvlm {
namespace relpose_detail {

// -1 (PVLM_ERR_ARG) for what pvlm_refine_relative_poses refuses.  MatchT: { int query, train; float distance; }
template <class MatchT>
inline int CheckArgs(int n_frames, const float* const* keypoints, const int* rows_kp, const int* img_rows, const int* img_cols, int n_pairs, const int* src, const int* tgt,
                     const long long* moff, const MatchT* m, const long long* ioff, const int* idx, const double* R, const double* t, const double* tri, int kind,
                     int max_num_iterations) {
  if ((kind != pvlm_relpose::kKindPixel && kind != pvlm_relpose::kKindAngle2) || max_num_iterations < 0 || n_frames < 0 || n_pairs < 0) return -1;
  if (n_pairs == 0) return 0;
  if (moff[0] != 0 || ioff[0] != 0) return -1;
  for (int p = 0; p < n_pairs; ++p) {
    if (src[p] < 0 || src[p] >= n_frames || tgt[p] < 0 || tgt[p] >= n_frames || moff[p + 1] < moff[p] || ioff[p + 1] < ioff[p]) return -1;
    const int f1 = src[p], f2 = tgt[p];
    if (ioff[p + 1] > ioff[p] && (img_rows[f1] <= 0 || img_cols[f1] <= 0 || img_rows[f2] <= 0 || img_cols[f2] <= 0 || !keypoints[f1] || !keypoints[f2])) return -1;
    for (long long i = ioff[p]; i < ioff[p + 1]; ++i) {
      if (idx[i] < 0 || idx[i] >= moff[p + 1] - moff[p]) return -1;
      const MatchT& r = m[moff[p] + idx[i]];
      if (r.query < 0 || r.query >= rows_kp[f1] || r.train < 0 || r.train >= rows_kp[f2]) return -1;
      for (int k = 0; k < 2; ++k)
        if (!std::isfinite(keypoints[f1][2 * (size_t)r.query + k]) || !std::isfinite(keypoints[f2][2 * (size_t)r.train + k])) return -1;
      for (int k = 0; k < 3; ++k) if (!std::isfinite(tri[3 * (size_t)i + k])) return -1;
    }
    for (int k = 0; k < 9; ++k) if (!std::isfinite(R[9 * (size_t)p + k])) return -1;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(t[3 * (size_t)p + k])) return -1;
  }
  return 0;
}

// one pair on the calling thread
template <class MatchT>
inline void RefineOne(const float* kp1, const float* kp2, int rows1, int cols1, int rows2, int cols2, const MatchT* m, const int* idx, int n, int kind, int max_num_iterations,
                      double* R, double* t, double* tri, unsigned char* ok, pvlm_relpose::Summary* sum, unsigned long long* accept_mask) {
  std::vector<double> obs(4 * (size_t)n), scr((size_t)pvlm_relpose::kScratchPerPoint * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const MatchT& r = m[idx[i]];
    pvlm_relpose::make_obs(kind, kp1[2 * (size_t)r.query], kp1[2 * (size_t)r.query + 1], rows1, cols1, &obs[4 * (size_t)i]);
    pvlm_relpose::make_obs(kind, kp2[2 * (size_t)r.train], kp2[2 * (size_t)r.train + 1], rows2, cols2, &obs[4 * (size_t)i + 2]);
  }
  pvlm_relpose::Pair P;
  P.n = n; P.kind = kind; P.rows1 = rows1; P.cols1 = cols1; P.rows2 = rows2; P.cols2 = cols2; P.obs = obs.data(); P.scr = scr.data();
  pvlm_relpose::Options opt;
  opt.max_num_iterations = max_num_iterations;
  pvlm_relpose::HostTeam team;
  pvlm_relpose::refine_pair(team, P, opt, R, t, tri, ok, sum, accept_mask);
}

// the host loop over a pair list: the arrays of pvlm_refine_relative_poses.  summaries, accept_masks: n_pairs or null.  Returns 0 or -1 with nothing written.
template <class MatchT>
inline int RefinePosesHost(int n_frames, const float* const* keypoints, const int* rows_kp, const int* img_rows, const int* img_cols, int n_pairs, const int* src, const int* tgt,
                           const long long* moff, const MatchT* m, const long long* ioff, const int* idx, double* R, double* t, double* tri, int kind, int max_num_iterations,
                           size_t n_threads, unsigned char* ok, pvlm_relpose::Summary* summaries, unsigned long long* accept_masks) {
  if (CheckArgs(n_frames, keypoints, rows_kp, img_rows, img_cols, n_pairs, src, tgt, moff, m, ioff, idx, R, t, tri, kind, max_num_iterations)) return -1;
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min(n_threads, (size_t)std::max(n_pairs, 1))), [&]() {
    for (int p = next++; p < n_pairs; p = next++) {
      const int f1 = src[p], f2 = tgt[p];
      pvlm_relpose::Summary s;
      RefineOne(keypoints[f1], keypoints[f2], img_rows[f1], img_cols[f1], img_rows[f2], img_cols[f2], m + moff[p], idx + ioff[p], (int)(ioff[p + 1] - ioff[p]), kind,
                max_num_iterations, R + 9 * (size_t)p, t + 3 * (size_t)p, tri + 3 * (size_t)ioff[p], ok + p, &s, accept_masks ? accept_masks + p : nullptr);
      if (summaries) summaries[p] = s;
    }
  });
  return 0;
}

// ================================================================================================
// the host tail of SfM::FilterImagePairs: scale from the depth maps, the pair graph, the final order
// ================================================================================================
struct DepthView { const uint16_t* data = nullptr; int rows = 0, cols = 0; bool empty() const { return !data || rows <= 0 || cols <= 0; } };

struct TailPair {
  std::pair<size_t, size_t> image_pair;
  double R[9], t[3];
  std::vector<double> tri;                      // 3 per point
  int points_with_depth = 0;
  double upper_scale = -1, lower_scale = -1;    // util/MatchPair.h's constructors
  size_t tag = 0;                               // the caller's index of the pair
};

// FastAtan2 (base/Math.h:15-29) and Equirectangular::CamToImage on doubles, as host/pvlm_host_internal.hpp restates them
inline double FastAtan2d(double y, double x) {
  const double ax = std::fabs(x), ay = std::fabs(y);
  const double a = std::min(ax, ay) / (std::max(ax, ay) + DBL_EPSILON);
  const double s = a * a;
  double r = ((-0.04432655554792128 * s + 0.1555786518463281) * s - 0.3258083974640975) * s * a + 0.9997878412794807 * a;
  if (ay > ax) r = 1.57079632679489661923 - r;
  if (x < 0) r = 3.14159265358979323846 - r;
  if (y < 0) r = -r;
  return r;
}
inline void CamToImaged(int rows, int cols, const double* cam, double* px) {
  const double lon = FastAtan2d(cam[0], cam[2]);
  const double lat = -FastAtan2d(cam[1], std::sqrt(cam[0] * cam[0] + cam[2] * cam[2]));
  px[0] = cols * (0.5 + lon / (2.0 * 3.14159265358979323846));
  px[1] = rows * (0.5 - lat / 3.14159265358979323846);
}

// SfM::SetTranslationScaleDepthMap(eq, pair) (:487-603), operation by operation.  eq_rows / eq_cols: frames[0]'s image size (upstream's one Equirectangular for all
// frames); rows1: the image rows of the pair's first frame (the half-size test).  Deliberate divergence: a rounded pixel that lies inside the image but outside the
// depth map it indexes (maps of two different sizes in one pair) skips the point; upstream reads out of bounds there.
inline bool SetScaleOne(int eq_rows, int eq_cols, int rows1, const DepthView& d1, const DepthView& d2, TailPair& pair) {
  if (d1.empty() || d2.empty()) return false;
  const bool half_size = d1.rows == (int)((rows1 + 1) / 2);
  pair.points_with_depth = 0;
  std::vector<double> scale;
  const size_t n = pair.tri.size() / 3;
  auto inside = [&](int col, int row) { return col >= 0 && row >= 0 && col + 1 <= eq_cols && row + 1 <= eq_rows; };   // Equirectangular::IsInside(cv::Point2i)
  for (size_t i = 0; i < n; ++i) {
    const double* p = pair.tri.data() + 3 * i;
    double px[2];
    CamToImaged(eq_rows, eq_cols, p, px);
    px[0] = px[0] / (1.0 + half_size); px[1] = px[1] / (1.0 + half_size);
    int row = (int)std::round(px[1]), col = (int)std::round(px[0]);
    if (!inside(col, row)) continue;
    if (row >= d1.rows || col >= d1.cols) continue;
    const double depth1 = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const float depth1_real = (float)(d1.data[(size_t)row * (size_t)d1.cols + (size_t)col] / 256.0);
    if (depth1_real <= 0) continue;
    const double scale1 = depth1_real / depth1;
    double q[3];
    for (int r = 0; r < 3; ++r) q[r] = (pair.R[3 * r] * p[0] + pair.R[3 * r + 1] * p[1] + pair.R[3 * r + 2] * p[2]) + pair.t[r];
    CamToImaged(eq_rows, eq_cols, q, px);
    px[0] = px[0] / (1.0 + half_size); px[1] = px[1] / (1.0 + half_size);
    row = (int)std::round(px[1]); col = (int)std::round(px[0]);
    if (!inside(col, row)) continue;
    if (row >= d2.rows || col >= d2.cols) continue;
    const double depth2 = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const float depth2_real = (float)(d2.data[(size_t)row * (size_t)d2.cols + (size_t)col] / 256.0);
    if (depth2_real <= 0) continue;
    const double scale2 = depth2_real / depth2;
    if (std::fabs(scale1 - scale2) / std::min(scale1, scale2) > 0.2) continue;
    scale.push_back(scale1); scale.push_back(scale2);
  }
  if (scale.size() < 10) return false;
  bool scale_is_good = true;
  std::vector<double> scale_preserve(scale);
  const size_t num_bins = 10;
  for (size_t iter = 0; iter < 2; iter++) {
    const size_t num_scale = scale.size();
    if (num_scale < 10) { scale_is_good = false; break; }
    const double max_scale = *std::max_element(scale.begin(), scale.end());
    const double min_scale = *std::min_element(scale.begin(), scale.end());
    if (max_scale / min_scale < 1.2) break;
    const double interval = (max_scale - min_scale) / num_bins;
    std::vector<std::vector<double>> histo(num_bins);
    for (const double& s : scale) {
      int bin_idx = (int)((s - min_scale - 1e-8) / interval);
      bin_idx = std::min(bin_idx, (int)(num_bins - 1));
      bin_idx = std::max(0, bin_idx);
      histo[(size_t)bin_idx].push_back(s);
    }
    scale.clear();
    for (const std::vector<double>& bin : histo)
      if (bin.size() > 0.1 * num_scale) scale.insert(scale.end(), bin.begin(), bin.end());
  }
  double final_scale = 0;
  if (scale_is_good) {
    for (const double& s : scale) final_scale += s;
    final_scale /= scale.size();
    pair.points_with_depth = (int)(scale.size() / 2);
    pair.upper_scale = *std::max_element(scale.begin(), scale.end());
    pair.lower_scale = *std::min_element(scale.begin(), scale.end());
  } else {
    std::nth_element(scale_preserve.begin(), scale_preserve.begin() + (std::ptrdiff_t)(scale_preserve.size() / 2), scale_preserve.end());
    final_scale = scale_preserve[scale_preserve.size() / 2];
    pair.upper_scale = 0; pair.lower_scale = 0;
    pair.points_with_depth = (int)(scale_preserve.size() / 2);
  }
  for (int k = 0; k < 3; ++k) pair.t[k] *= final_scale;
  for (double& v : pair.tri) v *= final_scale;
  return true;
}

// SfM::SetTranslationScaleDepthMap(keep_no_scale) (:605-679) without the file reads: the frames are visited from the one with the fewest pairs on, round the list;
// at each frame the still unprocessed pairs that touch it are taken in list order (what one thread gives upstream) and appended to the result when they got a scale
// or keep_no_scale is set.  frame_rows: the image rows of every frame.
inline bool SetScaleList(int eq_rows, int eq_cols, const std::vector<int>& frame_rows, const std::vector<DepthView>& depth, std::vector<TailPair>& pairs, bool keep_no_scale) {
  const size_t nf = frame_rows.size();
  std::vector<size_t> ref_count(nf, 0);
  for (const TailPair& p : pairs) { ref_count[p.image_pair.first]++; ref_count[p.image_pair.second]++; }
  const size_t start = nf ? (size_t)(std::min_element(ref_count.begin(), ref_count.end()) - ref_count.begin()) : 0;
  std::vector<size_t> order;
  for (size_t i = start; i < nf; ++i) order.push_back(i);
  for (size_t i = 0; i < start; ++i) order.push_back(i);
  std::vector<TailPair> good;
  std::set<std::pair<size_t, size_t>> processed;
  for (size_t idx1 : order)
    for (TailPair& p : pairs) {
      if (processed.count(p.image_pair) > 0) continue;
      if (p.image_pair.first != idx1 && p.image_pair.second != idx1) continue;
      const bool valid = SetScaleOne(eq_rows, eq_cols, frame_rows[p.image_pair.first], depth[p.image_pair.first], depth[p.image_pair.second], p) || keep_no_scale;
      processed.insert(p.image_pair);
      if (valid) good.push_back(p);
    }
  good.swap(pairs);
  return pairs.size() > 0;
}

// SetScaleList's visiting order with the per-pair step as a parameter: step(pair) -> scaled.  What the resident route runs with the results of ONE
// pvlm_set_translation_scales call in place of SetScaleOne (host/pvlm_host_sfm.cpp).
template <class Step>
inline bool SetScaleListWith(size_t n_frames, std::vector<TailPair>& pairs, bool keep_no_scale, Step&& step) {
  const size_t nf = n_frames;
  std::vector<size_t> ref_count(nf, 0);
  for (const TailPair& p : pairs) { ref_count[p.image_pair.first]++; ref_count[p.image_pair.second]++; }
  const size_t start = nf ? (size_t)(std::min_element(ref_count.begin(), ref_count.end()) - ref_count.begin()) : 0;
  std::vector<size_t> order;
  for (size_t i = start; i < nf; ++i) order.push_back(i);
  for (size_t i = 0; i < start; ++i) order.push_back(i);
  std::vector<TailPair> good;
  std::set<std::pair<size_t, size_t>> processed;
  for (size_t idx1 : order)
    for (TailPair& p : pairs) {
      if (processed.count(p.image_pair) > 0) continue;
      if (p.image_pair.first != idx1 && p.image_pair.second != idx1) continue;
      const bool valid = step(p) || keep_no_scale;
      processed.insert(p.image_pair);
      if (valid) good.push_back(p);
    }
  good.swap(pairs);
  return pairs.size() > 0;
}

// PoseGraph::KeepLargestEdgeBiconnected (sfm/PoseGraph.cpp:63-133) without lemon: the distinct (first, second) pairs are the edges (as SfM::LargestBiconnectedGraph
// builds its std::set; (a, b) and (b, a) are two parallel edges), the bridges are found by one depth-first search and removed, and of the connected components that
// remain (single nodes included) the one with the most nodes is returned.  Deliberate divergence: among components of equal size the one that holds the lowest frame
// id wins (upstream: the lowest component number lemon hands out).
inline std::set<size_t> LargestEdgeBiconnected(const std::vector<std::pair<size_t, size_t>>& pair_list) {
  const std::set<std::pair<size_t, size_t>> edge_set(pair_list.begin(), pair_list.end());
  const std::vector<std::pair<size_t, size_t>> edges(edge_set.begin(), edge_set.end());
  std::map<size_t, int> id_of;
  std::vector<size_t> frame_of;
  for (const auto& e : edges) { id_of.emplace(e.first, 0); id_of.emplace(e.second, 0); }
  for (auto& kv : id_of) { kv.second = (int)frame_of.size(); frame_of.push_back(kv.first); }     // nodes in ascending frame id
  const int nv = (int)frame_of.size();
  if (nv == 0) return {};
  std::vector<std::vector<std::pair<int, int>>> adj((size_t)nv);          // (neighbour, edge)
  for (size_t k = 0; k < edges.size(); ++k) {
    const int a = id_of[edges[k].first], b = id_of[edges[k].second];
    adj[(size_t)a].push_back({b, (int)k});
    if (a != b) adj[(size_t)b].push_back({a, (int)k});
  }
  std::vector<int> disc((size_t)nv, -1), low((size_t)nv, 0);
  std::vector<char> bridge(edges.size(), 0);
  int clock = 0;
  struct Item { int v, parent_edge; size_t next; };
  for (int root = 0; root < nv; ++root) {
    if (disc[(size_t)root] >= 0) continue;
    std::vector<Item> stack{{root, -1, 0}};
    disc[(size_t)root] = low[(size_t)root] = clock++;
    while (!stack.empty()) {
      Item& it = stack.back();
      if (it.next < adj[(size_t)it.v].size()) {
        const std::pair<int, int> e = adj[(size_t)it.v][it.next++];
        if (e.second == it.parent_edge) continue;
        if (disc[(size_t)e.first] >= 0) low[(size_t)it.v] = std::min(low[(size_t)it.v], disc[(size_t)e.first]);
        else { disc[(size_t)e.first] = low[(size_t)e.first] = clock++; stack.push_back({e.first, e.second, 0}); }
      } else {
        const Item done = it;
        stack.pop_back();
        if (!stack.empty()) {
          Item& up = stack.back();
          low[(size_t)up.v] = std::min(low[(size_t)up.v], low[(size_t)done.v]);
          if (low[(size_t)done.v] > disc[(size_t)up.v]) bridge[(size_t)done.parent_edge] = 1;
        }
      }
    }
  }
  std::vector<int> comp((size_t)nv, -1);
  std::vector<std::vector<int>> members;
  for (int s = 0; s < nv; ++s) {                                           // ascending frame id: component c holds the lowest id not in components 0 .. c - 1
    if (comp[(size_t)s] >= 0) continue;
    const int c = (int)members.size();
    members.push_back({});
    std::vector<int> todo{s};
    comp[(size_t)s] = c;
    while (!todo.empty()) {
      const int v = todo.back(); todo.pop_back();
      members[(size_t)c].push_back(v);
      for (const auto& e : adj[(size_t)v]) if (!bridge[(size_t)e.second] && comp[(size_t)e.first] < 0) { comp[(size_t)e.first] = c; todo.push_back(e.first); }
    }
  }
  size_t best = 0;
  for (size_t c = 1; c < members.size(); ++c) if (members[c].size() > members[best].size()) best = c;
  std::set<size_t> out;
  for (int v : members[best]) out.insert(frame_of[(size_t)v]);
  return out;
}

// SfM::LargestBiconnectedGraph (:780-799): the pairs with both frames in the surviving node set, in list order
inline std::vector<TailPair> LargestBiconnected(const std::vector<TailPair>& pairs, std::set<size_t>& nodes) {
  std::vector<std::pair<size_t, size_t>> e;
  for (const TailPair& p : pairs) e.push_back(p.image_pair);
  nodes = LargestEdgeBiconnected(e);
  std::vector<TailPair> good;
  if (nodes.empty()) return good;
  for (const TailPair& p : pairs) if (nodes.count(p.image_pair.first) > 0 && nodes.count(p.image_pair.second) > 0) good.push_back(p);
  return good;
}

// The final sort (:468-476) with upstream's comparator AS WRITTEN (first < first, else second < second): not a strict weak order, so std::sort's result on it is
// whatever the library's algorithm makes of it, and its introsort may even leave the range.  Here: the insertion sort libstdc++'s std::sort runs on up to 16
// elements (compare with the first element, else shift down while the comparator holds), for every length: defined for any comparator, and std::sort's own
// result wherever that is defined by the library.
template <class T, class Less>
inline void SortAsWritten(std::vector<T>& v, Less less) {
  for (size_t i = 1; i < v.size(); ++i) {
    T val = v[i];
    if (less(val, v[0])) { for (size_t j = i; j > 0; --j) v[j] = v[j - 1]; v[0] = val; }
    else { size_t j = i; while (j > 0 && less(val, v[j - 1])) { v[j] = v[j - 1]; --j; } v[j] = val; }
  }
}
inline bool PairLessAsWritten(const std::pair<size_t, size_t>& a, const std::pair<size_t, size_t>& b) {
  if (a.first < b.first) return true;
  else return a.second < b.second;
}

// :449-476 on the pairs the refinement leaves: scale, graph filter, sort.  The survivors replace `pairs`.
inline void FinishPairs(int eq_rows, int eq_cols, const std::vector<int>& frame_rows, const std::vector<DepthView>& depth, std::vector<TailPair>& pairs,
                        std::set<size_t>& covered_frames, bool keep_no_scale) {
  SetScaleList(eq_rows, eq_cols, frame_rows, depth, pairs, keep_no_scale);
  pairs = LargestBiconnected(pairs, covered_frames);
  SortAsWritten(pairs, [](const TailPair& a, const TailPair& b) { return PairLessAsWritten(a.image_pair, b.image_pair); });
}


}  // namespace relpose_detail
}  // namespace pvlm
