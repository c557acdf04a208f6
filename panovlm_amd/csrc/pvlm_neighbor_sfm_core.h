// K49: the definition of MVS::SelectNeighborSFM (mvs/MVS.cpp:248-332) — host and device.  Compiled for the device by pvlm_neighbor_sfm.hip and for the host by
// tests/cpp/neighbor_sfm_core_check.cpp and the host mirror (host/pvlm_host_neighbor.cpp); select_host below is upstream's loop as written and is what an uncertain
// row falls back to.
//
// Input: F views with poses T_wc (3 x 4, row-major) and T tracks in CSR form (track_offsets[T + 1], view_ids, points[3 T]); a track's views ascend (upstream reads
// them out of a std::set<pair<image, feature>>) and a view may occur twice.
//   contribution   for every track in order and every i < j of its views, id1 = views[i], id2 = views[j] (pair_terms below, every rounding upstream's):
//                  V1 = X - C1, V2 = X - C2 in double; depth = sqrt(x^2 + y^2 + z^2); angle = VectorAngle3D(V1, V2) * 180 / M_PI (base/Geometry.hpp:450-466: the
//                  cosine divided by norm1 * norm2, >= 1 gives 0, <= -1 gives M_PI, else acos); a = min(powf(float(angle / 10.0), 1.5f), 1.f), a FLOAT, widened
//                  back; s12 = f(depth1 / depth2), s21 = f(depth2 / depth1), f(s) = 1.6 * 1.6 / s / s if s > 1.6, 1 if s >= 1, else s * s;
//                  score(id1, id2) += s12 * a, score(id2, id1) += s21 * a with score a FLOAT matrix: every += is float(double(cell) + product) (add_to_cell);
//   order          the additions into one cell come in track order, and inside a track in (i, j) order;
//   selection      per row the columns with score > 0, sorted by std::greater<pair<float, size_t>> (score descending, ties by column DESCENDING), walked until
//                  neighbor_size are accepted; a candidate is accepted when ||t_nr|| > sq_distance_threshold with T_nr = T_wn^-1 T_wr.  Upstream compares the NORM,
//                  not its square, with the SQUARED threshold (:322); that is kept literally.  T_nr uses the rigid inverse (R_nr = R_wn^T R_wr, t_nr = R_wn^T (t_wr -
//                  t_wn), every sum from 0 in index order, as SelectNeighborKNN of the mirror has it), double, stored as float; the norm is taken of the doubles.
// Deliberate divergence: a track that names a view >= F or a view without a valid pose is refused (upstream would read a sentinel pose and produce NaNs).
//
// A TRACK THAT REPEATS A VIEW puts two contributions of one track into one cell (and some on the diagonal).  The device serialises it: one lane walks that track's
// (i, j) loop for its row as written, at the track's turn, so such rows stay on the device.
//
// CERTAINTY.  The device's acos and powf need not equal glibc's bit for bit.  Everything else of a contribution is correctly rounded IEEE arithmetic without
// contraction on both sides, so a product differs only through the float a: by at most 1 ulp, 2^-23 relative.  Each of the n additions into a cell rounds to float,
// and a rounding of a slightly different sum can differ by an ulp of the cell.  Hence |score_device - score_host| <= (n + 2) * 2^-23 * score (bound below), n the
// cell's contribution count, which the device keeps beside the score.  A row is UNCERTAIN when two candidates adjacent in the walk's order, up to and including the
// first one behind the last candidate the walk reaches, are closer than the sum of their bounds, or when a ||t_nr|| the walk tests lies within kNormBand (relative)
// of the threshold (the two sides compute the norm with the same operations; the band is margin, as K48's).  Uncertain rows are recomputed by select_host's row form.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define PVLM_NS_HD __host__ __device__ __forceinline__
#else
#define PVLM_NS_HD inline
#endif

namespace pvlm_neighbor_sfm {

constexpr double kAngleThreshold = 10.0, kScaleThreshold = 1.6;       // :261-262
constexpr double kNormBand = 1e-12;
constexpr double kPi = 3.14159265358979323846;                          // M_PI

struct Stats { long long n_candidates, n_contributions, n_repeat_tracks, n_uncertain; };      // == pvlm_neighbor_sfm_stats

// the centre of a view: the translation column of its 3 x 4 pose
PVLM_NS_HD void centre_of(const double* T_wc, long long view, double* C) { const double* p = T_wc + 12 * view; C[0] = p[3]; C[1] = p[7]; C[2] = p[11]; }

PVLM_NS_HD double scale_factor(double scale) {                          // :285-290
  if (scale > kScaleThreshold) return kScaleThreshold * kScaleThreshold / scale / scale;
  if (scale >= 1.0) return 1.0;
  return scale * scale;
}

// the two products of one (i, j) of a track: p12 goes to score(id1, id2), p21 to score(id2, id1)
PVLM_NS_HD void pair_terms(const double* X, const double* C1, const double* C2, double* p12, double* p21) {
  const double V1[3] = {X[0] - C1[0], X[1] - C1[1], X[2] - C1[2]}, V2[3] = {X[0] - C2[0], X[1] - C2[1], X[2] - C2[2]};
  const double depth1 = sqrt(V1[0] * V1[0] + V1[1] * V1[1] + V1[2] * V1[2]), depth2 = sqrt(V2[0] * V2[0] + V2[1] * V2[1] + V2[2] * V2[2]);
  double cos_angle = V1[0] * V2[0] + V1[1] * V2[1] + V1[2] * V2[2];
  cos_angle /= (depth1 * depth2);                                       // VectorAngle3D's norm1, norm2 are the same sums as the depths
  double angle;
  if (cos_angle >= 1.0) angle = 0.0;
  else if (cos_angle <= -1.0) angle = kPi;
  else angle = acos(cos_angle);
  angle = angle * 180 / kPi;
  const float pw = powf((float)(angle / kAngleThreshold), 1.5f);
  const double a = (double)(1.f < pw ? 1.f : pw);                       // std::min(pw, 1.f) as the library writes it
  *p12 = scale_factor(depth1 / depth2) * a;
  *p21 = scale_factor(depth2 / depth1) * a;
}

// float += double
PVLM_NS_HD float add_to_cell(float cell, double product) { return (float)((double)cell + product); }

// see CERTAINTY above
PVLM_NS_HD double bound(float score, int n) { return (double)(n + 2) * 1.1920928955078125e-07 * (double)score; }

// T_nr = T_wn^-1 T_wr by the rigid inverse; returns ||t_nr|| of the doubles
PVLM_NS_HD double relative_pose(const double* T_wn, const double* T_wr, float* R_nr, float* t_nr) {
  double t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      double acc = 0;
      for (int m = 0; m < 3; ++m) acc += T_wn[4 * m + r] * T_wr[4 * m + c];
      if (R_nr) R_nr[3 * r + c] = (float)acc;
    }
    double acc = 0;
    for (int m = 0; m < 3; ++m) acc += T_wn[4 * m + r] * (T_wr[4 * m + 3] - T_wn[4 * m + 3]);
    t[r] = acc;
    if (t_nr) t_nr[r] = (float)acc;
  }
  return sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
}

PVLM_NS_HD bool near_threshold(double norm, double threshold) { return fabs(norm - threshold) <= kNormBand * fabs(threshold); }

// one track's part of row `row`, as written: every (i, j), i < j, of the track that has `row` at either end, in (i, j) order.  Columns outside [col0, col1) are
// skipped (the device's column tile); cells / counts are indexed by column - col0.  What the device's one lane runs for a track that repeats a view, and what
// row_host runs for every track.
PVLM_NS_HD void track_into_row(const int* views, int len, const double* X, const double* T_wc, int row, int col0, int col1, float* cells, int* counts) {
  for (int i = 0; i < len; ++i)
    for (int j = i + 1; j < len; ++j) {
      const int id1 = views[i], id2 = views[j];
      if (id1 != row && id2 != row) continue;
      const bool in1 = id1 == row && id2 >= col0 && id2 < col1, in2 = id2 == row && id1 >= col0 && id1 < col1;
      if (!in1 && !in2) continue;
      double C1[3], C2[3], p12, p21;
      centre_of(T_wc, id1, C1); centre_of(T_wc, id2, C2);
      pair_terms(X, C1, C2, &p12, &p21);
      if (in1) { cells[id2 - col0] = add_to_cell(cells[id2 - col0], p12); if (counts) ++counts[id2 - col0]; }
      if (in2) { cells[id1 - col0] = add_to_cell(cells[id1 - col0], p21); if (counts) ++counts[id1 - col0]; }
    }
}

// ---- the call's host set-up and the literal host loops --------------------------------------------------------------------------------------

// nullptr, or what is wrong with the arguments
inline const char* check_args(int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets, const int* view_ids, const double* points,
                              int neighbor_size, double threshold) {
  if (F < 0 || T < 0 || neighbor_size < 0) return "a negative size";
  if ((F > 0 && (!T_wc || !pose_valid)) || !track_offsets || (T > 0 && !points)) return "null argument";
  if (!(threshold == threshold)) return "the threshold is not a number";
  if (track_offsets[0] != 0) return "track_offsets does not start at 0";
  for (int t = 0; t < T; ++t) {
    const int64_t len = track_offsets[t + 1] - track_offsets[t];
    if (len < 0 || len > INT32_MAX) return "track_offsets does not ascend";
  }
  if (track_offsets[T] > 0 && !view_ids) return "null argument";
  for (int t = 0; t < T; ++t)
    for (int64_t o = track_offsets[t]; o < track_offsets[t + 1]; ++o) {
      const int v = view_ids[o];
      if (v < 0 || v >= F) return "a track names a view out of range";
      if (!pose_valid[v]) return "a track names a view without a valid pose";
      if (o > track_offsets[t] && view_ids[o - 1] > v) return "the views of a track do not ascend";
    }
  return nullptr;
}

// The view -> track index: a counting sort by view, tracks ascending inside a view, one entry per (view, track) however often the track names the view.
//   view_off[F + 1]   the entries of view v are [view_off[v], view_off[v + 1]);
//   entry_track, entry_pos   the track and the position of the view's FIRST occurrence in it;
//   item_off[n_entries + 1]  running count of the lane items of the entries: len - 1 partners for an ordinary track, 1 item (the serial walk) for a repeat track;
//   repeat[T]         1 for a track that names a view twice.
struct Index {
  std::vector<int> view_off, entry_track, entry_pos;
  std::vector<long long> item_off;
  std::vector<unsigned char> repeat;
  long long n_contributions = 0, n_repeat_tracks = 0;
  void build(int F, int T, const int64_t* track_offsets, const int* view_ids) {
    view_off.assign((size_t)F + 1, 0); repeat.assign((size_t)T + 1, 0);
    n_contributions = n_repeat_tracks = 0;
    for (int t = 0; t < T; ++t) {
      const int64_t o0 = track_offsets[t], o1 = track_offsets[t + 1], len = o1 - o0;
      n_contributions += len * (len - 1);
      for (int64_t o = o0; o < o1; ++o) {
        if (o > o0 && view_ids[o] == view_ids[o - 1]) repeat[(size_t)t] = 1;
        else ++view_off[(size_t)view_ids[o] + 1];
      }
      n_repeat_tracks += repeat[(size_t)t];
    }
    for (int v = 0; v < F; ++v) view_off[(size_t)v + 1] += view_off[(size_t)v];
    const size_t E = (size_t)view_off[(size_t)F];
    entry_track.assign(E + 1, 0); entry_pos.assign(E + 1, 0); item_off.assign(E + 1, 0);
    std::vector<int> fill(view_off.begin(), view_off.end() - 1);
    for (int t = 0; t < T; ++t) {
      const int64_t o0 = track_offsets[t], o1 = track_offsets[t + 1];
      for (int64_t o = o0; o < o1; ++o) {
        if (o > o0 && view_ids[o] == view_ids[o - 1]) continue;
        const int e = fill[(size_t)view_ids[o]]++;
        entry_track[(size_t)e] = t; entry_pos[(size_t)e] = (int)(o - o0);
      }
    }
    long long run = 0;
    for (size_t e = 0; e < E; ++e) {
      item_off[e] = run;
      const int t = entry_track[e];
      run += repeat[(size_t)t] ? 1 : (track_offsets[t + 1] - track_offsets[t] - 1);
    }
    item_off[E] = run;
  }
};

struct RowResult { int n = 0; std::vector<int> ids; std::vector<float> R_nr, t_nr, scores; long long n_candidates = 0; };

// the walk over one finished score row (:305-328)
inline RowResult select_row_host(int F, const double* T_wc, int row, const float* score_row, int neighbor_size, double threshold) {
  RowResult out;
  std::vector<std::pair<float, size_t>> cand;
  for (size_t col = 0; col < (size_t)F; ++col) if (score_row[col] > 0) cand.push_back({score_row[col], col});
  std::sort(cand.begin(), cand.end(), std::greater<>());
  out.n_candidates = (long long)cand.size();
  for (size_t i = 0; i < cand.size() && out.n < neighbor_size; ++i) {
    float R[9], t[3];
    const double norm = relative_pose(T_wc + 12 * cand[i].second, T_wc + 12 * (size_t)row, R, t);
    if (norm > threshold) {
      out.ids.push_back((int)cand[i].second); out.scores.push_back(cand[i].first);
      out.R_nr.insert(out.R_nr.end(), R, R + 9); out.t_nr.insert(out.t_nr.end(), t, t + 3);
      ++out.n;
    }
  }
  return out;
}

// one row of the score matrix by the literal loop restricted to the tracks of that row (the other tracks add nothing to it): score_row[F], counts[F] or nullptr
inline void row_host(const Index& ix, int F, const double* T_wc, const int64_t* track_offsets, const int* view_ids, const double* points, int row, float* score_row,
                     int* counts) {
  std::fill(score_row, score_row + F, 0.f);
  if (counts) std::fill(counts, counts + F, 0);
  for (int e = ix.view_off[(size_t)row]; e < ix.view_off[(size_t)row + 1]; ++e) {
    const int t = ix.entry_track[(size_t)e];
    track_into_row(view_ids + track_offsets[t], (int)(track_offsets[t + 1] - track_offsets[t]), points + 3 * (size_t)t, T_wc, row, 0, F, score_row, counts);
  }
}

// MVS::SelectNeighborSFM as written: the dense F x F float matrix, the loop over all tracks and all (i, j), then the walk of every row.  Outputs as
// pvlm_mvs_select_neighbors_sfm's (the slots a row does not fill: id -1, the rest 0); 0, or -1 (PVLM_ERR_ARG) with *why set and nothing written.
inline int select_host(int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets, const int* view_ids, const double* points,
                       int neighbor_size, double threshold, int* n_neighbors, int* ids, float* R_nr, float* t_nr, float* scores, Stats* stats,
                       const char** why = nullptr) {
  const char* bad = check_args(F, T_wc, pose_valid, T, track_offsets, view_ids, points, neighbor_size, threshold);
  if (!bad && (!stats || (F > 0 && (!n_neighbors || (neighbor_size > 0 && (!ids || !R_nr || !t_nr || !scores)))))) bad = "null argument";
  if (why) *why = bad;
  if (bad) return -1;
  Stats st{0, 0, 0, 0};
  const size_t slots = (size_t)F * (size_t)neighbor_size;
  if (slots) { std::fill(ids, ids + slots, -1); std::fill(R_nr, R_nr + 9 * slots, 0.f); std::fill(t_nr, t_nr + 3 * slots, 0.f); std::fill(scores, scores + slots, 0.f); }
  std::vector<float> score((size_t)F * (size_t)F, 0.f);
  for (int t = 0; t < T; ++t) {
    const int* views = view_ids + track_offsets[t];
    const int len = (int)(track_offsets[t + 1] - track_offsets[t]);
    const double* X = points + 3 * (size_t)t;
    bool rep = false;
    for (int i = 0; i < len; ++i)
      for (int j = i + 1; j < len; ++j) {
        const int id1 = views[i], id2 = views[j];
        rep |= id1 == id2;
        double C1[3], C2[3], p12, p21;
        centre_of(T_wc, id1, C1); centre_of(T_wc, id2, C2);
        pair_terms(X, C1, C2, &p12, &p21);
        float& c12 = score[(size_t)id1 * F + id2]; c12 = add_to_cell(c12, p12);
        float& c21 = score[(size_t)id2 * F + id1]; c21 = add_to_cell(c21, p21);
        st.n_contributions += 2;
      }
    st.n_repeat_tracks += rep;
  }
  for (int row = 0; row < F; ++row) {
    const RowResult r = select_row_host(F, T_wc, row, score.data() + (size_t)row * F, neighbor_size, threshold);
    st.n_candidates += r.n_candidates;
    n_neighbors[row] = r.n;
    for (int k = 0; k < r.n; ++k) {
      const size_t at = (size_t)row * neighbor_size + k;
      ids[at] = r.ids[(size_t)k]; scores[at] = r.scores[(size_t)k];
      std::copy(r.R_nr.begin() + 9 * k, r.R_nr.begin() + 9 * k + 9, R_nr + 9 * at);
      std::copy(r.t_nr.begin() + 3 * k, r.t_nr.begin() + 3 * k + 3, t_nr + 3 * at);
    }
  }
  *stats = st;
  return 0;
}
}  // namespace pvlm_neighbor_sfm
