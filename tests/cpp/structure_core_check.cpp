// Host-compiled check of K32: the per-track cores of panovlm_amd/csrc/pvlm_triangulate_core.h (TriangulateNView, FilterTracksToFar) driven by
// serial loops, the TrackBuilder of panovlm_amd/host/pvlm_host_tracks.hpp, and the host logic of TriangulateTracks / EstimateStructure
// (panovlm_amd/host/pvlm_host_structure.hpp) with those loops behind its seam in place of the device calls.  tests/test_structure_cpu.py compares
// them with tests/structure_ref.py without a GPU; tests/test_structure_gpu.py compares the device calls with them bit for bit.
// TEST INFRASTRUCTURE ONLY — libpvlm.so has no host path.  Built with -ffp-contract=off.
#include <cstring>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_triangulate_core.h"
#include "../../panovlm_amd/host/pvlm_host_structure.hpp"

using namespace pvlm;

static const structure_detail::StructureKernels& HostKernels() {
  static const structure_detail::StructureKernels k = {
      [](int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, int, const double* T_cw, const unsigned char* frame_valid, double* points,
         unsigned char* status) {
        for (int t = 0; t < n_tracks; ++t)
          status[t] = (unsigned char)pvlm_triangulate::triangulate_track(rows, cols, off[t], off[t + 1], fid, kp, nullptr, T_cw, frame_valid, points + 3 * (size_t)t);
      },
      [](pvlm_filter_mode mode, int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, const double* points, int, const double* T_cw,
         double threshold, unsigned char* keep) {
        const double thr = pvlm_sfm_filter::filter_threshold((int)mode, threshold);
        for (int t = 0; t < n_tracks; ++t) keep[t] = pvlm_sfm_filter::keep_track((int)mode, rows, cols, off[t], off[t + 1], fid, kp, points + 3 * (size_t)t, T_cw, thr);
      },
      [](int n_tracks, const int64_t* off, const int* fid, const double* points, int, const double* t_wc, const unsigned char* frame_valid, double threshold,
         unsigned char* keep) {
        for (int t = 0; t < n_tracks; ++t) keep[t] = pvlm_triangulate::keep_track_far(off[t], off[t + 1], fid, points + 3 * (size_t)t, t_wc, frame_valid, threshold);
      }};
  return k;
}

static std::vector<MatchPair> to_pairs(int n_pairs, const int* pair_ij, const long long* match_off, const int* matches) {
  std::vector<MatchPair> mp((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    mp[p].image_pair = {(size_t)pair_ij[2 * p], (size_t)pair_ij[2 * p + 1]};
    for (long long m = match_off[p]; m < match_off[p + 1]; ++m) mp[p].matches.push_back({matches[2 * m], matches[2 * m + 1]});
  }
  return mp;
}

static std::vector<Frame> to_frames(int n_frames, int rows, int cols, const unsigned char* valid, const double* R_wc, const double* t_wc, const long long* kp_off,
                                    const float* kps) {
  std::vector<Frame> frames((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) {
    Frame& fr = frames[f];
    fr.id = f; fr.rows = rows; fr.cols = cols; fr.pose_valid = valid[f] != 0;
    for (int k = 0; k < 9; ++k) fr.R_wc[k] = R_wc[9 * f + k];
    for (int k = 0; k < 3; ++k) fr.t_wc[k] = t_wc[3 * f + k];
    for (long long k = kp_off[f]; k < kp_off[f + 1]; ++k) fr.keypoints.push_back({kps[2 * k], kps[2 * k + 1]});
  }
  return frames;
}

extern "C" {

// TrackBuilder.Build / Filter(length) / ExportTracks.  Outputs (capacity: one slot per match end): the track ids ascending, CSR offsets into
// (image, keypoint) pairs in std::set order; *max_id = GetMaxID().  Returns the number of tracks.
int chk_track_builder(int n_pairs, const int* pair_ij, const long long* match_off, const int* matches, unsigned length, unsigned* track_ids, long long* track_off,
                      unsigned* features, unsigned long long* max_id) {
  const std::vector<MatchPair> mp = to_pairs(n_pairs, pair_ij, match_off, matches);
  std::vector<std::pair<size_t, size_t>> pairs; std::vector<std::vector<std::pair<int, int>>> pm;
  for (const MatchPair& p : mp) { pairs.push_back(p.image_pair); pm.push_back(p.matches); }
  TrackBuilder tb;
  tb.Build(pairs, pm);
  tb.Filter(length);
  std::map<uint32_t, std::set<std::pair<uint32_t, uint32_t>>> tracks;
  tb.ExportTracks(tracks);
  *max_id = (unsigned long long)tb.GetMaxID();
  int n = 0; long long o = 0;
  track_off[0] = 0;
  for (const auto& tr : tracks) {
    track_ids[n] = tr.first;
    for (const auto& f : tr.second) { features[2 * o] = f.first; features[2 * o + 1] = f.second; ++o; }
    track_off[++n] = o;
  }
  return n;
}

// the loop of pvlm_triangulate_tracks: exactly one of kp (n_obs x 2) and bearings (n_obs x 3); frame_valid may be NULL
void chk_triangulate(int rows, int cols, int n_tracks, const long long* off, const int* fid, const float* kp, const float* bearings, const double* T_cw,
                     const unsigned char* frame_valid, double* points, unsigned char* status) {
  for (int t = 0; t < n_tracks; ++t)
    status[t] = (unsigned char)pvlm_triangulate::triangulate_track(rows, cols, off[t], off[t + 1], fid, kp, bearings, T_cw, frame_valid, points + 3 * (size_t)t);
}

// AtA (10 entries), the eigenvector of its smallest eigenvalue and its four eigenvalues, per track (any length)
void chk_nview_eig(int n_tracks, const long long* off, const int* fid, const float* bearings, const double* T_cw, double* ata, double* vec, double* w) {
  for (int t = 0; t < n_tracks; ++t) {
    double* a = ata + 10 * (size_t)t;
    for (int k = 0; k < 10; ++k) a[k] = 0.0;
    for (long long i = off[t]; i < off[t + 1]; ++i) pvlm_triangulate::ata_add(T_cw + 12 * (long long)fid[i], bearings + 3 * i, a);
    pvlm_triangulate::eig4_smallest(a, vec + 4 * (size_t)t, w + 4 * (size_t)t);
  }
}

void chk_filter_far(int n_tracks, const long long* off, const int* fid, const double* points, const double* t_wc, const unsigned char* frame_valid, double threshold,
                    unsigned char* keep) {
  for (int t = 0; t < n_tracks; ++t) keep[t] = pvlm_triangulate::keep_track_far(off[t], off[t + 1], fid, points + 3 * (size_t)t, t_wc, frame_valid, threshold);
}

// mode 0: TriangulateTracks; mode 1: CameraLidarOptimizer::EstimateStructure's body (then *ret = its return value); mode 2: FilterTracksToFar(threshold) on
// the structure of TriangulateTracks (then *ret = the number removed).  Outputs (capacity: one per match end): ids and points of the structure in its order.
int chk_structure(int mode, double threshold, int n_frames, int rows, int cols, const unsigned char* valid, const double* R_wc, const double* t_wc,
                  const long long* kp_off, const float* kps, int n_pairs, const int* pair_ij, const long long* match_off, const int* matches, unsigned* ids,
                  double* points, long long* ret) {
  const std::vector<Frame> frames = to_frames(n_frames, rows, cols, valid, R_wc, t_wc, kp_off, kps);
  const std::vector<MatchPair> mp = to_pairs(n_pairs, pair_ij, match_off, matches);
  std::vector<PointTrack> structure;
  *ret = 0;
  if (mode == 1) *ret = structure_detail::EstimateStructureWith(HostKernels(), frames, mp, structure) ? 1 : 0;
  else {
    structure = structure_detail::TriangulateTracksWith(HostKernels(), frames, mp);
    if (mode == 2) *ret = (long long)structure_detail::FilterTracksToFarWith(HostKernels(), frames, structure, threshold);
  }
  for (size_t i = 0; i < structure.size(); ++i) { ids[i] = structure[i].id; std::memcpy(points + 3 * i, structure[i].point_3d.data(), 24); }
  return (int)structure.size();
}

}  // extern "C"
