// pvlm_host_structure.hpp — the host logic of TriangulateTracks (sfm/Structure.cpp:8-69) and of the track filters around the per-track device
// calls, written against a seam: `StructureKernels` holds the calls.  pvlm_host_sfm.cpp fills it with pvlm_triangulate_tracks / pvlm_filter_tracks /
// pvlm_filter_tracks_far (the GPU); the CPU tests fill it with serial loops over the same per-track cores (tests/cpp/structure_core_check.cpp), so that track building,
// CSR assembly, compaction and order are tested without a device.  Not installed; not part of the interface.
#pragma once
#include <functional>

#include "pvlm_host.hpp"
#include "pvlm_host_tracks.hpp"

namespace pvlm {
namespace structure_detail {

struct StructureKernels {
  // pvlm_triangulate_tracks with keypoints, without the context
  std::function<void(int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, int n_frames, const double* T_cw,
                     const unsigned char* frame_valid, double* points, unsigned char* status)> triangulate;
  // pvlm_filter_tracks, without the context
  std::function<void(pvlm_filter_mode mode, int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, const double* points,
                     int n_frames, const double* T_cw, double threshold, unsigned char* keep)> filter;
  // pvlm_filter_tracks_far, without the context
  std::function<void(int n_tracks, const int64_t* off, const int* fid, const double* points, int n_frames, const double* t_wc, const unsigned char* frame_valid,
                     double threshold, unsigned char* keep)> filter_far;
};

// T_cw = T_wc^-1 of every frame, row-major 3 x 4: rigid, [R^T | -R^T t], each entry a sum in index order (upstream: Eigen's general 4x4 inverse,
// ~1e-16 apart); Matrix4d::Zero() for frames without a valid pose
inline std::vector<double> FramePoseTable(const std::vector<Frame>& frames) {
  std::vector<double> T((size_t)frames.size() * 12, 0.0);
  for (size_t f = 0; f < frames.size(); ++f) {
    if (!frames[f].IsPoseValid()) continue;
    const Matrix3d& R = frames[f].R_wc; const Vector3d& t = frames[f].t_wc;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[12 * f + 4 * r + c] = R[3 * c + r];
      T[12 * f + 4 * r + 3] = -(((R[r] * t[0]) + R[3 + r] * t[1]) + R[6 + r] * t[2]);
    }
  }
  return T;
}

// the tracks as the device calls take them: CSR offsets, frame ids and keypoints in std::set order (as upstream iterates), points
struct TrackTable {
  std::vector<int64_t> off; std::vector<int> fid; std::vector<float> kp; std::vector<double> X;
};
inline TrackTable MakeTrackTable(const std::vector<Frame>& frames, const std::vector<PointTrack>& tracks) {
  TrackTable tt;
  tt.off.assign(tracks.size() + 1, 0); tt.X.resize(tracks.size() * 3);
  for (size_t i = 0; i < tracks.size(); ++i) {
    for (const auto& pr : tracks[i].feature_pairs) {
      tt.fid.push_back((int)pr.first);
      const std::array<float, 2>& k = frames[pr.first].keypoints[pr.second];
      tt.kp.push_back(k[0]); tt.kp.push_back(k[1]);
    }
    tt.off[i + 1] = (int64_t)tt.fid.size();
    for (int k = 0; k < 3; ++k) tt.X[3 * i + k] = tracks[i].point_3d[k];
  }
  return tt;
}

// the surviving tracks in their order; returns the number removed
inline size_t Compact(std::vector<PointTrack>& tracks, const std::vector<unsigned char>& keep) {
  std::vector<PointTrack> valid;
  valid.reserve(tracks.size());
  for (size_t i = 0; i < tracks.size(); ++i) if (keep[i]) valid.push_back(std::move(tracks[i]));
  const size_t removed = tracks.size() - valid.size();
  valid.swap(tracks);
  return removed;
}

inline size_t FilterTracksWith(const StructureKernels& k, const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, pvlm_filter_mode mode, double threshold) {
  if (tracks.empty() || frames.empty()) return 0;
  const std::vector<double> T = FramePoseTable(frames);
  const TrackTable tt = MakeTrackTable(frames, tracks);
  std::vector<unsigned char> keep(tracks.size(), 1);
  // Equirectangular eq(frames[0].GetImageRows(), frames[0].GetImageCols())
  k.filter(mode, frames[0].GetImageRows(), frames[0].GetImageCols(), (int)tracks.size(), tt.off.data(), tt.fid.data(), tt.kp.data(), tt.X.data(),
           (int)frames.size(), T.data(), threshold, keep.data());
  return Compact(tracks, keep);
}

inline std::vector<PointTrack> TriangulateTracksWith(const StructureKernels& k, const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs) {
  std::vector<PointTrack> structure;
  std::vector<std::pair<size_t, size_t>> pairs;
  std::vector<std::vector<std::pair<int, int>>> pair_matches;
  for (const MatchPair& p : image_pairs) { pairs.push_back(p.image_pair); pair_matches.push_back(p.matches); }
  TrackBuilder tracks_builder;
  tracks_builder.Build(pairs, pair_matches);
  tracks_builder.Filter(3);
  std::map<uint32_t, std::set<std::pair<uint32_t, uint32_t>>> tracks;
  tracks_builder.ExportTracks(tracks);
  const size_t max_track_id = tracks_builder.GetMaxID();
  if (tracks.empty() || frames.empty()) return structure;                    // "Fail to estimate initial structure"
  // for (track_idx = 0; track_idx < max_track_id; track_idx++) if (tracks.count(track_idx)): the map in ascending id, the bound strict
  for (const auto& tr : tracks) {
    if (tr.first >= max_track_id) break;
    PointTrack t; t.id = tr.first; t.feature_pairs = tr.second;
    structure.push_back(std::move(t));
  }
  if (structure.empty()) return structure;
  const std::vector<double> T = FramePoseTable(frames);
  std::vector<unsigned char> frame_valid(frames.size());
  for (size_t f = 0; f < frames.size(); ++f) frame_valid[f] = frames[f].IsPoseValid() ? 1 : 0;
  TrackTable tt = MakeTrackTable(frames, structure);
  std::vector<unsigned char> status(structure.size(), 0);
  k.triangulate(frames[0].GetImageRows(), frames[0].GetImageCols(), (int)structure.size(), tt.off.data(), tt.fid.data(), tt.kp.data(), (int)frames.size(), T.data(),
                frame_valid.data(), tt.X.data(), status.data());
  std::vector<unsigned char> keep(structure.size());
  for (size_t i = 0; i < structure.size(); ++i) {
    keep[i] = status[i] == 0;
    for (int c = 0; c < 3; ++c) structure[i].point_3d[c] = tt.X[3 * i + c];
  }
  Compact(structure, keep);
  FilterTracksWith(k, frames, structure, PVLM_FILTER_ANGLE, 25);              // :64
  return structure;
}

inline size_t FilterTracksToFarWith(const StructureKernels& k, const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, double threshold) {
  if (tracks.empty()) return 0;
  std::vector<double> t_wc(frames.size() * 3);
  std::vector<unsigned char> frame_valid(frames.size());
  for (size_t f = 0; f < frames.size(); ++f) {
    for (int c = 0; c < 3; ++c) t_wc[3 * f + c] = frames[f].t_wc[c];                      // GetPose().block<3,1>(0,3)
    frame_valid[f] = frames[f].IsPoseValid() ? 1 : 0;
  }
  std::vector<int64_t> off(tracks.size() + 1, 0);
  std::vector<int> fid; std::vector<double> X(tracks.size() * 3);
  for (size_t i = 0; i < tracks.size(); ++i) {
    for (const auto& pr : tracks[i].feature_pairs) fid.push_back((int)pr.first);
    off[i + 1] = (int64_t)fid.size();
    for (int c = 0; c < 3; ++c) X[3 * i + c] = tracks[i].point_3d[c];
  }
  std::vector<unsigned char> keep(tracks.size(), 1);
  k.filter_far((int)tracks.size(), off.data(), fid.data(), X.data(), (int)frames.size(), t_wc.data(), frame_valid.data(), threshold, keep.data());
  return Compact(tracks, keep);
}

// CameraLidarOptimizer::EstimateStructure (joint_optimization/CameraLidarOptimizer.cpp:720-729)
inline bool EstimateStructureWith(const StructureKernels& k, const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<PointTrack>& structure) {
  structure = TriangulateTracksWith(k, frames, image_pairs);
  if (!FilterTracksToFarWith(k, frames, structure, 8)) return false;      // false when the filter removed nothing, as upstream writes it
  return true;
}

}  // namespace structure_detail
}  // namespace pvlm
