// pvlm_host_sfm.cpp — part of the C++ host mirror (pvlm_host.hpp): the global bundle adjustment of the SfM result and what calls it —
// SfMGlobalBA (util/Optimization.cpp:10-82), the track filters FilterTracksPixelResidual / FilterTracksAngleResidual (sfm/Structure.cpp:121-193),
// SfM::GlobalBundleAdjustment (sfm/SfM.cpp:1362-1383), MVS::RefineCameraPose (mvs/MVS.cpp:383-428) and
// CameraLidarOptimizer::GlobalBundleAdjustment (joint_optimization/CameraLidarOptimizer.cpp:732-740).
// Host logic only; the reprojection blocks are solved and the tracks are tested by libpvlm.so on the GPU (K9 / K31).
#include "pvlm_host_internal.hpp"

namespace pvlm {

namespace {

// T_cw = T_wc^-1, rigid: [R^T | -R^T t], each entry a sum in index order (upstream: Eigen's general 4x4 inverse, ~1e-16 apart)
void RigidInverse(const Matrix3d& R, const Vector3d& t, Matrix3d* Ri, Vector3d* ti) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) (*Ri)[3 * r + c] = R[3 * c + r];
    (*ti)[r] = -(((R[r] * t[0]) + R[3 + r] * t[1]) + R[6 + r] * t[2]);
  }
}

Matrix4d Compose(const Matrix3d& R, const Vector3d& t) { return {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1}; }

Matrix4d Mul4(const Matrix4d& A, const Matrix4d& B) {
  Matrix4d C;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j]; C[4 * i + j] = s; }
  return C;
}

size_t FilterTracks(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, pvlm_filter_mode mode, double threshold) {
  if (tracks.empty() || frames.empty()) return 0;
  std::vector<double> T((size_t)frames.size() * 12, 0.0);         // Matrix4d::Zero() for frames without a valid pose
  for (size_t f = 0; f < frames.size(); ++f) {
    if (!frames[f].IsPoseValid()) continue;
    Matrix3d Ri; Vector3d ti;
    RigidInverse(frames[f].R_wc, frames[f].t_wc, &Ri, &ti);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[12 * f + 4 * r + c] = Ri[3 * r + c]; T[12 * f + 4 * r + 3] = ti[r]; }
  }
  std::vector<int64_t> off(tracks.size() + 1, 0);
  std::vector<int> fid; std::vector<float> kp; std::vector<double> X(tracks.size() * 3);
  for (size_t i = 0; i < tracks.size(); ++i) {
    for (const auto& pr : tracks[i].feature_pairs) {            // std::set order, as upstream iterates
      fid.push_back((int)pr.first);
      const std::array<float, 2>& k = frames[pr.first].keypoints[pr.second];
      kp.push_back(k[0]); kp.push_back(k[1]);
    }
    off[i + 1] = (int64_t)fid.size();
    for (int k = 0; k < 3; ++k) X[3 * i + k] = tracks[i].point_3d[k];
  }
  std::vector<unsigned char> keep(tracks.size(), 1);
  Engine& e = Engine::Default();
  // Equirectangular eq(frames[0].GetImageRows(), frames[0].GetImageCols())
  e.Check(pvlm_filter_tracks(e.ctx(), mode, frames[0].GetImageRows(), frames[0].GetImageCols(), (int)tracks.size(), off.data(), fid.data(), kp.data(), X.data(),
                             (int)frames.size(), T.data(), threshold, keep.data()), "pvlm_filter_tracks");
  std::vector<PointTrack> valid;
  valid.reserve(tracks.size());
  for (size_t i = 0; i < tracks.size(); ++i) if (keep[i]) valid.push_back(std::move(tracks[i]));
  const size_t removed = tracks.size() - valid.size();
  valid.swap(tracks);
  return removed;
}

}  // namespace

bool SfMGlobalBA(std::vector<Frame>& frames, std::vector<PointTrack>& tracks, int residual_type, int num_threads, bool refine_structure, bool refine_rotation,
                 bool refine_translation, ceres_like::Solver::Summary* summary_out) {
  StageTimer stage_timer_("SfMGlobalBA");
  if (!refine_structure && !refine_rotation && !refine_translation) return false;        // :13-17
  std::vector<Vector3d> aa_cw(frames.size(), Vector3d{0, 0, 0}), t_cw(frames.size(), Vector3d{0, 0, 0});
  for (size_t i = 0; i < frames.size(); ++i) {
    if (!frames[i].IsPoseValid()) continue;
    Matrix3d R; Vector3d t;
    RigidInverse(frames[i].R_wc, frames[i].t_wc, &R, &t);
    t_cw[i] = t;
    RotationMatrixToAngleAxis(R, &aa_cw[i]);
  }
  ceres_like::Problem problem;
  AddCameraResidual(frames, aa_cw, t_cw, tracks, problem, residual_type, 1.0);
  for (size_t i = 0; i < frames.size(); ++i) {                                            // :39-47
    if (!frames[i].IsPoseValid()) continue;
    if (!refine_rotation) problem.SetParameterBlockConstant(aa_cw[i].data());
    if (!refine_translation) problem.SetParameterBlockConstant(t_cw[i].data());
  }
  if (!refine_structure)
    for (PointTrack& t : tracks) problem.SetParameterBlockConstant(t.point_3d.data());
  for (size_t i = 0; i < frames.size(); ++i) {                                            // :52-59: the first valid pose is the gauge
    if (!frames[i].IsPoseValid()) continue;
    problem.SetParameterBlockConstant(aa_cw[i].data());
    problem.SetParameterBlockConstant(t_cw[i].data());
    break;
  }
  ceres_like::Solver::Options options = SetOptionsSfM(num_threads);
  ceres_like::Solver::Summary summary;
  ceres_like::Solve(options, &problem, &summary);
  if (summary_out) *summary_out = summary;
  if (!summary.IsSolutionUsable()) return false;
  // :71-80.  A frame whose two blocks were both constant (the gauge frame, or every frame when neither rotation nor translation is refined)
  // keeps its pose bit for bit; upstream writes it back through the angle-axis round trip, ~1e-16 away.
  std::vector<bool> fixed(frames.size(), !refine_rotation && !refine_translation);
  for (size_t i = 0; i < frames.size(); ++i) if (frames[i].IsPoseValid()) { fixed[i] = true; break; }
  for (size_t i = 0; i < frames.size(); ++i) {
    if (!frames[i].IsPoseValid() || fixed[i]) continue;
    Matrix3d R; AngleAxisToRotationMatrix(aa_cw[i], &R);
    RigidInverse(R, t_cw[i], &frames[i].R_wc, &frames[i].t_wc);
  }
  return true;
}

size_t FilterTracksPixelResidual(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold) {
  if (threshold < 0) return 0;                                                            // Structure.cpp:123-124
  return FilterTracks(frames, tracks, PVLM_FILTER_PIXEL, threshold);
}

size_t FilterTracksAngleResidual(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold) {
  return FilterTracks(frames, tracks, PVLM_FILTER_ANGLE, threshold);
}

bool GlobalBundleAdjustment(std::vector<Frame>& frames, std::vector<PointTrack>& structure, int residual_type, float residual_threshold, bool refine_structure,
                            bool refine_rotation, bool refine_translation, int num_threads) {
  if (!SfMGlobalBA(frames, structure, residual_type, num_threads, refine_structure, refine_rotation, refine_translation)) return false;
  if (residual_type == ANGLE_RESIDUAL_1 || residual_type == ANGLE_RESIDUAL_2) FilterTracksAngleResidual(frames, structure, residual_threshold);
  else if (residual_type == PIXEL_RESIDUAL) FilterTracksPixelResidual(frames, structure, residual_threshold);
  return true;
}

bool RefineCameraPose(std::vector<Frame>& frames, std::vector<Velodyne>& lidars, std::vector<PointTrack>& structure, const Config& config) {
  if (structure.empty()) return false;
  std::vector<Matrix4d> T_cl(lidars.size());
  std::vector<bool> paired(lidars.size(), false);
  for (size_t i = 0; i < lidars.size() && i < frames.size(); ++i) {
    if (!lidars[i].IsPoseValid() || !frames[i].IsPoseValid()) continue;
    Matrix3d Ri; Vector3d ti;
    RigidInverse(frames[i].R_wc, frames[i].t_wc, &Ri, &ti);
    T_cl[i] = Mul4(Compose(Ri, ti), lidars[i].GetPose());
    paired[i] = true;
  }
  if (!SfMGlobalBA(frames, structure, PIXEL_RESIDUAL, config.num_threads, true, true, true)) return false;
  for (size_t i = 0; i < lidars.size(); ++i) {
    if (!paired[i] || !lidars[i].IsPoseValid() || !frames[i].IsPoseValid()) continue;
    const Matrix4d T = Mul4(frames[i].GetPose(), T_cl[i]);
    lidars[i].SetPose({T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]});
  }
  return true;
}

bool CameraLidarOptimizer::GlobalBundleAdjustment(std::vector<PointTrack>& structure, bool refine_structure, bool refine_rotation, bool refine_translation) {
  return SfMGlobalBA(frames, structure, ANGLE_RESIDUAL_1, config.num_threads, refine_structure, refine_rotation, refine_translation);
}

}  // namespace pvlm
