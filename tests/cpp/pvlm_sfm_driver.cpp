// Test driver of K31's host mirror (tests/test_sfm_ba_gpu.py): SfMGlobalBA, SfM::GlobalBundleAdjustment's body and MVS::RefineCameraPose's
// body on a scene read from a binary file, results written to another.
//   pvlm_sfm_driver ba      IN OUT residual_type refine_structure refine_rotation refine_translation
//   pvlm_sfm_driver gba     IN OUT residual_type threshold [threshold ...]     (one GlobalBundleAdjustment per threshold, in order)
//   pvlm_sfm_driver refine  IN OUT                                            (RefineCameraPose, every scan paired with its frame)
//   pvlm_sfm_driver mixed   IN OUT   one Problem with PanoramaReprojResidual_Pixel blocks (even tracks, HuberLoss(4.0)) and _2Angle blocks (odd
//                                    tracks, HuberLoss(4 deg)) as AddCameraResidual builds them, first frame constant, SetOptionsSfM, Solve
//   pvlm_sfm_driver clo_ba  IN OUT   CameraLidarOptimizer::GlobalBundleAdjustment(structure, true, true, true) on the file's frames
//   pvlm_sfm_driver eval2   kind(1|2) x y rows cols aa0 aa1 aa2 t0 t1 t2 X0 X1 X2 weight
//                                    CostFunction::Evaluate of one _2Angle / _Pixel block: prints r0 r1 and the 2 x 3 Jacobian of each block
// IN:  int32 n_frames, rows, cols, n_tracks, n_lidars; per frame: int32 valid, double R_wc[9], t_wc[3], int32 n_kp, float kp[2 n_kp];
//      per track: int32 n_obs, uint32 (frame, keypoint)[2 n_obs], double point[3]; per scan: double R_wl[9], t_wl[3]
// OUT: int32 ok; double initial_cost, final_cost; int32 successful_steps, unsuccessful_steps, residual_blocks; per frame: double R_wc[9], t_wc[3];
//      int32 n_tracks; per track: uint32 id, double point[3]; per scan: double R_wl[9], t_wl[3]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <typename T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s ba|gba|refine IN OUT ...\n", argv[0]); return 2; }
  const std::string cmd = argv[1];
  try {
    if (cmd == "eval2" && argc >= 17) {
      double v[15];
      for (int k = 0; k < 15; ++k) v[k] = atof(argv[2 + k]);
      const int kind = (int)v[0];
      ceres_like::CostFunction* c = kind == 2 ? PanoramaReprojResidual_Pixel::Create({v[1], v[2]}, (int)v[3], (int)v[4], v[14])
                                              : PanoramaReprojResidual_2Angle::Create({v[1], v[2]}, v[14]);
      const double* params[3] = {v + 5, v + 8, v + 11};
      double r[2], J0[6], J1[6], J2[6];
      double* jac[3] = {J0, J1, J2};
      const bool ok = c->Evaluate(params, r, jac);
      printf("eval2 %d %.17g %.17g", ok ? 1 : 0, r[0], r[1]);
      for (int b = 0; b < 3; ++b) for (int k = 0; k < 6; ++k) printf(" %.17g", jac[b][k]);
      printf("\n");
      delete c;
      return ok ? 0 : 1;
    }
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int32_t hdr[5]; rd(f, hdr, 5);
    std::vector<Frame> frames((size_t)hdr[0]);
    for (Frame& fr : frames) {
      int32_t valid = 0, nk = 0;
      rd(f, &valid, 1); rd(f, fr.R_wc.data(), 9); rd(f, fr.t_wc.data(), 3); rd(f, &nk, 1);
      fr.pose_valid = valid != 0; fr.rows = hdr[1]; fr.cols = hdr[2];
      fr.keypoints.resize((size_t)nk); rd(f, reinterpret_cast<float*>(fr.keypoints.data()), 2 * (size_t)nk);
    }
    std::vector<PointTrack> tracks((size_t)hdr[3]);
    for (size_t t = 0; t < tracks.size(); ++t) {
      int32_t n = 0; rd(f, &n, 1);
      std::vector<uint32_t> pr(2 * (size_t)n); rd(f, pr.data(), pr.size());
      for (int k = 0; k < n; ++k) tracks[t].feature_pairs.insert({pr[2 * k], pr[2 * k + 1]});
      rd(f, tracks[t].point_3d.data(), 3);
      tracks[t].id = (uint32_t)t;
    }
    std::vector<Velodyne> lidars((size_t)hdr[4]);
    for (Velodyne& l : lidars) { Matrix3d R; Vector3d t; rd(f, R.data(), 9); rd(f, t.data(), 3); l.SetPose(R, t); }
    if (!f) { fprintf(stderr, "short input\n"); return 2; }
    int32_t ok = 0;
    ceres_like::Solver::Summary sm;
    if (cmd == "ba" && argc >= 8) {
      ok = SfMGlobalBA(frames, tracks, atoi(argv[4]), 1, atoi(argv[5]) != 0, atoi(argv[6]) != 0, atoi(argv[7]) != 0, &sm);
    } else if (cmd == "gba" && argc >= 6) {
      ok = 1;
      for (int k = 5; k < argc && ok; ++k) ok = GlobalBundleAdjustment(frames, tracks, atoi(argv[4]), (float)atof(argv[k]));
    } else if (cmd == "mixed") {
      std::vector<Vector3d> aa(frames.size(), Vector3d{0, 0, 0}), t(frames.size(), Vector3d{0, 0, 0});
      for (size_t i = 0; i < frames.size(); ++i) {
        Matrix3d Rcw; for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rcw[3 * r + c] = frames[i].R_wc[3 * c + r];
        for (int r = 0; r < 3; ++r) t[i][r] = -(((frames[i].R_wc[r] * frames[i].t_wc[0]) + frames[i].R_wc[3 + r] * frames[i].t_wc[1]) + frames[i].R_wc[6 + r] * frames[i].t_wc[2]);
        RotationMatrixToAngleAxis(Rcw, &aa[i]);
      }
      ceres_like::Problem problem;
      ceres_like::LossFunction* pix_loss = new ceres_like::HuberLoss(4.0);
      ceres_like::LossFunction* ang_loss = new ceres_like::HuberLoss(4.0 * M_PI / 180.0);
      const int rows = hdr[1], cols = hdr[2];
      for (size_t q = 0; q < tracks.size(); ++q)
        for (const auto& pr : tracks[q].feature_pairs) {
          const std::array<float, 2>& kp = frames[pr.first].keypoints[pr.second];
          if (q % 2 == 0) {
            problem.AddResidualBlock(PanoramaReprojResidual_Pixel::Create({(double)kp[0], (double)kp[1]}, rows, cols), pix_loss, aa[pr.first].data(),
                                     t[pr.first].data(), tracks[q].point_3d.data());
          } else {
            const float sx = (float)((2 * kp[0] / cols - 1) * M_PI), sy = (float)((0.5 - kp[1] / rows) * M_PI);
            problem.AddResidualBlock(PanoramaReprojResidual_2Angle::Create({(double)sx, (double)sy}), ang_loss, aa[pr.first].data(), t[pr.first].data(),
                                     tracks[q].point_3d.data());
          }
        }
      problem.SetParameterBlockConstant(aa[0].data()); problem.SetParameterBlockConstant(t[0].data());
      ceres_like::Solve(SetOptionsSfM(1), &problem, &sm);
      ok = sm.IsSolutionUsable();
      for (size_t i = 0; i < frames.size(); ++i) {          // the angle-axis parameters as they are, in the pose slots (R_wc <- aa, 0..; t_wc <- t_cw)
        frames[i].R_wc = Matrix3d{aa[i][0], aa[i][1], aa[i][2], 0, 0, 0, 0, 0, 0}; frames[i].t_wc = t[i];
      }
    } else if (cmd == "clo_ba") {
      Config cfg; cfg.num_threads = 1;
      const Matrix4d I4 = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      CameraLidarOptimizer clo(I4, lidars, frames, cfg);
      ok = clo.GlobalBundleAdjustment(tracks, true, true, true);
      frames = clo.GetFrames();
    } else if (cmd == "refine") {
      Config cfg; cfg.num_threads = 1;
      ok = RefineCameraPose(frames, lidars, tracks, cfg);
    } else {
      fprintf(stderr, "bad command\n"); return 2;
    }
    std::ofstream o(argv[3], std::ios::binary);
    wr(o, &ok, 1);
    const double costs[2] = {sm.initial_cost, sm.final_cost}; wr(o, costs, 2);
    const int32_t st[3] = {sm.num_successful_steps, sm.num_unsuccessful_steps, sm.num_residual_blocks}; wr(o, st, 3);
    for (const Frame& fr : frames) { wr(o, fr.R_wc.data(), 9); wr(o, fr.t_wc.data(), 3); }
    const int32_t nt = (int32_t)tracks.size(); wr(o, &nt, 1);
    for (const PointTrack& t : tracks) { wr(o, &t.id, 1); wr(o, t.point_3d.data(), 3); }
    for (const Velodyne& l : lidars) { const Matrix4d T = l.GetPose(); const double Rt[12] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10], T[3], T[7], T[11]}; wr(o, Rt, 12); }
    return o ? 0 : 1;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
