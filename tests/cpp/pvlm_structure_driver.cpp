// Test driver of K32's host mirror (tests/test_structure_gpu.py): the structure is built from the image matches, never handed in.
//   pvlm_structure_driver chain IN OUT residual_type threshold
//       TriangulateTracks(frames, pairs); CameraLidarOptimizer::EstimateStructure(pairs) on the same frames; then SfM::GlobalBundleAdjustment's body
//       (SfMGlobalBA with the summary, then the filter of the residual type) on the optimizer's structure
//   pvlm_structure_driver mvs IN OUT            the free EstimateStructure (MVS::EstimateStructure's body); no bundle adjustment
// IN:  int32 n_frames, rows, cols, n_pairs; per frame: int32 valid, double R_wc[9], t_wc[3], int32 n_kp, float kp[2 n_kp];
//      per pair: int32 first, second, n_matches, int32 (queryIdx, trainIdx)[2 n_matches]
// OUT: the layout of pvlm_sfm_driver (int32 ok; double initial_cost, final_cost; int32 successful_steps, unsuccessful_steps, residual_blocks; per frame: double
//      R_wc[9], t_wc[3]; int32 n_tracks; per track: uint32 id, double point[3]), then int32 n_triangulated, estimate_ret, n_estimated;
//      per triangulated track: uint32 id, double point[3]; per estimated track: uint32 id
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <typename T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s chain|mvs IN OUT ...\n", argv[0]); return 2; }
  const std::string cmd = argv[1];
  try {
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int32_t hdr[4]; rd(f, hdr, 4);
    std::vector<Frame> frames((size_t)hdr[0]);
    for (Frame& fr : frames) {
      int32_t valid = 0, nk = 0;
      rd(f, &valid, 1); rd(f, fr.R_wc.data(), 9); rd(f, fr.t_wc.data(), 3); rd(f, &nk, 1);
      fr.pose_valid = valid != 0; fr.rows = hdr[1]; fr.cols = hdr[2];
      fr.keypoints.resize((size_t)nk); rd(f, reinterpret_cast<float*>(fr.keypoints.data()), 2 * (size_t)nk);
    }
    std::vector<MatchPair> pairs((size_t)hdr[3]);
    for (MatchPair& p : pairs) {
      int32_t h[3]; rd(f, h, 3);
      p.image_pair = {(size_t)h[0], (size_t)h[1]};
      std::vector<int32_t> m(2 * (size_t)h[2]); rd(f, m.data(), m.size());
      for (int k = 0; k < h[2]; ++k) p.matches.push_back({m[2 * k], m[2 * k + 1]});
    }
    if (!f) { fprintf(stderr, "short input\n"); return 2; }
    int32_t ok = 0, estimate_ret = 0;
    ceres_like::Solver::Summary sm;
    std::vector<PointTrack> triangulated, estimated, structure;
    if (cmd == "chain" && argc >= 6) {
      triangulated = TriangulateTracks(frames, pairs);
      Config cfg; cfg.num_threads = 1;
      const Matrix4d I4 = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      CameraLidarOptimizer clo(I4, std::vector<Velodyne>(), frames, cfg);
      estimate_ret = clo.EstimateStructure(pairs) ? 1 : 0;
      estimated = clo.GetStructure();
      structure = estimated;
      const int residual_type = atoi(argv[4]);
      ok = SfMGlobalBA(frames, structure, residual_type, 1, true, true, true, &sm);
      if (ok) {
        if (residual_type == PIXEL_RESIDUAL) FilterTracksPixelResidual(frames, structure, (float)atof(argv[5]));
        else FilterTracksAngleResidual(frames, structure, (float)atof(argv[5]));
      }
    } else if (cmd == "mvs") {
      ok = EstimateStructure(frames, pairs, structure);
      triangulated = structure;
    } else {
      fprintf(stderr, "bad command\n"); return 2;
    }
    std::ofstream o(argv[3], std::ios::binary);
    wr(o, &ok, 1);
    const double costs[2] = {sm.initial_cost, sm.final_cost}; wr(o, costs, 2);
    const int32_t st[3] = {sm.num_successful_steps, sm.num_unsuccessful_steps, sm.num_residual_blocks}; wr(o, st, 3);
    for (const Frame& fr : frames) { wr(o, fr.R_wc.data(), 9); wr(o, fr.t_wc.data(), 3); }
    const int32_t nt = (int32_t)structure.size(); wr(o, &nt, 1);
    for (const PointTrack& t : structure) { wr(o, &t.id, 1); wr(o, t.point_3d.data(), 3); }
    const int32_t tail[3] = {(int32_t)triangulated.size(), estimate_ret, (int32_t)estimated.size()}; wr(o, tail, 3);
    for (const PointTrack& t : triangulated) { wr(o, &t.id, 1); wr(o, t.point_3d.data(), 3); }
    for (const PointTrack& t : estimated) wr(o, &t.id, 1);
    return o ? 0 : 1;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
