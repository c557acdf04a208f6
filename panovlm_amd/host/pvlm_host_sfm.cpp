// pvlm_host_sfm.cpp — part of the C++ host mirror (pvlm_host.hpp): the global bundle adjustment of the SfM result and what calls it —
// SfMGlobalBA (util/Optimization.cpp:10-82), the track filters FilterTracksPixelResidual / FilterTracksAngleResidual (sfm/Structure.cpp:121-193),
// SfM::GlobalBundleAdjustment (sfm/SfM.cpp:1362-1383), MVS::RefineCameraPose (mvs/MVS.cpp:383-428) and
// CameraLidarOptimizer::GlobalBundleAdjustment (joint_optimization/CameraLidarOptimizer.cpp:732-740); and what builds the structure they refine —
// TriangulateTracks / FilterTracksToFar (sfm/Structure.cpp:8-119), CameraLidarOptimizer::EstimateStructure (:720-729), MVS::EstimateStructure
// (mvs/MVS.cpp:44-59); and the step between the relative and the global poses — EstimateGlobalTranslation with TranslationAveragingDLT / L2 / SoftL1 / L2IRLS, ReIndex,
// SetToOrigin (sfm/SfM.cpp:1047-1344, sfm/TranslationAveraging.cpp; K42) after EstimateGlobalRotation with FindTriplet, FilterByTriplet, FilterPairs and
// RotationAveragingSpanningTree / RefineL1 / L1 / L2 (sfm/SfM.cpp:705-905, sfm/RotationAveraging.cpp, sfm/PoseGraph.cpp:195-226; K40) and RotationAveragingLeastSquare (K45).
// Host logic only; the reprojection blocks are solved and the tracks are triangulated and tested by libpvlm.so on the GPU (K9 / K31 / K32).
#include <array>
#include <queue>

#include "pvlm_host_internal.hpp"
#include "pvlm_host_structure.hpp"
#include "../csrc/pvlm_triangulate_core.h"
#include "pvlm_host_match.hpp"
#include "pvlm_host_essential.hpp"
#include "pvlm_host_vlad.hpp"
#include "pvlm_host_relpose.hpp"
#include "../csrc/pvlm_depthfill_core.h"
#include "pvlm_host_transavg.hpp"
#include "pvlm_host_rotavg.hpp"
#include "pvlm_host_bata.hpp"
#include "pvlm_host_rotstart.hpp"
#include "pvlm_host_transdir.hpp"
#include "pvlm_host_translp.hpp"
#include "../csrc/pvlm_triplet_core.h"

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

// the per-track device calls behind the seam of pvlm_host_structure.hpp
const structure_detail::StructureKernels& DeviceKernels() {
  static const structure_detail::StructureKernels k = {
      [](int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, int n_frames, const double* T_cw, const unsigned char* frame_valid,
         double* points, unsigned char* status) {
        Engine& e = Engine::Default();
        e.Check(pvlm_triangulate_tracks(e.ctx(), rows, cols, n_tracks, off, fid, kp, nullptr, n_frames, T_cw, frame_valid, points, status), "pvlm_triangulate_tracks");
      },
      [](pvlm_filter_mode mode, int rows, int cols, int n_tracks, const int64_t* off, const int* fid, const float* kp, const double* points, int n_frames,
         const double* T_cw, double threshold, unsigned char* keep) {
        Engine& e = Engine::Default();
        e.Check(pvlm_filter_tracks(e.ctx(), mode, rows, cols, n_tracks, off, fid, kp, points, n_frames, T_cw, threshold, keep), "pvlm_filter_tracks");
      },
      [](int n_tracks, const int64_t* off, const int* fid, const double* points, int n_frames, const double* t_wc, const unsigned char* frame_valid, double threshold,
         unsigned char* keep) {
        Engine& e = Engine::Default();
        e.Check(pvlm_filter_tracks_far(e.ctx(), n_tracks, off, fid, points, n_frames, t_wc, frame_valid, threshold, keep), "pvlm_filter_tracks_far");
      }};
  return k;
}

size_t FilterTracks(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, pvlm_filter_mode mode, double threshold) {
  return structure_detail::FilterTracksWith(DeviceKernels(), frames, tracks, mode, threshold);
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

// ---- K32 --------------------------------------------------------------------------------------------------------------------------------
std::vector<PointTrack> TriangulateTracks(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs) {
  StageTimer stage_timer_("TriangulateTracks");
  return structure_detail::TriangulateTracksWith(DeviceKernels(), frames, image_pairs);
}

size_t FilterTracksToFar(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold) {
  return structure_detail::FilterTracksToFarWith(DeviceKernels(), frames, tracks, threshold);
}

Vector3d Triangulate2View(const Matrix3d& R_21, const Vector3d& t_21, const std::array<float, 3>& p1, const std::array<float, 3>& p2) {
  Vector3d P;
  pvlm_triangulate::triangulate_2view(R_21.data(), t_21.data(), p1.data(), p2.data(), P.data());
  return P;
}

Vector3d TriangulateNView(const std::vector<Matrix3d>& R_cw_list, const std::vector<Vector3d>& t_cw_list, const std::vector<std::array<float, 3>>& points) {
  if (R_cw_list.size() != t_cw_list.size() || R_cw_list.size() != points.size()) throw std::invalid_argument("TriangulateNView: list sizes differ");   // upstream asserts
  const size_t n = points.size();
  std::vector<double> T(12 * n); std::vector<int> fid(n); std::vector<float> b(3 * n);
  for (size_t i = 0; i < n; ++i) {
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[12 * i + 4 * r + c] = R_cw_list[i][3 * r + c]; T[12 * i + 4 * r + 3] = t_cw_list[i][r]; }
    fid[i] = (int)i;
    for (int k = 0; k < 3; ++k) b[3 * i + k] = points[i][k];
  }
  Vector3d X;
  pvlm_triangulate::triangulate_track(0, 0, 0, (long long)n, fid.data(), nullptr, b.data(), T.data(), nullptr, X.data());
  return X;
}

// ---- K33 --------------------------------------------------------------------------------------------------------------------------------
std::vector<DMatch> MatchSIFT(const std::vector<float>& descriptor1, const std::vector<float>& descriptor2, const float dist_ratio_threshold) {
  std::vector<DMatch> out;
  for (const match_detail::Match& m : match_detail::MatchRows(descriptor1.data(), (int)(descriptor1.size() / 128), descriptor2.data(), (int)(descriptor2.size() / 128),
                                                              dist_ratio_threshold))
    out.push_back(DMatch{m.query, m.train, m.distance});
  return out;
}

namespace {
// the pair list as the entry points take it; false when a pair names a frame that is not there or a frame's descriptor is not 128 floats per keypoint
bool PairLists(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<int>* rows, std::vector<const float*>* desc, std::vector<int>* src,
               std::vector<int>* tgt) {
  for (const Frame& f : frames) {
    if (f.descriptor.size() != 128 * f.keypoints.size()) return false;             // one descriptor row per keypoint
    rows->push_back((int)f.keypoints.size()); desc->push_back(f.descriptor.data());
  }
  for (const MatchPair& p : image_pairs) {
    if (p.image_pair.first >= frames.size() || p.image_pair.second >= frames.size()) return false;
    src->push_back((int)p.image_pair.first); tgt->push_back((int)p.image_pair.second);
  }
  return true;
}
}  // namespace

bool MatchImagePairs(const std::vector<Frame>& frames, std::vector<MatchPair>& image_pairs, const float ratio, const int matches_threshold) {
  StageTimer stage_timer_("MatchImagePairs");
  if (matches_threshold < 0) return false;
  std::vector<int> rows, src, tgt; std::vector<const float*> desc;
  if (!PairLists(frames, image_pairs, &rows, &desc, &src, &tgt)) return false;
  Engine& e = Engine::Default();
  pvlm_descset* set = nullptr;
  e.Check(pvlm_descset_create(e.ctx(), (int)frames.size(), rows.data(), 128, desc.data(), &set), "pvlm_descset_create");
  struct Release { pvlm_ctx* c; pvlm_descset* s; ~Release() { pvlm_descset_destroy(c, s); } } release{e.ctx(), set};
  long long capacity = 0, needed = 0;
  for (int s : src) capacity += rows[(size_t)s];
  std::vector<unsigned char> keep(image_pairs.size()); std::vector<long long> off(image_pairs.size() + 1, 0); std::vector<pvlm_match> rec((size_t)std::max<long long>(capacity, 1));
  e.Check(pvlm_match_pairs(e.ctx(), set, (int)image_pairs.size(), src.data(), tgt.data(), ratio, matches_threshold, 0, keep.data(), off.data(), rec.data(), capacity, &needed,
                           nullptr), "pvlm_match_pairs");
  std::vector<MatchPair> good_pair;
  for (size_t p = 0; p < image_pairs.size(); ++p) {
    if (!keep[p]) continue;
    MatchPair g; g.image_pair = image_pairs[p].image_pair;
    for (long long k = off[p]; k < off[p + 1]; ++k) g.matches.push_back({rec[(size_t)k].query, rec[(size_t)k].train});
    good_pair.push_back(std::move(g));
  }
  good_pair.swap(image_pairs);
  return true;
}

bool MatchImagePairsHost(const std::vector<Frame>& frames, std::vector<MatchPair>& image_pairs, const float ratio, const int matches_threshold, const int num_threads) {
  std::vector<int> rows, src, tgt; std::vector<const float*> desc;
  if (!PairLists(frames, image_pairs, &rows, &desc, &src, &tgt)) return false;
  std::vector<unsigned char> keep; std::vector<std::vector<match_detail::Match>> matches;
  if (match_detail::MatchPairsHost((int)frames.size(), desc.data(), rows.data(), (int)image_pairs.size(), src.data(), tgt.data(), ratio, matches_threshold,
                                   (size_t)std::max(num_threads, 1), keep, matches)) return false;
  std::vector<MatchPair> good_pair;
  for (size_t p = 0; p < image_pairs.size(); ++p) {
    if (!keep[p]) continue;
    MatchPair g; g.image_pair = image_pairs[p].image_pair;
    for (const match_detail::Match& m : matches[p]) g.matches.push_back({m.query, m.train});
    good_pair.push_back(std::move(g));
  }
  good_pair.swap(image_pairs);
  return true;
}

// ---- K35 --------------------------------------------------------------------------------------------------------------------------------
namespace {
bool DescLists(const std::vector<Frame>& frames, std::vector<int>* rows, std::vector<const float*>* desc) {
  for (const Frame& f : frames) {
    if (f.descriptor.size() != 128 * f.keypoints.size()) return false;
    rows->push_back((int)f.keypoints.size()); desc->push_back(f.descriptor.data());
  }
  return true;
}
}  // namespace

VLADMatcher::VLADMatcher(const std::vector<Frame>& frames, const int normalization_type, const unsigned long long seed, const bool host, const int num_threads, pvlm_descset* set)
    : frames_(frames), normalization_type_(normalization_type), num_threads_(std::max(num_threads, 1)), seed_(seed), host_(host), set_(set) {
  std::vector<int> rows; std::vector<const float*> desc;
  valid_ = DescLists(frames, &rows, &desc);
  if (!valid_ || host_ || set_) return;
  Engine& e = Engine::Default();
  e.Check(pvlm_descset_create(e.ctx(), (int)frames.size(), rows.data(), 128, desc.data(), &set_), "pvlm_descset_create");
  own_set_ = true;
}

VLADMatcher::~VLADMatcher() {
  if (!vlad_ && !own_set_) return;
  Engine& e = Engine::Default();
  if (vlad_) pvlm_vladset_destroy(e.ctx(), vlad_);
  if (own_set_) pvlm_descset_destroy(e.ctx(), set_);
}

bool VLADMatcher::GenerateCodeBook(float ratio, const int book_size, const int max_iteration) {
  if (!valid_ || ratio > 1 || ratio < 0) return false;
  std::vector<int> rows; std::vector<const float*> desc;
  DescLists(frames_, &rows, &desc);
  vlad_detail::Rng rng(seed_);
  std::vector<int> train;
  if (ratio < 1) for (long long f : vlad_detail::DrawDistinct((long long)(ratio * frames_.size()), (long long)frames_.size(), rng)) train.push_back((int)f);
  else for (size_t f = 0; f < frames_.size(); ++f) train.push_back((int)f);
  long long n = 0;
  for (int f : train) n += rows[(size_t)f];
  if (book_size < 1 || book_size > n) return false;
  const std::vector<long long> init = vlad_detail::DrawDistinct(book_size, n, rng);
  codebook_.assign((size_t)book_size * 128, 0.0f); alive_.assign((size_t)book_size, 0); book_size_ = book_size;
  if (host_)
    return vlad_detail::KmeansHost((int)frames_.size(), desc.data(), rows.data(), (int)train.size(), train.data(), book_size, max_iteration, init.data(), (size_t)num_threads_,
                                   codebook_.data(), alive_.data(), nullptr, nullptr, nullptr) == 0;
  Engine& e = Engine::Default();
  e.Check(pvlm_vlad_kmeans(e.ctx(), set_, (int)train.size(), train.data(), book_size, max_iteration, init.data(), 0, codebook_.data(), alive_.data(), nullptr, nullptr),
          "pvlm_vlad_kmeans");
  return true;
}

bool VLADMatcher::ComputeVLADEmbedding() {
  if (!valid_ || frames_.empty() || codebook_.empty()) return false;
  if (host_) {
    std::vector<int> rows; std::vector<const float*> desc;
    DescLists(frames_, &rows, &desc);
    host_vlad_.assign(frames_.size() * (size_t)book_size_ * 128, 0.0f);
    return vlad_detail::EmbedHost((int)frames_.size(), desc.data(), rows.data(), book_size_, codebook_.data(), alive_.data(), normalization_type_, (size_t)num_threads_,
                                  host_vlad_.data()) == 0;
  }
  Engine& e = Engine::Default();
  if (vlad_) { pvlm_vladset_destroy(e.ctx(), vlad_); vlad_ = nullptr; }
  e.Check(pvlm_vlad_embed(e.ctx(), set_, book_size_, codebook_.data(), alive_.data(), normalization_type_, 0, &vlad_, nullptr), "pvlm_vlad_embed");
  return true;
}

std::vector<std::vector<size_t>> VLADMatcher::FindNeighbors(int neighbor_size) {
  const size_t n = frames_.size();
  std::vector<std::vector<size_t>> all(n);
  if (neighbor_size < 1 || n == 0 || (host_ ? host_vlad_.empty() : !vlad_)) return all;
  const size_t m = std::min((size_t)neighbor_size, n);
  std::vector<int> nb(n * m);
  if (host_) vlad_detail::NeighborsHost(host_vlad_.data(), (int)n, book_size_, neighbor_size, (size_t)num_threads_, nb.data(), nullptr);
  else { Engine& e = Engine::Default(); e.Check(pvlm_vlad_neighbors(e.ctx(), vlad_, neighbor_size, nb.data(), nullptr), "pvlm_vlad_neighbors"); }
  for (size_t i = 0; i < n; ++i) all[i].assign(nb.begin() + (long)(i * m), nb.begin() + (long)((i + 1) * m));
  return all;
}

namespace {
bool InitImagePairsWith(const std::vector<Frame>& frames, const int frame_match_type, std::vector<MatchPair>& image_pairs, const unsigned long long seed, const int book_size,
                        const bool host, const int num_threads) {
  if (frame_match_type & (GPS | GPS_VLAD)) return false;
  for (const Frame& f : frames) if (f.descriptor.size() != 128 * f.keypoints.size()) return false;
  const size_t n = frames.size();
  std::vector<MatchPair> out;
  auto push = [&out](size_t i, size_t j) { MatchPair p; p.image_pair = {i, j}; out.push_back(std::move(p)); };
  if (frame_match_type & EXHAUSTIVE) {
    for (size_t i = 0; i < n; ++i) for (size_t j = i + 1; j < n; ++j) push(i, j);
    image_pairs.swap(out);
    return image_pairs.size() > 0;
  }
  std::set<std::pair<size_t, size_t>> pairs;
  if (frame_match_type & CONTIGUOUS) {
    const size_t neighbor_size = 20;
    for (size_t i = 0; i < n; ++i)
      for (size_t j = i + 1; j < i + neighbor_size && j < n; ++j) { push(i, j); pairs.insert({i, j}); }
  }
  if (frame_match_type & VLAD) {
    const int neighbor_size = std::max((int)(n / 40), 15);
    VLADMatcher vlad(frames, RESIDUAL_NORMALIZATION_PWR_LAW, seed, host, num_threads);
    if (!vlad.GenerateCodeBook(0.5f, book_size) || !vlad.ComputeVLADEmbedding()) return false;
    const std::vector<std::vector<size_t>> neighbors_all = vlad.FindNeighbors(neighbor_size);
    for (size_t i = 0; i < n; ++i)
      for (const size_t neighbor : neighbors_all[i]) {
        if (neighbor == i) continue;
        const size_t min_id = std::min(i, neighbor), max_id = std::max(i, neighbor);
        if (pairs.count({min_id, max_id}) == 0) { push(min_id, max_id); pairs.insert({min_id, max_id}); }
      }
  }
  image_pairs.swap(out);
  return image_pairs.size() > 0;
}
}  // namespace

bool InitImagePairs(const std::vector<Frame>& frames, const int frame_match_type, std::vector<MatchPair>& image_pairs, const unsigned long long seed, const int book_size) {
  StageTimer stage_timer_("InitImagePairs");
  return InitImagePairsWith(frames, frame_match_type, image_pairs, seed, book_size, false, 16);
}

bool InitImagePairsHost(const std::vector<Frame>& frames, const int frame_match_type, std::vector<MatchPair>& image_pairs, const unsigned long long seed, const int book_size,
                        const int num_threads) {
  return InitImagePairsWith(frames, frame_match_type, image_pairs, seed, book_size, true, num_threads);
}

// ---- K34 --------------------------------------------------------------------------------------------------------------------------------
Matrix3d ComputeEssential(const std::vector<std::array<float, 3>>& points1, const std::vector<std::array<float, 3>>& points2) {
  if (points1.size() != points2.size()) throw std::invalid_argument("ComputeEssential: list sizes differ");   // upstream asserts
  Matrix3d E;
  pvlm_essential::compute_essential(points1.empty() ? nullptr : points1[0].data(), points2.empty() ? nullptr : points2[0].data(), (int)points1.size(), E.data());
  return E;
}

bool DecomposeEssential(const Matrix3d& E_21, std::vector<Matrix3d>& rotations, std::vector<Vector3d>& translations) {
  double R[36], t[12];
  pvlm_essential::decompose(E_21.data(), R, t);
  rotations.assign(4, Matrix3d()); translations.assign(4, Vector3d());
  for (int j = 0; j < 4; ++j) { std::copy(R + 9 * j, R + 9 * j + 9, rotations[(size_t)j].begin()); std::copy(t + 3 * j, t + 3 * j + 3, translations[(size_t)j].begin()); }
  return true;
}

Matrix3d FindEssentialACRANSAC(const std::vector<DMatch>& matches, const std::vector<std::array<float, 3>>& points1, const std::vector<std::array<float, 3>>& points2,
                               const int max_iterations, std::vector<size_t>& inlier_idx, const std::pair<size_t, size_t>& image_pair, const int run,
                               const EssentialOptions& options) {
  Matrix3d E{}; inlier_idx.clear();
  const int n = (int)matches.size();
  if (n <= pvlm_essential::kMinSample || max_iterations < 1) return E;
  std::vector<pvlm_essential::Match> m((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (matches[(size_t)i].queryIdx < 0 || (size_t)matches[(size_t)i].queryIdx >= points1.size() || matches[(size_t)i].trainIdx < 0 || (size_t)matches[(size_t)i].trainIdx >= points2.size())
      throw std::invalid_argument("FindEssentialACRANSAC: a match names a keypoint that is not there");
    m[(size_t)i] = pvlm_essential::Match{matches[(size_t)i].queryIdx, matches[(size_t)i].trainIdx, matches[(size_t)i].distance};
  }
  std::vector<double> tab(2 + 2 * ((size_t)n + 1));
  pvlm_essential::nfa_tables(n, tab.data());
  pvlm_essential::ChainResult ch;
  pvlm_essential::run_chain(points1[0].data(), points2[0].data(), m.data(), n, tab.data(), options.seed, (int)image_pair.first, (int)image_pair.second, run, max_iterations,
                            options.fresh_sample ? pvlm_essential::kFreshSample : 0u, ch);
  std::copy(ch.E, ch.E + 9, E.begin());
  inlier_idx.assign(ch.inliers.begin(), ch.inliers.end());
  return E;
}

int CheckRT(const Matrix3d& R_21, const Vector3d& t_21, const std::vector<bool>& is_inlier, const std::vector<DMatch>& matches, const std::vector<std::array<float, 3>>& keypoints1,
            const std::vector<std::array<float, 3>>& keypoints2, std::vector<Vector3d>& triangulated_points, std::vector<size_t>& inlier_idx) {
  if (is_inlier.size() != matches.size()) throw std::invalid_argument("CheckRT: is_inlier and matches differ in size");   // upstream asserts
  double cos_reject;
  if (!essential_detail::CosReject(&cos_reject)) throw std::runtime_error("CheckRT: this libm's acos is not monotone around 3 degrees");
  triangulated_points.clear(); inlier_idx.clear();
  for (size_t i = 0; i < matches.size(); ++i) {
    if (!is_inlier[i]) continue;
    Vector3d P;
    if (pvlm_essential::check_point(R_21.data(), t_21.data(), keypoints1.at((size_t)matches[i].queryIdx).data(), keypoints2.at((size_t)matches[i].trainIdx).data(), cos_reject, P.data())) {
      triangulated_points.push_back(P); inlier_idx.push_back(i);
    }
  }
  return (int)inlier_idx.size();
}

namespace {
// the inputs of the two K34 loops: bearings of every keypoint (eq.ImageToCam(kp.pt), the cv::Point2i overload as everywhere in the SfM stage), pair and match lists
struct EssentialInputs {
  std::vector<std::vector<float>> bearings; std::vector<const float*> ptr; std::vector<int> rows, src, tgt; std::vector<long long> off; std::vector<pvlm_match> matches;
  bool Fill(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs) {
    bearings.resize(frames.size());
    for (size_t f = 0; f < frames.size(); ++f) {
      const Frame& fr = frames[f];
      bearings[f].resize(3 * fr.keypoints.size() + 3);
      for (size_t k = 0; k < fr.keypoints.size(); ++k) pvlm_sfm_filter::image_to_cam_point2i(fr.rows, fr.cols, fr.keypoints[k][0], fr.keypoints[k][1], bearings[f].data() + 3 * k);
      ptr.push_back(bearings[f].data()); rows.push_back((int)fr.keypoints.size());
    }
    off.push_back(0);
    for (const MatchPair& p : image_pairs) {
      if (p.image_pair.first >= frames.size() || p.image_pair.second >= frames.size()) return false;
      src.push_back((int)p.image_pair.first); tgt.push_back((int)p.image_pair.second);
      for (const auto& m : p.matches) {
        if (m.first < 0 || m.first >= rows[p.image_pair.first] || m.second < 0 || m.second >= rows[p.image_pair.second]) return false;
        matches.push_back(pvlm_match{m.first, m.second, 0.0f});
      }
      off.push_back((long long)matches.size());
    }
    return true;
  }
};
RelativePair MakeRelativePair(const MatchPair& p, const double* R, const double* t, const int* idx, const double* tri, long long count) {
  RelativePair g; g.image_pair = p.image_pair; g.matches = p.matches;
  std::copy(R, R + 9, g.R_21.begin()); std::copy(t, t + 3, g.t_21.begin());
  for (long long k = 0; k < count; ++k) { g.inlier_idx.push_back((size_t)idx[k]); g.triangulated.push_back(Vector3d{tri[3 * k], tri[3 * k + 1], tri[3 * k + 2]}); }
  return g;
}
}  // namespace

bool FilterImagePairs(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<RelativePair>& good_pair, const int triangulation_num_threshold,
                      const EssentialOptions& options) {
  StageTimer stage_timer_("FilterImagePairs");
  EssentialInputs in;
  if (!in.Fill(frames, image_pairs)) return false;
  Engine& e = Engine::Default();
  const size_t np = image_pairs.size();
  const long long capacity = (long long)in.matches.size();
  long long needed = 0;
  std::vector<unsigned char> keep(np); std::vector<double> R(9 * np + 9), t(3 * np + 3), tri(3 * (size_t)capacity + 3); std::vector<long long> off(np + 1, 0);
  std::vector<int> idx((size_t)capacity + 1);
  const pvlm_essential_params prm{options.n_runs, options.max_iterations, triangulation_num_threshold, options.seed};
  e.Check(pvlm_filter_image_pairs(e.ctx(), (int)frames.size(), in.ptr.data(), in.rows.data(), (int)np, in.src.data(), in.tgt.data(), in.off.data(), in.matches.data(), &prm,
                                  options.fresh_sample ? PVLM_FLAG_ESSENTIAL_FRESH_SAMPLE : 0u, keep.data(), R.data(), t.data(), off.data(), idx.data(), tri.data(), capacity, &needed,
                                  nullptr), "pvlm_filter_image_pairs");
  good_pair.clear();
  for (size_t p = 0; p < np; ++p)
    if (keep[p]) good_pair.push_back(MakeRelativePair(image_pairs[p], R.data() + 9 * p, t.data() + 3 * p, idx.data() + off[p], tri.data() + 3 * off[p], off[p + 1] - off[p]));
  return true;
}

bool FilterImagePairsHost(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<RelativePair>& good_pair, const int triangulation_num_threshold,
                          const EssentialOptions& options, const int num_threads) {
  EssentialInputs in;
  if (!in.Fill(frames, image_pairs)) return false;
  static_assert(sizeof(pvlm_match) == sizeof(pvlm_essential::Match), "the match record of the core is the ABI's");
  std::vector<pvlm_essential::PairResult> res;
  if (essential_detail::FilterPairsHost((int)frames.size(), in.ptr.data(), in.rows.data(), (int)image_pairs.size(), in.src.data(), in.tgt.data(), in.off.data(),
                                        reinterpret_cast<const pvlm_essential::Match*>(in.matches.data()), options.n_runs, options.max_iterations, triangulation_num_threshold,
                                        options.seed, options.fresh_sample ? pvlm_essential::kFreshSample : 0u, (size_t)std::max(num_threads, 1), res)) return false;
  good_pair.clear();
  for (size_t p = 0; p < image_pairs.size(); ++p)
    if (res[p].keep) good_pair.push_back(MakeRelativePair(image_pairs[p], res[p].R, res[p].t, res[p].inlier_idx.data(), res[p].triangulated.data(), (long long)res[p].inlier_idx.size()));
  return true;
}

// ================================================================================================
// K36: RefineRelativePose, SetTranslationScaleDepthMap, LargestBiconnectedGraph, FilterImagePairsFull
// ================================================================================================
namespace {
int RelposeKind(int residual_type) {
  if (residual_type == PIXEL_RESIDUAL) return pvlm_relpose::kKindPixel;
  if (residual_type == ANGLE_RESIDUAL_2) return pvlm_relpose::kKindAngle2;
  throw std::invalid_argument("SfMLocalBA: PIXEL_RESIDUAL or ANGLE_RESIDUAL_2 (ANGLE_RESIDUAL_1 is not implemented for the two-view adjustment)");
}
// the arrays of pvlm_refine_relative_poses from a pair list
struct RelposeInputs {
  std::vector<std::vector<float>> kp; std::vector<const float*> ptr; std::vector<int> rows_kp, img_rows, img_cols, src, tgt, idx; std::vector<long long> moff, ioff;
  std::vector<pvlm_match> matches; std::vector<double> R, t, tri;
  bool Fill(const std::vector<Frame>& frames, const std::vector<RelativePair>& pairs) {
    for (const Frame& fr : frames) {
      kp.emplace_back(2 * fr.keypoints.size() + 2);
      for (size_t k = 0; k < fr.keypoints.size(); ++k) { kp.back()[2 * k] = fr.keypoints[k][0]; kp.back()[2 * k + 1] = fr.keypoints[k][1]; }
      rows_kp.push_back((int)fr.keypoints.size()); img_rows.push_back(fr.GetImageRows()); img_cols.push_back(fr.GetImageCols());
    }
    for (const auto& v : kp) ptr.push_back(v.data());
    moff.push_back(0); ioff.push_back(0);
    for (const RelativePair& p : pairs) {
      if (p.image_pair.first >= frames.size() || p.image_pair.second >= frames.size() || p.inlier_idx.size() != p.triangulated.size()) return false;
      src.push_back((int)p.image_pair.first); tgt.push_back((int)p.image_pair.second);
      for (const auto& m : p.matches) matches.push_back(pvlm_match{m.first, m.second, 0.0f});
      moff.push_back((long long)matches.size());
      for (size_t k = 0; k < p.inlier_idx.size(); ++k) { idx.push_back((int)p.inlier_idx[k]); tri.insert(tri.end(), p.triangulated[k].begin(), p.triangulated[k].end()); }
      ioff.push_back((long long)idx.size());
      R.insert(R.end(), p.R_21.begin(), p.R_21.end()); t.insert(t.end(), p.t_21.begin(), p.t_21.end());
    }
    matches.push_back(pvlm_match{0, 0, 0.0f}); idx.push_back(0); tri.resize(tri.size() + 3); R.resize(R.size() + 9); t.resize(t.size() + 3);   // never empty
    return true;
  }
  void Store(std::vector<RelativePair>& pairs) const {
    for (size_t p = 0; p < pairs.size(); ++p) {
      std::copy(R.begin() + 9 * (std::ptrdiff_t)p, R.begin() + 9 * (std::ptrdiff_t)p + 9, pairs[p].R_21.begin());
      std::copy(t.begin() + 3 * (std::ptrdiff_t)p, t.begin() + 3 * (std::ptrdiff_t)p + 3, pairs[p].t_21.begin());
      for (size_t k = 0; k < pairs[p].triangulated.size(); ++k)
        for (int c = 0; c < 3; ++c) pairs[p].triangulated[k][(size_t)c] = tri[3 * ((size_t)ioff[p] + k) + (size_t)c];
    }
  }
};
relpose_detail::TailPair ToTail(const RelativePair& p, size_t tag) {
  relpose_detail::TailPair t;
  t.image_pair = p.image_pair; t.tag = tag; t.points_with_depth = p.points_with_depth; t.upper_scale = p.upper_scale; t.lower_scale = p.lower_scale;
  std::copy(p.R_21.begin(), p.R_21.end(), t.R); std::copy(p.t_21.begin(), p.t_21.end(), t.t);
  for (const Vector3d& X : p.triangulated) t.tri.insert(t.tri.end(), X.begin(), X.end());
  return t;
}
void FromTail(const relpose_detail::TailPair& t, RelativePair& p) {
  std::copy(t.t, t.t + 3, p.t_21.begin());
  for (size_t k = 0; k < p.triangulated.size(); ++k) p.triangulated[k] = {t.tri[3 * k], t.tri[3 * k + 1], t.tri[3 * k + 2]};
  p.points_with_depth = t.points_with_depth; p.upper_scale = t.upper_scale; p.lower_scale = t.lower_scale;
}
std::vector<relpose_detail::DepthView> DepthViews(const std::vector<Frame>& frames, const DepthMaps& d) {
  std::vector<relpose_detail::DepthView> v(frames.size());
  for (size_t f = 0; f < frames.size() && f < d.maps.size(); ++f) {
    if (d.maps[f].empty()) continue;
    if (f >= d.rows.size() || f >= d.cols.size() || d.rows[f] <= 0 || d.cols[f] <= 0 || d.maps[f].size() != (size_t)d.rows[f] * (size_t)d.cols[f])
      throw std::invalid_argument("DepthMaps: map " + std::to_string(f) + " is not rows x cols");
    v[f].data = d.maps[f].data(); v[f].rows = d.rows[f]; v[f].cols = d.cols[f];
  }
  return v;
}
// :449-476 on the pairs the refinement leaves
void FinishImagePairs(const std::vector<Frame>& frames, const DepthMaps& depth_maps, std::vector<RelativePair>& good_pair, std::set<size_t>& covered_frames, bool keep_no_scale) {
  std::vector<relpose_detail::TailPair> tail;
  for (size_t p = 0; p < good_pair.size(); ++p) tail.push_back(ToTail(good_pair[p], p));
  std::vector<int> frame_rows;
  for (const Frame& f : frames) frame_rows.push_back(f.GetImageRows());
  relpose_detail::FinishPairs(frames.empty() ? 0 : frames[0].GetImageRows(), frames.empty() ? 0 : frames[0].GetImageCols(), frame_rows, DepthViews(frames, depth_maps), tail,
                              covered_frames, keep_no_scale);
  std::vector<RelativePair> out;
  for (const relpose_detail::TailPair& t : tail) { out.push_back(good_pair[t.tag]); FromTail(t, out.back()); }
  good_pair.swap(out);
}
}  // namespace

bool RefineRelativePosesHost(const std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, int residual_type, std::vector<bool>* ok, const int num_threads) {
  const int kind = RelposeKind(residual_type);
  RelposeInputs in;
  if (!in.Fill(frames, image_pairs)) return false;
  std::vector<unsigned char> good(image_pairs.size() + 1);
  if (relpose_detail::RefinePosesHost((int)frames.size(), in.ptr.data(), in.rows_kp.data(), in.img_rows.data(), in.img_cols.data(), (int)image_pairs.size(), in.src.data(),
                                      in.tgt.data(), in.moff.data(), in.matches.data(), in.ioff.data(), in.idx.data(), in.R.data(), in.t.data(), in.tri.data(), kind, 50,
                                      (size_t)std::max(num_threads, 1), good.data(), nullptr, nullptr)) return false;
  in.Store(image_pairs);
  if (ok) { ok->assign(image_pairs.size(), false); for (size_t p = 0; p < image_pairs.size(); ++p) (*ok)[p] = good[p] != 0; }
  return true;
}

bool RefineRelativePoses(const std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, int residual_type, std::vector<bool>* ok) {
  StageTimer stage_timer_("RefineRelativePoses");
  const int kind = RelposeKind(residual_type);
  RelposeInputs in;
  if (!in.Fill(frames, image_pairs)) return false;
  Engine& e = Engine::Default();
  std::vector<unsigned char> good(image_pairs.size() + 1);
  const pvlm_relpose_params prm{(pvlm_ba_kind)kind, 50};
  const pvlm_status st = pvlm_refine_relative_poses(e.ctx(), (int)frames.size(), in.ptr.data(), in.rows_kp.data(), in.img_rows.data(), in.img_cols.data(), (int)image_pairs.size(),
                                                    in.src.data(), in.tgt.data(), in.moff.data(), in.matches.data(), in.ioff.data(), in.idx.data(), in.R.data(), in.t.data(),
                                                    in.tri.data(), &prm, good.data(), nullptr);
  if (st == PVLM_ERR_ARG) return false;
  e.Check(st, "pvlm_refine_relative_poses");
  in.Store(image_pairs);
  if (ok) { ok->assign(image_pairs.size(), false); for (size_t p = 0; p < image_pairs.size(); ++p) (*ok)[p] = good[p] != 0; }
  return true;
}

bool SfMLocalBA(const Frame& frame1, const Frame& frame2, int residual_type, RelativePair& image_pair) {
  std::vector<RelativePair> one{image_pair};
  one[0].image_pair = {0, 1};
  std::vector<bool> ok;
  if (!RefineRelativePosesHost({frame1, frame2}, one, residual_type, &ok, 1)) return false;
  one[0].image_pair = image_pair.image_pair;
  image_pair = one[0];
  return ok[0];
}

bool RefineRelativePose(const std::vector<Frame>& frames, RelativePair& image_pair) {
  return SfMLocalBA(frames.at(image_pair.image_pair.first), frames.at(image_pair.image_pair.second), PIXEL_RESIDUAL, image_pair);
}

bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DepthMaps& depth_maps, RelativePair& image_pair) {
  const std::vector<relpose_detail::DepthView> dv = DepthViews(frames, depth_maps);
  relpose_detail::TailPair t = ToTail(image_pair, 0);
  const bool ok = relpose_detail::SetScaleOne(frames.at(0).GetImageRows(), frames.at(0).GetImageCols(), frames.at(image_pair.image_pair.first).GetImageRows(),
                                              dv.at(image_pair.image_pair.first), dv.at(image_pair.image_pair.second), t);
  FromTail(t, image_pair);
  return ok;
}

bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DepthMaps& depth_maps, std::vector<RelativePair>& image_pairs, const bool keep_no_scale) {
  std::vector<relpose_detail::TailPair> tail;
  for (size_t p = 0; p < image_pairs.size(); ++p) {
    if (image_pairs[p].image_pair.first >= frames.size() || image_pairs[p].image_pair.second >= frames.size()) throw std::invalid_argument("SetTranslationScaleDepthMap: a pair names a frame that is not there");
    tail.push_back(ToTail(image_pairs[p], p));
  }
  std::vector<int> frame_rows;
  for (const Frame& f : frames) frame_rows.push_back(f.GetImageRows());
  const bool any = relpose_detail::SetScaleList(frames.empty() ? 0 : frames[0].GetImageRows(), frames.empty() ? 0 : frames[0].GetImageCols(), frame_rows, DepthViews(frames, depth_maps),
                                                tail, keep_no_scale);
  std::vector<RelativePair> out;
  for (const relpose_detail::TailPair& t : tail) { out.push_back(image_pairs[t.tag]); FromTail(t, out.back()); }
  image_pairs.swap(out);
  return any;
}

std::vector<RelativePair> LargestBiconnectedGraph(const std::vector<RelativePair>& pairs, std::set<size_t>& nodes) {
  std::vector<std::pair<size_t, size_t>> edges;
  for (const RelativePair& p : pairs) edges.push_back(p.image_pair);
  nodes = relpose_detail::LargestEdgeBiconnected(edges);
  std::vector<RelativePair> good;
  for (const RelativePair& p : pairs) if (nodes.count(p.image_pair.first) > 0 && nodes.count(p.image_pair.second) > 0) good.push_back(p);
  return good;
}

bool FilterImagePairsFull(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                          std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale, const EssentialOptions& options) {
  if (!FilterImagePairs(frames, image_pairs, good_pair, triangulation_num_threshold, options)) return false;
  if (!RefineRelativePoses(frames, good_pair, PIXEL_RESIDUAL, nullptr)) return false;
  FinishImagePairs(frames, depth_maps, good_pair, covered_frames, keep_no_scale);
  return true;
}

bool FilterImagePairsFullHost(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                              std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale, const EssentialOptions& options,
                              const int num_threads) {
  if (!FilterImagePairsHost(frames, image_pairs, good_pair, triangulation_num_threshold, options, num_threads)) return false;
  if (!RefineRelativePosesHost(frames, good_pair, PIXEL_RESIDUAL, nullptr, num_threads)) return false;
  FinishImagePairs(frames, depth_maps, good_pair, covered_frames, keep_no_scale);
  return true;
}

bool EstimateStructure(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<PointTrack>& structure) {
  structure = TriangulateTracks(frames, image_pairs);
  return structure.size() > 0;
}

bool CameraLidarOptimizer::EstimateStructure(const std::vector<MatchPair>& image_pairs) {
  StageTimer stage_timer_("EstimateStructure");
  return structure_detail::EstimateStructureWith(DeviceKernels(), frames, image_pairs, structure);
}

// ================================================================================================
// K37: DepthCompletion, ComputeDepthImage
// ================================================================================================
std::vector<float> DepthCompletion(const std::vector<float>& image, const int rows, const int cols, const float max_depth) {
  if (rows <= 0 || cols <= 0 || image.size() != (size_t)rows * (size_t)cols) throw std::invalid_argument("DepthCompletion: the image is not rows x cols");
  if (!std::isfinite(max_depth) || !(max_depth > 0.f)) throw std::invalid_argument("DepthCompletion: max_depth must be finite and > 0");
  for (float v : image) if (!pvlm_depthfill::input_ok(v)) throw std::invalid_argument("DepthCompletion: a depth is negative or not finite");
  std::vector<float> dense(image.size());
  pvlm_depthfill::complete_host(rows, cols, image.data(), max_depth, dense.data(), nullptr);
  return dense;
}

namespace {
// the arrays of pvlm_compute_depth_images from the scans, and the result as DepthMaps
struct DepthImageCall {
  int rows, cols;
  std::vector<long long> first; std::vector<float> xyz; std::vector<uint16_t> out;
  DepthImageCall(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, int image_rows, int image_cols, float max_depth, bool half_size, bool host_maps = true) {
    if (clouds.size() != frames.size()) throw std::invalid_argument("ComputeDepthImage: lidars.size() != frames.size()");
    if (image_rows <= 0 || image_cols <= 0 || !std::isfinite(max_depth) || !(max_depth > 0.f)) throw std::invalid_argument("ComputeDepthImage: image size or max_depth");
    rows = half_size ? (image_rows + 1) / 2 : image_rows; cols = half_size ? (image_cols + 1) / 2 : image_cols;
    first.push_back(0);
    for (const PointCloud& c : clouds) {
      for (const PointXYZI& p : c) { xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z); }
      first.push_back((long long)(xyz.size() / 3));
    }
    xyz.resize(xyz.size() + 3);                                                // never empty
    if (host_maps) out.resize(clouds.size() * (size_t)rows * (size_t)cols + 1);
  }
  DepthMaps Maps() const {
    DepthMaps d;
    const size_t n = (size_t)rows * (size_t)cols;
    for (size_t f = 0; f + 1 < first.size(); ++f) { d.maps.emplace_back(out.begin() + (std::ptrdiff_t)(f * n), out.begin() + (std::ptrdiff_t)((f + 1) * n)); d.rows.push_back(rows); d.cols.push_back(cols); }
    return d;
  }
};
}  // namespace

DepthMaps ComputeDepthImage(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows, const int image_cols,
                            const float max_depth, const bool half_size) {
  StageTimer stage_timer_("ComputeDepthImage");
  DepthImageCall call(frames, clouds, image_rows, image_cols, max_depth, half_size);
  Engine& e = Engine::Default();
  e.Check(pvlm_compute_depth_images(e.ctx(), call.rows, call.cols, (int)clouds.size(), call.first.data(), call.xyz.data(), T_cl.data(), 4u, max_depth, call.out.data(), nullptr),
          "pvlm_compute_depth_images");
  return call.Maps();
}

DepthMaps ComputeDepthImageHost(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows, const int image_cols,
                                const float max_depth, const bool half_size, const int num_threads) {
  DepthImageCall call(frames, clouds, image_rows, image_cols, max_depth, half_size);
  pvlm_depthfill::depth_images_host(call.rows, call.cols, (int)clouds.size(), call.first.data(), call.xyz.data(), T_cl.data(), 4u, max_depth, call.out.data(),
                                    (size_t)std::max(num_threads, 1));
  return call.Maps();
}

// ================================================================================================
// K39: resident depth maps, SetTranslationScaleDepthMap on the device
// ================================================================================================
DeviceDepthMaps::~DeviceDepthMaps() { if (set_) pvlm_depthset_destroy(Engine::Default().ctx(), set_); }
DeviceDepthMaps& DeviceDepthMaps::operator=(DeviceDepthMaps&& o) noexcept {
  if (this != &o) { if (set_) pvlm_depthset_destroy(Engine::Default().ctx(), set_); set_ = o.set_; n_frames_ = o.n_frames_; o.set_ = nullptr; o.n_frames_ = 0; }
  return *this;
}
std::pair<int, int> DeviceDepthMaps::Info(size_t frame) const {
  int r = 0, c = 0;
  if (!set_ || frame >= n_frames_ || pvlm_depthset_info(set_, (int)frame, &r, &c) != PVLM_OK) throw std::invalid_argument("DeviceDepthMaps: frame " + std::to_string(frame) + " is not there");
  return {r, c};
}

DeviceDepthMaps ComputeDepthImageResident(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows,
                                          const int image_cols, const float max_depth, const bool half_size) {
  StageTimer stage_timer_("ComputeDepthImageResident");
  DepthImageCall call(frames, clouds, image_rows, image_cols, max_depth, half_size, false);
  Engine& e = Engine::Default();
  pvlm_depthset* set = nullptr;
  e.Check(pvlm_depthset_compute(e.ctx(), call.rows, call.cols, (int)clouds.size(), call.first.data(), call.xyz.data(), T_cl.data(), 4u, max_depth, &set, nullptr),
          "pvlm_depthset_compute");
  return DeviceDepthMaps(set, clouds.size());
}

DeviceDepthMaps UploadDepthMaps(const DepthMaps& d) {
  Engine& e = Engine::Default();
  pvlm_depthset* set = nullptr;
  e.Check(pvlm_depthset_create(e.ctx(), (int)d.maps.size(), &set), "pvlm_depthset_create");
  DeviceDepthMaps out(set, d.maps.size());
  for (size_t f = 0; f < d.maps.size(); ++f) {
    if (d.maps[f].empty()) continue;
    if (f >= d.rows.size() || f >= d.cols.size() || d.rows[f] <= 0 || d.cols[f] <= 0 || d.maps[f].size() != (size_t)d.rows[f] * (size_t)d.cols[f])
      throw std::invalid_argument("DepthMaps: map " + std::to_string(f) + " is not rows x cols");
    e.Check(pvlm_depthset_upload(e.ctx(), set, (int)f, d.rows[f], d.cols[f], d.maps[f].data()), "pvlm_depthset_upload");
  }
  return out;
}

std::vector<uint16_t> ReadDepthMap(const DeviceDepthMaps& depth_maps, size_t frame, int* rows, int* cols) {
  const std::pair<int, int> rc = depth_maps.Info(frame);
  if (rows) *rows = rc.first;
  if (cols) *cols = rc.second;
  std::vector<uint16_t> out((size_t)rc.first * (size_t)rc.second);
  if (out.empty()) return out;
  Engine& e = Engine::Default();
  e.Check(pvlm_depthset_read(e.ctx(), depth_maps.set(), (int)frame, out.data()), "pvlm_depthset_read");
  return out;
}

bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DeviceDepthMaps& depth_maps, std::vector<RelativePair>& image_pairs, const bool keep_no_scale) {
  StageTimer stage_timer_("SetTranslationScale");
  if (!depth_maps.set() || depth_maps.size() < frames.size()) throw std::invalid_argument("SetTranslationScaleDepthMap: the depth set holds fewer frames than the list");
  std::vector<relpose_detail::TailPair> tail;
  // the arrays of ONE call over the distinct pairs: the first of equal image_pairs is the one upstream's order reaches
  std::map<std::pair<size_t, size_t>, size_t> slot_of;
  std::vector<size_t> slot(image_pairs.size(), (size_t)-1);
  std::vector<int> src, tgt, pwd; std::vector<long long> off{0}; std::vector<double> R, t, tri, up, lo;
  for (size_t p = 0; p < image_pairs.size(); ++p) {
    const RelativePair& rp = image_pairs[p];
    if (rp.image_pair.first >= frames.size() || rp.image_pair.second >= frames.size()) throw std::invalid_argument("SetTranslationScaleDepthMap: a pair names a frame that is not there");
    tail.push_back(ToTail(rp, p));
    if (!slot_of.emplace(rp.image_pair, src.size()).second) continue;
    slot[p] = src.size();
    src.push_back((int)rp.image_pair.first); tgt.push_back((int)rp.image_pair.second);
    const relpose_detail::TailPair& tp = tail.back();
    R.insert(R.end(), tp.R, tp.R + 9); t.insert(t.end(), tp.t, tp.t + 3); tri.insert(tri.end(), tp.tri.begin(), tp.tri.end());
    off.push_back((long long)(tri.size() / 3));
    pwd.push_back(tp.points_with_depth); up.push_back(tp.upper_scale); lo.push_back(tp.lower_scale);
  }
  std::vector<int> frame_rows((size_t)depth_maps.size(), 0);
  for (size_t f = 0; f < frames.size(); ++f) frame_rows[f] = frames[f].GetImageRows();
  const size_t n = src.size();
  std::vector<unsigned char> ok(n + 1, 0);
  R.resize(R.size() + 9); t.resize(t.size() + 3); tri.resize(tri.size() + 3); pwd.push_back(0); up.push_back(0); lo.push_back(0); src.push_back(0); tgt.push_back(0);   // never empty
  if (n > 0) {
    Engine& e = Engine::Default();
    e.Check(pvlm_set_translation_scales(e.ctx(), depth_maps.set(), frames[0].GetImageRows(), frames[0].GetImageCols(), frame_rows.data(), (int)n, src.data(), tgt.data(),
                                        off.data(), R.data(), t.data(), tri.data(), ok.data(), pwd.data(), up.data(), lo.data(), nullptr),
            "pvlm_set_translation_scales");
  }
  const bool any = relpose_detail::SetScaleListWith(frames.size(), tail, keep_no_scale, [&](relpose_detail::TailPair& tp) {
    const size_t k = slot[tp.tag];                       // the first of its image_pair: the only one the order reaches
    std::copy(t.begin() + 3 * (std::ptrdiff_t)k, t.begin() + 3 * (std::ptrdiff_t)k + 3, tp.t);
    std::copy(tri.begin() + 3 * (std::ptrdiff_t)off[k], tri.begin() + 3 * (std::ptrdiff_t)off[k + 1], tp.tri.begin());
    tp.points_with_depth = pwd[k]; tp.upper_scale = up[k]; tp.lower_scale = lo[k];
    return ok[k] != 0;
  });
  std::vector<RelativePair> out;
  for (const relpose_detail::TailPair& tp : tail) { out.push_back(image_pairs[tp.tag]); FromTail(tp, out.back()); }
  image_pairs.swap(out);
  return any;
}

bool FilterImagePairsFull(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DeviceDepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                          std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale, const EssentialOptions& options) {
  if (!FilterImagePairs(frames, image_pairs, good_pair, triangulation_num_threshold, options)) return false;
  if (!RefineRelativePoses(frames, good_pair, PIXEL_RESIDUAL, nullptr)) return false;
  SetTranslationScaleDepthMap(frames, depth_maps, good_pair, keep_no_scale);
  good_pair = LargestBiconnectedGraph(good_pair, covered_frames);
  relpose_detail::SortAsWritten(good_pair, [](const RelativePair& a, const RelativePair& b) { return relpose_detail::PairLessAsWritten(a.image_pair, b.image_pair); });
  return true;
}

// ================================================================================================
// K42: translation averaging — TranslationAveragingDLT / L2 / SoftL1 / L2IRLS (sfm/TranslationAveraging.cpp), ReIndex, SetToOrigin, EstimateGlobalTranslation;
// K44: TranslationAveragingBATA (sfm/TranslationAveraging.cpp:483-525 around sfm/BATA.cpp); K46: TranslationAveragingL2Chordal (:206-274), TranslationAveragingLUD (:527-660)
// ================================================================================================
namespace {
// the arrays of pvlm_transavg_* and pvlm_rotavg_* from a pair list: the pair indices and R_21 always, t_21 for the former, the rotations for the latter
struct PairGraphInputs {
  std::vector<int> first, second; std::vector<double> R, t, rot;
  // false: a pair names a camera past n_cameras
  bool Fill(const std::vector<RelativePair>& pairs, size_t n_cameras, bool with_t = true) {
    for (const RelativePair& p : pairs) {
      if (p.image_pair.first >= n_cameras || p.image_pair.second >= n_cameras) return false;
      first.push_back((int)p.image_pair.first); second.push_back((int)p.image_pair.second);
      R.insert(R.end(), p.R_21.begin(), p.R_21.end());
      if (with_t) t.insert(t.end(), p.t_21.begin(), p.t_21.end());
    }
    first.push_back(0); second.push_back(0); R.resize(R.size() + 9); t.resize(t.size() + 3);   // never empty
    return true;
  }
  // with the rotations instead of t_21; false also when there is no rotation
  bool Fill(const std::vector<RelativePair>& pairs, const std::vector<Matrix3d>& rotations) {
    if (!Fill(pairs, rotations.size(), false)) return false;
    for (const Matrix3d& m : rotations) rot.insert(rot.end(), m.begin(), m.end());
    return !rotations.empty();
  }
  void Read(std::vector<Matrix3d>& rotations) const { for (size_t c = 0; c < rotations.size(); ++c) std::copy(rot.begin() + 9 * c, rot.begin() + 9 * c + 9, rotations[c].begin()); }
};
bool RotationIsZero(const Frame& f) { for (double v : f.R_wc) if (v != 0.0) return false; return true; }
// sensors/Frame.cpp:203-208 on the numbers themselves: the translation finite and the rotation not zero
bool PoseValidAsWritten(const Frame& f) { return std::isfinite(f.t_wc[0]) && std::isfinite(f.t_wc[1]) && std::isfinite(f.t_wc[2]) && !RotationIsZero(f); }
void SetTranslationOf(Frame& f, const Vector3d& t_wc) { f.t_wc = t_wc; f.pose_valid = PoseValidAsWritten(f); }
Vector3d MinusRt(const Matrix3d& R, const Vector3d& t) {       // -R t
  return {-(R[0] * t[0] + R[1] * t[1] + R[2] * t[2]), -(R[3] * t[0] + R[4] * t[1] + R[5] * t[2]), -(R[6] * t[0] + R[7] * t[1] + R[8] * t[2])};
}
bool Say(const TranslationOptions& o, const char* m) { if (o.message) *o.message = m; return false; }
}  // namespace

bool TranslationAveragingDLT(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const bool host) {
  PairGraphInputs in;
  if (!in.Fill(image_pairs, global_translations.size())) return false;      // upstream writes past the matrix here (sfm/SfM.cpp:1183 is the caller that can do it)
  const int F = (int)global_translations.size(), P = (int)image_pairs.size();
  std::vector<double> out(3 * (size_t)F + 3, 0.0);
  int info = 0;
  if (host) { if (transavg_detail::DltHost(F, P, in.first.data(), in.second.data(), in.R.data(), in.t.data(), out.data(), &info)) return false; }
  else { Engine& e = Engine::Default(); e.Check(pvlm_transavg_dlt(e.ctx(), F, P, in.first.data(), in.second.data(), in.R.data(), in.t.data(), out.data(), &info), "pvlm_transavg_dlt"); }
  if (info != 0) return false;
  for (int c = 0; c < F; ++c) global_translations[(size_t)c] = {out[3 * (size_t)c], out[3 * (size_t)c + 1], out[3 * (size_t)c + 2]};
  return true;
}

bool TranslationAveragingL2(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, std::vector<double>& scales, const size_t origin_idx,
                            std::vector<double>& weight, double& costs, const double loss_a, const float upper_scale_ratio, const float lower_scale_ratio, const bool host) {
  PairGraphInputs in;
  const int F = (int)global_translations.size(), P = (int)image_pairs.size();
  if (!in.Fill(image_pairs, global_translations.size()) || scales.size() != image_pairs.size() || weight.size() != image_pairs.size()) return false;
  std::vector<double> x(3 * (size_t)F + 3, 0.0), s(scales), w(weight);
  for (int c = 0; c < F; ++c) for (int k = 0; k < 3; ++k) x[3 * (size_t)c + k] = global_translations[(size_t)c][(size_t)k];
  s.push_back(0.0); w.push_back(0.0);
  pvlm_transavg_summary sum{0, 0, 0, 0, 0};
  if (host) {
    pvlm_pairgraph::Summary hs;
    if (transavg_detail::SolveHost(F, P, in.first.data(), in.second.data(), in.R.data(), in.t.data(), s.data(), (int)origin_idx, x.data(), w.data(), loss_a, upper_scale_ratio,
                                   lower_scale_ratio, 50, &hs)) return false;
    sum.initial_cost = hs.initial_cost; sum.final_cost = hs.final_cost; sum.termination = hs.termination;
  } else {
    Engine& e = Engine::Default();
    const pvlm_transavg_params prm{loss_a, upper_scale_ratio, lower_scale_ratio, 50};
    e.Check(pvlm_transavg_solve(e.ctx(), F, P, in.first.data(), in.second.data(), in.R.data(), in.t.data(), s.data(), (int)origin_idx, x.data(), w.data(), &prm, &sum), "pvlm_transavg_solve");
  }
  if (sum.termination == pvlm_pairgraph::kCostNotFinite || !std::isfinite(sum.final_cost)) return false;       // summary.IsSolutionUsable()
  for (int c = 0; c < F; ++c) global_translations[(size_t)c] = {x[3 * (size_t)c], x[3 * (size_t)c + 1], x[3 * (size_t)c + 2]};
  std::copy(s.begin(), s.begin() + P, scales.begin()); std::copy(w.begin(), w.begin() + P, weight.begin());
  costs = sum.final_cost;
  return true;
}

namespace {
// :176-183, :424-432: the length of t_21, or 1 for a pair that never got a scale
std::vector<double> StartScales(const std::vector<RelativePair>& image_pairs) {
  std::vector<double> scales(image_pairs.size());
  for (size_t i = 0; i < image_pairs.size(); ++i) {
    const Vector3d& t = image_pairs[i].t_21;
    scales[i] = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (image_pairs[i].lower_scale < 0 || image_pairs[i].upper_scale < 0) scales[i] = 1;
  }
  return scales;
}
}  // namespace

bool TranslationAveragingSoftL1(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const double l1_loss_threshold,
                                const float upper_scale_ratio, const float lower_scale_ratio, const bool host) {
  std::vector<double> scales = StartScales(image_pairs), weight(image_pairs.size(), 1.0);
  double costs = 0;
  return TranslationAveragingL2(image_pairs, global_translations, scales, origin_idx, weight, costs, l1_loss_threshold, upper_scale_ratio, lower_scale_ratio, host);
}

bool TranslationAveragingL2IRLS(std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const int num_iteration,
                                const float upper_scale_ratio, const float lower_scale_ratio, const bool host, int* iterations_run) {
  std::vector<double> scales = StartScales(image_pairs), weight(image_pairs.size(), 1.0);
  double curr_cost = 0, last_cost = 0;
  if (iterations_run) *iterations_run = 0;
  for (int iter = 0; iter < num_iteration; ++iter) {
    if (!TranslationAveragingL2(image_pairs, global_translations, scales, origin_idx, weight, curr_cost, 0.01, upper_scale_ratio, lower_scale_ratio, host)) return false;
    if (iterations_run) *iterations_run = iter + 1;
    if (std::fabs(last_cost - curr_cost) / curr_cost < 0.05 || curr_cost < 10) break;       // :443 as written
    last_cost = curr_cost;
    std::vector<RelativePair> good_matches; std::vector<double> good_scales, good_weight;
    for (size_t i = 0; i < scales.size(); ++i) {
      if (scales[i] < 0) continue;
      good_scales.push_back(scales[i]); good_weight.push_back(weight[i]); good_matches.push_back(image_pairs[i]);
    }
    if (good_scales.size() != scales.size()) { good_scales.swap(scales); good_weight.swap(weight); good_matches.swap(image_pairs); }
  }
  return true;
}

bool TranslationAveragingBATA(const std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                              const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const BATAConfig& config, const unsigned long long seed, const bool host,
                              std::vector<double>* start_scales) {
  (void)origin_idx;                                                      // upstream only asserts that its translation is zero (:489)
  const int P = (int)image_pairs.size();
  if (P == 0) return false;
  std::vector<int> first, second; std::vector<double> dir, given, draw((size_t)P), scales((size_t)P);
  size_t max_id = 0, min_id = (size_t)-1;
  for (const RelativePair& pair : image_pairs) {
    const auto it = new_to_old.find(pair.image_pair.first);
    if (it == new_to_old.end() || it->second >= frames.size() || pair.image_pair.first > 0x3fffffff || pair.image_pair.second > 0x3fffffff) return false;
    const Matrix3d& R = frames[it->second].R_wc; const Vector3d& t = pair.t_21;
    const double v[3] = {R[0] * t[0] + R[1] * t[1] + R[2] * t[2], R[3] * t[0] + R[4] * t[1] + R[5] * t[2], R[6] * t[0] + R[7] * t[1] + R[8] * t[2]};      // :496
    double scale = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(scale > 0.0) || !std::isfinite(scale)) return false;
    for (int k = 0; k < 3; ++k) dir.push_back(v[k] / scale);              // sfm/BATA.cpp:195
    if (scale > 0.99 && scale < 1.01) scale = -1;                        // sfm/BATA.cpp:192-193
    given.push_back(scale);
    first.push_back((int)pair.image_pair.first); second.push_back((int)pair.image_pair.second);
    max_id = std::max(max_id, std::max(pair.image_pair.first, pair.image_pair.second)); min_id = std::min(min_id, std::min(pair.image_pair.first, pair.image_pair.second));
  }
  {
    uint64_t st = seed ^ 0xba7a5ca1e5ull;
    auto next = [&st]() { uint64_t z = (st += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); };
    for (int p = 0; p < P; ++p) {
      if (given[(size_t)p] >= 0) { draw[(size_t)p] = 1.0; continue; }    // not read
      double u = 0.0;
      while (u == 0.0) u = std::fabs((double)(next() >> 11) * (2.0 / 9007199254740992.0) - 1.0);
      draw[(size_t)p] = u;
    }
  }
  pvlm_bata::start_scales(P, given.data(), draw.data(), scales.data());
  if (start_scales) *start_scales = scales;
  const int n_cameras = (int)max_id + 1, F = (int)(max_id - min_id) + 1;
  std::vector<double> out(3 * (size_t)n_cameras + 3, 0.0);
  int info = 0;
  if (host) {
    pvlm_bata::Params prm;
    prm.delta = config.delta; prm.init_iteration = config.init_iteration; prm.inner_iteration = config.inner_iteration; prm.outer_iteration = config.outer_iteration;
    prm.robust_threshold = config.robust_threshold;
    if (bata_detail::SolveHost(n_cameras, P, first.data(), second.data(), dir.data(), scales.data(), &prm, out.data(), nullptr, nullptr, &info)) return false;
  } else {
    Engine& e = Engine::Default();
    const pvlm_bata_params prm{config.delta, config.init_iteration, config.inner_iteration, config.outer_iteration, config.robust_threshold};
    e.Check(pvlm_transavg_bata(e.ctx(), n_cameras, P, first.data(), second.data(), dir.data(), scales.data(), &prm, out.data(), nullptr, nullptr, &info), "pvlm_transavg_bata");
  }
  if (info != 0) return false;
  for (int i = 0; i < F; ++i) if (new_to_old.find((size_t)i) == new_to_old.end() || new_to_old.find((size_t)i)->second >= frames.size()) return false;      // :521 reads past the map
  global_translations.assign((size_t)F, Vector3d{0, 0, 0});
  for (int i = 0; i < F; ++i) {
    const Matrix3d& R = frames[new_to_old.find((size_t)i)->second].R_wc;     // R_cw = R_wc^T; t_cw = -R_cw centre (:519-523)
    const double* c = &out[3 * (size_t)i];
    global_translations[(size_t)i] = {-(R[0] * c[0] + R[3] * c[1] + R[6] * c[2]), -(R[1] * c[0] + R[4] * c[1] + R[7] * c[2]), -(R[2] * c[0] + R[5] * c[1] + R[8] * c[2])};
  }
  return true;
}

namespace {
// What the two K46 functions share: the centres t_wc = -R_wc t_cw of every camera (:216-220, :544-548), per pair dir = R_w2 t_21.normalized() (:225-226, :623) and
// the way back, t_cw = -R_cw t_wc (:267-271, :654-658).  false: a camera without a frame, a pair past the cameras, a t_21 without a direction.
struct DirectionInputs {
  std::vector<int> first, second; std::vector<double> dir, centres;
  bool Fill(const std::vector<RelativePair>& pairs, const std::vector<Frame>& frames, const std::vector<Vector3d>& t_cw, const std::map<size_t, size_t>& new_to_old) {
    const size_t F = t_cw.size();
    centres.assign(3 * F + 3, 0.0);
    for (size_t i = 0; i < F; ++i) {
      const auto it = new_to_old.find(i);
      if (it == new_to_old.end() || it->second >= frames.size()) return false;
      const Vector3d c = MinusRt(frames[it->second].R_wc, t_cw[i]);
      for (size_t k = 0; k < 3; ++k) centres[3 * i + k] = c[k];
    }
    first.clear(); second.clear(); dir.clear();
    for (const RelativePair& p : pairs) {
      if (p.image_pair.first >= F || p.image_pair.second >= F) return false;
      const Matrix3d& R = frames[new_to_old.find(p.image_pair.second)->second].R_wc;
      double d[3];
      if (!pvlm_transavg::direction(p.t_21.data(), d)) return false;
      for (int r = 0; r < 3; ++r) dir.push_back(R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
      first.push_back((int)p.image_pair.first); second.push_back((int)p.image_pair.second);
    }
    const bool ok = pvlm_transdir::check_pairs((int)F, (int)pairs.size(), first.data(), second.data(), dir.data()) == nullptr;      // a frame whose R_wc is no rotation
    first.push_back(0); second.push_back(0); dir.resize(dir.size() + 3);      // never empty
    return ok;
  }
  void Read(const std::vector<Frame>& frames, const std::map<size_t, size_t>& new_to_old, std::vector<Vector3d>& t_cw) const {
    for (size_t i = 0; i < t_cw.size(); ++i) {
      const Matrix3d& R = frames[new_to_old.find(i)->second].R_wc; const double* c = &centres[3 * i];
      t_cw[i] = {-(R[0] * c[0] + R[3] * c[1] + R[6] * c[2]), -(R[1] * c[0] + R[4] * c[1] + R[7] * c[2]), -(R[2] * c[0] + R[5] * c[1] + R[8] * c[2])};
    }
  }
};
bool Usable(const pvlm_transdir_summary& s) { return s.termination != pvlm_pairgraph::kCostNotFinite && std::isfinite(s.final_cost); }       // summary.IsSolutionUsable()
pvlm_transdir_summary FromCore(const pvlm_pairgraph::Summary& h) { return {h.initial_cost, h.final_cost, h.successful_steps, h.unsuccessful_steps, h.termination}; }
}  // namespace

bool TranslationAveragingL2Chordal(const std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                                   const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const double l2_loss_threshold, const bool host) {
  DirectionInputs in;
  if (!in.Fill(image_pairs, frames, global_translations, new_to_old)) return false;
  const int F = (int)global_translations.size(), P = (int)image_pairs.size();
  pvlm_transdir_summary sum{0, 0, 0, 0, 0};
  if (host) {
    pvlm_pairgraph::Summary hs;
    if (transdir_detail::ChordalHost(F, P, in.first.data(), in.second.data(), in.dir.data(), (int)origin_idx, in.centres.data(), l2_loss_threshold, 300, &hs)) return false;
    sum = FromCore(hs);
  } else {
    Engine& e = Engine::Default();
    const pvlm_transdir_chordal_params prm{l2_loss_threshold, 300};
    e.Check(pvlm_transavg_chordal(e.ctx(), F, P, in.first.data(), in.second.data(), in.dir.data(), (int)origin_idx, in.centres.data(), &prm, &sum), "pvlm_transavg_chordal");
  }
  if (!Usable(sum)) return false;
  in.Read(frames, new_to_old, global_translations);
  return true;
}

// K47: TranslationAveragingL1 (sfm/TranslationAveraging.cpp:277-417)
bool TranslationAveragingL1(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const bool host,
                            pvlm_translp_summary* summary_out, const bool device_triplets) {
  const size_t F = global_translations.size();
  if (origin_idx >= F || global_translations[origin_idx] != Vector3d{0, 0, 0}) return false;             // upstream asserts (:281)
  std::map<std::pair<size_t, size_t>, size_t> image_pair_to_idx;                                         // :285-291: a repeated pair resolves to its last index
  for (size_t i = 0; i < image_pairs.size(); ++i) {
    const std::pair<size_t, size_t>& p = image_pairs[i].image_pair;
    if (!(p.first < p.second) || p.second >= F) return false;
    image_pair_to_idx[p] = i;
  }
  // the call's pair list: the distinct pairs in the map's order
  std::vector<int> first, second, trip_pairs;
  std::vector<double> R21, t21, t(3 * F, 0.0);
  std::set<std::pair<size_t, size_t>> edges;
  std::map<std::pair<size_t, size_t>, int> place;
  for (const auto& kv : image_pair_to_idx) {
    const RelativePair& p = image_pairs[kv.second];
    place[kv.first] = (int)first.size();
    first.push_back((int)kv.first.first); second.push_back((int)kv.first.second);
    R21.insert(R21.end(), p.R_21.begin(), p.R_21.end()); t21.insert(t21.end(), p.t_21.begin(), p.t_21.end());
    edges.insert(kv.first);
  }
  if (device_triplets) FindTripletDevice(edges, &trip_pairs, host);            // K48: `place` is the position in the set's order, which is what it indexes by
  else for (const Triplet& tr : FindTriplet(edges)) { trip_pairs.push_back(place[{tr.i, tr.j}]); trip_pairs.push_back(place[{tr.j, tr.k}]); trip_pairs.push_back(place[{tr.i, tr.k}]); }
  if (trip_pairs.size() / 3 > (size_t)INT_MAX) return false;
  const int P = (int)first.size(), T = (int)trip_pairs.size() / 3;
  first.push_back(0); second.push_back(0); R21.resize(R21.size() + 9); t21.resize(t21.size() + 3); trip_pairs.push_back(0);      // never empty
  pvlm_translp_summary sum{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const pvlm_translp_params prm{60, 1e-9, 1e-9};
  if (host) {
    pvlm_translp::Params hp; pvlm_translp::Summary hs;
    if (translp_detail::L1Host((int)F, P, first.data(), second.data(), R21.data(), t21.data(), T, trip_pairs.data(), (int)origin_idx, t.data(), nullptr, &hp, &hs)) return false;
    sum = {hs.gamma, hs.dual_objective, hs.gap, hs.primal_residual, hs.dual_residual, hs.iterations, hs.bumps, hs.n_components, hs.n_loose, hs.termination};
  } else {
    Engine& e = Engine::Default();
    e.Check(pvlm_transavg_l1(e.ctx(), (int)F, P, first.data(), second.data(), R21.data(), t21.data(), T, trip_pairs.data(), (int)origin_idx, t.data(), nullptr, &prm, &sum),
            "pvlm_transavg_l1");
  }
  if (summary_out) *summary_out = sum;
  // no triplets: the programme has no rows, every column is free and stays zero
  if (sum.termination != pvlm_translp::kConverged && sum.termination != pvlm_translp::kNoTriplets) return false;      // "Solve linear program failed"
  for (size_t i = 0; i < F; ++i) global_translations[i] = {t[3 * i], t[3 * i + 1], t[3 * i + 2]};                     // :411-414
  return true;
}

bool TranslationAveragingLUD(std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                             const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const int num_iteration, const float upper_scale_ratio,
                             const float lower_scale_ratio, const bool host, int* iterations_run) {
  std::vector<double> scales = StartScales(image_pairs), weight(image_pairs.size(), 1.0);
  DirectionInputs in;
  if (!in.Fill(image_pairs, frames, global_translations, new_to_old)) return false;
  const int F = (int)global_translations.size();
  double curr_cost = 0, last_cost = 0;
  if (iterations_run) *iterations_run = 0;
  for (int iter = 0; iter < num_iteration; ++iter) {
    const int P = (int)image_pairs.size();
    std::vector<double> s(scales), w(weight);
    s.push_back(0.0); w.push_back(0.0);
    pvlm_transdir_summary sum{0, 0, 0, 0, 0};
    curr_cost = 0;
    if (host) {
      pvlm_pairgraph::Summary hs;
      if (transdir_detail::LudHost(F, P, in.first.data(), in.second.data(), in.dir.data(), s.data(), w.data(), (int)origin_idx, in.centres.data(), upper_scale_ratio, lower_scale_ratio,
                                   50, &curr_cost, &hs)) return false;
      sum = FromCore(hs);
    } else {
      Engine& e = Engine::Default();
      const pvlm_transdir_lud_params prm{upper_scale_ratio, lower_scale_ratio, 50};
      e.Check(pvlm_transavg_lud(e.ctx(), F, P, in.first.data(), in.second.data(), in.dir.data(), s.data(), w.data(), (int)origin_idx, in.centres.data(), &prm, &curr_cost, &sum),
              "pvlm_transavg_lud");
    }
    if (!Usable(sum)) return false;
    std::copy(s.begin(), s.begin() + P, scales.begin()); std::copy(w.begin(), w.begin() + P, weight.begin());
    if (iterations_run) *iterations_run = iter + 1;
    if (std::fabs(last_cost - curr_cost) / curr_cost < 0.05 || curr_cost < 10) break;       // :628 as written
    last_cost = curr_cost;
    // :635-651 as written.  No input reaches it: a scaled pair is held at or above 0.5 s0 and an unscaled one at or above 1 by its parameter bound, onto which the
    // clamp puts every candidate, so no scale is ever negative here (K42's L2IRLS carries the same loop for the same reason)
    std::vector<RelativePair> good_matches; std::vector<double> good_scales, good_weight;
    for (size_t i = 0; i < scales.size(); ++i) {
      if (scales[i] < 0) continue;
      good_scales.push_back(scales[i]); good_weight.push_back(weight[i]); good_matches.push_back(image_pairs[i]);
    }
    if (good_scales.size() != scales.size()) {
      good_scales.swap(scales); good_weight.swap(weight); good_matches.swap(image_pairs);
      const std::vector<double> centres = in.centres;                     // the pair arrays follow the list; the centres are carried over
      if (!in.Fill(image_pairs, frames, global_translations, new_to_old)) return false;
      in.centres = centres;
    }
  }
  in.Read(frames, new_to_old, global_translations);
  return true;
}

void ReIndex(const std::vector<RelativePair>& pairs, std::map<size_t, size_t>& forward, std::map<size_t, size_t>& backward) {
  forward.clear(); backward.clear();
  std::set<size_t> old_id;
  for (const RelativePair& pair : pairs) { old_id.insert(pair.image_pair.first); old_id.insert(pair.image_pair.second); }
  for (const RelativePair& pair : pairs)
    for (const size_t id : {pair.image_pair.first, pair.image_pair.second})
      if (forward.find(id) == forward.end()) {
        const size_t dist = (size_t)std::distance(old_id.begin(), old_id.find(id));
        forward[id] = dist; backward[dist] = id;
      }
}

bool SetToOrigin(std::vector<Frame>& frames, size_t frame_idx) {
  if (frame_idx > frames.size()) return false;                                  // `>` as written (:1387)
  if (frame_idx == frames.size() || !PoseValidAsWritten(frames[frame_idx])) {   // (== size: upstream reads past the list)
    for (frame_idx = 0; frame_idx < frames.size(); ++frame_idx) if (PoseValidAsWritten(frames[frame_idx])) break;
    if (frame_idx == frames.size()) return false;                               // no frame has a pose (upstream reads past the list)
  }
  const Matrix3d Ro = frames[frame_idx].R_wc; const Vector3d to = frames[frame_idx].t_wc;
  for (Frame& f : frames) {
    if (!PoseValidAsWritten(f)) continue;
    // T_ic = T_iw T_wc(origin), the new pose its inverse: R' = Ro^T R_i, t' = Ro^T (t_i - t_o), by rigid inverses (upstream: Eigen's general 4 x 4 inverse, ~1e-16 apart)
    Matrix3d Ri; Vector3d ti, Ric_t;
    RigidInverse(f.R_wc, f.t_wc, &Ri, &ti);
    Matrix3d Ric;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Ric[3 * r + c] = Ri[3 * r] * Ro[c] + Ri[3 * r + 1] * Ro[3 + c] + Ri[3 * r + 2] * Ro[6 + c];
      Ric_t[r] = (Ri[3 * r] * to[0] + Ri[3 * r + 1] * to[1] + Ri[3 * r + 2] * to[2]) + ti[r];
    }
    Matrix3d Rn; Vector3d tn;
    RigidInverse(Ric, Ric_t, &Rn, &tn);
    f.R_wc = Rn; f.t_wc = tn; f.pose_valid = PoseValidAsWritten(f);
  }
  return true;
}

bool EstimateGlobalTranslation(std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, const int method, const TranslationOptions& o) {
  if (!o.gps_path.empty() || o.init_translation_GPS) return Say(o, "GPS is not supported");
  // the frames with a global rotation (:1067-1080)
  std::set<size_t> frame_with_rotation;
  for (const Frame& f : frames) if (!RotationIsZero(f)) frame_with_rotation.insert((size_t)f.id);
  std::vector<RelativePair> pair_with_rotation;
  for (const RelativePair& pair : image_pairs)
    if (frame_with_rotation.count(pair.image_pair.first) > 0 && frame_with_rotation.count(pair.image_pair.second) > 0) pair_with_rotation.push_back(pair);
  std::vector<RelativePair> pair_with_scale, pair_without_scale;
  for (const RelativePair& p : pair_with_rotation) (p.upper_scale >= 0 && p.lower_scale >= 0 ? pair_with_scale : pair_without_scale).push_back(p);
  std::set<size_t> largest_component_nodes;
  image_pairs = LargestBiconnectedGraph(o.use_all_pairs_ta ? pair_with_rotation : pair_with_scale, largest_component_nodes);
  if (image_pairs.empty()) return Say(o, "no nodes are bi-edge connected");
  for (const RelativePair& p : image_pairs) if (p.image_pair.first >= frames.size() || p.image_pair.second >= frames.size()) return Say(o, "a pair names a frame that is not there");
  pair_with_rotation.clear();
  // the start: zero for camera 0, uniform [-1, 1] for the others (upstream: Eigen's Random() after srand(time); here splitmix64 on options.seed)
  std::vector<Vector3d> global_translations(largest_component_nodes.size(), Vector3d{0, 0, 0});
  {
    uint64_t st = o.seed;
    auto next = [&st]() { uint64_t z = (st += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); };
    for (size_t i = 1; i < global_translations.size(); ++i) for (int k = 0; k < 3; ++k) global_translations[i][(size_t)k] = (double)(next() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  }
  // 1. the global re-indexing (:1148-1159)
  std::map<size_t, size_t> old_to_new_global, new_to_old_global;
  ReIndex(image_pairs, old_to_new_global, new_to_old_global);
  for (RelativePair& pair : pair_with_scale) { pair.image_pair.first = old_to_new_global[pair.image_pair.first]; pair.image_pair.second = old_to_new_global[pair.image_pair.second]; }
  for (RelativePair& pair : image_pairs) { pair.image_pair.first = old_to_new_global[pair.image_pair.first]; pair.image_pair.second = old_to_new_global[pair.image_pair.second]; }
  size_t origin_idx = 0;
  // 2. the DLT start on the scaled pairs (:1165-1216)
  if (o.init_translation_DLT && !pair_with_scale.empty()) {
    std::map<size_t, size_t> old_to_new, new_to_old;
    pair_with_scale = LargestBiconnectedGraph(pair_with_scale, largest_component_nodes);
    ReIndex(pair_with_scale, old_to_new, new_to_old);
    for (RelativePair& pair : pair_with_scale) { pair.image_pair.first = old_to_new[pair.image_pair.first]; pair.image_pair.second = old_to_new[pair.image_pair.second]; }
    std::vector<Vector3d> global_translation_scale(largest_component_nodes.size());
    // :1183 as written: ALL pairs under the global indices into an output sized by the scaled component.  Every index fits when the scaled pairs cover the same
    // frames; when one does not, upstream writes out of range — refused here
    for (const RelativePair& p : image_pairs)
      if (p.image_pair.first >= global_translation_scale.size() || p.image_pair.second >= global_translation_scale.size())
        return Say(o, "Translation average DLT: the pair list names a camera past the scaled component (sfm/SfM.cpp:1183 writes out of range here)");
    if (global_translation_scale.empty() || !TranslationAveragingDLT(image_pairs, global_translation_scale, o.host)) return Say(o, "Translation average DLT failed");
    origin_idx = new_to_old_global[new_to_old[0]];
    for (size_t i = 0; i < global_translation_scale.size(); ++i) {
      Frame& f = frames[new_to_old_global[new_to_old[i]]];
      SetTranslationOf(f, MinusRt(f.R_wc, global_translation_scale[i]));
    }
    SetToOrigin(frames, origin_idx);
    for (size_t i = 0; i < global_translations.size(); ++i) {
      const auto it = new_to_old_global.find(i);
      if (it == new_to_old_global.end()) continue;
      if (!PoseValidAsWritten(frames[it->second])) continue;
      Matrix3d Ri; Vector3d ti;
      RigidInverse(frames[it->second].R_wc, frames[it->second].t_wc, &Ri, &ti);
      global_translations[i] = ti;
    }
    origin_idx = old_to_new_global[origin_idx];
  }
  // 3. the averaging
  bool success = false;
  if (method == TRANSLATION_AVERAGING_SOFTL1)
    success = TranslationAveragingSoftL1(image_pairs, global_translations, origin_idx, 0.01, o.upper_scale_ratio, o.lower_scale_ratio, o.host);
  else if (method == TRANSLATION_AVERAGING_L2IRLS)
    success = TranslationAveragingL2IRLS(image_pairs, global_translations, origin_idx, o.num_iteration_L2IRLS, o.upper_scale_ratio, o.lower_scale_ratio, o.host);
  else if (method == TRANSLATION_AVERAGING_BATA && o.enable_bata)      // :1285-1294; behind the flag: see TranslationOptions
    success = TranslationAveragingBATA(image_pairs, frames, global_translations, new_to_old_global, origin_idx, o.bata, o.seed, o.host);
  else if (method == TRANSLATION_AVERAGING_CHORDAL && o.enable_chordal)      // :1254-1263; behind the flag: see TranslationOptions
    success = TranslationAveragingL2Chordal(image_pairs, frames, global_translations, new_to_old_global, origin_idx, 0.5, o.host);
  else if (method == TRANSLATION_AVERAGING_LUD && o.enable_lud)        // :1295-1305; behind the flag
    success = TranslationAveragingLUD(image_pairs, frames, global_translations, new_to_old_global, origin_idx, o.num_iteration_L2IRLS, o.upper_scale_ratio, o.lower_scale_ratio, o.host);
  else if (method == TRANSLATION_AVERAGING_L1 && o.enable_l1)          // :1264-1273; behind the flag
    success = TranslationAveragingL1(image_pairs, global_translations, origin_idx, o.host, nullptr, o.device_triplets);
  else return Say(o, "Translaton average method not supported");       // L1, BATA, chordal and LUD only behind their flags; the text is upstream's (:1308)
  if (!success)
    return Say(o, method == TRANSLATION_AVERAGING_SOFTL1 ? "Translation average Soft L1 failed" : method == TRANSLATION_AVERAGING_BATA ? "Translation average BATA failed" :
                  method == TRANSLATION_AVERAGING_CHORDAL ? "Translation average chordal failed" : method == TRANSLATION_AVERAGING_LUD ? "Translation average LUD failed" : method == TRANSLATION_AVERAGING_L1 ? "Translation average L1 failed" :
                  "Translation average L2 IRLS failed");
  for (RelativePair& pair : image_pairs) { pair.image_pair.first = new_to_old_global[pair.image_pair.first]; pair.image_pair.second = new_to_old_global[pair.image_pair.second]; }
  std::set<size_t> frame_with_translation;
  for (size_t i = 0; i < global_translations.size(); ++i) {
    Frame& f = frames[new_to_old_global[i]];
    SetTranslationOf(f, MinusRt(f.R_wc, global_translations[i]));       // t_wc = -R_wc t_cw
    frame_with_translation.insert(new_to_old_global[i]);
  }
  std::vector<RelativePair> good_pair;
  for (const RelativePair& p : image_pairs) {
    const size_t idx1 = p.image_pair.first, idx2 = p.image_pair.second;
    if (frame_with_translation.count(idx1) && frame_with_translation.count(idx2) && frame_with_rotation.count(idx1) && frame_with_rotation.count(idx2)) good_pair.push_back(p);
  }
  good_pair.swap(image_pairs);
  return true;
}

// ================================================================================================
// K40: rotation averaging — FindTriplet, FilterByTriplet, FilterPairs, RotationAveragingSpanningTree / RefineL1 / L1 / L2 (sfm/RotationAveraging.cpp), EstimateGlobalRotation
// ================================================================================================
namespace {
bool Say(const RotationOptions& o, const char* m) { if (o.message) *o.message = m; return false; }
Matrix3d MulNT(const Matrix3d& A, const Matrix3d& B) { Matrix3d C; pvlm_rotavg::mul_nt(A.data(), B.data(), C.data()); return C; }
}  // namespace

std::vector<Triplet> FindTriplet(const std::set<std::pair<size_t, size_t>>& edges) {
  std::vector<Triplet> triplets;
  std::map<uint32_t, std::set<uint32_t>> adjacency;            // upstream: an unordered_map that is only looked up, never walked
  for (const std::pair<size_t, size_t>& e : edges) { adjacency[(uint32_t)e.first].insert((uint32_t)e.second); adjacency[(uint32_t)e.second].insert((uint32_t)e.first); }
  std::vector<uint32_t> node_candidate;
  for (const std::pair<size_t, size_t>& e : edges) {
    const std::set<uint32_t>& neighbor1 = adjacency.find((uint32_t)e.first)->second;
    const std::set<uint32_t>& neighbor2 = adjacency.find((uint32_t)e.second)->second;
    node_candidate.clear();
    std::set_intersection(neighbor1.cbegin(), neighbor1.cend(), neighbor2.cbegin(), neighbor2.cend(), std::back_inserter(node_candidate));
    for (const uint32_t node : node_candidate) {
      std::array<uint32_t, 3> idx = {node, (uint32_t)e.first, (uint32_t)e.second};
      std::sort(idx.begin(), idx.end());
      triplets.push_back(Triplet{idx[0], idx[1], idx[2]});
    }
    adjacency[(uint32_t)e.first].erase((uint32_t)e.second);
    adjacency[(uint32_t)e.second].erase((uint32_t)e.first);
  }
  return triplets;
}

std::vector<RelativePair> FilterByTriplet(const std::vector<RelativePair>& init_pairs, const double angle_threshold, std::set<size_t>& covered_frames) {
  covered_frames.clear();
  std::set<std::pair<size_t, size_t>> pairs;
  std::map<std::pair<size_t, size_t>, Matrix3d> map_rotations;
  for (const RelativePair& p : init_pairs) {
    if (!(p.image_pair.first < p.image_pair.second)) return {};                 // upstream asserts
    pairs.insert(p.image_pair);
    map_rotations[p.image_pair] = p.R_21;
  }
  const std::vector<Triplet> triplets = FindTriplet(pairs);
  pairs.clear();
  for (const Triplet& t : triplets) {
    const Matrix3d& R_21 = map_rotations[{t.i, t.j}]; const Matrix3d& R_32 = map_rotations[{t.j, t.k}]; const Matrix3d& R_31 = map_rotations[{t.i, t.k}];
    Matrix3d a, rot;
    pvlm_rotavg::mul_tn(R_31.data(), R_32.data(), a.data());                    // (R_13 R_32) R_21
    pvlm_rotavg::mul_nn(a.data(), R_21.data(), rot.data());
    double cos_theta = (rot[0] + rot[4] + rot[8]) / 3.0;                        // as written (:740): the trace over 3
    cos_theta = std::min(1.0, std::max(cos_theta, -1.0));
    const double angle_error = std::acos(cos_theta) * 180.0 / M_PI;
    if (angle_error < angle_threshold) {
      pairs.insert({t.i, t.j}); pairs.insert({t.j, t.k}); pairs.insert({t.i, t.k});
    }
  }
  std::vector<RelativePair> pairs_after_triplet_filter;
  for (const RelativePair& m : init_pairs) if (pairs.count(m.image_pair) > 0) pairs_after_triplet_filter.push_back(m);
  return LargestBiconnectedGraph(pairs_after_triplet_filter, covered_frames);
}

// K48: the two functions above through pvlm_triplets_find / pvlm_triplets_filter (host: the host compile of csrc/pvlm_triplet_core.h)
std::vector<Triplet> FindTripletDevice(const std::set<std::pair<size_t, size_t>>& edges, std::vector<int>* triplet_pairs, const bool host) {
  if (triplet_pairs) triplet_pairs->clear();
  std::vector<int> first, second;
  first.reserve(edges.size()); second.reserve(edges.size());
  size_t n_cameras = 0;
  for (const std::pair<size_t, size_t>& e : edges) {
    if (!(e.first < e.second) || e.second >= (size_t)INT_MAX) return {};
    first.push_back((int)e.first); second.push_back((int)e.second);
    n_cameras = std::max(n_cameras, e.second + 1);
  }
  const int F = (int)n_cameras, P = (int)first.size();
  first.push_back(0); second.push_back(0);                                    // never empty
  std::vector<int> trip, pairs3;
  long long needed = 0, capacity = 0;
  // a sizing call (no output wanted: the count alone), then the call that writes
  for (int round = 0; round < 2; ++round) {
    trip.assign(3 * (size_t)capacity + 1, 0);
    if (triplet_pairs) pairs3.assign(3 * (size_t)capacity + 1, 0);
    int* want_trip = round ? trip.data() : nullptr;
    int* want_pairs = round && triplet_pairs ? pairs3.data() : nullptr;
    if (host) {
      if (pvlm_triplet::find_host(F, P, first.data(), second.data(), want_trip, want_pairs, capacity, &needed, nullptr)) throw std::runtime_error("FindTripletDevice: refused");
    } else {
      Engine& e = Engine::Default();
      e.Check(pvlm_triplets_find(e.ctx(), F, P, first.data(), second.data(), want_trip, want_pairs, capacity, &needed, nullptr), "pvlm_triplets_find");
    }
    capacity = needed;
  }
  std::vector<Triplet> triplets((size_t)needed);
  for (size_t t = 0; t < triplets.size(); ++t) triplets[t] = Triplet{(uint32_t)trip[3 * t], (uint32_t)trip[3 * t + 1], (uint32_t)trip[3 * t + 2]};
  if (triplet_pairs) { pairs3.resize(3 * (size_t)needed); triplet_pairs->swap(pairs3); }
  return triplets;
}

std::vector<RelativePair> FilterByTripletDevice(const std::vector<RelativePair>& init_pairs, const double angle_threshold, std::set<size_t>& covered_frames, const bool host,
                                                pvlm_triplet_stats* stats_out) {
  covered_frames.clear();
  std::map<std::pair<size_t, size_t>, size_t> last;                            // a pair named twice: its last entry's rotation, as the map assignment of FilterByTriplet
  size_t n_cameras = 0;
  for (size_t i = 0; i < init_pairs.size(); ++i) {
    const std::pair<size_t, size_t>& p = init_pairs[i].image_pair;
    if (!(p.first < p.second) || p.second >= (size_t)INT_MAX) return {};      // upstream asserts
    last[p] = i;
    n_cameras = std::max(n_cameras, p.second + 1);
  }
  std::vector<int> first, second;
  std::vector<double> R;
  first.reserve(last.size()); second.reserve(last.size()); R.reserve(9 * last.size() + 9);
  for (const auto& kv : last) {
    first.push_back((int)kv.first.first); second.push_back((int)kv.first.second);
    const Matrix3d& m = init_pairs[kv.second].R_21;
    R.insert(R.end(), m.begin(), m.end());
  }
  const int F = (int)n_cameras, P = (int)first.size();
  first.push_back(0); second.push_back(0); R.resize(R.size() + 9);            // never empty
  std::vector<unsigned char> keep((size_t)P + 1, 0);
  pvlm_triplet_stats st{0, 0, 0, 0};
  // the library wants a finite threshold; `angle_error < angle_threshold` as written keeps nothing at or below 0 (NaN included) and everything above 180
  const double threshold = std::isnan(angle_threshold) ? 0.0 : std::min(std::max(angle_threshold, 0.0), 181.0);
  if (host) {
    pvlm_triplet::Stats hs{0, 0, 0, 0};
    if (pvlm_triplet::filter_host(F, P, first.data(), second.data(), R.data(), threshold, keep.data(), &hs)) throw std::runtime_error("FilterByTripletDevice: refused");
    st = {hs.n_triplets, hs.n_kept_triplets, hs.n_uncertain, hs.n_kept_pairs};
  } else {
    Engine& e = Engine::Default();
    e.Check(pvlm_triplets_filter(e.ctx(), F, P, first.data(), second.data(), R.data(), threshold, keep.data(), &st), "pvlm_triplets_filter");
  }
  if (stats_out) *stats_out = st;
  std::set<std::pair<size_t, size_t>> kept;
  size_t at = 0;
  for (const auto& kv : last) if (keep[at++]) kept.insert(kept.end(), kv.first);
  std::vector<RelativePair> pairs_after_triplet_filter;
  for (const RelativePair& m : init_pairs) if (kept.count(m.image_pair) > 0) pairs_after_triplet_filter.push_back(m);
  return LargestBiconnectedGraph(pairs_after_triplet_filter, covered_frames);
}

std::vector<RelativePair> FilterPairs(const std::vector<RelativePair>& image_pairs, const std::vector<Matrix3d>& global_rotations, double angle_threshold, double* threshold_out) {
  std::vector<double> errors;
  errors.reserve(image_pairs.size());
  for (const RelativePair& p : image_pairs) {
    double e[3];
    pvlm_rotavg::pair_error(global_rotations[p.image_pair.first].data(), global_rotations[p.image_pair.second].data(), p.R_21.data(), e);
    errors.push_back(std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
  }
  double threshold = 0;
  if (angle_threshold > 0) threshold = angle_threshold / 180.0 * M_PI;
  else if (!errors.empty()) {                                                   // X84: median + 5.2 MAD, both taken at position size / 2
    std::vector<double> data(errors);
    std::vector<double>::iterator mid = data.begin() + errors.size() / 2;
    std::nth_element(data.begin(), mid, data.end());
    const double median = *mid;
    for (size_t i = 0; i < errors.size(); ++i) data[i] = std::fabs(errors[i] - median);
    std::nth_element(data.begin(), mid, data.end());
    threshold = median + 5.2 * (*mid);
  }
  if (threshold_out) *threshold_out = threshold;
  std::set<size_t> valid_pair_idx, invalid_pair_idx;
  for (size_t i = 0; i < errors.size(); ++i) (errors[i] < threshold ? valid_pair_idx : invalid_pair_idx).insert(i);
  // :101-165: every frame wants neighbor_size pairs before it and after it within `range` frames
  std::vector<std::pair<int, int>> num_neighbor_frames(global_rotations.size(), std::make_pair(0, 0));
  const size_t range = 10; const int neighbor_size = 3;
  for (const size_t idx : valid_pair_idx) {
    const RelativePair& p = image_pairs[idx];
    if ((p.image_pair.second - p.image_pair.first) <= range) { num_neighbor_frames[p.image_pair.first].second++; num_neighbor_frames[p.image_pair.second].first++; }
  }
  std::map<int, std::vector<int>> bad_frames;
  for (size_t i = 0; i < num_neighbor_frames.size(); ++i)
    if (num_neighbor_frames[i].first < neighbor_size || num_neighbor_frames[i].second < neighbor_size) bad_frames[(int)i] = std::vector<int>();
  for (const size_t idx : invalid_pair_idx) {
    const RelativePair& p = image_pairs[idx];
    if ((p.image_pair.second - p.image_pair.first) <= range) {
      if (bad_frames.find((int)p.image_pair.first) != bad_frames.end() && num_neighbor_frames[p.image_pair.first].second < neighbor_size) bad_frames[(int)p.image_pair.first].push_back((int)idx);
      if (bad_frames.find((int)p.image_pair.second) != bad_frames.end() && num_neighbor_frames[p.image_pair.second].first < neighbor_size) bad_frames[(int)p.image_pair.second].push_back((int)idx);
    }
  }
  for (auto& it : bad_frames) {
    const int frame_id = it.first;
    if (num_neighbor_frames[(size_t)frame_id].first >= neighbor_size && num_neighbor_frames[(size_t)frame_id].second >= neighbor_size) continue;
    // upstream: std::sort by the error alone; equal errors are ordered by the pair index here
    std::sort(it.second.begin(), it.second.end(), [&](const int a, const int b) { return errors[(size_t)a] < errors[(size_t)b] || (errors[(size_t)a] == errors[(size_t)b] && a < b); });
    for (size_t count = 0; num_neighbor_frames[(size_t)frame_id].first < neighbor_size && count < it.second.size(); ++count) {
      const RelativePair& p = image_pairs[(size_t)it.second[count]];
      if (p.image_pair.second != (size_t)frame_id) continue;
      valid_pair_idx.insert((size_t)it.second[count]);
      num_neighbor_frames[p.image_pair.first].second++; num_neighbor_frames[p.image_pair.second].first++;
      invalid_pair_idx.erase((size_t)it.second[count]);
    }
    for (size_t count = 0; num_neighbor_frames[(size_t)frame_id].second < neighbor_size && count < it.second.size(); ++count) {
      const RelativePair& p = image_pairs[(size_t)it.second[count]];
      if (p.image_pair.first != (size_t)frame_id) continue;
      valid_pair_idx.insert((size_t)it.second[count]);
      num_neighbor_frames[p.image_pair.first].second++; num_neighbor_frames[p.image_pair.second].first++;
      invalid_pair_idx.erase((size_t)it.second[count]);
    }
  }
  std::vector<RelativePair> valid_pairs;
  for (const size_t idx : valid_pair_idx) valid_pairs.push_back(image_pairs[idx]);
  return valid_pairs;
}

bool RotationAveragingSpanningTree(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx) {
  const size_t F = global_rotations.size();
  if (start_idx >= F) return false;
  std::vector<size_t> root(F);
  for (size_t c = 0; c < F; ++c) root[c] = c;
  auto find = [&](size_t c) { while (root[c] != c) { root[c] = root[root[c]]; c = root[c]; } return c; };
  struct Edge { size_t to, pair; bool child_is_first; };
  std::vector<std::vector<Edge>> tree(F);
  for (size_t p = 0; p < image_pairs.size(); ++p) {
    const size_t i = image_pairs[p].image_pair.first, j = image_pairs[p].image_pair.second;
    if (i >= F || j >= F) return false;
    const size_t a = find(i), b = find(j);
    if (a == b) continue;
    root[a] = b;
    tree[i].push_back(Edge{j, p, false}); tree[j].push_back(Edge{i, p, true});
  }
  std::vector<char> seen(F, 0);
  std::queue<size_t> queue;
  global_rotations[start_idx] = Matrix3d{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  seen[start_idx] = 1; queue.push(start_idx);
  size_t reached = 1;
  while (!queue.empty()) {
    const size_t c = queue.front(); queue.pop();
    for (const Edge& e : tree[c]) {
      if (seen[e.to]) continue;
      const Matrix3d& R = image_pairs[e.pair].R_21;                             // child = second: R_cp = R_21; child = first: R_cp = R_21^T
      if (e.child_is_first) pvlm_rotavg::mul_tn(R.data(), global_rotations[c].data(), global_rotations[e.to].data());
      else pvlm_rotavg::mul_nn(R.data(), global_rotations[c].data(), global_rotations[e.to].data());
      seen[e.to] = 1; queue.push(e.to); ++reached;
    }
  }
  return reached == F;
}

bool RotationAveragingRefineL1(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx, const bool host) {
  PairGraphInputs in;
  if (!in.Fill(image_pairs, global_rotations)) return false;
  const int F = (int)global_rotations.size(), P = (int)image_pairs.size();
  pvlm_rotavg_l1_summary sum{0, 0, 0, 0};
  if (host) {
    pvlm_rotavg::L1Summary hs;
    if (rotavg_detail::L1Host(F, P, in.first.data(), in.second.data(), in.R.data(), (int)start_idx, in.rot.data(), &hs)) return false;
    sum.info = hs.info;
  } else {
    Engine& e = Engine::Default();
    if (pvlm_rotavg_l1(e.ctx(), F, P, in.first.data(), in.second.data(), in.R.data(), (int)start_idx, in.rot.data(), &sum) != PVLM_OK) return false;
  }
  in.Read(global_rotations);                                                    // the rotations of the last completed iteration, also when info > 0
  return sum.info == 0;
}

bool RotationAveragingL1(std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx, double angle_threshold, const bool host) {
  if (!RotationAveragingSpanningTree(image_pairs, global_rotations, start_idx)) return false;
  if (!RotationAveragingRefineL1(image_pairs, global_rotations, start_idx, host)) return false;
  image_pairs = FilterPairs(image_pairs, global_rotations, angle_threshold);
  return true;
}

bool RotationAveragingL2(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, const bool host) {
  PairGraphInputs in;
  if (!in.Fill(image_pairs, global_rotations)) return false;
  const int F = (int)global_rotations.size(), P = (int)image_pairs.size();
  pvlm_rotavg_l2_summary sum{0, 0, 0, 0, 0};
  if (host) {
    pvlm_pairgraph::Summary hs;
    if (rotavg_detail::L2Host(F, P, in.first.data(), in.second.data(), in.R.data(), in.rot.data(), 0.07, 50, &hs)) return false;
    sum.final_cost = hs.final_cost; sum.termination = hs.termination;
  } else {
    Engine& e = Engine::Default();
    const pvlm_rotavg_l2_params prm{0.07, 50};
    if (pvlm_rotavg_l2(e.ctx(), F, P, in.first.data(), in.second.data(), in.R.data(), in.rot.data(), &prm, &sum) != PVLM_OK) return false;
  }
  if (sum.termination == pvlm_pairgraph::kCostNotFinite || !std::isfinite(sum.final_cost) || !pvlm_pairgraph::finite_all(in.rot.data(), 9 * (size_t)F)) return false;
  in.Read(global_rotations);
  return true;
}

bool RotationAveragingLeastSquare(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, const bool host) {
  if (global_rotations.empty() || image_pairs.empty()) return false;                 // :188-192
  std::vector<Matrix3d> start(global_rotations.size(), Matrix3d{{0, 0, 0, 0, 0, 0, 0, 0, 0}});
  if (!RotationAveragingSpanningTree(image_pairs, start, 0)) return false;
  PairGraphInputs in;
  if (!in.Fill(image_pairs, start)) return false;
  const int F = (int)start.size(), P = (int)image_pairs.size();
  int info = 0;
  if (host) {
    const pvlm_rotstart::Params prm;
    pvlm_rotstart::Summary hs;
    if (rotstart_detail::LeastSquareHost(F, P, in.first.data(), in.second.data(), in.R.data(), in.rot.data(), &prm, &hs)) return false;
    info = hs.info;
  } else {
    Engine& e = Engine::Default();
    const pvlm_rotavg_lsq_params prm{1e-9, 1e-12, 100};
    pvlm_rotavg_lsq_summary sum{0, 0, 0, 0.0, {0.0, 0.0, 0.0}};
    if (pvlm_rotavg_least_square(e.ctx(), F, P, in.first.data(), in.second.data(), in.R.data(), in.rot.data(), &prm, &sum) != PVLM_OK) return false;
    info = sum.info;
  }
  if (info != 0) return false;
  in.Read(global_rotations);
  return true;
}

bool EstimateGlobalRotation(std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, const int method, const RotationOptions& o) {
  if (!o.use_all_pairs_ra) {
    std::vector<RelativePair> pairs_with_scale;
    for (const RelativePair& p : image_pairs) if (p.upper_scale >= 0 && p.lower_scale >= 0) pairs_with_scale.push_back(p);
    pairs_with_scale.swap(image_pairs);
  }
  for (const RelativePair& p : image_pairs) {
    if (p.image_pair.first >= frames.size() || p.image_pair.second >= frames.size()) return Say(o, "a pair names a frame that is not there");
    if (!(p.image_pair.first < p.image_pair.second)) return Say(o, "a pair with first >= second (upstream asserts)");
  }
  std::set<size_t> covered_frames;
  image_pairs = LargestBiconnectedGraph(image_pairs, covered_frames);
  image_pairs = o.device_triplets ? FilterByTripletDevice(image_pairs, 0.1, covered_frames, o.host) : FilterByTriplet(image_pairs, 0.1, covered_frames);
  if (image_pairs.empty()) return Say(o, "no pair is left after the graph and triplet filters");
  std::map<size_t, size_t> old_to_new, new_to_old;
  ReIndex(image_pairs, old_to_new, new_to_old);
  for (RelativePair& pair : image_pairs) { pair.image_pair.first = old_to_new[pair.image_pair.first]; pair.image_pair.second = old_to_new[pair.image_pair.second]; }
  std::vector<Matrix3d> global_rotations(old_to_new.size(), Matrix3d{{0, 0, 0, 0, 0, 0, 0, 0, 0}});
  if (method == ROTATION_AVERAGING_L1) {
    if (!RotationAveragingL1(image_pairs, global_rotations, 0, -1, o.host)) return Say(o, "Rotation averaging L1 failed");
    if (!RotationAveragingL2(image_pairs, global_rotations, o.host) && o.message) *o.message = "Rotation averaging refine L2 failed";       // reported, not returned (:886-887)
  } else if (method == ROTATION_AVERAGING_L2 && o.enable_l2_start) {              // :859-869; behind the flag: see RotationOptions
    if (!RotationAveragingLeastSquare(image_pairs, global_rotations, o.host)) return Say(o, "Rotation averaging L2 failed");
    if (!RotationAveragingL2(image_pairs, global_rotations, o.host) && o.message) *o.message = "Rotation averaging refine L2 failed";       // reported, not returned (:867-868)
  } else return Say(o, "Rotation averaging method not supported: L2 needs the eigenvectors of a dense 3 F x 3 F matrix for its start and is not built");
  for (RelativePair& pair : image_pairs) {
    pair.R_21 = MulNT(global_rotations[pair.image_pair.second], global_rotations[pair.image_pair.first]);      // R_2w R_1w^T
    pair.image_pair.first = new_to_old[pair.image_pair.first]; pair.image_pair.second = new_to_old[pair.image_pair.second];
  }
  for (size_t i = 0; i < global_rotations.size(); ++i) {
    Frame& f = frames[new_to_old[i]];
    const Matrix3d& R = global_rotations[i];
    f.R_wc = Matrix3d{{R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]}};                                 // the averaging gives R_cw, a frame keeps R_wc
    f.pose_valid = PoseValidAsWritten(f);
  }
  return true;
}

}  // namespace pvlm
