// pvlm_host.hpp — C++ host side above the C ABI (include/pvlm.h), mirroring PanoVLM's own
// interfaces for the ICP hot path so that a PanoVLM maintainer (and the parity tests) can call it
// with the names, argument meaning and error behaviour of the reference:
//
//   lidar_mapping/LidarFeatureAssociate.h:22-125   Point2Line / Line2Line / Point2Plane,
//                                                  FindNeighbors, AssociatePoint2Plane, AssociateLine2Line
//   base/CostFunction.h:350-934                    Point2Plane_{Meter,Angle}, Point2Line_{Meter,Angle},
//                                                  Plane2Plane_Global, PlaneIOUResidual  (::Create)
//   util/Optimization.h:39-158                     AddLidarPointToPlaneResidual, AddLidarLineToLineResidual2,
//                                                  AddCameraLidarResidual, SetOptionsLidar
//   lidar_mapping/LidarLineMatch.h, util/Tracks.h  LidarLineMatch::GenerateTracks (line tracks)
//   lidar_mapping/LidarOdometry.h:40-81            LidarOdometry::RefinePose / EstimatePose
//   joint_optimization/CameraLidarLineAssociate.h  CameraLidarLineAssociate::AssociateByAngle
//   sensors/Velodyne.h:80-91,213-233               the Velodyne data contract + frame transforms
//   sensors/Equirectangular.h                      Equirectangular (host, scalar)
//
// Eigen / PCL / Ceres are not dependencies: small POD types stand in for Eigen::Vector3d etc. and
// the ceres:: classes the reference touches (CostFunction, LossFunction, Problem, Solver) are
// re-declared in namespace pvlm::ceres_like with the same member names.  All heavy work goes
// through libpvlm.so (HIP); nothing here computes a residual on the CPU.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pvlm.h"

namespace pvlm {

using Vector2d = std::array<double, 2>;
using Vector3d = std::array<double, 3>;
using Vector4d = std::array<double, 4>;
using Vector6d = std::array<double, 6>;
using Matrix3d = std::array<double, 9>;   // row-major
using Matrix4d = std::array<double, 16>;  // row-major

struct PointXYZI { float x, y, z, intensity; };  // pcl::PointXYZI payload
using PointCloud = std::vector<PointXYZI>;

// sensors/Velodyne.h:57-66
enum PointClassification { POINT_NORMAL = 0x01, POINT_LESS_SHARP = 0x02, POINT_SHARP = 0x04, POINT_FLAT = 0x08, POINT_GROUND = 0x10,
                           POINT_DISABLE = 0x20, POINT_OCCLUDED = 0x40 };
// sensors/Velodyne.h:50-55
enum ExtractionMethod { LOAM = 1, DOUBLE_EXTRACTION = 2, ADAPTIVE = 3 };

// Ring-ordered view of one scan, built by Velodyne::ReOrderVLP (private members of the reference's Velodyne,
// sensors/Velodyne.h:97-120) and the per-point working arrays of ExtractFeatures (freed by the reference at the end of
// the call; kept here when a trace is asked for, for the parity tests).
struct RingLayout {
  std::vector<float> range_image;                      // N_SCANS x horizon_scans, row-major; 0 = no return
  std::vector<std::pair<int, int>> point_idx_to_image; // cloud_scan index -> (ring, column)
  std::vector<int> image_to_point_idx;                 // (ring, column) -> cloud_scan index, -1 = empty
  std::vector<int> scanStartInd, scanEndInd;           // per ring: first + 5, last - 5 (inclusive)
};
struct ExtractionTrace {
  std::vector<float> curvature;
  std::vector<int> state, sort_ind, left_neighbor, right_neighbor;
};

// base/Config.h:111-130 — the knobs the hot path reads (defaults = config/Room.txt:67-79)
struct Config {
  bool angle_residual = true;
  bool point_to_line_residual = false;
  bool line_to_line_residual = true;
  bool point_to_plane_residual = true;
  bool normalize_distance = true;
  double point_to_line_dis_threshold = 0.3;
  double point_to_plane_dis_threshold = 1.0;
  double lidar_plane_tolerance = 0.05;
  double lidar_weight = 1.0;
  double camera_lidar_weight = 1.0;
  double camera_weight = 1.0;
  int num_threads = 25;
  int num_iteration_lidar = 7;
  // feature extraction (base/Config.h:72-76; config/Room.txt:32-35 sets max_curvature = 1000)
  int extraction_method = ADAPTIVE;
  float max_curvature = 5;
  float intersection_angle_threshold = 5;
  bool lidar_segmentation = true;
};

// Wall-clock seconds accumulated per stage of the mirrored call surface (association, track building, solve, ...)
// since the process started — what tools/room_like_odometry.py prints beside the end-to-end time.
void AddStageSeconds(const char* name, double seconds);   // wall-clock accounting of the host stages (see StageSeconds)
const std::map<std::string, double>& StageSeconds();
const std::map<std::string, long>& StageCalls();       // how many times each stage ran

// The process-wide engine (one pvlm_ctx).  Throws std::runtime_error when no GPU / library.
class Engine {
 public:
  static Engine& Default();
  static void SetDevice(int device);  // before first use
  pvlm_ctx* ctx() const { return ctx_; }
  void Check(pvlm_status st, const char* what) const;
  ~Engine();
 private:
  explicit Engine(int device);
  pvlm_ctx* ctx_ = nullptr;
};

// ---- sensors/Velodyne.h data contract ---------------------------------------------------------------
class Velodyne {
 public:
  int id = 0;
  bool valid = true;
  std::string name;                               // file name of the raw scan
  PointCloud cloud;                               // raw points as loaded (LoadLidar), camera-style axes
  PointCloud cornerLessSharp, surfFlat, surfLessFlat;
  int N_SCANS = 16;                               // sensors/Velodyne.h:72-73 (constructor arguments upstream)
  int horizon_scans = 1800;
  PointCloud cloud_scan;                          // ReOrderVLP: the scan ring by ring, intensity = ring id
  PointCloud cornerSharp;
  PointCloud cornerBeforeFilter;                  // cornerLessSharp as ExtractEdgeFeatures2 left it (sensors/Velodyne.cpp:1271)
  std::vector<PointCloud> edge_segmented;
  std::vector<std::set<int>> point_to_segment;
  std::vector<Vector6d> segment_coeffs;  // LiDAR-local (point, unit direction)
  std::vector<Vector3d> end_points;      // 2 per segment, LiDAR-local

  Velodyne() { SetRotation({0, 0, 0, 0, 0, 0, 0, 0, 0}); SetTranslation({INFINITY, INFINITY, INFINITY}); }
  // The pose setters hand the new pose to the scan's device copy (pvlm_scan_set_pose: the resident clouds stay where they are, like the host's);
  // MarkWorld gives the device copy back to the engine's context (InvalidateDevice -> pvlm_scan_destroy), whose pool is not thread-safe: call
  // them from the thread that owns the engine, never from workers.
  void SetPose(const Matrix3d& R_wl, const Vector3d& t_wl) { R_wl_ = R_wl; t_wl_ = t_wl; PoseChanged(); }
  void SetRotation(const Matrix3d& R_wl) { R_wl_ = R_wl; PoseChanged(); }
  void SetTranslation(const Vector3d& t_wl) { t_wl_ = t_wl; PoseChanged(); }
  const Matrix3d& GetRotation() const { return R_wl_; }
  const Vector3d& GetTranslation() const { return t_wl_; }
  Matrix4d GetPose() const;
  bool IsPoseValid() const;                       // sensors/Velodyne.cpp:1894-1899
  bool IsInWorldCoordinate() const { return world_; }
  void MarkWorld(bool w = true) { world_ = w; InvalidateDevice(); }  // clouds already carry world-frame floats
  Vector3d World2Local(const Vector3d& p) const;  // sensors/Velodyne.cpp:1850-1853
  Vector3d Local2World(const Vector3d& p) const;  // :1856-1859
  // LoadLidar (sensors/Velodyne.cpp:92-145): reads a .pcd file (the PCL formats: ascii, binary, binary_compressed; fields
  // x y z [intensity], float32), drops non-finite points (pcl::removeNaNFromPointCloud), drops points closer than 0.5 m
  // (removeClosedPointCloud, :148-172), swaps the axes to the camera convention (x, y, z) -> (x, -z, y) and marks the scan
  // invalid when fewer than 4000 points remain.  Returns false when the file cannot be read (the reference logs and returns).
  bool LoadLidar(std::string file_path = "");
  // sensors/Velodyne.cpp:1635-1674: motion compensation of the raw cloud — point i of n moves by i / n of the way from this scan's pose to T_we (the pose
  // at the sweep's end); the feature clouds are cleared as upstream clears them.  One scan: a batch of one; UndistortBatch: one device call for all.
  bool UndistortCloud(const Matrix4d& T_we);
  void Reset();                                   // sensors/Velodyne.cpp:1676-1720: everything but the raw cloud, the pose and the flags
  static void UndistortBatch(const std::vector<Velodyne*>& scans, const std::vector<Matrix4d>& T_we);
  // ReOrderVLP (sensors/Velodyne.cpp:371-526): firing order -> ring order, range image, ring/column of every point.
  void ReOrderVLP();
  // ExtractFeatures (sensors/Velodyne.cpp:531-760), method ADAPTIVE only (config/Room.txt:32), PLANAR BRANCH: optional
  // range-image Segmentation (:1438-1586), adaptive-window curvature (:623-657), per-sector sort (:707-723),
  // ExtractEdgeFeatures2 (:883-1000) and ExtractPlaneFeatures2 (:1098-1189, surfLessFlat through the 0.2 m voxel grid).
  // Fills cornerSharp / cornerLessSharp (intensity = index into cloud_scan) / surfFlat / surfLessFlat and, between the
  // edge and the planar picks like upstream (:752), runs EdgeToLine unless edge_to_line is false (cornerLessSharp is then
  // the reference's cornerBeforeFilter and no segments exist).  Sequential per scan (a state machine, a BFS and greedy
  // non-maximum suppression over 28.8 k points): host code, like upstream; run it under `omp parallel for` over scans
  // as lidar_mapping/LidarOdometry.cpp:131-147 does.  Throws std::invalid_argument for another method.
  void ExtractFeatures(float max_curvature = 50, float intersect_angle_threshold = 5, int method = ADAPTIVE, bool segment = true,
                       ExtractionTrace* trace = nullptr, bool edge_to_line = true);
  // EdgeToLine (sensors/Velodyne.cpp:1269-1324) with ExtractLineFeatures (sensors/LidarLineExtraction.cpp:296-389): line
  // segments grown from the edge points -> edge_segmented / segment_coeffs / end_points / point_to_segment, cornerLessSharp
  // and cornerSharp filtered down to the members of segments.  Upstream's RANSAC line fit of a fused group
  // (pcl::SACSegmentation, :150-160) is replaced by the exhaustive 2-point maximum-consensus line (host/pvlm_lines.cpp).
  // grown: the growth phase done ahead for this scan's edge points by K27 (pvlm_line_grow_batch: every (start point, neighbour pair) task of the scan grown on the
  // GPU) — the walk over the start points, the fusion and the filters run here on its segments.  Null (or a result the device gave back, status != 0): the growth
  // runs here too, segment after segment as upstream.  PVLM_EDGE_GROW=tasks: the host itself grows every task through the kernel's code (csrc/pvlm_linegrow_core.h)
  // and replays the walk — the CPU check of the task formulation (tests/test_lines_cpu.py).
  void EdgeToLine(const pvlm_line_grow_result* grown = nullptr);
  // ReOrderVLP + ExtractFeatures for MANY scans: the per-point / per-ring stages (ring and column of every return, range image,
  // Segmentation, adaptive-window curvature — sensors/Velodyne.cpp:371-526, :1438-1586, :623-657), the sector orders, the picks of
  // ExtractEdgeFeatures2 / ExtractPlaneFeatures2 and the pcl::VoxelGrid of the less-flat points (:883-1000, :1098-1189) run on the GPU
  // (pvlm_ring_extract_batch_picks; a call's scans go as a few device batches that overlap the host work of the previous one), EdgeToLine
  // and the assembly of the clouds on `num_threads` host threads.  A scan with a ring the device left undecided, and every scan of a
  // batch the device refused (non-finite coordinate, capacity), takes the host's own picks / extraction.  Every scan ends
  // up exactly as ReOrderVLP() + ExtractFeatures(...) leave it (tests/test_host_gpu.py), except that Layout().range_image and
  // .image_to_point_idx are only filled when traces are asked for (nothing downstream reads them).  Scans that ReOrderVLP /
  // ExtractFeatures would leave alone (invalid, already re-ordered, no points) are skipped; all scans of a call share N_SCANS and
  // horizon_scans of the first.  Call from the thread that owns the engine.
  static void ExtractFeaturesBatch(const std::vector<Velodyne*>& scans, float max_curvature = 50, float intersect_angle_threshold = 5, int method = ADAPTIVE,
                                   bool segment = true, bool edge_to_line = true, int num_threads = 1, std::vector<ExtractionTrace>* traces = nullptr);
  // Segmentation (sensors/Velodyne.cpp:1438-1586): the points of small range-image components dropped from cloud_scan; returns 1 like upstream
  // (sensors/Velodyne.h:184).  Needs the range image ReOrderVLP built.
  int Segmentation();
  // ReOrderVLP() + Segmentation() for MANY scans (the first loop of Texture::ColorizeLidarPointCloud, mvs/Texture.cpp:29-37): one
  // pvlm_ring_extract_batch(segment = 1) per part of the list, cloud_scan / point_idx_to_image / scanStartInd / scanEndInd assembled from its source, ring_col
  // and ring_count as ExtractFeaturesBatch does, on `num_threads` host threads; Layout().range_image and .image_to_point_idx are not filled (nothing
  // downstream reads them).  Scans already re-ordered (cloud_scan not empty), scans with no points, scans whose range-image shape differs from the first
  // batched one and every scan of a part the device refused (a non-finite coordinate) take the per-scan host path, ReOrderVLP() then Segmentation(), so
  // each ends up as those two calls leave it.  The deliberate divergence: an invalid scan is left untouched (an empty cloud_scan after LoadLidar) —
  // upstream runs Segmentation() on it without a range image, which is undefined behaviour.  Call from the thread that owns the engine.
  static void SegmentBatch(const std::vector<Velodyne*>& scans, int num_threads = 1);
  const RingLayout& Layout() const { return layout_; }
  void Transform2LidarWorld();                    // :1773-1808  (float clouds, in place)
  void Transform2Local();                         // :1810-1848
  // Every scan of the list to the world (local) frame — the loops of LidarOdometry.cpp:148-152 and :120-130 over all scans: the host's clouds are
  // transformed scan-parallel, the device copies of the resident scans IN PLACE by one pvlm_scan_transform_batch (K26: the same float arithmetic,
  // the voxel grids rebuilt from device-side bounding boxes on the way to the world frame) — a scan is uploaded once per EstimatePose, not once per
  // outer iteration.  PVLM_HOST_REUPLOAD=1: the device copies are dropped instead and uploaded again by the next association (the round-5 path;
  // tests compare the two).
  static void TransformBatch(const std::vector<Velodyne*>& scans, bool to_world, int num_threads);

  // device mirror of the clouds (uploaded lazily by the association entry points)
  pvlm_scan* DeviceScan() const;
  static void UploadBatch(const std::vector<const Velodyne*>& scans);   // all of them that are not resident yet, in one pvlm_scan_upload_batch
  void InvalidateDevice() const;
  void PoseChanged() const;                       // the device copy learns the pose the setters stored
  ~Velodyne();
  Velodyne(const Velodyne& o);
  Velodyne& operator=(const Velodyne& o);

 private:
  Matrix3d R_wl_;
  Vector3d t_wl_;
  bool world_ = false;
  RingLayout layout_;
  // the second half of ExtractFeatures (:707-753, ExtractEdgeFeatures2, EdgeToLine, ExtractPlaneFeatures2) from the per-point arrays
  // per-point arrays the picks read (cloud_scan.size() entries each; the caller keeps them alive).  Window ends: left / right, or — when both are
  // null — index -+ half_window (-1 = no window).  sorted / sector_host: the sector orders of pvlm_ring_result, or null = sort every sector here.
  struct PickInputs {
    const float* curvature; const float* range; const int* left; const int* right; const int* half_window; const int* sorted; const unsigned char* sector_host;
  };
  void PickFeatures(float max_curvature, float intersect_angle_threshold, const PickInputs& in, ExtractionTrace* trace, bool edge_to_line);
  // the same from the picks the device made (pvlm_ring_extract_batch_picks, K24): the clouds are assembled ring by ring, EdgeToLine runs here
  void AssemblePicks(const pvlm_ring_result& r, ExtractionTrace* trace, bool edge_to_line, const pvlm_line_grow_result* grown = nullptr);
  mutable pvlm_scan* dev_ = nullptr;
};

// ---- lidar_mapping/LidarFeatureAssociate.h ------------------------------------------------------------
struct Point2Plane { Vector3d point; Vector4d plane_coeff; };
struct Point2Line { Vector3d point, line_point1, line_point2; };
struct Line2Line { int neighbor_line_idx, ref_line_idx; Vector3d line_point1, line_point2; };

std::vector<std::vector<int>> FindNeighbors(const std::vector<Velodyne>& lidars, const int neighbor_size);
std::vector<std::vector<int>> FindNeighborsConsecutive(const std::vector<Velodyne>& lidars, const int neighbor_size);
std::vector<Point2Plane> AssociatePoint2Plane(const Velodyne& ref_lidar, const Velodyne& nei_lidar, double plane_tolerance,
                                              const float dist_threshold = 0.7f, bool visualization = false);
std::vector<Line2Line> AssociateLine2Line(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const float dist_threshold = 0.7f,
                                          bool visualization = false);
// The k-NN based variants (lidar_mapping/LidarFeatureAssociate.cpp:238-440, :478-548; used when
// config.point_to_line_residual is set — not by the Room/Floor configs).  The 5-NN search in ref.cornerLessSharp runs on
// the GPU (pvlm_knn), the per-query 5-point PCA / segment counting on the host.
std::vector<Point2Line> AssociatePoint2Line(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const float dist_threshold = 0.7f,
                                            bool visualization = false);
std::vector<Point2Line> AssociatePoint2LineSegmentKNN(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const float dist_threshold = 0.7f,
                                                      bool visualization = false);
std::vector<Point2Line> AssociatePoint2LineSegment(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const float dist_threshold = 0.7f,
                                                   bool visualization = false);
std::vector<Line2Line> AssociateLine2LineKNN(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const float dist_threshold = 0.7f,
                                             bool visualization = false);
// Extension (not in PanoVLM): the AssociateLine2Line calls of a whole outer iteration in one GPU launch;
// result[k] equals AssociateLine2Line(*pairs[k].first, *pairs[k].second, dist_threshold).
std::vector<std::vector<Line2Line>> AssociateLine2LineBatch(const std::vector<std::pair<const Velodyne*, const Velodyne*>>& pairs,
                                                            const float dist_threshold = 0.7f);
std::vector<Vector6d> TransformLines(const std::vector<Vector6d>& line_coeffs, const Matrix4d& T);
std::vector<Line2Line> FindAssociations(const Velodyne& ref_lidar, const Velodyne& nei_lidar, const std::vector<Vector6d>& ref_world,
                                        const std::vector<Vector6d>& nei_world, const std::vector<int>& line_matrix);

// ---- util/Tracks.h + lidar_mapping/LidarLineMatch.h ----------------------------------------------------
struct LineTrack {
  uint32_t id = 0;
  std::set<std::pair<uint32_t, uint32_t>> feature_pairs;  // {lidar id, line id}
  bool IsInside(const std::pair<uint32_t, uint32_t>& p) const { return feature_pairs.count(p) > 0; }
};
struct Exchange;
class LidarLineMatch {
 public:
  explicit LidarLineMatch(const std::vector<Velodyne>& lidars) : lidars_(lidars) {}
  void SetNeighborSize(int n) { neighbor_size_ = n; }
  void SetMinTrackLength(int n) { min_track_length_ = n; }
  // Sharded run: this rank associates the pairs of the scans [first, last) only — AssociateLine2Line of :68 is per pair —
  // and the matches of all ranks are concatenated through the exchange (two small all-reduces: the match counts per pair, then the matches)
  // before the union-find, which every rank runs on the complete list: the tracks are the same on every rank and equal to the one-process run's.
  void SetShard(const Exchange* exchange, size_t first, size_t last) { exchange_ = exchange; first_ = first; last_ = last; }
  bool GenerateTracks();
  const std::vector<LineTrack>& GetTracks() const { return tracks_; }
 private:
  const std::vector<Velodyne>& lidars_;
  int neighbor_size_ = 4, min_track_length_ = 3;
  std::vector<LineTrack> tracks_;
  const Exchange* exchange_ = nullptr;
  size_t first_ = 0, last_ = 0;
};

// ---- the ceres:: surface the reference touches -----------------------------------------------------------
namespace ceres_like {

class CostFunction {
 public:
  virtual ~CostFunction() {}
  // ceres::CostFunction::Evaluate: parameters = {aa_r, t_r, aa_n, t_n}; jacobians may be null, and each
  // jacobians[i] may be null.  Evaluated on the GPU (one-row residual set) — API parity, not the fast path.
  // The reprojection functor has THREE blocks {aa_cw, t_cw, point_3d} (num_blocks == 3).
  bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const;
  int num_blocks = 4;
  int kind = 0;
  unsigned flags = 0;
  double weight = 1.0;
  std::vector<double> row;  // the ABI row of this block
};
class LossFunction { public: virtual ~LossFunction() {} virtual pvlm_loss kind() const = 0; virtual double a() const = 0; };
class HuberLoss : public LossFunction {
 public:
  explicit HuberLoss(double a) : a_(a) {}
  pvlm_loss kind() const override { return PVLM_LOSS_HUBER; }
  double a() const override { return a_; }
 private:
  double a_;
};

class Problem {
 public:
  Problem();
  ~Problem();
  // Takes ownership of cost (and of loss, shared by many blocks like in Ceres).
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* aa_r, double* t_r, double* aa_n, double* t_n);
  // Bulk form (extension): n blocks of one functor on the same four parameter blocks, rows = n x stride in the ABI row
  // layout of include/pvlm.h — what n X::Create + AddResidualBlock calls would add, without n heap objects.
  void AddResidualRows(int kind, unsigned flags, double weight, LossFunction* loss, double* aa_r, double* t_r, double* aa_n, double* t_n,
                       const double* rows, size_t n);
  // Three-block form of AddCameraResidual (util/Optimization.cpp:198-201): camera pose + a free 3-D point.
  // The point blocks live on the GPU during Solve and are eliminated there (Schur complement).
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* aa_c, double* t_c, double* point_3d);
  // Device-resident hand-off: a residual set produced by the association kernels; segment p uses
  // the parameter blocks (aa[ref_p], t[ref_p], aa[nei_p], t[nei_p]) of the given lists (ids = list index).
  void AddResidualSet(pvlm_resset* set, LossFunction* loss, std::vector<Vector3d>* aa_list, std::vector<Vector3d>* t_list);
  void SetParameterBlockConstant(double* block);
  // Registers every (angle-axis, translation) pair of the two lists as a pose, in list order, before any residual block
  // is added: pose ids then equal list indices on every rank of a sharded solve (otherwise ids follow first use).
  void RegisterPoses(std::vector<Vector3d>& aa_list, std::vector<Vector3d>& t_list);
  int NumResidualBlocks() const;
  struct Impl;
  Impl* impl() const { return impl_; }
 private:
  Problem(const Problem&) = delete;
  Impl* impl_;
};

}  // namespace ceres_like

// ---- multi-GPU: how the ranks of a sharded solve add up their normal equations ------------
// One process per GPU.  Every rank holds all scans and the full pose vector; a rank builds residual blocks only for its
// block of REFERENCE scans (the `i` loop of util/Optimization.cpp:521-560 and :345-441), evaluates them on its GPU and
// the ranks sum [cost | g | 6x6 blocks] once per evaluation.  Everything else of the LM iteration is replicated: the
// summed system is bit-identical on every rank, so every rank takes the same decisions and no parameter broadcast is needed.
// allreduce_sum: in place on a HOST buffer, must leave the same bits on every rank (RCCL's ring all-reduce does; the
// file exchange sums in rank order).
struct Exchange {
  int world = 1, rank = 0;
  std::function<void(double* buf, size_t count)> allreduce_sum;
  bool active() const { return world > 1 && (bool)allreduce_sum; }
  // block partition of n reference scans, the same rule as panovlm_amd/sharding.py
  std::pair<size_t, size_t> Range(size_t n) const { return {n * (size_t)rank / (size_t)world, n * ((size_t)rank + 1) / (size_t)world}; }
  // contiguous ranges of (nearly) equal summed weight: boundary r is the first scan whose weight prefix reaches r / world of the
  // total.  With weight(i) = sum of the query counts of i's neighbour scans this is SURVEY.md §8 E's "rebalancing by sum Nq":
  // temporal neighbour lists give every scan the same weight, loop-closure pairs make some scans heavier.  Every rank computes
  // the same boundaries from the same (replicated) weights.  All-zero weights: Range(n).
  std::pair<size_t, size_t> BalancedRange(const std::vector<double>& weight, int of_rank = -1) const;
};
// RCCL over xGMI through the C ABI (pvlm_comm_* on the engine's context): `id` = the 128 bytes rank 0 got from
// pvlm_comm_unique_id, carried to the other ranks by the launcher.  Collective: every rank calls it.
Exchange MakeRcclExchange(int world, int rank, const unsigned char id[128]);
// Ranks on one host exchanging through a directory (functional tests on a one-GPU box; not a fast path).
Exchange MakeFileExchange(int world, int rank, const std::string& dir);

namespace ceres_like {

enum LinearSolverType { DENSE_SCHUR, SPARSE_SCHUR, ITERATIVE_SCHUR };
struct Solver {
  struct Options {
    const Exchange* exchange = nullptr;   // sharded solve: see Exchange (the Problem must have its poses registered with RegisterPoses)
    bool minimizer_progress_to_stdout = false;
    int num_threads = 1;
    int max_num_iterations = 50;
    int max_linear_solver_iterations = 500;
    LinearSolverType linear_solver_type = DENSE_SCHUR;
    // Ceres 2.0 trust-region defaults ([recalled])
    double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32;
    double min_relative_decrease = 1e-3, function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
    double min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
  };
  struct Summary {
    double initial_cost = 0, final_cost = 0;
    int num_successful_steps = 0, num_unsuccessful_steps = 0;
    int num_residual_blocks = 0;
    bool usable = false;
    std::string message;
    std::vector<double> cost_history;
    bool IsSolutionUsable() const { return usable; }
    std::string BriefReport() const;
  };
};
void Solve(const Solver::Options& options, Problem* problem, Solver::Summary* summary);

}  // namespace ceres_like

// ---- base/CostFunction.h functors: X::Create(...) ------------------------------------------------------
struct Point2Plane_Meter { static ceres_like::CostFunction* Create(const Vector3d& curr_point, const Vector4d& plane, const double weight = 1); };
struct Point2Plane_Angle { static ceres_like::CostFunction* Create(const Vector3d& curr_point, const Vector4d& plane, const bool normalize, const double weight = 1); };
struct Point2Line_Meter { static ceres_like::CostFunction* Create(const Vector3d& curr_point, const Vector3d& last_point_a, const Vector3d& last_point_b, const double weight = 1); };
struct Point2Line_Angle { static ceres_like::CostFunction* Create(const Vector3d& curr_point, const Vector3d& last_point_a, const Vector3d& last_point_b, const bool normalize, const double weight = 1); };
struct Plane2Plane_Global { static ceres_like::CostFunction* Create(const Vector3d& plane_ref, const Vector3d& point_a, const Vector3d& point_b, const double w = 1.0); };
struct PlaneIOUResidual { static ceres_like::CostFunction* Create(const Vector4d& ref_plane, const Vector3d& middle_neighbor, const Vector3d& middle_ref, const double angle, const double weight = 1.0); };
// base/CostFunction.h:218-247 — AutoDiffCostFunction<.,1,3,3,3> on (angleAxis_cw, t_cw, point_3d)
struct PanoramaReprojResidual_1Angle { static ceres_like::CostFunction* Create(const Vector3d& pt, double weight = 1.0); };
constexpr int kReprojKind = 100;   // CostFunction::kind of the three-block functor (not a pvlm_functor)
// base/CostFunction.h:178-214 — AutoDiffCostFunction<.,2,3,3,3>: pt = sphere angles (lon, lat) of the keypoint (K31)
struct PanoramaReprojResidual_2Angle { static ceres_like::CostFunction* Create(const Vector2d& pt, double weight = 1.0); };
// base/CostFunction.h:249-288 — AutoDiffCostFunction<.,2,3,3,3>: pt = keypoint pixel (x, y), rows x cols image (K31)
struct PanoramaReprojResidual_Pixel { static ceres_like::CostFunction* Create(const Vector2d& pt, const int rows, const int cols, double weight = 1.0); };
constexpr int kReprojKind2Angle = 101, kReprojKindPixel = 102;
inline pvlm_ba_kind ReprojBaKind(int cost_kind) {
  return cost_kind == kReprojKindPixel ? PVLM_BA_PIXEL : (cost_kind == kReprojKind2Angle ? PVLM_BA_ANGLE2 : PVLM_BA_ANGLE1);
}

// ---- util/Optimization.h ---------------------------------------------------------------------------------
size_t AddLidarPointToPlaneResidual(const std::vector<std::vector<int>>& neighbors, const std::vector<Velodyne>& lidars,
                                    std::vector<Vector3d>& angleAxis_lw_list, std::vector<Vector3d>& t_lw_list,
                                    ceres_like::Problem& problem, double point_to_plane_dis_threshold, double plane_tolerance,
                                    bool angle_residual, bool normalized_distance, double weight = 1.0,
                                    const std::pair<size_t, size_t>* ref_range = nullptr /* sharded run: reference scans [first, second) only */);
// util/Optimization.cpp:443-504 — only pairs of consecutive scans (|n_idx - i| <= 1) get point-to-line blocks
size_t AddLidarPointToLineResidual(const std::vector<std::vector<int>>& neighbors, const std::vector<Velodyne>& lidars,
                                   std::vector<Vector3d>& angleAxis_lw_list, std::vector<Vector3d>& t_lw_list, ceres_like::Problem& problem,
                                   double point_to_line_dis_threshold, bool use_segment, bool angle_residual, bool normalized_distance,
                                   double weight = 1.0, const std::pair<size_t, size_t>* ref_range = nullptr);
size_t AddLidarLineToLineResidual2(const std::vector<std::vector<int>>& neighbors, const std::vector<Velodyne>& lidars,
                                   std::vector<Vector3d>& angleAxis_lw_list, std::vector<Vector3d>& t_lw_list,
                                   ceres_like::Problem& problem, const std::vector<LineTrack>& lidar_line_tracks,
                                   double point_to_line_dis_threshold, bool angle_residual, bool normalized_distance, double weight = 1.0,
                                   const std::pair<size_t, size_t>* ref_range = nullptr);
// AddCameraLidarResidual (util/Optimization.cpp:564-607): two blocks per matched line pair —
// Plane2Plane_Global (weight line_pair.weight * weight) and PlaneIOUResidual (weight 2 * weight) — on
// (angleAxis_cw[frame], t_cw[frame], angleAxis_lw[lidar], t_lw[lidar]).  `frame_pose_valid[f]` stands for
// frames[f].IsPoseValid(); rows/cols are the panorama size (frames[0].GetImageRows/Cols).
struct CameraLidarLinePair;
size_t AddCameraLidarResidual(int rows, int cols, const std::vector<bool>& frame_pose_valid, const std::vector<Velodyne>& lidars,
                              std::vector<Vector3d>& angleAxis_cw_list, std::vector<Vector3d>& t_cw_list,
                              std::vector<Vector3d>& angleAxis_lw_list, std::vector<Vector3d>& t_lw_list,
                              const std::map<std::pair<size_t, size_t>, std::vector<CameraLidarLinePair>>& line_pairs,
                              ceres_like::LossFunction* loss_function, ceres_like::Problem& problem, double weight);
ceres_like::Solver::Options SetOptionsLidar(const int num_threads, const int lidar_size);
ceres_like::Solver::Options SetOptionsSfM(const int num_threads);                      // util/Optimization.cpp:608-634
// util/Tracks.h:109-133 — a triangulated feature track: (frame index, keypoint index) pairs + the 3-D point
struct PointTrack {
  uint32_t id = 0xffffffffu;
  std::set<std::pair<uint32_t, uint32_t>> feature_pairs;
  Vector3d point_3d{{0, 0, 0}};
};
enum RESIDUAL_TYPE { ANGLE_RESIDUAL_1 = 0, ANGLE_RESIDUAL_2 = 1, PIXEL_RESIDUAL = 2 };
struct Frame;
// AddCameraResidual (util/Optimization.cpp:172-222): one block per (track, observation) whose frame has a valid pose.
//   ANGLE_RESIDUAL_1 (the one Optimize uses, CameraLidarOptimizer.cpp:431-432): PanoramaReprojResidual_1Angle, bearing =
//     eq.ImageToCam(keypoint.pt) — which resolves to the cv::Point2i overload, i.e. the keypoint is rounded to the nearest
//     pixel (cvRound) and un-projected in float; HuberLoss(4 deg).
//   ANGLE_RESIDUAL_2: PanoramaReprojResidual_2Angle on eq.ImageToSphere(keypoint.pt) (float template); HuberLoss(4 deg).
//   PIXEL_RESIDUAL: PanoramaReprojResidual_Pixel on keypoint.pt widened to double; HuberLoss(4.0).
size_t AddCameraResidual(const std::vector<Frame>& frames, std::vector<Vector3d>& angleAxis_cw_list, std::vector<Vector3d>& t_cw_list,
                         std::vector<PointTrack>& structure, ceres_like::Problem& problem, int residual_type, double weight);

// ---- K31: global bundle adjustment of the SfM result and the track filters after it ---------------------------------
// SfMGlobalBA (util/Optimization.cpp:10-82): T_cw = GetPose()^-1 (rigid inverse, the mirror's convention; upstream's general
// Eigen inverse differs by ~1e-16) -> angle-axis, AddCameraResidual(residual_type, weight 1), constant blocks for
// refine_rotation / translation / structure = false, the FIRST valid frame's aa and t constant, SetOptionsSfM, Solve.  Returns false
// when all three refine flags are false or the solution is not usable; otherwise writes SetPose(T_cw^-1) back into the valid frames and
// the refined points into the tracks.  The reprojection blocks are solved on the GPU (K9 / K31, points eliminated there).
bool SfMGlobalBA(std::vector<Frame>& frames, std::vector<PointTrack>& tracks, int residual_type, int num_threads, bool refine_structure = true,
                 bool refine_rotation = true, bool refine_translation = true, ceres_like::Solver::Summary* summary = nullptr);
// FilterTracksPixelResidual / FilterTracksAngleResidual (sfm/Structure.cpp:121-193) on the GPU (pvlm_filter_tracks): the surviving tracks
// keep their order; returns the number removed.  Invalid frames use T_cw = 0 and are not skipped (an observation there projects to the
// image centre, pixel filter, or gives a NaN cosine that never rejects, angle filter).  threshold < 0: the pixel filter removes nothing.
size_t FilterTracksPixelResidual(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold);
size_t FilterTracksAngleResidual(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold);
// SfM::GlobalBundleAdjustment (sfm/SfM.cpp:1362-1383): SfMGlobalBA then the filter of the residual type (pixel for PIXEL_RESIDUAL,
// angle for the angle types).  False when the BA fails (the structure is then left unfiltered).
bool GlobalBundleAdjustment(std::vector<Frame>& frames, std::vector<PointTrack>& structure, int residual_type, float residual_threshold,
                            bool refine_structure = true, bool refine_rotation = true, bool refine_translation = true, int num_threads = 1);
// MVS::RefineCameraPose (mvs/MVS.cpp:383-428): keeps T_cl = T_wc^-1 T_wl of every frame / scan pair valid on both sides, runs the pixel
// BA with everything free, then re-poses the scans as T_wc T_cl.  The image scale of upstream's frames does not exist in the mirror: the
// BA works on full-resolution keypoints, which is what upstream's SetImageScale(0) restores.  The PCD / pose-file exports are left out.
bool RefineCameraPose(std::vector<Frame>& frames, std::vector<Velodyne>& lidars, std::vector<PointTrack>& structure, const Config& config);

// util/FileIO.cpp:11-79, :168-191 — pose text files: one row per pose, optional name + 12 numbers
// (R row-major interleaved with t: r00 r01 r02 tx r10 r11 r12 ty r20 r21 r22 tz); rows containing
// "inf"/"nan" are invalid poses (R = 0, t = inf) and are kept only when with_invalid is set.
// ExportPoseT writes with the ostream default precision (6 significant digits) like the reference;
// pass precision = 17 for a lossless file.
bool ReadPoseT(std::string file_path, bool with_invalid, std::vector<Matrix3d>& rotation_list, std::vector<Vector3d>& trans_list,
               std::vector<std::string>& name_list);
void ExportPoseT(const std::string file_path, const std::vector<Matrix3d>& rotation_list, const std::vector<Vector3d>& trans_list,
                 const std::vector<std::string>& name_list, int precision = 6);

// FormLine(points, tolerance, dis_threshold) of base/Geometry.hpp:220-260 on n x 3 doubles: false (and a zero line) when the
// points do not form a line; line = (centroid, unit direction)
bool FormLine3D(const double* pts, int n, double tolerance, double dis_threshold, double* line);

// ceres/rotation.h pieces the callers use (lidar_mapping/LidarOdometry.cpp:31,105)
void RotationMatrixToAngleAxis(const Matrix3d& R, Vector3d* angle_axis);
void AngleAxisToRotationMatrix(const Vector3d& angle_axis, Matrix3d* R);

// ---- lidar_mapping/LidarOdometry.h --------------------------------------------------------------------------
class LidarOdometry {
 public:
  LidarOdometry(const std::vector<Velodyne>& lidars, const Config& config) : lidars(lidars), config(config) {}
  // EstimatePose(max_iteration): outer loop of LidarOdometry.cpp:116-187 WITHOUT the feature extraction
  // (the scans handed in already carry their feature clouds — SURVEY.md §8 A0 / "next" row N3).
  bool EstimatePose(const int max_iteration);
  bool RefinePose(double& cost, int& steps, bool use_segment);
  // lidar_mapping/LidarOdometry.cpp:189-263 without the PCD export: every scan with a usable pose is motion-compensated with the pose that ends its sweep
  // (the next usable scan's pose through SlerpPose; the last scan continues the motion of the one before), all scans in one device call
  bool UndistortLidars(const float gap_time);
  // lidar_mapping/LidarOdometry.cpp:306-: upstream reloads the raw scans from their files before the motion compensation (EstimatePose moved the clouds to the
  // world frame and back in float, and may have dropped them); the in-memory form of that reload: scan k gets clouds[k] again
  void ReloadClouds(const std::vector<PointCloud>& clouds);
  void ResetAllLidars();                          // lidar_mapping/LidarOdometry.cpp:295-304 (the reload of an empty cloud is LoadLidar's business)
  // lidar_mapping/LidarOdometry.cpp:323-348: the fused map of every (skip + 1)-th scan in the world frame (FuseLidarScans below; one device call)
  PointCloud FuseLidar(int skip = 2, double min_range = 0, double max_range = 100);
  const std::vector<Velodyne>& GetLidarData() const { return lidars; }
  std::vector<Matrix3d> GetGlobalRotation() const;
  std::vector<Vector3d> GetGlobalTranslation() const;
  // per-outer-iteration log (cost, successful steps, residual blocks) for tests
  struct IterLog { double cost; int steps; int residual_blocks; };
  std::vector<IterLog> log;
  // sharded runs, per outer iteration: this rank's range of reference scans, the association queries (sum Nq over the pairs of
  // a rank's reference scans) of EVERY rank — computed from the replicated neighbour lists — and this rank's own residual blocks
  struct ShardLog { size_t first, last; std::vector<double> queries_per_rank; int local_blocks; };
  std::vector<ShardLog> shard_log;
  // Sharded run (one process per GPU): set before EstimatePose / RefinePose on every rank.  Association and
  // residual evaluation are done for the rank's block of reference scans only; poses, neighbour lists and line tracks are
  // replicated.  residual_blocks in the log is then the sum over the ranks.
  void SetExchange(const Exchange& e) { exchange_ = e; }
 private:
  std::vector<Velodyne> lidars;
  Config config;
  Exchange exchange_;
};

// The body of LidarOdometry::FuseLidar / CameraLidarOptimizer::FuseLidar (lidar_mapping/LidarOdometry.cpp:323-348): scans i = 0, skip + 1, 2 (skip + 1), ... that
// are valid with a valid pose (the stride does not re-sync after a skipped scan); an empty `cloud` is reloaded from `name` (LoadLidar: cloud_scan untouched, and a
// reload that leaves the scan invalid still contributes, as upstream's check came before it); the points of cloud_scan when it is non-empty, of cloud otherwise.
// Point selection and transform: pvlm_fuse_scans (K29), one call for all scans.  The one deliberate divergence: skip < 0, which never ends upstream, throws
// std::invalid_argument.
PointCloud FuseLidarScans(std::vector<Velodyne>& lidars, int skip, double min_range, double max_range);
// pcl::io::savePCDFileBinary<pcl::PointXYZI>(path, cloud): header lines "# .PCD v0.7 - Point Cloud Data file format", VERSION 0.7, FIELDS x y z intensity,
// SIZE 4 4 4 4, TYPE F F F F, COUNT 1 1 1 1, WIDTH n, HEIGHT 1, VIEWPOINT 0 0 0 1 0 0 0, POINTS n, DATA binary, then n packed 16-byte records.  An empty
// cloud writes nothing and returns false (PCL refuses it).  The layout is recalled from PCL 1.x, not pinned against a PCL build.
bool SavePCDFileBinary(const std::string& file_path, const PointCloud& cloud);

// base/Geometry.hpp:572-583: the pose a fraction `ratio` of the way from pose_w1 to pose_w2 (rotation by slerp, translation of T_21 scaled)
Matrix4d SlerpPose(const Matrix4d& pose_w1, const Matrix4d& pose_w2, double ratio);

// ---- sensors/Equirectangular.h + joint_optimization/CameraLidarLineAssociate.h -------------------------------
struct CameraLidarLinePair {
  std::array<float, 4> image_line{{0, 0, 0, 0}};
  Vector3d lidar_line_start{{0, 0, 0}}, lidar_line_end{{0, 0, 0}};
  int image_line_id = -1, lidar_line_id = -1;
  float angle = -1, weight = 1;
};
class CameraLidarLineAssociate {
 public:
  CameraLidarLineAssociate(int rows, int cols) : rows(rows), cols(cols) {}
  // AssociateByAngle (CameraLidarLineAssociate.cpp:340-475): `lidar` carries LOCAL-frame corner points.
  void AssociateByAngle(const std::vector<std::array<float, 4>>& lines, const Velodyne& lidar, const Matrix4d& T_cl,
                        const bool multiple_association = true, const std::vector<bool>& image_line_mask = {},
                        const std::vector<bool>& lidar_line_mask = {});
  // Same with the vote matrix (n_lines x n_segments, from pvlm_cam_lidar_votes[_batch]) handed in — lets
  // AssociateLineMulti run the voting loops of all (frame, LiDAR) pairs in one launch.
  void AssociateByAngleWithVotes(const std::vector<std::array<float, 4>>& lines, const Velodyne& lidar, const Matrix4d& T_cl, const int* votes,
                                 const bool multiple_association = true, const std::vector<bool>& image_line_mask = {},
                                 const std::vector<bool>& lidar_line_mask = {});
  const std::vector<CameraLidarLinePair>& GetAssociatedPairs() const { return line_pairs; }
 private:
  void Filter(bool filter_by_angle, bool filter_by_length);
  void UniqueLinePair(const std::vector<std::array<float, 4>>& lines, const std::vector<Vector3d>& lidar_lines_endpoint);
  int rows, cols;
  std::vector<CameraLidarLinePair> line_pairs;
};


// util/Visualization.h:407-441 — sparse LiDAR depth image (uint16 depth * 256, row-major rows x cols) seen from the
// camera: the LiDAR-seeded depth prior of mvs/MVS.cpp:510-514.  `cloud` is in the LiDAR frame.
std::vector<uint16_t> ProjectLidar2PanoramaDepth(const PointCloud& cloud, const int rows, const int cols, const Matrix4d& T_cl, const size_t size = 3);

// ---- joint_optimization/CameraLidarOptimizer.h (mapping mode) --------------------------------------------------
// sensors/Frame.h contract as far as the path needs it: image size, pose T_wc, the detected image lines
// (image_lines_all[frame].GetLines()).
// cv::Mat of type CV_8UC1 as far as the feature path reads it (the grey image of a frame, a mask): rows x cols bytes, row-major; no pixels = an empty Mat
struct GrayImage {
  int rows = 0, cols = 0;
  std::vector<unsigned char> pixels;
  bool empty() const { return pixels.empty(); }
};
// cv::KeyPoint as SIFT fills it (pt.x, pt.y, size, angle, response, octave): the record of pvlm_sift_keypoint (K41)
struct KeyPoint { float x, y, size, angle, response; int octave; };

struct Frame {
  int id = 0, rows = 2880, cols = 5760;
  Matrix3d R_wc{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  Vector3d t_wc{{0, 0, 0}};
  bool pose_valid = true;
  std::vector<std::array<float, 4>> lines;
  std::vector<std::array<float, 2>> keypoints;   // GetKeyPoints()[k].pt (SIFT keypoints, pixels)
  std::vector<float> descriptor;                 // GetDescriptor(): rows x 128 floats, row-major, row k the SIFT descriptor of keypoints[k] (K33)
  std::vector<KeyPoint> keypoints_all;           // the full records behind `keypoints` (sensors/Frame.h: keypoints_all), filled by ExtractKeyPoints / ReadImages (K41)
  GrayImage img_gray;                            // LoadImageGray's result; ReadImages releases it as upstream does
  std::vector<float> sift_rows;                  // the plain descriptor rows of keypoints_all as ExtractKeyPoints' device call returned them (ComputeDescriptor's source)
  // sensors/Frame.cpp:110-121.  ExtractKeyPoints: ExtractSIFTQuadtree(img_gray, keypoints_all, 0, num_keypoints, mask) as ONE pvlm_sift_extract call that also
  // brings the plain descriptor rows (the pyramid exists only inside that call), `keypoints` set beside it.  ComputeDescriptor: those rows, RootSIFT applied on
  // request -- bit for bit ComputeSIFTDescriptor(img_gray, keypoints_all, descriptor, root_sift), which it falls back to (host compile) only when keypoints_all did
  // not come from ExtractKeyPoints alone.  One image per call: SfM's loop is ReadImages below.
  bool ExtractKeyPoints(int num_keypoints, const GrayImage& mask);
  bool ComputeDescriptor(bool root_sift);
  bool IsPoseValid() const { return pose_valid; }
  int GetImageRows() const { return rows; }
  int GetImageCols() const { return cols; }
  Matrix4d GetPose() const { return {R_wc[0], R_wc[1], R_wc[2], t_wc[0], R_wc[3], R_wc[4], R_wc[5], t_wc[1], R_wc[6], R_wc[7], R_wc[8], t_wc[2], 0, 0, 0, 1}; }
};

// ---- K32: structure from the image matches (sfm/Structure.cpp:8-119, sfm/Triangulate.cpp, util/Tracks.cpp) ---------------------------------
// base/Serialization.h's MatchPair as far as TriangulateTracks reads it: the two images and the (queryIdx, trainIdx) of every cv::DMatch,
// queryIdx a keypoint of image_pair.first, trainIdx one of image_pair.second
struct MatchPair {
  std::pair<size_t, size_t> image_pair;
  std::vector<std::pair<int, int>> matches;
};
// TriangulateTracks (sfm/Structure.cpp:8-69): TrackBuilder.Build / Filter(3) / ExportTracks (util/Tracks.cpp, on the union-find the line tracks
// use), every track with an id < GetMaxID() (strict, as upstream writes it) triangulated in ONE pvlm_triangulate_tracks call (K32), the tracks
// with an infinite coordinate dropped (a NaN point stays: upstream's trap), then FilterTracksAngleResidual(frames, structure, 25).  The output is
// in ascending track id: what one thread gives upstream, whose own order is whatever its OpenMP critical section gives.  A track with an
// observation in a frame without a valid pose is dropped (status 2 of pvlm_triangulate_tracks, the deliberate divergence documented in pvlm.h).
std::vector<PointTrack> TriangulateTracks(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs);
// FilterTracksToFar (:87-119) on the GPU (pvlm_filter_tracks_far): a track goes when the mean distance of its point to its valid frames' centres
// exceeds threshold x the largest distance between two of those centres.  The surviving tracks keep their order; returns the number removed.
size_t FilterTracksToFar(const std::vector<Frame>& frames, std::vector<PointTrack>& tracks, const double& threshold);
// Triangulate2View (sfm/Triangulate.cpp:8-28) and TriangulateNView (:198-226) on host vectors: csrc/pvlm_triangulate_core.h compiled for the
// host, for callers with a handful of points.  Bearings are cv::Point3f; fewer than two views give +inf on all coordinates.
Vector3d Triangulate2View(const Matrix3d& R_21, const Vector3d& t_21, const std::array<float, 3>& p1, const std::array<float, 3>& p2);
Vector3d TriangulateNView(const std::vector<Matrix3d>& R_cw_list, const std::vector<Vector3d>& t_cw_list, const std::vector<std::array<float, 3>>& points);
// MVS::EstimateStructure (mvs/MVS.cpp:44-59): structure = TriangulateTracks(frames, image_pairs), true when it is not empty.  No SetImageScale and
// no points.bin export, for the reasons RefineCameraPose gives; the match pairs are the caller's (upstream: ReadMatchPair) or MatchImagePairs' (K33).
bool EstimateStructure(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<PointTrack>& structure);

// ---- K33: the image matches (util/SIFT.cpp:130-162, sfm/SfM.cpp:229-295) --------------------------------------------------------------------------
// cv::DMatch as far as the pipeline reads it
struct DMatch { int queryIdx, trainIdx; float distance; };
// MatchSIFT (util/SIFT.cpp:130-162, the brute-force branch): knnMatch(descriptor1, descriptor2, 2) and the ratio test
// distance0 < dist_ratio_threshold * distance1, on two host arrays of rows x 128 floats: csrc/pvlm_match_core.h compiled for the host, for a
// caller with one small pair.  A descriptor2 of one row gives no matches (upstream reads out of bounds there, see pvlm.h).
std::vector<DMatch> MatchSIFT(const std::vector<float>& descriptor1, const std::vector<float>& descriptor2, const float dist_ratio_threshold);
// SfM::MatchImagePairs (sfm/SfM.cpp:229-295) on the GPU: the descriptors of all frames go to the device once (pvlm_descset_create), every pair is
// matched and filtered there in ONE pvlm_match_pairs call (K33), and image_pairs is replaced by the surviving pairs with their matches, in the
// order of the input list (upstream: the order of an OpenMP critical section).  ratio is config.sift_match_dist_threshold.  The frames keep their
// descriptors (upstream releases them); no after_sift_match.txt.  False (image_pairs untouched) for a negative matches_threshold, a pair that names a
// frame that is not there, or a frame whose descriptor is not 128 floats per keypoint.
// The result feeds TriangulateTracks / EstimateStructure as it is.
bool MatchImagePairs(const std::vector<Frame>& frames, std::vector<MatchPair>& image_pairs, const float ratio, const int matches_threshold);
// the same on the host compile of the core, the pairs spread over num_threads workers: the baseline tools/match_bench.py times
bool MatchImagePairsHost(const std::vector<Frame>& frames, std::vector<MatchPair>& image_pairs, const float ratio, const int matches_threshold, const int num_threads = 16);

// ---- K41: SIFT keypoints and descriptors (util/SIFT.cpp:10-128, sensors/Frame.cpp:110-121, sfm/SfM.cpp:15-42) ---------------------------------------------------
// The definition is pvlm.h's K41 (csrc/pvlm_sift_core.h), with its divergences from OpenCV's SIFT.  A mask is an image of the same size or empty.
// ExtractSIFT (util/SIFT.cpp:22-30): detect(img_gray, keypoints, mask) of SIFT::create(num_sift), one pvlm_sift_extract call without descriptors; false for num_sift <= 0, a side below 8
// pixels, a mask of another size, or no keypoint.
bool ExtractSIFT(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, const int num_sift = 8096, const GrayImage& mask = GrayImage());
// ExtractSIFTQuadtree (:82-118) at tree_depth 0, what Frame::ExtractKeyPoints calls: one cell, the whole image, i.e. ExtractSIFT appended to `keypoints`; any other
// depth returns false and leaves `keypoints` untouched.  The default depth is therefore 0 here, not upstream's 1: a caller who relies on defaults gets the served case.
bool ExtractSIFTQuadtree(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, const int tree_depth = 0, const int num_sift = 8096, const GrayImage& mask = GrayImage());
// ComputeSIFTDescriptor (:120-128): the descriptors of ARBITRARY given keypoints, rows x 128 floats.  The C ABI computes descriptors only together with the detection
// (the pyramid lives inside that call), so this one-image call runs the host compile of the core (the pyramid, then every keypoint on the worker pool): about 2 s for
// a 5760 x 2880 panorama on 16 threads, bit-identical to the device's rows.  It is NOT on the path of ReadImages or of Frame::ExtractKeyPoints + ComputeDescriptor,
// which take their rows from the device call; it serves a caller with keypoints of its own.  Open: a compute-only entry point.
bool ComputeSIFTDescriptor(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, std::vector<float>& descriptor, const bool root_sift = false);
// RootSIFT (:10-21) on rows x 128 floats: per row L1-normalise, square root, x 512 (upstream's order of operations); a zero row stays zero.
void RootSIFT(std::vector<float>& descriptor);
// detect + compute of one image on the host compile of the core, on num_threads workers: the baseline tools/sift_bench.py times, and the fallback without a device
bool ExtractSIFTHost(const GrayImage& img_gray, const GrayImage& mask, const int num_sift, const bool root_sift, std::vector<KeyPoint>& keypoints,
                     std::vector<float>& descriptor, const int num_threads = 16);
// Fills `image` with the grey image of frame `frame` (frames[frame].rows x cols); false = no image.
using GrayImageProvider = std::function<bool(size_t frame, GrayImage& image)>;
// SfM::ReadImages (sfm/SfM.cpp:15-42) for frames that exist already (id, rows, cols): in id order, images_per_call frames at a time, the images asked of the
// provider, ONE pvlm_sift_extract call per group (ExtractKeyPoints and ComputeDescriptor of every frame of the group; its buffers sized by num_sift per image plus
// room for ties, a second call only if more keypoints tie at the threshold than that room), keypoints_all / keypoints / descriptor filled, the images released.  False (frames untouched) when an image is missing or of another size than the first, or num_sift <= 0.
bool ReadImages(std::vector<Frame>& frames, GrayImageProvider images, const GrayImage& mask, const int num_sift, const bool root_sift, const int images_per_call = 8);
// the pvlm_sift_extract calls the functions above have made in this process (what the driver counts)
long SiftDeviceCalls();

// ---- K34: relative poses from the matches (sfm/SfM.cpp:298-480, base/EssentialMatrix.cpp, base/ACRansac_NFA.cpp) ---------------------------------
// base/Serialization.h's MatchPair as FilterImagePairs leaves it, up to and not including RefineRelativePose
struct RelativePair {
  std::pair<size_t, size_t> image_pair;
  std::vector<std::pair<int, int>> matches;     // (queryIdx, trainIdx), as in MatchPair
  Matrix3d R_21; Vector3d t_21;
  std::vector<size_t> inlier_idx;               // CheckRT's inliers of the winning run, indices into matches, ascending
  std::vector<Vector3d> triangulated;           // their points in the first camera's frame
  int points_with_depth = 0;                    // K36, SetTranslationScaleDepthMap: the triangulated points with a real depth in both depth maps ...
  double upper_scale = -1, lower_scale = -1;    // ... and the largest / smallest scale kept (0 = the median fall-back; -1 = never scaled: util/MatchPair.h's constructors)
  MatchPair AsMatchPair() const { MatchPair p; p.image_pair = image_pair; p.matches = matches; return p; }
};
// what upstream fixes in the source (40 runs of 300 iterations) and what it draws from std::random_device (here: a seed, see csrc/pvlm_essential_core.h)
struct EssentialOptions { int n_runs = 40; int max_iterations = 300; unsigned long long seed = 0; bool fresh_sample = false; };
// ComputeEssential (base/EssentialMatrix.cpp:10-40) and DecomposeEssential (:151-178) on the host compile of csrc/pvlm_essential_core.h (cyclic Jacobi for both of
// Eigen's decompositions: parity by tolerance)
Matrix3d ComputeEssential(const std::vector<std::array<float, 3>>& points1, const std::vector<std::array<float, 3>>& points2);
bool DecomposeEssential(const Matrix3d& E_21, std::vector<Matrix3d>& rotations, std::vector<Vector3d>& translations);
// FindEssentialACRANSAC (:180-288) on the host: ONE run (`run` selects the stream of the pair (first, second)); zero matrix = no model.  `precision` is gone:
// upstream forces ac_ransac_mode.  Fewer than 9 matches give zero (see pvlm.h).
Matrix3d FindEssentialACRANSAC(const std::vector<DMatch>& matches, const std::vector<std::array<float, 3>>& points1, const std::vector<std::array<float, 3>>& points2,
                               const int max_iterations, std::vector<size_t>& inlier_idx, const std::pair<size_t, size_t>& image_pair = {0, 1}, const int run = 0,
                               const EssentialOptions& options = EssentialOptions());
// SfM::CheckRT (sfm/SfM.cpp:1478-1547) without parallax (its reader is commented out upstream)
int CheckRT(const Matrix3d& R_21, const Vector3d& t_21, const std::vector<bool>& is_inlier, const std::vector<DMatch>& matches, const std::vector<std::array<float, 3>>& keypoints1,
            const std::vector<std::array<float, 3>>& keypoints2, std::vector<Vector3d>& triangulated_points, std::vector<size_t>& inlier_idx);
// the loop of SfM::FilterImagePairs over every pair, up to and not including RefineRelativePose, in ONE pvlm_filter_image_pairs call (K34): the surviving pairs with
// R_21, t_21, inlier_idx and triangulated, in the order of the input list.  The bearings are eq.ImageToCam of the frames' keypoints (:311-319).  False for a pair or
// a match that names what is not there.  Chains after MatchImagePairs.
bool FilterImagePairs(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<RelativePair>& good_pair, const int triangulation_num_threshold,
                      const EssentialOptions& options = EssentialOptions());
// the same on the host compile of the core, the pairs spread over num_threads workers: the baseline tools/essential_bench.py times
bool FilterImagePairsHost(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, std::vector<RelativePair>& good_pair, const int triangulation_num_threshold,
                          const EssentialOptions& options = EssentialOptions(), const int num_threads = 16);

// ---- K36: the rest of SfM::FilterImagePairs (sfm/SfM.cpp:436-476): RefineRelativePose, the scale from the depth maps, the pair graph ---------------------------------
// SfMLocalBA (util/Optimization.cpp:84-170) for one pair on the host compile of csrc/pvlm_relpose_core.h: camera 1 the identity and constant, camera 2 and the pair's
// triangulated points free, two blocks per inlier; residual_type PIXEL_RESIDUAL (HuberLoss(4.0)) or ANGLE_RESIDUAL_2 (HuberLoss(4 deg)); ANGLE_RESIDUAL_1 throws.  The
// write-back: R_21 from the angle-axis, t_21 normalised, the points divided by |t|.  Returns isfinite(final cost).  The header lists the deliberate divergences.
bool SfMLocalBA(const Frame& frame1, const Frame& frame2, int residual_type, RelativePair& image_pair);
// SfM::RefineRelativePose (sfm/SfM.cpp:482-485): SfMLocalBA(frames[first], frames[second], PIXEL_RESIDUAL, pair)
bool RefineRelativePose(const std::vector<Frame>& frames, RelativePair& image_pair);
// every pair of the list in ONE pvlm_refine_relative_poses call (K36).  ok (or null): per pair what SfMLocalBA returns.  False, with the list untouched, for what the
// call refuses (a frame, match or inlier index out of range, a value that is not finite).
bool RefineRelativePoses(const std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, int residual_type = PIXEL_RESIDUAL, std::vector<bool>* ok = nullptr);
// the same on the host compile of the core, the pairs spread over num_threads workers: the baseline tools/relpose_bench.py times and the equality partner of the call
bool RefineRelativePosesHost(const std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, int residual_type = PIXEL_RESIDUAL, std::vector<bool>* ok = nullptr,
                             const int num_threads = 16);
// The depth maps of the frames (upstream: frames[i].depth_map, a CV_16U image of depth x 256 read from a file): maps[f] is rows[f] x cols[f], row-major; an empty
// vector means the frame has none.  ComputeDepthImage / ComputeDepthImageHost below (K37) make them from the LiDAR scans.
struct DepthMaps { std::vector<std::vector<uint16_t>> maps; std::vector<int> rows, cols; };
// ---- K37: the depth maps (util/DepthCompletion.cpp:154-316, sfm/SfM.cpp:170-226) ---------------------------------------------------------------
// DepthCompletion(sparse_depth, max_depth) on the whole-image host loop of csrc/pvlm_depthfill_core.h (the stages, the OpenCV semantics they rest on and the
// deliberate divergence of the bilateral filter are stated there): image is rows x cols floats, row-major, metres; returns the dense image.  A negative or
// non-finite value throws std::invalid_argument.  For a caller with one image; pvlm_depth_completion takes batches on the GPU.
std::vector<float> DepthCompletion(const std::vector<float>& image, const int rows, const int cols, const float max_depth);
// The loop of SfM::ComputeDepthImage over all frames in ONE pvlm_compute_depth_images call (K37): for frame i ProjectLidar2PanoramaDepth(clouds[i], rows, cols, T_cl,
// 4), DepthCompletion(.., max_depth), x 256, CV_16U, with rows = (image_rows + 1) / 2 and cols = (image_cols + 1) / 2 when half_size (upstream's choice) and the image
// size otherwise.  clouds[i] is the scan of frame i in the LiDAR frame, T_cl the one calibration.  Upstream's lidars.size() != frames.size() refusal:
// std::invalid_argument.  No visualisation, no files.  The result is what FilterImagePairsFull takes.
DepthMaps ComputeDepthImage(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows, const int image_cols,
                            const float max_depth, const bool half_size = true);
// the same on the host loop of the core, the frames spread over num_threads workers: the baseline tools/depthfill_bench.py times and the equality partner of the call
DepthMaps ComputeDepthImageHost(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows, const int image_cols,
                                const float max_depth, const bool half_size = true, const int num_threads = 16);
// SfM::SetTranslationScaleDepthMap(eq, pair) (:487-603) operation by operation: the half-size test, round, IsInside, the 0.2 consistency test, two histogram passes
// (the 1e-8 offset, the clamped bin index, the > 0.1 num_scale keep rule), the nth_element median fall-back.  The host route: right for maps that exist only as files and are read once; maps made by K37 take the DeviceDepthMaps route below.
bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DepthMaps& depth_maps, RelativePair& image_pair);
// the list form (:605-679): the frames are visited from the one with the fewest pairs on, the pairs that touch a frame in list order; a pair without a scale stays
// only when keep_no_scale.  Returns whether any pair is left.
bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DepthMaps& depth_maps, std::vector<RelativePair>& image_pairs, const bool keep_no_scale);
// SfM::LargestBiconnectedGraph (:780-799; PoseGraph::KeepLargestEdgeBiconnected sfm/PoseGraph.cpp:63-133) without lemon: bridges by one depth-first search, then the
// connected component with the most nodes.  Deliberate divergence: among components of equal size the one that holds the lowest frame id wins.
std::vector<RelativePair> LargestBiconnectedGraph(const std::vector<RelativePair>& pairs, std::set<size_t>& nodes);
// SfM::FilterImagePairs (:298-480) end to end: FilterImagePairs (K34), RefineRelativePoses (K36; a failed refinement is kept, upstream's `continue` is commented
// out), SetTranslationScaleDepthMap, LargestBiconnectedGraph, and the final sort with upstream's comparator as written (first <, else second <; run as the insertion
// sort std::sort uses on short ranges, see pvlm_host_relpose.hpp).  good_pair and covered_frames are upstream's image_pairs and covered_frames afterwards.
bool FilterImagePairsFull(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                          std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale, const EssentialOptions& options = EssentialOptions());
// the same through FilterImagePairsHost and RefineRelativePosesHost (no device)
bool FilterImagePairsFullHost(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                              std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale,
                              const EssentialOptions& options = EssentialOptions(), const int num_threads = 16);

// ---- K39: the depth maps kept on the device, the scales set there --------------------------------------------------------------------------------------------
// The owner of a pvlm_depthset of the engine's context: the maps of all frames where K37 writes them (ComputeDepthImageResident) or where UploadDepthMaps puts
// them.  Movable, not copyable.  Destroy it on the thread that owns the engine.
class DeviceDepthMaps {
 public:
  DeviceDepthMaps() = default;
  explicit DeviceDepthMaps(pvlm_depthset* set, size_t n_frames) : set_(set), n_frames_(n_frames) {}
  ~DeviceDepthMaps();
  DeviceDepthMaps(DeviceDepthMaps&& o) noexcept : set_(o.set_), n_frames_(o.n_frames_) { o.set_ = nullptr; o.n_frames_ = 0; }
  DeviceDepthMaps& operator=(DeviceDepthMaps&& o) noexcept;
  DeviceDepthMaps(const DeviceDepthMaps&) = delete;
  DeviceDepthMaps& operator=(const DeviceDepthMaps&) = delete;
  pvlm_depthset* set() const { return set_; }
  size_t size() const { return n_frames_; }
  // rows and cols of a frame's map; 0 x 0: the frame has none
  std::pair<int, int> Info(size_t frame) const;
 private:
  pvlm_depthset* set_ = nullptr;
  size_t n_frames_ = 0;
};
// ComputeDepthImage with the maps left on the device (pvlm_depthset_compute): nothing of them crosses to the host
DeviceDepthMaps ComputeDepthImageResident(const std::vector<Frame>& frames, const std::vector<PointCloud>& clouds, const Matrix4d& T_cl, const int image_rows,
                                          const int image_cols, const float max_depth, const bool half_size = true);
// host maps (read from files) to the device, one allocation per frame; an empty vector stays an empty frame
DeviceDepthMaps UploadDepthMaps(const DepthMaps& depth_maps);
// one map back (what a caller needs to write upstream's depth file of the frame); an empty vector for an empty frame
std::vector<uint16_t> ReadDepthMap(const DeviceDepthMaps& depth_maps, size_t frame, int* rows = nullptr, int* cols = nullptr);
// the list form of SetTranslationScaleDepthMap on resident maps: ONE pvlm_set_translation_scales call (K39) on the distinct pairs of the list, then upstream's
// visiting order (as above) with the call's results in place of the per-pair step.  The same list, bit for bit, as the DepthMaps overload gives on the same maps.
bool SetTranslationScaleDepthMap(const std::vector<Frame>& frames, const DeviceDepthMaps& depth_maps, std::vector<RelativePair>& image_pairs, const bool keep_no_scale);
// FilterImagePairsFull on resident maps: K34, K36, K39, then LargestBiconnectedGraph and the sort on the host
bool FilterImagePairsFull(const std::vector<Frame>& frames, const std::vector<MatchPair>& image_pairs, const DeviceDepthMaps& depth_maps, std::vector<RelativePair>& good_pair,
                          std::set<size_t>& covered_frames, const int triangulation_num_threshold, const bool keep_no_scale, const EssentialOptions& options = EssentialOptions());

// ---- K42: translation averaging (sfm/TranslationAveraging.cpp:31-204, :419-481; sfm/SfM.cpp:908-934, :1047-1344, :1385-1421) ----------------------------------
// sfm/SfM.h:71-76.  SOFTL1 and L2IRLS are built, and BATA (K44), CHORDAL and LUD (K46, below) behind TranslationOptions::enable_bata / enable_chordal / enable_lud;
// L1 (the triplet minimax programme, K47, below) behind enable_l1.  Without its flag a method gets upstream's "not supported".
enum TranslationAveragingMethod { TRANSLATION_AVERAGING_SOFTL1 = 1, TRANSLATION_AVERAGING_L1 = 2, TRANSLATION_AVERAGING_CHORDAL = 3, TRANSLATION_AVERAGING_L2IRLS = 4,
                                  TRANSLATION_AVERAGING_BATA = 5, TRANSLATION_AVERAGING_LUD = 6 };
// sfm/BATA.h's BATAConfig: what TranslationAveragingBATA hands BATA (upstream: always the defaults, :516)
struct BATAConfig { double delta = 1e-6; int init_iteration = 10, inner_iteration = 10, outer_iteration = 10; double robust_threshold = 0.1; };
// what base/Config.h holds for the stage, and what upstream draws from srand(time): the start translations are uniform [-1, 1] from splitmix64 on `seed` (K34's
// answer to std::random_device).  host = true runs every solve through the host compile of csrc/pvlm_transavg_core.h (pvlm_host_transavg.hpp; no device).
// message: where the text of upstream's LOG(ERROR) goes when the call returns false.
struct TranslationOptions {
  bool use_all_pairs_ta = true, init_translation_DLT = true, init_translation_GPS = false;
  std::string gps_path;
  int num_iteration_L2IRLS = 10;
  float upper_scale_ratio = 1.3f, lower_scale_ratio = 0.9f;
  unsigned long long seed = 0;
  bool host = false;
  std::string* message = nullptr;
  // Method 5 (BATA, K44) runs only when this is set.  The flag exists because tests/test_transavg_cpu.py::test_estimate_methods_not_built pins method 5 under default
  // options to upstream's "not supported" text and existing tests do not change; a later change that may edit that test removes it.
  bool enable_bata = false;
  BATAConfig bata;
  // Methods 3 (chordal) and 6 (LUD), K46, run only when these are set: the same test pins them under default options, for the same reason.
  bool enable_chordal = false, enable_lud = false;
  // Method 2 (L1, K47) runs only when this is set: the same test pins it under default options, for the same reason.
  bool enable_l1 = false;
  // Method 2 takes its triplets from FindTripletDevice (K48, pvlm_host_triplet.hpp) instead of FindTriplet and the std::map lookups when this is set.  Opt-in, as
  // the flags above: without it the call runs the code it always ran.
  bool device_triplets = false;
};
// TranslationAveragingDLT (:31-84) through pvlm_transavg_dlt: the normal equations with camera 0 fixed at zero.  Upstream's SparseQR returns SOME basic solution of a
// system that is rank-deficient by the gauge t_i = R_i c; every caller runs SetToOrigin afterwards, which cancels the difference.  false: a pair names a camera
// past global_translations (upstream writes out of range), or the system is not positive definite (a pair graph that is not connected).
bool TranslationAveragingDLT(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const bool host = false);
// TranslationAveragingL2 (:87-169) through pvlm_transavg_solve (see pvlm.h for the definition and its divergences).  loss_a stands for the ceres::LossFunction*:
// SoftLOneLoss(loss_a), none when negative.  `weight` is read by nobody upstream (the functor never applies it) and is only written.  false: the summary is not usable.
bool TranslationAveragingL2(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, std::vector<double>& scales, const size_t origin_idx,
                            std::vector<double>& weight, double& costs, const double loss_a, const float upper_scale_ratio, const float lower_scale_ratio, const bool host = false);
// :171-204
bool TranslationAveragingSoftL1(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const double l1_loss_threshold,
                                const float upper_scale_ratio, const float lower_scale_ratio, const bool host = false);
// :419-481: at most num_iteration solves; stops when the cost moved by less than 5 % or is below 10 (as written, :443); after a solve that did not stop, the pairs whose
// scale went negative are dropped from image_pairs.  iterations_run: the solves done.
bool TranslationAveragingL2IRLS(std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const int num_iteration,
                                const float upper_scale_ratio, const float lower_scale_ratio, const bool host = false, int* iterations_run = nullptr);
// K44 — TranslationAveragingBATA (:483-525) through pvlm_transavg_bata (see pvlm.h for the definition and its divergences), as written: per pair the observation
// R_wc(frames[new_to_old[first]]) t_21, its norm as the start scale — none when 0.99 < norm < 1.01 (sfm/BATA.cpp:191-193) — and its direction; the centres come back
// as -R_cw centre per camera (:519-523).  Upstream draws the start scale of a pair without one as |Eigen's Random()| after srand(time) (sfm/BATA.cpp:64); here it is
// |uniform[-1, 1]| from splitmix64 on seed ^ 0xba7a5ca1e5ull — a stream of its own, distinct from the start translations' (which run on the seed itself) — with an
// exact zero drawn again.  config stands for upstream's default-constructed BATAConfig.  global_translations is resized to max_id - min_id + 1 as upstream's
// assignment does.  start_scales: when given, the scales handed to the solver (the tests look at the draw).  false: no pairs, a camera without an entry in
// new_to_old, a relative translation of zero length or not finite, or info != 0 (not positive definite / not finite).
bool TranslationAveragingBATA(const std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                              const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const BATAConfig& config = BATAConfig(), const unsigned long long seed = 0,
                              const bool host = false, std::vector<double>* start_scales = nullptr);
// K46 — TranslationAveragingL2Chordal (:206-274) through pvlm_transavg_chordal (see pvlm.h for the definition and its divergences), as written: t_cw -> t_wc at
// entry with the rotation of frames[new_to_old[i]] (:216-220), per pair dir = R_w2 t_21.normalized() (:225-226), HuberLoss(l2_loss_threshold), back to t_cw at exit
// (:267-271).  false: a camera without an entry in new_to_old, a pair that names a camera past global_translations, a relative translation of zero length or not
// finite, or a summary that is not usable (the initial cost not finite: two cameras on one point).
bool TranslationAveragingL2Chordal(const std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                                   const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const double l2_loss_threshold, const bool host = false);
// K46 — TranslationAveragingLUD (:527-660) through pvlm_transavg_lud, as written: the start scales are |t_21|, or 1 for a pair without lower_scale / upper_scale
// (:536-542), the weights start at 1; at most num_iteration solves, each followed by the new weights and sum_e = sum |e| (:615-626); the loop stops when
// |last - curr| / curr < 0.05 || curr < 10 (:628); after a solve that did not stop, the pairs whose scale went negative are dropped from image_pairs (:635-651).
// No input reaches that drop: every scale is held at or above 0.5 s0 or 1 by its parameter bound and the clamp puts every candidate on it; it is built as written.
// iterations_run: the solves done.  false: as for the chordal function.
bool TranslationAveragingLUD(std::vector<RelativePair>& image_pairs, const std::vector<Frame>& frames, std::vector<Vector3d>& global_translations,
                             const std::map<size_t, size_t>& new_to_old, const size_t origin_idx, const int num_iteration, const float upper_scale_ratio,
                             const float lower_scale_ratio, const bool host = false, int* iterations_run = nullptr);
// K47 — TranslationAveragingL1 (:277-417) through pvlm_transavg_l1 (see pvlm.h for the definition and its divergences: an interior-point method, a point near the
// centre of the optimal face where upstream returns a vertex, further triplet components pinned, cameras in no triplet left at zero), as written: the triplets of
// PoseGraph::FindTriplet over the pair list, a repeated pair resolved to its last index through the map (:289); upstream's new_to_old is read by nobody and is not
// taken.  The call starts from t = 0.  summary: the call's, when given.  false: global_translations[origin_idx] not zero (upstream asserts), a pair with
// first >= second or a camera past global_translations (upstream reads another pair's data or writes out of range), or a solve that did not converge ("Solve linear
// program failed").  A pair list without a triplet leaves every translation zero and returns true.
// device_triplets: the triplets and their pair indices come from FindTripletDevice (K48: pvlm_triplets_find; with host, the host compile of its core) instead of
// FindTriplet and three std::map lookups per triplet; the same triplet_pairs either way.
bool TranslationAveragingL1(const std::vector<RelativePair>& image_pairs, std::vector<Vector3d>& global_translations, const size_t origin_idx, const bool host = false,
                            pvlm_translp_summary* summary = nullptr, const bool device_triplets = false);
// SfM::ReIndex (sfm/SfM.cpp:908-934): the frame ids of a pair list onto 0 .. n - 1 in ascending order
void ReIndex(const std::vector<RelativePair>& pairs, std::map<size_t, size_t>& forward, std::map<size_t, size_t>& backward);
// SfM::SetToOrigin (:1385-1421) without the structure: every valid pose into the frame of frames[frame_idx] (the first valid frame when that one has no pose).
// A pose is valid as sensors/Frame.cpp:203-208 writes it (finite translation, rotation not zero); pose_valid is kept equal to that.
bool SetToOrigin(std::vector<Frame>& frames, size_t frame_idx);
// SfM::EstimateGlobalTranslation (:1047-1344), operation by operation: the frames with a rotation, the scaled / unscaled split, LargestBiconnectedGraph, both
// re-indexings, the DLT start with its SetToOrigin, the solve, t_wc = -R_wc t_cw, the final filter of the pairs.  frames[i].R_wc holds the global rotations (all zero:
// none); image_pairs is replaced by the pairs with a global pose.  Divergences: the random start (TranslationOptions::seed); :1183 hands the DLT ALL pairs under the
// global indices with an output sized by the scaled component — followed as written whenever every index fits, refused with a message when one does not (upstream
// writes out of range); GPS is not supported.
bool EstimateGlobalTranslation(std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, const int method, const TranslationOptions& options = TranslationOptions());

// ---- K40: rotation averaging (sfm/RotationAveraging.cpp:11-183, :278-582; sfm/PoseGraph.cpp:195-226; sfm/SfM.cpp:705-778, :811-905) ------------------------------
// base/common.h.  L1 (the method of both shipped configs) is built, and L2 (its start RotationAveragingLeastSquare: K45, below) behind
// RotationOptions::enable_l2_start; without the flag EstimateGlobalRotation returns false for method 2 with the message it has always had.
enum RotationAveragingMethod { ROTATION_AVERAGING_L1 = 1, ROTATION_AVERAGING_L2 = 2 };
// what base/Config.h holds for the stage.  host = true runs every solve through the host compiles of csrc/pvlm_rotavg_core.h and csrc/pvlm_rotstart_core.h
// (pvlm_host_rotavg.hpp, pvlm_host_rotstart.hpp; no device).  message: where the text of upstream's LOG(ERROR) goes when the call returns false.
struct RotationOptions {
  bool use_all_pairs_ra = true;
  bool host = false;
  std::string* message = nullptr;
  // Method 2 (the least-square start, K45, then RotationAveragingL2) runs only when this is set.  The flag exists because tests/test_rotavg_cpu.py::
  // test_estimate_global_rotation_host and tests/test_rotavg_gpu.py pin method 2 under default options to its refusal and existing tests do not change; a later
  // change that may edit those tests removes it.
  bool enable_l2_start = false;
  // FilterByTriplet(pairs, 0.1) runs as FilterByTripletDevice (K48, pvlm_host_triplet.hpp) when this is set.  Opt-in: without it the call runs the code it always ran.
  bool device_triplets = false;
};
struct Triplet { uint32_t i, j, k; };
// PoseGraph::FindTriplet (sfm/PoseGraph.cpp:195-226): per edge in the set's order, the nodes adjacent to both its ends, then the edge leaves the adjacency
std::vector<Triplet> FindTriplet(const std::set<std::pair<size_t, size_t>>& edges);
// SfM::FilterByTriplet (:705-778) as written: a triplet is kept when acos(clamp(trace(R_13 R_32 R_21) / 3)) in degrees is below angle_threshold; the pairs of the
// kept triplets, then LargestBiconnectedGraph.  Every pair must have first < second (upstream asserts): an empty list comes back otherwise.
std::vector<RelativePair> FilterByTriplet(const std::vector<RelativePair>& init_pairs, const double angle_threshold, std::set<size_t>& covered_frames);
// FilterPairs (sfm/RotationAveraging.cpp:11-183): the X84 threshold (median + 5.2 MAD of the pair errors) when angle_threshold <= 0, then the frame rule of
// :101-165 (three neighbours before and three after within 10 frames, filled from the rejected pairs by ascending error).  threshold_out: the threshold in radians.
std::vector<RelativePair> FilterPairs(const std::vector<RelativePair>& image_pairs, const std::vector<Matrix3d>& global_rotations, double angle_threshold,
                                      double* threshold_out = nullptr);
// RotationAveragingSpanningTree (:278-315).  DIVERGENCE: upstream runs lemon's Kruskal over all-equal weights, whose edge order nothing here can pin down; this is
// Kruskal over the pairs in list order by union-find, the tree walked breadth-first from start_idx (a node's tree edges in the order they were taken); a child's
// rotation is R_cp R_parent.  false: the pairs do not reach every camera, or name one past global_rotations.
bool RotationAveragingSpanningTree(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx);
// RotationAveragingRefineL1 (:428-582), weight function 1, through pvlm_rotavg_l1 (see pvlm.h for the definition and its divergences).  false: the library refused
// the arguments (a camera pair named twice, which upstream's map would collapse, among them) or an IRLS system could not be factorised (:553-557).
bool RotationAveragingRefineL1(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx, const bool host = false);
// RotationAveragingL1 (:376-426): the spanning tree, the refinement, FilterPairs.  rotations_after_L1.txt is not written.
bool RotationAveragingL1(std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, size_t start_idx, double angle_threshold, const bool host = false);
// RotationAveragingL2 (:317-374) through pvlm_rotavg_l2.  false: the result is not finite, or the library refused the arguments — a pair list that FilterPairs left
// in more than one piece among them (upstream refines every piece; here the rotations stay as they came).
bool RotationAveragingL2(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, const bool host = false);
// K45 — RotationAveragingLeastSquare (:185-275) through pvlm_rotavg_least_square (see pvlm.h for the definition and its one divergence: the three eigenvectors come
// from shift-and-invert subspace iteration on the block-sparse matrix, not from a dense decomposition; the result depends on their span alone).  The iteration starts
// from RotationAveragingSpanningTree(pairs, rotations, 0).  global_rotations is written only on success.  false: no camera or no pair (upstream's "not enough
// data"), the pairs do not reach every camera, the library refused the arguments, or info != 0.
bool RotationAveragingLeastSquare(const std::vector<RelativePair>& image_pairs, std::vector<Matrix3d>& global_rotations, const bool host = false);
// SfM::EstimateGlobalRotation (:811-905), operation by operation: the use_all_pairs_ra filter, LargestBiconnectedGraph, FilterByTriplet(0.1), ReIndex, then
// method 1: RotationAveragingL1(pairs, rotations, 0, -1), RotationAveragingL2 (a failure is only reported, as upstream); method 2 with enable_l2_start:
// RotationAveragingLeastSquare (a failure returns false with upstream's "Rotation averaging L2 failed"), RotationAveragingL2 (reported only; no FilterPairs on this
// route, :859-869); then pair.R_21 = R_2w R_1w^T and frames[i].R_wc.  image_pairs is replaced by the pairs that survive.  false with a message: no pair survives
// the filters, a pair with first >= second, method 2 without its flag, or the first stage of the method failed.
bool EstimateGlobalRotation(std::vector<Frame>& frames, std::vector<RelativePair>& image_pairs, const int method, const RotationOptions& options = RotationOptions());

// ---- K35: the image pairs (sfm/VLAD.cpp, sfm/SfM.cpp:49-168) ------------------------------------------------------------------------------------------------
// base/common.h's FrameMatchMethod and sfm/VLAD.h's normalisation types
enum FrameMatchMethod { EXHAUSTIVE = 1, CONTIGUOUS = 2, VLAD = 4, GPS = 8, GPS_VLAD = 16 };
enum VLADNormalization { SIGNED_SQUARE_ROOTING = 0, INTRA_NORMALIZATION = 1, RESIDUAL_NORMALIZATION_PWR_LAW = 2 };
// sfm/VLAD.h's VLADMatcher on the GPU (K35): the three steps keep upstream's signatures.  The descriptors go to the device once, in the constructor (or the caller's
// set is used); the codebook is learned by pvlm_vlad_kmeans, the vectors stay on the device (pvlm_vlad_embed), the neighbour lists come from pvlm_vlad_neighbors.
// The draws (the `ratio` subset of the frames, the initial centre rows: distinct indices, unsorted, as CreateRandomArray gives them) come from a generator seeded
// with `seed` (upstream: an unseeded std::mt19937; there is nothing to be equal to).  host = true runs the same three steps through the host loops of
// csrc/pvlm_vlad_core.h on num_threads workers (no device): the baseline and the equality partner.
class VLADMatcher {
 public:
  VLADMatcher(const std::vector<Frame>& frames, const int normalization_type = RESIDUAL_NORMALIZATION_PWR_LAW, const unsigned long long seed = 0, const bool host = false,
              const int num_threads = 16, pvlm_descset* set = nullptr);
  ~VLADMatcher();
  VLADMatcher(const VLADMatcher&) = delete;
  VLADMatcher& operator=(const VLADMatcher&) = delete;
  bool GenerateCodeBook(float ratio, const int book_size = 128, const int max_iteration = 25);
  bool ComputeVLADEmbedding();
  std::vector<std::vector<size_t>> FindNeighbors(int neighbor_size);
  const std::vector<float>& GetCodeBook() const { return codebook_; }
  const std::vector<unsigned char>& GetAlive() const { return alive_; }
 private:
  const std::vector<Frame>& frames_;
  int normalization_type_, num_threads_, book_size_ = 0;
  unsigned long long seed_;
  bool host_, own_set_ = false, valid_ = true;
  pvlm_descset* set_ = nullptr;
  pvlm_vladset* vlad_ = nullptr;
  std::vector<float> codebook_, host_vlad_;
  std::vector<unsigned char> alive_;
};
// SfM::InitImagePairs (sfm/SfM.cpp:49-168) for EXHAUSTIVE, CONTIGUOUS (window 20) and VLAD (max(n / 40, 15) neighbours, ratio 0.5, 128 words, 25 iterations), with
// upstream's pair order and its de-duplication set; the VLAD part on the GPU (K35), the descriptor set created once.  GPS and GPS_VLAD return false and leave
// image_pairs untouched (the mirror's Frame has no GPS), as does a frame whose descriptor is not 128 floats per keypoint.  Otherwise true when there is a pair.
// book_size is upstream's default; the tests pass a smaller one for their small scenes.
bool InitImagePairs(const std::vector<Frame>& frames, const int frame_match_type, std::vector<MatchPair>& image_pairs, const unsigned long long seed = 0,
                    const int book_size = 128);
// the same through the host loops of the core on num_threads workers: the baseline tools/vlad_bench.py times and the equality partner of the tests
bool InitImagePairsHost(const std::vector<Frame>& frames, const int frame_match_type, std::vector<MatchPair>& image_pairs, const unsigned long long seed = 0,
                        const int book_size = 128, const int num_threads = 16);

// ---- mvs/MVS.h:45-57, mvs/MVS.cpp:334-382 — who the neighbours of a reference view are (the `nei` / R_nr / t_nr arguments of
// pvlm_mvs_*).  SelectNeighborKNN: the 3 x neighbor_size nearest camera centres (float32, as pcl::KdTreeFLANN returns them),
// the first hit skipped as "self", candidates closer than the squared distance threshold skipped, the first neighbor_size
// kept; T_nr = T_wn^-1 T_wr in double, stored as float (cv::Matx33f / cv::Vec3f).  The rigid inverse is used where
// upstream calls Eigen's general Matrix4d::inverse() — equal to ~1e-16 before the rounding to float.
struct NeighborInfo {
  size_t id = 0;
  std::array<float, 9> R_nr{};   // reference -> neighbour, row-major
  std::array<float, 3> t_nr{};
};
std::vector<std::vector<NeighborInfo>> SelectNeighborKNN(const std::vector<Frame>& frames, int neighbor_size, float sq_distance_threshold);
// SelectNeighborSFM (mvs/MVS.cpp:248-332, K49) and the dispatch SelectNeighborViews (:66-79): pvlm_host_neighbor.hpp

// ---- mvs/MVS.cpp:2168-2334 — MVS::FuseDepthImages(use_filtered_depth = true), the second half of MVS::FuseDepthMaps (:224-231; the first
// half, MergeDepthImages, is a loop over pvlm_mvs_depth_to_cloud).  The greedy confidence-weighted fusion walks frames by decreasing
// neighbour count and pixels in raster order; a pixel's fate depends on every claim made before it, so this is host code here as
// upstream.  DepthFrame holds the cv::Mat members of sensors/Frame.h the function touches.  Upstream's bookkeeping is kept: a depth map
// is released after (neighbours + 1) visits and read again from the depth FILE when needed as a neighbour (depth_file: the unfiltered
// estimate <id>_geo.bin / _pho.bin; empty = no file), a reference whose map is gone is skipped, the claim lists survive the `continue`
// of the sky-colour test.  depth_filter maps are modified (depths in front of which an accepted point lies are zeroed).
struct DepthFrame {
  int id = 0;
  std::vector<float> depth_filter;       // rows x cols, empty = cv::Mat::empty()
  std::vector<float> depth_file;         // rows x cols or empty
  std::vector<float> conf;               // rows x cols: <id>_filter.bin
  std::vector<unsigned char> bgr;        // rows x cols x 3
  Matrix4d T_wc{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
};
struct PointXYZRGB { float x, y, z; unsigned char r, g, b; };
std::vector<PointXYZRGB> FuseDepthImages(int rows, int cols, std::vector<DepthFrame>& frames, const std::vector<std::vector<NeighborInfo>>& neighbors, float max_depth,
                                         float depth_diff_threshold);

// ---- mvs/Texture.h, mvs/Texture.cpp — the coloured LiDAR map (main.cpp:524-552) ---------------------------------------------------------------
// A frame's colour image as the caller decoded it (no JPEG decoding here): rows x cols BGR8 pixels, row-major, 3 cols bytes per row — the size of
// frames[i] (GetImageRows / GetImageCols), i.e. already scaled as Frame::GetImageColor would return it.
struct ColorImage {
  int rows = 0, cols = 0;
  std::vector<unsigned char> bgr;
};
// Fills `image` with the colour image of frame `frame`; false = no image (ColorizeLidarPointCloud throws std::runtime_error).
using ColorImageProvider = std::function<bool(size_t frame, ColorImage& image)>;

// PointXYZRGB{x, y, z, r, g, b} as the 16-byte PCD record pcl::PointXYZRGB writes: x y z, then the colour word b | g << 8 | r << 16 | 255 << 24
inline unsigned ColourWord(const PointXYZRGB& p) { return (unsigned)p.b | ((unsigned)p.g << 8) | ((unsigned)p.r << 16) | (255u << 24); }

class Texture {
 public:
  // mvs/Texture.cpp:10-12.  images: where ColorizeLidarPointCloud gets frame i's colour image; it asks for the images of `images_per_call` pairs, colours
  // them in one device call and drops them before it asks for the next ones, so the images held at any time are those of one call.
  Texture(const std::vector<Velodyne>& lidars, const std::vector<Frame>& frames, const Config& config, ColorImageProvider images = nullptr)
      : lidars(lidars), frames(frames), config(config), images_(std::move(images)) {}
  void SetImageProvider(ColorImageProvider images) { images_ = std::move(images); }
  int images_per_call = 16;
  // mvs/Texture.cpp:14-80: every scan with a valid pose is loaded again (LoadLidar(name)) and segmented (Velodyne::SegmentBatch); then for every pair i whose
  // scan and frame poses are valid, the points of cloud_scan in range whose pixel of frame i is not sky are kept with that pixel's colour, in the LiDAR frame
  // (pvlm_colorize_scans, K30; T_cl = T_wc^-1 T_wl with the rigid inverse, the project's convention — see SelectNeighborKNN).  Deliberate divergences:
  // lidars and frames of different sizes throw std::invalid_argument (upstream asserts); an invalid scan (Velodyne::valid false) contributes no points
  // (upstream's Segmentation of it is undefined behaviour).
  bool ColorizeLidarPointCloud(const double min_dist = 0, const double max_dist = 1000);
  // mvs/Texture.cpp:82-97: the coloured clouds of pairs i = 0, skip + 1, ... whose scan pose is valid, moved to the world frame (pcl::transformPointCloud in
  // double, pvlm_fuse::transform_point; the colour copied) and concatenated, on host threads.  skip < 0 throws std::invalid_argument (upstream asserts).
  std::vector<PointXYZRGB> FuseCloud(int skip = 1);
  const std::vector<std::vector<PointXYZRGB>>& GetColoredLidar() const { return lidar_colored; }
  const std::vector<Velodyne>& GetLidars() const { return lidars; }

 private:
  std::vector<Velodyne> lidars;
  std::vector<Frame> frames;
  std::vector<std::vector<PointXYZRGB>> lidar_colored;   // LiDAR frame
  const Config config;
  ColorImageProvider images_;
};
// pcl::io::savePCDFileBinary<pcl::PointXYZRGB>: FIELDS x y z rgb, SIZE 4 4 4 4, TYPE F F F F, COUNT 1 1 1 1, then n 16-byte records x y z and the bytes
// b g r 255.  Recalled from PCL 1.x, not pinned against a PCL build.  An empty cloud writes nothing and returns false, as for PointXYZI.
bool SavePCDFileBinary(const std::string& file_path, const std::vector<PointXYZRGB>& cloud);

class CameraLidarOptimizer {
 public:
  using LinePairs = std::map<std::pair<size_t, size_t>, std::vector<CameraLidarLinePair>>;
  // LiDAR scans are handed in in their LOCAL frame with feature clouds + segments (ExtractLidarLines, :151-175)
  CameraLidarOptimizer(const Matrix4d& T_cl, const std::vector<Velodyne>& lidars, const std::vector<Frame>& frames, const Config& config,
                       int neighbor_size_joint = 3, int num_iteration_joint = 5)
      : T_cl_init(T_cl), lidars(lidars), frames(frames), config(config), neighbor_size_joint(neighbor_size_joint), num_iteration_joint(num_iteration_joint) {}
  // JointOptimize(true), MAPPING mode loop of CameraLidarOptimizer.cpp:260-285.  The SfM reprojection term
  // (AddCameraResidual, free 3-D points) is added when a structure has been set (SetStructure stands for
  // ReadPointTracks(points.bin), :255); with an empty structure the problem has the LiDAR terms only.
  bool JointOptimize();
  void SetStructure(const std::vector<PointTrack>& s) { structure = s; }
  const std::vector<PointTrack>& GetStructure() const { return structure; }
  // CameraLidarOptimizer.cpp:720-729: structure = TriangulateTracks(frames, image_pairs), then FilterTracksToFar(frames, structure, 8); false when
  // that filter removed NOTHING (upstream's `if(!FilterTracksToFar(...)) return false`, kept as written), the structure stays filled either way
  bool EstimateStructure(const std::vector<MatchPair>& image_pairs);
  std::vector<std::vector<int>> NeighborEachFrame(const int neighbor_size, const bool temporal) const;   // :551-610
  LinePairs AssociateLineMulti(const int neighbor_size, const bool temporal = true);                      // :331-384
  int Optimize(const LinePairs& line_pairs, std::vector<PointTrack>& structure, const bool refine_camera_rotation, const bool refine_camera_trans,
               const bool refine_lidar_rotation, const bool refine_lidar_trans, const bool refine_structure, double& cost, int& steps);   // :387-548
  int Optimize(const LinePairs& line_pairs, const bool refine_camera_rotation, const bool refine_camera_trans, const bool refine_lidar_rotation,
               const bool refine_lidar_trans, double& cost, int& steps) {                                  // no SfM term
    std::vector<PointTrack> none;
    return Optimize(line_pairs, none, refine_camera_rotation, refine_camera_trans, refine_lidar_rotation, refine_lidar_trans, true, cost, steps);
  }
  // Calibration mode, CameraLidarOptimizer.cpp:32-87: ONE unknown, the camera <- LiDAR transform, refined on the associated line pairs
  // with Plane2Plane_Relative (residual in DEGREES, Huber 2 deg expressed in radians as upstream has it) and PlaneRelativeIOUResidual
  // (weight 2, half of the image line's arc, no loss).  Returns 1 like upstream; the result is GetOptimizedTcl().
  int Optimize(const LinePairs& line_pairs, const Matrix4d& T_cl, double* final_cost = nullptr, int* successful_steps = nullptr, int* residual_blocks = nullptr);
  const Matrix4d& GetOptimizedTcl() const { return T_cl_optimized; }
  const std::vector<Velodyne>& GetLidars() const { return lidars; }
  const std::vector<Frame>& GetFrames() const { return frames; }
  // CameraLidarOptimizer.cpp:732-740: SfMGlobalBA(frames, structure, ANGLE_RESIDUAL_1, num_threads, refine flags) on this optimizer's frames
  // and the caller's structure, as upstream
  bool GlobalBundleAdjustment(std::vector<PointTrack>& structure, bool refine_structure, bool refine_rotation, bool refine_translation);
  // joint_optimization/CameraLidarOptimizer.cpp:777-802: the same body as LidarOdometry::FuseLidar (FuseLidarScans)
  PointCloud FuseLidar(int skip, double min_range, double max_range);
  struct IterLog { double cost; int steps; int residual_blocks; size_t line_pairs; std::vector<double> cost_history; };
  std::vector<IterLog> log;
 private:
  Matrix4d T_cl_init;
  Matrix4d T_cl_optimized = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<Velodyne> lidars;
  std::vector<Frame> frames;
  std::vector<PointTrack> structure;
  Config config;
  int neighbor_size_joint, num_iteration_joint;
  int last_blocks_ = 0;
  std::vector<double> last_history_;
};

}  // namespace pvlm

#include "pvlm_host_triplet.hpp"
#include "pvlm_host_neighbor.hpp"
