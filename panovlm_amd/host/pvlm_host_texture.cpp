// pvlm_host_texture.cpp — part of the C++ host mirror (pvlm_host.hpp): mvs/Texture.cpp (the coloured LiDAR map) and Velodyne::SegmentBatch.
// Host logic only; the range test, projection, HSV test and compaction of every point run in libpvlm.so on the GPU (K30).
#include "pvlm_host_internal.hpp"
#include "../csrc/pvlm_fuse_core.h"

namespace pvlm {

// ================================================================================================
// Velodyne::SegmentBatch — ReOrderVLP (sensors/Velodyne.cpp:371-526) + Segmentation (:1438-1586) for many scans
// ================================================================================================
void Velodyne::SegmentBatch(const std::vector<Velodyne*>& scans, int num_threads) {
  std::vector<Velodyne*> batched, host;
  for (Velodyne* v : scans) {
    if (!v || !v->valid) continue;                                  // the divergence: left untouched (upstream: Segmentation without a range image)
    const bool shape_ok = batched.empty() || (v->N_SCANS == batched[0]->N_SCANS && v->horizon_scans == batched[0]->horizon_scans);
    if (!v->cloud_scan.empty() || v->cloud.empty() || !shape_ok || (v->N_SCANS != 16 && v->N_SCANS != 32 && v->N_SCANS != 64)) host.push_back(v);
    else batched.push_back(v);
  }
  if (batched.empty() && host.empty()) return;
  // the device copies of the scans that are about to change go back here, on the thread that owns the engine
  for (Velodyne* v : batched) v->InvalidateDevice();
  for (Velodyne* v : host) v->InvalidateDevice();
  const size_t n_threads = std::max<size_t>(1, std::min<size_t>((size_t)std::max(num_threads, 1), (size_t)std::max(1u, std::thread::hardware_concurrency())));
  // per scan on the host: ReOrderVLP returns early for a scan already re-ordered, and Segmentation needs the range image it builds
  auto host_segment = [](Velodyne& v) {
    v.ReOrderVLP();
    const RingLayout& L = v.Layout();
    if (L.range_image.size() == (size_t)v.N_SCANS * (size_t)v.horizon_scans && L.point_idx_to_image.size() == v.cloud_scan.size()) v.Segmentation();
  };
  if (!batched.empty()) {
    Engine& e = Engine::Default();
    const int rings = batched[0]->N_SCANS, horizon = batched[0]->horizon_scans;
    constexpr size_t kPart = 256;                                   // scans per device batch (bounds its pinned arrays)
    for (size_t first = 0; first < batched.size(); first += kPart) {
      const size_t count = std::min(kPart, batched.size() - first);
      std::vector<pvlm_raw_scan> raw(count);
      for (size_t j = 0; j < count; ++j) { const PointCloud& c = batched[first + j]->cloud; raw[j] = pvlm_raw_scan{&c[0].x, (int)c.size(), (int)(sizeof(PointXYZI) / sizeof(float))}; }
      pvlm_ring_batch* batch = nullptr;
      const pvlm_status rc = pvlm_ring_extract_batch(e.ctx(), (int)count, raw.data(), rings, horizon, 1, &batch);
      struct Release { pvlm_ctx* c; pvlm_ring_batch* b; ~Release() { if (b) pvlm_ring_batch_destroy(c, b); } } release{e.ctx(), batch};
      if (rc == PVLM_ERR_REFUSED) {
        // a non-finite coordinate (upstream gives such a point ring -1 and skips it): these scans go through the host path, which does the same
        fprintf(stderr, "SegmentBatch: %s — the per-scan host path takes these %zu scans\n", pvlm_last_error(e.ctx()), count);
        for (size_t j = 0; j < count; ++j) host.push_back(batched[first + j]);
        continue;
      }
      e.Check(rc, "pvlm_ring_extract_batch");
      std::atomic<size_t> next{0};
      pvlm_run_workers(std::min(n_threads, count), [&]() {
        for (size_t j = next++; j < count; j = next++) {
          Velodyne& v = *batched[first + j];
          pvlm_ring_result r;
          if (pvlm_ring_batch_scan(batch, (int)j, &r) != PVLM_OK) throw std::runtime_error("pvlm_ring_batch_scan failed");
          RingLayout& L = v.layout_;
          L = RingLayout();
          L.scanStartInd.assign(rings, 0); L.scanEndInd.assign(rings, 0);
          const int n = r.n_kept;
          v.cloud_scan.resize((size_t)n);
          L.point_idx_to_image.resize((size_t)n);
          for (int i = 0; i < n; ++i) {
            const PointXYZI& p = v.cloud[(size_t)r.source[i]];
            const int ring = r.ring_col[i] >> 16;
            v.cloud_scan[(size_t)i] = PointXYZI{p.x, p.y, p.z, (float)ring};
            L.point_idx_to_image[(size_t)i] = std::pair<int, int>(ring, r.ring_col[i] & 0xFFFF);
          }
          int begin = 0;
          for (int q = 0; q < rings; ++q) { L.scanStartInd[q] = begin + 5; begin += r.ring_count[q]; L.scanEndInd[q] = begin - 6; }
        }
      });
    }
  }
  std::atomic<size_t> next{0};
  pvlm_run_workers(std::min(n_threads, host.size()), [&]() { for (size_t j = next++; j < host.size(); j = next++) host_segment(*host[j]); });
}

// ================================================================================================
// Texture — mvs/Texture.cpp:14-97
// ================================================================================================
namespace {

// T_cl = T_wc^-1 T_wl, the rigid inverse; rows 0..2 (12 doubles).  Each entry a sum in index order, as tests/colorize_ref.py::camera_from_lidar restates it.
void CameraFromLidar(const Frame& f, const Matrix4d& T_wl, double* T_cl) {
  const Matrix3d& R = f.R_wc;
  const Vector3d& t = f.t_wc;
  double inv[16] = {0};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) inv[4 * r + c] = R[3 * c + r];
    inv[4 * r + 3] = -(((R[r] * t[0]) + R[3 + r] * t[1]) + R[6 + r] * t[2]);
  }
  inv[15] = 1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double acc = inv[4 * r] * T_wl[c];
      for (int k = 1; k < 4; ++k) acc += inv[4 * r + k] * T_wl[4 * k + c];
      T_cl[4 * r + c] = acc;
    }
}

}  // namespace

bool Texture::ColorizeLidarPointCloud(const double min_dist, const double max_dist) {
  StageTimer stage_timer_("coloured LiDAR map (Texture::ColorizeLidarPointCloud)");
  if (lidars.empty() || frames.empty()) { fprintf(stderr, "lidar or frames are empty\n"); return false; }
  if (lidars.size() != frames.size()) throw std::invalid_argument("Texture::ColorizeLidarPointCloud: lidars and frames differ in size (upstream asserts)");
  lidar_colored.assign(lidars.size(), std::vector<PointXYZRGB>());
  std::vector<Velodyne*> todo;
  for (Velodyne& l : lidars) {
    if (!l.IsPoseValid()) continue;
    l.LoadLidar(l.name);
    todo.push_back(&l);
  }
  Velodyne::SegmentBatch(todo, config.num_threads);
  std::vector<size_t> pairs;
  for (size_t i = 0; i < lidars.size(); ++i)
    if (lidars[i].IsPoseValid() && frames[i].IsPoseValid() && lidars[i].valid && !lidars[i].cloud_scan.empty()) pairs.push_back(i);
  if (!pairs.empty() && !images_) throw std::invalid_argument("Texture::ColorizeLidarPointCloud: no image provider (SetImageProvider)");
  Engine& e = Engine::Default();
  const size_t per_call = (size_t)std::max(images_per_call, 1);
  for (size_t g0 = 0; g0 < pairs.size(); g0 += per_call) {
    const size_t g1 = std::min(pairs.size(), g0 + per_call);
    std::vector<ColorImage> img(g1 - g0);
    std::vector<std::array<double, 12>> T(g1 - g0);
    std::vector<pvlm_colorize_pair> desc(g1 - g0);
    long long total = 0;
    for (size_t k = g0; k < g1; ++k) {
      const size_t i = pairs[k];
      ColorImage& im = img[k - g0];
      if (!images_(i, im)) throw std::runtime_error("Texture::ColorizeLidarPointCloud: no colour image for frame " + std::to_string(i));
      if (im.rows != frames[i].GetImageRows() || im.cols != frames[i].GetImageCols() || im.bgr.size() != (size_t)im.rows * im.cols * 3)
        throw std::invalid_argument("Texture::ColorizeLidarPointCloud: the image of frame " + std::to_string(i) + " is not rows x cols BGR8 of the frame");
      CameraFromLidar(frames[i], lidars[i].GetPose(), T[k - g0].data());
      const PointCloud& c = lidars[i].cloud_scan;
      desc[k - g0] = pvlm_colorize_pair{&c[0].x, (int)c.size(), (int)(sizeof(PointXYZI) / sizeof(float)), T[k - g0].data(), im.bgr.data(), im.rows, im.cols, 3ll * im.cols};
      total += (long long)c.size();
    }
    std::vector<float> rec((size_t)total * 4);
    std::vector<long long> per(desc.size());
    long long kept = 0;
    e.Check(pvlm_colorize_scans(e.ctx(), (int)desc.size(), desc.data(), min_dist, max_dist, rec.data(), total, &kept, per.data()), "pvlm_colorize_scans");
    long long at = 0;
    for (size_t k = g0; k < g1; ++k) {
      std::vector<PointXYZRGB>& out = lidar_colored[pairs[k]];
      out.resize((size_t)per[k - g0]);
      for (PointXYZRGB& p : out) {
        const float* q = &rec[(size_t)at++ * 4];
        uint32_t w; std::memcpy(&w, q + 3, 4);
        p.x = q[0]; p.y = q[1]; p.z = q[2];
        p.b = (unsigned char)(w & 255u); p.g = (unsigned char)((w >> 8) & 255u); p.r = (unsigned char)((w >> 16) & 255u);
      }
    }
  }
  return lidar_colored.size() > 0;
}

std::vector<PointXYZRGB> Texture::FuseCloud(int skip) {
  if (skip < 0) throw std::invalid_argument("Texture::FuseCloud: skip < 0 (upstream asserts)");
  std::vector<size_t> sel, at{0};
  for (size_t i = 0; i < lidar_colored.size(); i += (size_t)skip + 1) {
    if (!lidars[i].IsPoseValid()) continue;
    sel.push_back(i);
    at.push_back(at.back() + lidar_colored[i].size());
  }
  std::vector<PointXYZRGB> fused(at.back());
  std::atomic<size_t> next{0};
  const size_t n_threads = std::max<size_t>(1, std::min<size_t>({(size_t)std::max(config.num_threads, 1), sel.size(), (size_t)std::max(1u, std::thread::hardware_concurrency())}));
  pvlm_run_workers(n_threads, [&]() {
    for (size_t k = next++; k < sel.size(); k = next++) {
      const Matrix4d T = lidars[sel[k]].GetPose();
      const std::vector<PointXYZRGB>& src = lidar_colored[sel[k]];
      PointXYZRGB* dst = fused.data() + at[k];
      for (size_t j = 0; j < src.size(); ++j) {
        float q[3];
        pvlm_fuse::transform_point(T.data(), src[j].x, src[j].y, src[j].z, q);
        dst[j] = src[j];
        dst[j].x = q[0]; dst[j].y = q[1]; dst[j].z = q[2];
      }
    }
  });
  return fused;
}

}  // namespace pvlm
