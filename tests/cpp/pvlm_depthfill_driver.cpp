// Test driver of K37's host mirror (tests/test_depthfill_gpu.py, tests/test_depthfill_cpu.py) on the six-frame scene of pvlm_relpose_driver.cpp, which it makes itself.
//   pvlm_depthfill_driver        ComputeDepthImage (GPU) against ComputeDepthImageHost bit for bit, then MatchImagePairs -> FilterImagePairsFull with the device's maps
//                                against FilterImagePairsFullHost with the host's
//   pvlm_depthfill_driver host   ComputeDepthImageHost -> MatchImagePairsHost -> FilterImagePairsFullHost only: no device is touched
// Six panoramas on a 2 m circle see 300 points; the LiDAR scan of a frame is those points in the frame's camera frame (T_cl = identity), so the depth maps are no
// longer given, as they are to pvlm_relpose_driver, but completed from the scans: half-size, size 4, max_depth 40.  The pair list is the triangles 0-1-2 and 3-4-5
// joined by the bridge 2-3; the triangle 0-1-2 must survive in upstream's order, every pair with a scale from its depth maps and |t_21| within 2 % of the true
// baseline: a scan point's window holds its own depth (up to 1 / 256 m), the completion leaves it there unless a nearer point's window overlaps it, and
// SetTranslationScaleDepthMap's histogram drops those.  Exit 0 when all of that holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static uint32_t g_state = 20261018u;
static double rnd() { g_state = g_state * 1664525u + 1013904223u; return (double)(g_state >> 8) / 16777216.0; }

static std::array<float, 2> pixel_of(const double* X, int rows, int cols) {
  const double n = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  const double lon = std::atan2(X[0], X[2]), lat = std::asin(X[1] / n);
  return {(float)((lon / (2 * M_PI) + 0.5) * cols), (float)((lat / M_PI + 0.5) * rows)};
}

int main(int argc, char** argv) {
  try {
    const int rows = 720, cols = 1440, n = 300, F = 6;
    const float max_depth = 40.f;
    const bool host_only = argc > 1 && !std::strcmp(argv[1], "host");
    std::vector<Frame> frames((size_t)F);
    std::vector<Matrix3d> R_cw((size_t)F); std::vector<Vector3d> t_cw((size_t)F);
    std::vector<PointCloud> clouds((size_t)F);
    for (int f = 0; f < F; ++f) {
      frames[(size_t)f].rows = rows; frames[(size_t)f].cols = cols; frames[(size_t)f].id = f;
      const double a = 0.15 * f, c = std::cos(a), s = std::sin(a);
      R_cw[(size_t)f] = {c, 0, s, 0, 1, 0, -s, 0, c};
      const double centre[3] = {2.0 * std::cos(1.2 * f), 0.1 * f, 2.0 * std::sin(1.2 * f)};
      for (int r = 0; r < 3; ++r) t_cw[(size_t)f][(size_t)r] = -(R_cw[(size_t)f][3 * r] * centre[0] + R_cw[(size_t)f][3 * r + 1] * centre[1] + R_cw[(size_t)f][3 * r + 2] * centre[2]);
    }
    for (int i = 0; i < n; ++i) {
      double X[3] = {24 * rnd() - 12, 8 * rnd() - 4, 24 * rnd() - 12};
      if (std::fabs(X[0]) + std::fabs(X[2]) < 6.0) { X[0] += 6.0; X[2] -= 6.0; }
      double d[128], norm = 0;
      for (double& v : d) { v = rnd(); norm += v * v; }
      for (int f = 0; f < F; ++f) {
        double Y[3];
        for (int r = 0; r < 3; ++r) Y[r] = R_cw[(size_t)f][3 * r] * X[0] + R_cw[(size_t)f][3 * r + 1] * X[1] + R_cw[(size_t)f][3 * r + 2] * X[2] + t_cw[(size_t)f][(size_t)r];
        frames[(size_t)f].keypoints.push_back(pixel_of(Y, rows, cols));
        const double amp = 0.0005 + 0.01 * rnd();
        for (int k = 0; k < 128; ++k) frames[(size_t)f].descriptor.push_back((float)((d[k] + amp * rnd()) / std::sqrt(norm)));
        clouds[(size_t)f].push_back(PointXYZI{(float)Y[0], (float)Y[1], (float)Y[2], 0.f});
      }
    }
    const Matrix4d T_cl{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    try {                                                                      // upstream's lidars.size() != frames.size()
      std::vector<PointCloud> fewer(clouds.begin(), clouds.begin() + 2);
      (void)ComputeDepthImageHost(frames, fewer, T_cl, rows, cols, max_depth);
      fprintf(stderr, "ComputeDepthImageHost took 2 scans for 6 frames\n"); return 1;
    } catch (const std::invalid_argument&) {}
    const DepthMaps host_maps = ComputeDepthImageHost(frames, clouds, T_cl, rows, cols, max_depth, true, 8);
    const DepthMaps dev_maps = host_only ? host_maps : ComputeDepthImage(frames, clouds, T_cl, rows, cols, max_depth);
    size_t filled = 0;
    for (int f = 0; f < F; ++f) {
      if (host_maps.rows[(size_t)f] != (rows + 1) / 2 || host_maps.cols[(size_t)f] != (cols + 1) / 2 || dev_maps.maps[(size_t)f] != host_maps.maps[(size_t)f]) {
        fprintf(stderr, "depth map %d: device and host differ\n", f); return 1;
      }
      for (uint16_t v : host_maps.maps[(size_t)f]) filled += v > 0;
    }
    printf("%s: %d depth maps of %d x %d, %zu pixels filled\n", host_only ? "host route only (no device)" : "device maps equal host maps", F, (rows + 1) / 2, (cols + 1) / 2, filled);
    std::vector<MatchPair> pairs;
    for (auto e : {std::pair<size_t, size_t>{3, 4}, {1, 2}, {0, 1}, {2, 3}, {4, 5}, {0, 2}, {3, 5}}) { MatchPair p; p.image_pair = e; pairs.push_back(p); }
    if (!(host_only ? MatchImagePairsHost(frames, pairs, 0.8f, 50, 8) : MatchImagePairs(frames, pairs, 0.8f, 50)) || pairs.size() != 7) { fprintf(stderr, "MatchImagePairs dropped a pair (%zu left)\n", pairs.size()); return 1; }
    EssentialOptions opt; opt.seed = 7; opt.n_runs = 8; opt.max_iterations = 150;
    std::vector<RelativePair> dev, host; std::set<size_t> cov_dev, cov_host;
    if (!FilterImagePairsFullHost(frames, pairs, host_maps, host, cov_host, 20, false, opt, 8)) { fprintf(stderr, "FilterImagePairsFullHost refused its input\n"); return 1; }
    if (host_only) { dev = host; cov_dev = cov_host; }
    else if (!FilterImagePairsFull(frames, pairs, dev_maps, dev, cov_dev, 20, false, opt)) { fprintf(stderr, "FilterImagePairsFull refused its input\n"); return 1; }
    if (dev.size() != host.size() || cov_dev != cov_host) { fprintf(stderr, "device keeps %zu pairs, host %zu\n", dev.size(), host.size()); return 1; }
    const std::pair<size_t, size_t> want[3] = {{0, 1}, {0, 2}, {1, 2}};
    if (dev.size() != 3 || cov_dev != std::set<size_t>{0, 1, 2}) { fprintf(stderr, "%zu pairs survive, expected the triangle 0-1-2\n", dev.size()); return 1; }
    for (size_t k = 0; k < dev.size(); ++k) {
      const RelativePair& g = dev[k]; const RelativePair& h = host[k];
      if (g.image_pair != h.image_pair || g.image_pair != want[k]) { fprintf(stderr, "pair %zu is (%zu, %zu)\n", k, g.image_pair.first, g.image_pair.second); return 1; }
      if (g.points_with_depth != h.points_with_depth) { fprintf(stderr, "pair %zu: device and host count different points with depth\n", k); return 1; }
      const size_t a = g.image_pair.first, b = g.image_pair.second;
      Matrix3d R; Vector3d t;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { double s = 0; for (int q = 0; q < 3; ++q) s += R_cw[b][3 * r + q] * R_cw[a][3 * c + q]; R[(size_t)(3 * r + c)] = s; }
      for (int r = 0; r < 3; ++r) { double s = t_cw[b][(size_t)r]; for (int c = 0; c < 3; ++c) s -= R[(size_t)(3 * r + c)] * t_cw[a][(size_t)c]; t[(size_t)r] = s; }
      double nt = 0, ng = 0;
      for (int i = 0; i < 3; ++i) { nt += t[(size_t)i] * t[(size_t)i]; ng += g.t_21[(size_t)i] * g.t_21[(size_t)i]; }
      const double ratio = std::sqrt(ng / nt);
      printf("pair (%zu, %zu): inliers %zu, points with depth %d, scale %.4f .. %.4f, |t| / truth %.4f\n", a, b, g.inlier_idx.size(), g.points_with_depth, g.lower_scale,
             g.upper_scale, ratio);
      if (!(g.upper_scale >= 0) || g.points_with_depth <= 0 || !(std::fabs(ratio - 1.0) <= 0.02)) { fprintf(stderr, "pair %zu: no scale from the depth maps, or outside the bound\n", k); return 1; }
    }
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
