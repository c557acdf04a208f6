// Test driver of K39's host mirror (tests/test_scale_gpu.py) on the six-frame scene of pvlm_depthfill_driver.cpp, which it makes itself: the same scene through both
// pvlm:: routes, both results printed.
//   host-map route   ComputeDepthImage (the maps come to the host)      -> FilterImagePairsFull(.., DepthMaps, ..)        (the scale set by the host step)
//   resident route   ComputeDepthImageResident (the maps stay resident) -> FilterImagePairsFull(.., DeviceDepthMaps, ..)  (the scale set by K39)
//   pvlm_scale_driver        keep_no_scale = false
//   pvlm_scale_driver keep   keep_no_scale = true
// Every pair of both lists is printed with its doubles as bit patterns; exit 0 when the two lists are equal: same order, poses, points, points_with_depth,
// upper_scale and lower_scale, the same covered frames, and ReadDepthMap of every frame equal to the host-map route's map.
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
    const bool keep_no_scale = argc > 1 && !std::strcmp(argv[1], "keep");
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
    const DepthMaps host_maps = ComputeDepthImage(frames, clouds, T_cl, rows, cols, max_depth);
    const DeviceDepthMaps dev_maps = ComputeDepthImageResident(frames, clouds, T_cl, rows, cols, max_depth);
    for (int f = 0; f < F; ++f) {
      int r = 0, c = 0;
      if (ReadDepthMap(dev_maps, (size_t)f, &r, &c) != host_maps.maps[(size_t)f] || r != host_maps.rows[(size_t)f] || c != host_maps.cols[(size_t)f]) {
        fprintf(stderr, "depth map %d: the resident map and the downloaded one differ\n", f); return 1;
      }
    }
    printf("resident maps equal host maps: %d maps of %d x %d\n", F, (rows + 1) / 2, (cols + 1) / 2);
    std::vector<MatchPair> pairs;
    for (auto e : {std::pair<size_t, size_t>{3, 4}, {1, 2}, {0, 1}, {2, 3}, {4, 5}, {0, 2}, {3, 5}}) { MatchPair p; p.image_pair = e; pairs.push_back(p); }
    if (!MatchImagePairs(frames, pairs, 0.8f, 50) || pairs.size() != 7) { fprintf(stderr, "MatchImagePairs dropped a pair (%zu left)\n", pairs.size()); return 1; }
    EssentialOptions opt; opt.seed = 7; opt.n_runs = 8; opt.max_iterations = 150;
    std::vector<RelativePair> a, b; std::set<size_t> cov_a, cov_b;
    if (!FilterImagePairsFull(frames, pairs, host_maps, a, cov_a, 20, keep_no_scale, opt)) { fprintf(stderr, "FilterImagePairsFull (host maps) refused its input\n"); return 1; }
    if (!FilterImagePairsFull(frames, pairs, dev_maps, b, cov_b, 20, keep_no_scale, opt)) { fprintf(stderr, "FilterImagePairsFull (resident maps) refused its input\n"); return 1; }
    auto bits = [](double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; };
    auto show = [&](const char* route, const std::vector<RelativePair>& list, const std::set<size_t>& cov) {
      printf("%s: %zu pairs, %zu frames covered\n", route, list.size(), cov.size());
      for (const RelativePair& p : list) {
        unsigned long long h = 1469598103934665603ull;                              // FNV-1a over the bits of the pose and of every point
        auto mix = [&](double v) { h = (h ^ bits(v)) * 1099511628211ull; };
        for (double v : p.R_21) mix(v);
        for (double v : p.t_21) mix(v);
        for (const Vector3d& X : p.triangulated) for (double v : X) mix(v);
        printf("%s pair (%zu, %zu): points %zu with depth %d upper %016llx lower %016llx t %016llx %016llx %016llx pose+points %016llx\n", route, p.image_pair.first,
               p.image_pair.second, p.triangulated.size(), p.points_with_depth, bits(p.upper_scale), bits(p.lower_scale), bits(p.t_21[0]), bits(p.t_21[1]), bits(p.t_21[2]), h);
      }
    };
    show("host-map route", a, cov_a);
    show("resident route", b, cov_b);
    bool same = a.size() == b.size() && cov_a == cov_b;
    for (size_t k = 0; same && k < a.size(); ++k) {
      const RelativePair& g = a[k]; const RelativePair& h = b[k];
      same = g.image_pair == h.image_pair && g.points_with_depth == h.points_with_depth && bits(g.upper_scale) == bits(h.upper_scale) && bits(g.lower_scale) == bits(h.lower_scale) &&
             g.inlier_idx == h.inlier_idx && g.triangulated.size() == h.triangulated.size() && !std::memcmp(g.R_21.data(), h.R_21.data(), sizeof(double) * 9) &&
             !std::memcmp(g.t_21.data(), h.t_21.data(), sizeof(double) * 3);
      for (size_t i = 0; same && i < g.triangulated.size(); ++i) same = !std::memcmp(g.triangulated[i].data(), h.triangulated[i].data(), sizeof(double) * 3);
    }
    if (!same) { fprintf(stderr, "the two routes differ\n"); return 1; }
    size_t scaled = 0;
    for (const RelativePair& p : b) scaled += p.upper_scale >= 0;
    printf("routes equal: %zu pairs, %zu with a scale, keep_no_scale %d\n", b.size(), scaled, (int)keep_no_scale);
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
