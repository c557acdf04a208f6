// Test driver of K34's host mirror (tests/test_essential_gpu.py): the chain MatchImagePairs -> FilterImagePairs on a synthetic scene it makes itself.
//   pvlm_essential_driver
// Two panoramas see 400 points; X_2 = R X_1 + t.  Every point gets a random unit descriptor, shared by its two keypoints up to a small perturbation; a quarter of
// the second frame's keypoints are moved to a random pixel (gross outliers with a good descriptor).  MatchImagePairs makes the matches from the descriptors,
// FilterImagePairs (GPU) and FilterImagePairsHost must agree bit for bit, the pair must be kept and its pose must be within the bound of
// tests/test_essential_cpu.py's scene of the same kind (twice 3.3045 degrees of rotation, twice 0.6126 degrees of direction).  Exit 0 when all of that holds.
// Before RefineRelativePose the pose depends on the draws (a hypothesis is fitted to every point sampled so far, outliers included): with this seed the host
// loops give 0.018 and 0.012 degrees here.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static uint32_t g_state = 20261018u;
static double rnd() { g_state = g_state * 1664525u + 1013904223u; return (double)(g_state >> 8) / 16777216.0; }

// the pixel of a camera-frame direction in a rows x cols panorama: the inverse of eq.ImageToCam (x right, y down, z forward; longitude atan2(x, z), latitude asin(y))
static std::array<float, 2> pixel_of(const double* X, int rows, int cols) {
  const double n = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  const double lon = std::atan2(X[0], X[2]), lat = std::asin(X[1] / n);
  return {(float)((lon / (2 * M_PI) + 0.5) * cols), (float)((lat / M_PI + 0.5) * rows)};
}

int main() {
  try {
    const int rows = 2880, cols = 5760, n = 400;
    const double ang = 0.2, c = std::cos(ang), s = std::sin(ang), t[3] = {1.0, 0.2, -0.1};
    const Matrix3d R{c, 0, s, 0, 1, 0, -s, 0, c};
    std::vector<Frame> frames(2);
    for (Frame& f : frames) { f.rows = rows; f.cols = cols; }
    for (int i = 0; i < n; ++i) {
      double X[3] = {8 * rnd() - 4, 4 * rnd() - 2, 8 * rnd() - 4};
      if (std::fabs(X[0]) + std::fabs(X[2]) < 1.0) X[2] += 2.0;
      double Y[3];
      for (int r = 0; r < 3; ++r) Y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
      frames[0].keypoints.push_back(pixel_of(X, rows, cols));
      if (i % 4 == 3) frames[1].keypoints.push_back({(float)(rnd() * (cols - 1)), (float)(rnd() * (rows - 1))});
      else frames[1].keypoints.push_back(pixel_of(Y, rows, cols));
      double d[128], norm = 0;
      for (double& v : d) { v = rnd(); norm += v * v; }
      const double u = rnd(), amp = 0.0005 + 0.02 * u * u;       // distances spread over a decade: the 0.8 dmax filter of MatchImagePairs keeps most of them
      for (int k = 0; k < 128; ++k) { frames[0].descriptor.push_back((float)(d[k] / std::sqrt(norm))); frames[1].descriptor.push_back((float)((d[k] + amp * rnd()) / std::sqrt(norm))); }
    }
    std::vector<MatchPair> pairs(1);
    pairs[0].image_pair = {0, 1};
    if (!MatchImagePairs(frames, pairs, 0.8f, 50) || pairs.size() != 1) { fprintf(stderr, "MatchImagePairs dropped the pair\n"); return 1; }
    printf("matches: %zu\n", pairs[0].matches.size());
    EssentialOptions opt; opt.seed = 7;                        // upstream's 40 runs of 300 iterations, the seed of tests/test_essential_cpu.py
    std::vector<RelativePair> dev, host;
    if (!FilterImagePairs(frames, pairs, dev, 20, opt) || !FilterImagePairsHost(frames, pairs, host, 20, opt, 4)) { fprintf(stderr, "FilterImagePairs refused its input\n"); return 1; }
    if (dev.size() != 1 || host.size() != 1) { fprintf(stderr, "kept %zu (device) / %zu (host) pairs, expected 1\n", dev.size(), host.size()); return 1; }
    const RelativePair& g = dev[0]; const RelativePair& h = host[0];
    if (g.R_21 != h.R_21 || g.t_21 != h.t_21 || g.inlier_idx != h.inlier_idx || g.triangulated != h.triangulated) { fprintf(stderr, "device and host results differ\n"); return 1; }
    double tr = 0, dot = 0, nt = 0;
    for (int i = 0; i < 9; ++i) tr += g.R_21[(size_t)i] * R[(size_t)i];
    for (int i = 0; i < 3; ++i) { dot += g.t_21[(size_t)i] * t[i]; nt += t[i] * t[i]; }
    const double rot = std::acos(std::fmax(-1.0, std::fmin(1.0, (tr - 1) / 2))) * 180 / M_PI, dir = std::acos(std::fmax(-1.0, std::fmin(1.0, dot / std::sqrt(nt)))) * 180 / M_PI;
    size_t bad = 0;
    for (size_t k : g.inlier_idx) bad += (pairs[0].matches[k].first % 4 == 3) ? 1 : 0;
    printf("inliers: %zu (of them moved keypoints: %zu), rotation error %.6g deg, direction error %.6g deg\n", g.inlier_idx.size(), bad, rot, dir);
    if (bad != 0 || rot > 2 * 3.3045 || dir > 2 * 0.6126) { fprintf(stderr, "pose or inliers outside the bound\n"); return 1; }
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
