// Test driver of K36's host mirror (tests/test_relpose_gpu.py, tests/test_relpose_cpu.py, tools/relpose_bench.py) on a synthetic scene it makes itself.
//   pvlm_relpose_driver [dump-file]      MatchImagePairs -> FilterImagePairsFull on the GPU against FilterImagePairsFullHost
//   pvlm_relpose_driver host             MatchImagePairsHost -> FilterImagePairsFullHost only: no device is touched
//   pvlm_relpose_driver solve-route N    times, on N pairs, one ceres_like::Solve + pvlm_baset per pair (what the tree could do before K36) against ONE
//                                        RefineRelativePoses call and against RefineRelativePosesHost on 16 threads; prints one JSON line
// Six panoramas on a 2 m circle see 300 points; every point has a random unit descriptor shared by its keypoints up to a small perturbation.  The pair list is the
// triangles 0-1-2 and 3-4-5 joined by the bridge 2-3.  Every frame has a half-size depth map that holds the true depth (x 256) around the pixel each point rounds
// to and nothing elsewhere.  FilterImagePairsFull (GPU: K34, K36, then the host tail) must give the same pairs in the same order as FilterImagePairsFullHost, with
// poses within 1e-6; the bridge goes, of the two equally large triangles the one with the lower frame ids survives: (0,1) (0,2) (1,2) in that order, each with a
// scale from the histogram path and |t_21| within 2 % of the true baseline, and a rotation / direction within 0.05 degrees of the truth (the refined pose; K34's own
// bound before the refinement is degrees).  Exit 0 when all of that holds.  The dump-file gets one line per surviving pair.
#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static uint32_t g_state = 20261018u;
static double rnd() { g_state = g_state * 1664525u + 1013904223u; return (double)(g_state >> 8) / 16777216.0; }

static std::array<float, 2> pixel_of(const double* X, int rows, int cols) {
  const double n = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  const double lon = std::atan2(X[0], X[2]), lat = std::asin(X[1] / n);
  return {(float)((lon / (2 * M_PI) + 0.5) * cols), (float)((lat / M_PI + 0.5) * rows)};
}

// SfMLocalBA as the tree could run it before K36: one ceres_like::Problem per pair (two PanoramaReprojResidual_Pixel blocks per inlier, HuberLoss(4.0), camera 1
// constant), solved by ceres_like::Solve, whose every linearisation, step and cost is a handful of pvlm_baset launches.  Returns the LM iterations taken.
static int SolveRoute(const std::vector<Frame>& frames, RelativePair& p) {
  const Frame& f1 = frames[p.image_pair.first]; const Frame& f2 = frames[p.image_pair.second];
  Vector3d aa1{0, 0, 0}, t1{0, 0, 0}, aa2, t2 = p.t_21;
  RotationMatrixToAngleAxis(p.R_21, &aa2);
  std::vector<Vector3d> X = p.triangulated;
  ceres_like::Problem problem;
  ceres_like::LossFunction* loss = new ceres_like::HuberLoss(4.0);
  for (size_t i = 0; i < X.size(); ++i) {
    const std::pair<int, int>& m = p.matches[p.inlier_idx[i]];
    const std::array<float, 2>& a = f1.keypoints[(size_t)m.first]; const std::array<float, 2>& b = f2.keypoints[(size_t)m.second];
    problem.AddResidualBlock(PanoramaReprojResidual_Pixel::Create({(double)a[0], (double)a[1]}, f1.rows, f1.cols), loss, aa1.data(), t1.data(), X[i].data());
    problem.AddResidualBlock(PanoramaReprojResidual_Pixel::Create({(double)b[0], (double)b[1]}, f2.rows, f2.cols), loss, aa2.data(), t2.data(), X[i].data());
  }
  if (X.empty()) { delete loss; return 0; }
  problem.SetParameterBlockConstant(aa1.data()); problem.SetParameterBlockConstant(t1.data());
  ceres_like::Solver::Options options = SetOptionsSfM(1);
  ceres_like::Solver::Summary summary;
  ceres_like::Solve(options, &problem, &summary);
  AngleAxisToRotationMatrix(aa2, &p.R_21);
  const double scale = std::sqrt(t2[0] * t2[0] + t2[1] * t2[1] + t2[2] * t2[2]);
  for (int k = 0; k < 3; ++k) p.t_21[(size_t)k] = t2[(size_t)k] / scale;
  for (size_t i = 0; i < X.size(); ++i) p.triangulated[i] = {X[i][0] / scale, X[i][1] / scale, X[i][2] / scale};
  return summary.num_successful_steps - 1 + summary.num_unsuccessful_steps;
}

static double Seconds(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

// the three routes on n pairs (K34's output for the scene's seven pairs, repeated round the list): every route starts from the same poses and points
static int SolveRouteBench(const std::vector<Frame>& frames, const std::vector<MatchPair>& pairs, const EssentialOptions& opt, int n) {
  std::vector<RelativePair> k34;
  if (!FilterImagePairs(frames, pairs, k34, 20, opt) || k34.empty() || n < 1) { fprintf(stderr, "no pairs to refine\n"); return 1; }
  std::vector<RelativePair> list;
  for (int k = 0; k < n; ++k) list.push_back(k34[(size_t)k % k34.size()]);
  size_t inliers = 0;
  for (const RelativePair& p : list) inliers += p.inlier_idx.size();
  std::vector<RelativePair> a = list, b = list, c = list;
  { std::vector<RelativePair> w(list.begin(), list.begin() + 1); std::vector<RelativePair> w2 = w; SolveRoute(frames, w[0]); RefineRelativePoses(frames, w2); }    // warm-up of both device routes
  auto t0 = std::chrono::steady_clock::now();
  long iterations = 0;
  for (RelativePair& p : a) iterations += SolveRoute(frames, p);
  const double solve_s = Seconds(t0);
  t0 = std::chrono::steady_clock::now();
  if (!RefineRelativePoses(frames, b)) return 1;
  const double call_s = Seconds(t0);
  t0 = std::chrono::steady_clock::now();
  if (!RefineRelativePosesHost(frames, c, PIXEL_RESIDUAL, nullptr, 16)) return 1;
  const double host_s = Seconds(t0);
  double worst = 0;                                           // the routes agree: the Solve route against the call
  for (size_t p = 0; p < a.size(); ++p) {
    for (int i = 0; i < 9; ++i) worst = std::fmax(worst, std::fabs(a[p].R_21[(size_t)i] - b[p].R_21[(size_t)i]));
    for (int i = 0; i < 3; ++i) worst = std::fmax(worst, std::fabs(a[p].t_21[(size_t)i] - b[p].t_21[(size_t)i]));
  }
  printf("{\"solve_route_pairs\": %d, \"solve_route_inliers\": %zu, \"solve_route_s\": %.6f, \"solve_route_ms_per_pair\": %.4f, \"solve_route_lm_iterations\": %ld, "
         "\"one_call_s\": %.6f, \"one_call_ms_per_pair\": %.4f, \"host16_s\": %.6f, \"solve_route_over_one_call\": %.2f, \"max_pose_difference_solve_route_vs_call\": %.3g}\n",
         n, inliers, solve_s, 1e3 * solve_s / n, iterations, call_s, 1e3 * call_s / n, host_s, solve_s / call_s, worst);
  return 0;                                                   // a timing: the difference is reported, the tests hold the routes to their bounds
}

int main(int argc, char** argv) {
  try {
    const int rows = 720, cols = 1440, n = 300, F = 6;
    const bool host_only = argc > 1 && !std::strcmp(argv[1], "host");
    const bool solve_route = argc > 2 && !std::strcmp(argv[1], "solve-route");
    std::vector<Frame> frames((size_t)F);
    std::vector<Matrix3d> R_cw((size_t)F); std::vector<Vector3d> t_cw((size_t)F);
    DepthMaps depth;
    for (int f = 0; f < F; ++f) {
      frames[(size_t)f].rows = rows; frames[(size_t)f].cols = cols; frames[(size_t)f].id = f;
      const double a = 0.15 * f, c = std::cos(a), s = std::sin(a);
      R_cw[(size_t)f] = {c, 0, s, 0, 1, 0, -s, 0, c};
      const double centre[3] = {2.0 * std::cos(1.2 * f), 0.1 * f, 2.0 * std::sin(1.2 * f)};
      for (int r = 0; r < 3; ++r) t_cw[(size_t)f][(size_t)r] = -(R_cw[(size_t)f][3 * r] * centre[0] + R_cw[(size_t)f][3 * r + 1] * centre[1] + R_cw[(size_t)f][3 * r + 2] * centre[2]);
      depth.maps.emplace_back((size_t)(rows / 2) * (size_t)(cols / 2), (uint16_t)0); depth.rows.push_back(rows / 2); depth.cols.push_back(cols / 2);
    }
    for (int i = 0; i < n; ++i) {
      double X[3] = {24 * rnd() - 12, 8 * rnd() - 4, 24 * rnd() - 12};
      if (std::fabs(X[0]) + std::fabs(X[2]) < 6.0) { X[0] += 6.0; X[2] -= 6.0; }
      double d[128], norm = 0;
      for (double& v : d) { v = rnd(); norm += v * v; }
      for (int f = 0; f < F; ++f) {
        double Y[3];
        for (int r = 0; r < 3; ++r) Y[r] = R_cw[(size_t)f][3 * r] * X[0] + R_cw[(size_t)f][3 * r + 1] * X[1] + R_cw[(size_t)f][3 * r + 2] * X[2] + t_cw[(size_t)f][(size_t)r];
        const std::array<float, 2> px = pixel_of(Y, rows, cols);
        frames[(size_t)f].keypoints.push_back(px);
        const double amp = 0.0005 + 0.01 * rnd();
        for (int k = 0; k < 128; ++k) frames[(size_t)f].descriptor.push_back((float)((d[k] + amp * rnd()) / std::sqrt(norm)));
        const double dist = std::sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
        // a 5 x 5 patch of the true depth: the adjusted point projects within a pixel or two of the keypoint
        const int r0 = (int)std::lround(px[1] / 2.0), c0 = (int)std::lround(px[0] / 2.0);
        for (int dr = -2; dr <= 2; ++dr)
          for (int dc = -2; dc <= 2; ++dc) {
            const int rr = r0 + dr, cc = c0 + dc;
            if (rr >= 0 && rr < rows / 2 && cc >= 0 && cc < cols / 2) depth.maps[(size_t)f][(size_t)rr * (size_t)(cols / 2) + (size_t)cc] = (uint16_t)std::lround(dist * 256.0);
          }
      }
    }
    std::vector<MatchPair> pairs;
    for (auto e : {std::pair<size_t, size_t>{3, 4}, {1, 2}, {0, 1}, {2, 3}, {4, 5}, {0, 2}, {3, 5}}) { MatchPair p; p.image_pair = e; pairs.push_back(p); }
    if (!(host_only ? MatchImagePairsHost(frames, pairs, 0.8f, 50, 8) : MatchImagePairs(frames, pairs, 0.8f, 50)) || pairs.size() != 7) { fprintf(stderr, "MatchImagePairs dropped a pair (%zu left)\n", pairs.size()); return 1; }
    EssentialOptions opt; opt.seed = 7; opt.n_runs = 8; opt.max_iterations = 150;
    if (solve_route) return SolveRouteBench(frames, pairs, opt, std::atoi(argv[2]));
    std::vector<RelativePair> dev, host; std::set<size_t> cov_dev, cov_host;
    if (!FilterImagePairsFullHost(frames, pairs, depth, host, cov_host, 20, false, opt, 8)) { fprintf(stderr, "FilterImagePairsFullHost refused its input\n"); return 1; }
    if (host_only) { dev = host; cov_dev = cov_host; }
    else if (!FilterImagePairsFull(frames, pairs, depth, dev, cov_dev, 20, false, opt)) { fprintf(stderr, "FilterImagePairsFull refused its input\n"); return 1; }
    if (dev.size() != host.size() || cov_dev != cov_host) { fprintf(stderr, "device keeps %zu pairs, host %zu\n", dev.size(), host.size()); return 1; }
    FILE* dump = argc > 1 && !host_only ? fopen(argv[1], "w") : nullptr;
    const std::pair<size_t, size_t> want[3] = {{0, 1}, {0, 2}, {1, 2}};
    if (dev.size() != 3 || cov_dev != std::set<size_t>{0, 1, 2}) { fprintf(stderr, "%zu pairs survive, expected the triangle 0-1-2\n", dev.size()); return 1; }
    printf("%s\n", host_only ? "host route only (no device)" : "device against host");
    for (size_t k = 0; k < dev.size(); ++k) {
      const RelativePair& g = dev[k]; const RelativePair& h = host[k];
      if (g.image_pair != h.image_pair || g.image_pair != want[k]) { fprintf(stderr, "pair %zu is (%zu, %zu)\n", k, g.image_pair.first, g.image_pair.second); return 1; }
      double worst = 0;
      for (int i = 0; i < 9; ++i) worst = std::fmax(worst, std::fabs(g.R_21[(size_t)i] - h.R_21[(size_t)i]));
      for (int i = 0; i < 3; ++i) worst = std::fmax(worst, std::fabs(g.t_21[(size_t)i] - h.t_21[(size_t)i]));
      if (!(worst <= 1e-6) || g.inlier_idx != h.inlier_idx || g.points_with_depth != h.points_with_depth) { fprintf(stderr, "pair %zu: device and host differ by %.3g\n", k, worst); return 1; }
      // the truth: T_21 = T_2w T_w1
      const size_t a = g.image_pair.first, b = g.image_pair.second;
      Matrix3d R; Vector3d t;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { double s = 0; for (int q = 0; q < 3; ++q) s += R_cw[b][3 * r + q] * R_cw[a][3 * c + q]; R[(size_t)(3 * r + c)] = s; }
      }
      for (int r = 0; r < 3; ++r) { double s = t_cw[b][(size_t)r]; for (int c = 0; c < 3; ++c) s -= R[(size_t)(3 * r + c)] * t_cw[a][(size_t)c]; t[(size_t)r] = s; }
      double tr = 0, dot = 0, nt = 0, ng = 0;
      for (int i = 0; i < 9; ++i) tr += g.R_21[(size_t)i] * R[(size_t)i];
      for (int i = 0; i < 3; ++i) { dot += g.t_21[(size_t)i] * t[(size_t)i]; nt += t[(size_t)i] * t[(size_t)i]; ng += g.t_21[(size_t)i] * g.t_21[(size_t)i]; }
      const double rot = std::acos(std::fmax(-1.0, std::fmin(1.0, (tr - 1) / 2))) * 180 / M_PI;
      const double dir = std::acos(std::fmax(-1.0, std::fmin(1.0, dot / std::sqrt(nt * ng)))) * 180 / M_PI, ratio = std::sqrt(ng / nt);
      printf("pair (%zu, %zu): inliers %zu, points with depth %d, scale %.4f .. %.4f, |t| / truth %.4f, rotation error %.3g deg, direction error %.3g deg, device - host %.3g\n", a, b,
             g.inlier_idx.size(), g.points_with_depth, g.lower_scale, g.upper_scale, ratio, rot, dir, worst);
      if (dump) fprintf(dump, "%zu %zu %zu %d %.17g %.17g %.17g\n", a, b, g.inlier_idx.size(), g.points_with_depth, g.t_21[0], g.t_21[1], g.t_21[2]);
      if (!(g.upper_scale > 0) || !(std::fabs(ratio - 1.0) <= 0.02) || !(rot <= 0.05) || !(dir <= 0.05)) { fprintf(stderr, "pair %zu: scale or pose outside the bound\n", k); return 1; }
    }
    if (dump) fclose(dump);
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
