// Test driver of K47's host mirror (tests/test_translp_cpu.py, tests/test_translp_gpu.py): reads a pose graph from a text file, runs EstimateGlobalTranslation with
// method 2 or TranslationAveragingL1 by hand through the host compile of the core (`host`) or through the device (`device`) and prints the result.
//   pvlm_translp_driver estimate host|device <file> <enable_l1> <seed>
//   pvlm_translp_driver l1 host|device <file> <unused> <unused>
// File (the format of tests/cpp/pvlm_transavg_driver.cpp): F, then per frame `id R_wc(9) t_wc(3)`; P, then per pair `first second R_21(9) t_21(3) upper_scale
// lower_scale`.  `inf` is read as such.
// Output (17 significant digits): `ok 0|1`, `message <text>`, `frame <i> <valid> t_wc(3) R_wc(9)` per frame, `pair <first> <second>` per surviving pair; for l1 (the
// frames are the cameras, camera 0 the origin): `ok`, `summary gamma dual_objective gap primal_residual dual_residual iterations bumps n_components n_loose
// termination`, `t <i> x y z` per camera (t_cw as the function leaves it).
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static double Num(std::istream& in) { std::string s; in >> s; return std::strtod(s.c_str(), nullptr); }

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_translp_driver.cpp\n"); return 2; }
  const std::string mode = argv[1];
  const bool host = std::strcmp(argv[2], "host") == 0;
  std::ifstream in(argv[3]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  const int F = (int)Num(in);
  std::vector<Frame> frames((size_t)F);
  for (Frame& f : frames) {
    f.id = (int)Num(in);
    for (double& v : f.R_wc) v = Num(in);
    for (double& v : f.t_wc) v = Num(in);
    f.pose_valid = false;
  }
  const int P = (int)Num(in);
  std::vector<RelativePair> pairs((size_t)P);
  for (RelativePair& p : pairs) {
    p.image_pair.first = (size_t)Num(in); p.image_pair.second = (size_t)Num(in);
    for (double& v : p.R_21) v = Num(in);
    for (double& v : p.t_21) v = Num(in);
    p.upper_scale = Num(in); p.lower_scale = Num(in);
  }
  if (mode == "estimate") {
    std::string message;
    TranslationOptions o;
    o.host = host; o.seed = std::strtoull(argv[5], nullptr, 10); o.enable_l1 = std::atoi(argv[4]) != 0; o.message = &message;
    const bool ok = EstimateGlobalTranslation(frames, pairs, TRANSLATION_AVERAGING_L1, o);
    std::printf("ok %d\nmessage %s\n", ok ? 1 : 0, message.c_str());
    for (int i = 0; i < F; ++i) {
      const Frame& f = frames[(size_t)i];
      std::printf("frame %d %d", i, f.IsPoseValid() ? 1 : 0);
      for (double v : f.t_wc) std::printf(" %.17g", v);
      for (double v : f.R_wc) std::printf(" %.17g", v);
      std::printf("\n");
    }
    for (const RelativePair& p : pairs) std::printf("pair %zu %zu\n", p.image_pair.first, p.image_pair.second);
    return 0;
  }
  if (mode == "l1") {
    std::vector<Vector3d> t((size_t)F, Vector3d{0, 0, 0});
    pvlm_translp_summary s{0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
    const bool ok = TranslationAveragingL1(pairs, t, 0, host, &s);
    std::printf("ok %d\nsummary %.17g %.17g %.17g %.17g %.17g %d %d %d %d %d\n", ok ? 1 : 0, s.gamma, s.dual_objective, s.gap, s.primal_residual, s.dual_residual, s.iterations,
                s.bumps, s.n_components, s.n_loose, s.termination);
    for (int i = 0; i < F; ++i) std::printf("t %d %.17g %.17g %.17g\n", i, t[(size_t)i][0], t[(size_t)i][1], t[(size_t)i][2]);
    return 0;
  }
  return 2;
}
