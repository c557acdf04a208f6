// Test driver of K46's host mirror (tests/test_transdir_cpu.py, tests/test_transdir_gpu.py): reads a pose graph from a text file, runs EstimateGlobalTranslation,
// TranslationAveragingL2Chordal or TranslationAveragingLUD through the host compile of the core (`host`) or through the device (`device`) and prints the result.
//   pvlm_transdir_driver estimate host|device <file> <method> <seed>          (enable_chordal and enable_lud set)
//   pvlm_transdir_driver chordal host|device <file> <unused>
//   pvlm_transdir_driver lud host|device <file> <num_iteration>
// File (the format of tests/cpp/pvlm_transavg_driver.cpp): F, then per frame `id R_wc(9) t_wc(3)`; P, then per pair `first second R_21(9) t_21(3) upper_scale
// lower_scale`.  `inf` is read as such.
// Output (17 significant digits): `ok 0|1`, `message <text>`, `frame <i> <valid> t_wc(3) R_wc(9)` per frame, `pair <first> <second>` per surviving pair; for chordal
// and lud (the frames are the cameras, new_to_old the identity, the start the DLT with camera 0 at zero): `ok`, `iterations <n>` (the LUD solves done), `pairs <n>`,
// `t <i> x y z` per camera (t_cw as the function leaves it).
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
  if (argc < 5) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_transdir_driver.cpp\n"); return 2; }
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
    if (argc < 6) return 2;
    std::string message;
    TranslationOptions o;
    o.host = host; o.seed = std::strtoull(argv[5], nullptr, 10); o.enable_chordal = true; o.enable_lud = true; o.message = &message;
    const bool ok = EstimateGlobalTranslation(frames, pairs, std::atoi(argv[4]), o);
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
  if (mode == "chordal" || mode == "lud") {
    std::map<size_t, size_t> identity;
    for (int i = 0; i < F; ++i) identity[(size_t)i] = (size_t)i;
    std::vector<Vector3d> t((size_t)F, Vector3d{0, 0, 0});
    bool ok = TranslationAveragingDLT(pairs, t, host);
    int iterations = 0;
    if (ok && mode == "chordal") ok = TranslationAveragingL2Chordal(pairs, frames, t, identity, 0, 0.5, host);
    if (ok && mode == "lud") ok = TranslationAveragingLUD(pairs, frames, t, identity, 0, std::atoi(argv[4]), 1.3f, 0.9f, host, &iterations);
    std::printf("ok %d\niterations %d\npairs %zu\n", ok ? 1 : 0, iterations, pairs.size());
    for (int i = 0; i < F; ++i) std::printf("t %d %.17g %.17g %.17g\n", i, t[(size_t)i][0], t[(size_t)i][1], t[(size_t)i][2]);
    return 0;
  }
  return 2;
}
