// Test driver of K45's host mirror (tests/test_rotstart_cpu.py, tests/test_rotstart_gpu.py): reads a pose graph from a text file and runs, through the host compiles
// of the cores (`host`) or through the device (`device`),
//   pvlm_rotstart_driver estimate host|device <file> <method> <use_all_pairs 0|1> <enable_l2_start 0|1>     EstimateGlobalRotation
//   pvlm_rotstart_driver chain host|device <file> <method> <seed> <enable_l2_start 0|1>                      EstimateGlobalRotation, then EstimateGlobalTranslation (method 1)
//   pvlm_rotstart_driver lsq host|device <file>                                                              RotationAveragingLeastSquare on the pairs of the file
// File and output: the formats of tests/cpp/pvlm_rotavg_driver.cpp (`ok`, `message`, `frame`, `pair`, `rotation` lines, 17 significant digits).
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
  if (argc < 4) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_rotstart_driver.cpp\n"); return 2; }
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
  if (mode == "estimate" || mode == "chain") {
    if (argc < 7) return 2;
    std::string message;
    RotationOptions o;
    o.host = host; o.message = &message; o.enable_l2_start = std::atoi(argv[6]) != 0;
    if (mode == "estimate") o.use_all_pairs_ra = std::atoi(argv[5]) != 0;
    bool ok = EstimateGlobalRotation(frames, pairs, std::atoi(argv[4]), o);
    std::printf("ok %d\nmessage %s\n", ok ? 1 : 0, message.c_str());
    if (mode == "chain" && ok) {
      TranslationOptions t;
      t.host = host; t.seed = std::strtoull(argv[5], nullptr, 10); t.message = &message;
      message.clear();
      ok = EstimateGlobalTranslation(frames, pairs, TRANSLATION_AVERAGING_SOFTL1, t);
      std::printf("translation_ok %d\ntranslation_message %s\n", ok ? 1 : 0, message.c_str());
    }
    for (size_t i = 0; i < frames.size(); ++i) {
      const Frame& f = frames[i];
      std::printf("frame %zu %d", i, f.IsPoseValid() ? 1 : 0);
      for (double v : f.t_wc) std::printf(" %.17g", v);
      for (double v : f.R_wc) std::printf(" %.17g", v);
      std::printf("\n");
    }
    for (const RelativePair& p : pairs) {
      std::printf("pair %zu %zu", p.image_pair.first, p.image_pair.second);
      for (double v : p.R_21) std::printf(" %.17g", v);
      std::printf("\n");
    }
    return 0;
  }
  if (mode == "lsq") {
    std::vector<Matrix3d> R_cw((size_t)F, Matrix3d{{-7, -7, -7, -7, -7, -7, -7, -7, -7}});
    const bool ok = RotationAveragingLeastSquare(pairs, R_cw, host);
    std::printf("ok %d\n", ok ? 1 : 0);
    for (int i = 0; i < F; ++i) { std::printf("rotation %d", i); for (double v : R_cw[(size_t)i]) std::printf(" %.17g", v); std::printf("\n"); }
    return 0;
  }
  return 2;
}
