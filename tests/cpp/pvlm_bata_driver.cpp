// Test driver of K44's host mirror (tests/test_bata_cpu.py, tests/test_bata_gpu.py): reads a pose graph from a text file, runs EstimateGlobalTranslation or
// TranslationAveragingBATA through the host compile of the core (`host`) or through the device (`device`) and prints the result.
//   pvlm_bata_driver estimate host|device <file> <method> <seed> <use_all_pairs 0|1> <init_translation_DLT 0|1> <enable_bata 0|1>
//   pvlm_bata_driver bata host|device <file> <seed>
// File (the format of tests/cpp/pvlm_transavg_driver.cpp): F, then per frame `id R_wc(9) t_wc(3)`; P, then per pair `first second R_21(9) t_21(3) upper_scale
// lower_scale`.  `inf` is read as such.
// Output (17 significant digits): `ok 0|1`, `message <text>`, `frame <i> <valid> t_wc(3) R_wc(9)` per frame, `pair <first> <second>` per surviving pair; for bata
// (the frames are the cameras, new_to_old the identity): `ok`, `t <i> x y z` per camera (t_cw as the function leaves it), `scale0 <p> <v>` per pair (the start scale).
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
  if (argc < 5) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_bata_driver.cpp\n"); return 2; }
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
    if (argc < 9) return 2;
    std::string message;
    TranslationOptions o;
    o.host = host; o.seed = std::strtoull(argv[5], nullptr, 10); o.use_all_pairs_ta = std::atoi(argv[6]) != 0; o.init_translation_DLT = std::atoi(argv[7]) != 0;
    o.enable_bata = std::atoi(argv[8]) != 0; o.message = &message;
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
  if (mode == "bata") {
    std::map<size_t, size_t> identity;
    for (int i = 0; i < F; ++i) identity[(size_t)i] = (size_t)i;
    std::vector<Vector3d> t((size_t)F, Vector3d{0, 0, 0});
    std::vector<double> start;
    const bool ok = TranslationAveragingBATA(pairs, frames, t, identity, 0, BATAConfig(), std::strtoull(argv[4], nullptr, 10), host, &start);
    std::printf("ok %d\n", ok ? 1 : 0);
    for (size_t i = 0; i < t.size(); ++i) std::printf("t %zu %.17g %.17g %.17g\n", i, t[i][0], t[i][1], t[i][2]);
    for (size_t p = 0; p < start.size(); ++p) std::printf("scale0 %zu %.17g\n", p, start[p]);
    return 0;
  }
  return 2;
}
