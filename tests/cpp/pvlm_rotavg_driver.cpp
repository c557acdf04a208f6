// Test driver of K40's host mirror (tests/test_rotavg_cpu.py, tests/test_rotavg_gpu.py): reads a pose graph from a text file and runs, through the host compile of
// the core (`host`) or through the device (`device`),
//   pvlm_rotavg_driver estimate host|device <file> <method> <use_all_pairs 0|1>     EstimateGlobalRotation
//   pvlm_rotavg_driver chain host|device <file> <method> <seed>                      EstimateGlobalRotation, then EstimateGlobalTranslation (method 1) on its result
//   pvlm_rotavg_driver triplets host <file>                                          FindTriplet on the pairs of the file
//   pvlm_rotavg_driver filter_triplet host <file> <angle_threshold>                  FilterByTriplet
//   pvlm_rotavg_driver filter_pairs host <file>                                      FilterPairs(pairs, R_cw = the frames' R_wc^T, -1): the X84 threshold and the list
//   pvlm_rotavg_driver tree host <file> <start_idx>                                  RotationAveragingSpanningTree
// File: F, then per frame `id R_wc(9) t_wc(3)`; P, then per pair `first second R_21(9) t_21(3) upper_scale lower_scale`.  `inf` is read as such.
// Output (17 significant digits): `ok 0|1`, `message <text>`, `frame <i> <valid> t_wc(3) R_wc(9)` per frame, `pair <first> <second> R_21(9)` per surviving pair,
// `triplet i j k`, `covered <frame>`, `threshold <radians>`, `rotation <i> R_cw(9)`.
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static double Num(std::istream& in) { std::string s; in >> s; return std::strtod(s.c_str(), nullptr); }

static void PrintPairs(const std::vector<RelativePair>& pairs) {
  for (const RelativePair& p : pairs) {
    std::printf("pair %zu %zu", p.image_pair.first, p.image_pair.second);
    for (double v : p.R_21) std::printf(" %.17g", v);
    std::printf("\n");
  }
}
static void PrintFrames(const std::vector<Frame>& frames) {
  for (size_t i = 0; i < frames.size(); ++i) {
    const Frame& f = frames[i];
    std::printf("frame %zu %d", i, f.IsPoseValid() ? 1 : 0);
    for (double v : f.t_wc) std::printf(" %.17g", v);
    for (double v : f.R_wc) std::printf(" %.17g", v);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_rotavg_driver.cpp\n"); return 2; }
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
    if (argc < 6) return 2;
    std::string message;
    RotationOptions o;
    o.host = host; o.message = &message;
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
    PrintFrames(frames);
    PrintPairs(pairs);
    return 0;
  }
  if (mode == "triplets") {
    std::set<std::pair<size_t, size_t>> edges;
    for (const RelativePair& p : pairs) edges.insert(p.image_pair);
    for (const Triplet& t : FindTriplet(edges)) std::printf("triplet %u %u %u\n", t.i, t.j, t.k);
    return 0;
  }
  if (mode == "filter_triplet") {
    if (argc < 5) return 2;
    std::set<size_t> covered;
    PrintPairs(FilterByTriplet(pairs, std::strtod(argv[4], nullptr), covered));
    for (size_t c : covered) std::printf("covered %zu\n", c);
    return 0;
  }
  if (mode == "filter_pairs") {
    std::vector<Matrix3d> R_cw((size_t)F);
    for (int i = 0; i < F; ++i) { const Matrix3d& R = frames[(size_t)i].R_wc; R_cw[(size_t)i] = Matrix3d{{R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]}}; }
    double threshold = 0;
    const std::vector<RelativePair> kept = FilterPairs(pairs, R_cw, -1, &threshold);
    std::printf("threshold %.17g\n", threshold);
    PrintPairs(kept);
    return 0;
  }
  if (mode == "tree") {
    if (argc < 5) return 2;
    std::vector<Matrix3d> R_cw((size_t)F);
    const bool ok = RotationAveragingSpanningTree(pairs, R_cw, (size_t)std::atoi(argv[4]));
    std::printf("ok %d\n", ok ? 1 : 0);
    for (int i = 0; i < F; ++i) { std::printf("rotation %d", i); for (double v : R_cw[(size_t)i]) std::printf(" %.17g", v); std::printf("\n"); }
    return 0;
  }
  return 2;
}
