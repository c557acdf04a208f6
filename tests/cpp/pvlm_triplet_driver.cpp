// Test driver of K48's host mirror (tests/test_triplet_cpu.py, tests/test_triplet_gpu.py): reads a pose graph from a text file and runs, through the host compile
// of the core (`host`) or through the device (`device`),
//   pvlm_triplet_driver find host|device <file>                                   FindTriplet with TranslationAveragingL1's three map lookups per triplet
//                                                                                 (`ref_triplet`, `ref_tpairs`), then FindTripletDevice (`triplet`, `tpairs`)
//   pvlm_triplet_driver filter host|device <file> <angle_threshold> <device 0|1>  FilterByTriplet (0) or FilterByTripletDevice (1)
//   pvlm_triplet_driver estimate host|device <file> <method> <device_triplets>    EstimateGlobalRotation
//   pvlm_triplet_driver l1 host|device <file> <device_triplets>                   TranslationAveragingL1 (the frames are the cameras, camera 0 the origin)
//   pvlm_triplet_driver bench host <file> <angle_threshold>                       one-thread wall clock of the host walk (tools/triplet_bench.py): one `bench {json}` line
// File (the format of tests/cpp/pvlm_rotavg_driver.cpp): F, then per frame `id R_wc(9) t_wc(3)`; P, then per pair `first second R_21(9) t_21(3) upper_scale
// lower_scale`.  `inf` and `nan` are read as such.
// Output (17 significant digits): `ok 0|1`, `message <text>`, `frame <i> <valid> t_wc(3) R_wc(9)` per frame, `pair <first> <second> R_21(9)` per surviving pair,
// `covered <frame>`, `stats n_triplets n_kept_triplets n_uncertain n_kept_pairs`, `summary` and `t` as tests/cpp/pvlm_translp_driver.cpp.
// TEST INFRASTRUCTURE ONLY.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"
#include "../../panovlm_amd/csrc/pvlm_triplet_core.h"

using namespace pvlm;

static double Num(std::istream& in) { std::string s; in >> s; return std::strtod(s.c_str(), nullptr); }

static void PrintPairs(const std::vector<RelativePair>& pairs) {
  for (const RelativePair& p : pairs) {
    std::printf("pair %zu %zu", p.image_pair.first, p.image_pair.second);
    for (double v : p.R_21) std::printf(" %.17g", v);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: see the head of tests/cpp/pvlm_triplet_driver.cpp\n"); return 2; }
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
  if (mode == "find") {
    std::set<std::pair<size_t, size_t>> edges;
    for (const RelativePair& p : pairs) edges.insert(p.image_pair);
    std::map<std::pair<size_t, size_t>, int> place;
    for (const std::pair<size_t, size_t>& e : edges) { const int at = (int)place.size(); place[e] = at; }
    for (const Triplet& t : FindTriplet(edges)) {
      std::printf("ref_triplet %u %u %u\n", t.i, t.j, t.k);
      std::printf("ref_tpairs %d %d %d\n", place[{t.i, t.j}], place[{t.j, t.k}], place[{t.i, t.k}]);
    }
    std::vector<int> tp;
    const std::vector<Triplet> found = FindTripletDevice(edges, &tp, host);
    for (size_t k = 0; k < found.size(); ++k) {
      std::printf("triplet %u %u %u\n", found[k].i, found[k].j, found[k].k);
      std::printf("tpairs %d %d %d\n", tp[3 * k], tp[3 * k + 1], tp[3 * k + 2]);
    }
    return 0;
  }
  if (mode == "filter") {
    if (argc < 6) return 2;
    std::set<size_t> covered;
    const double threshold = std::strtod(argv[4], nullptr);
    if (std::atoi(argv[5]) != 0) {
      pvlm_triplet_stats st{-1, -1, -1, -1};
      PrintPairs(FilterByTripletDevice(pairs, threshold, covered, host, &st));
      std::printf("stats %lld %lld %lld %lld\n", st.n_triplets, st.n_kept_triplets, st.n_uncertain, st.n_kept_pairs);
    } else PrintPairs(FilterByTriplet(pairs, threshold, covered));
    for (size_t c : covered) std::printf("covered %zu\n", c);
    return 0;
  }
  if (mode == "estimate") {
    if (argc < 6) return 2;
    std::string message;
    RotationOptions o;
    o.host = host; o.message = &message; o.device_triplets = std::atoi(argv[5]) != 0;
    const bool ok = EstimateGlobalRotation(frames, pairs, std::atoi(argv[4]), o);
    std::printf("ok %d\nmessage %s\n", ok ? 1 : 0, message.c_str());
    for (size_t i = 0; i < frames.size(); ++i) {
      const Frame& f = frames[i];
      std::printf("frame %zu %d", i, f.IsPoseValid() ? 1 : 0);
      for (double v : f.t_wc) std::printf(" %.17g", v);
      for (double v : f.R_wc) std::printf(" %.17g", v);
      std::printf("\n");
    }
    PrintPairs(pairs);
    return 0;
  }
  if (mode == "bench") {
    // one thread, wall clock: the host mirror's walk as its two consumers run it, and the host compile of the K48 core beside it
    if (argc < 5) return 2;
    const double threshold = std::strtod(argv[4], nullptr);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
    std::set<std::pair<size_t, size_t>> edges;
    std::map<std::pair<size_t, size_t>, int> place;
    std::vector<int> first, second;
    std::vector<double> R;
    for (const RelativePair& p : pairs) edges.insert(p.image_pair);
    for (const std::pair<size_t, size_t>& e : edges) { const int at = (int)place.size(); place[e] = at; first.push_back((int)e.first); second.push_back((int)e.second); }
    std::map<std::pair<size_t, size_t>, size_t> last;
    for (size_t i = 0; i < pairs.size(); ++i) last[pairs[i].image_pair] = i;
    for (const auto& kv : last) R.insert(R.end(), pairs[kv.second].R_21.begin(), pairs[kv.second].R_21.end());
    auto t0 = now();
    const std::vector<Triplet> triplets = FindTriplet(edges);
    const double find_s = since(t0);
    t0 = now();
    std::vector<int> trip_pairs;
    for (const Triplet& tr : triplets) { trip_pairs.push_back(place[{tr.i, tr.j}]); trip_pairs.push_back(place[{tr.j, tr.k}]); trip_pairs.push_back(place[{tr.i, tr.k}]); }
    const double place_s = since(t0);
    std::set<size_t> covered;
    t0 = now();
    const std::vector<RelativePair> filtered = FilterByTriplet(pairs, threshold, covered);
    const double filter_all_s = since(t0);
    // the list FilterByTriplet hands its LargestBiconnectedGraph, from the core's keep bytes; that step alone
    const int Fc = F, Pc = (int)first.size();
    std::vector<unsigned char> keep((size_t)Pc + 1, 0);
    pvlm_triplet::Stats st{0, 0, 0, 0};
    first.push_back(0); second.push_back(0); R.resize(R.size() + 9);
    t0 = now();
    const int rc = pvlm_triplet::filter_host(Fc, Pc, first.data(), second.data(), R.data(), threshold, keep.data(), &st);
    const double core_filter_s = since(t0);
    std::vector<RelativePair> kept;
    for (const RelativePair& p : pairs) if (keep[(size_t)place[p.image_pair]]) kept.push_back(p);
    t0 = now();
    const std::vector<RelativePair> again = LargestBiconnectedGraph(kept, covered);
    const double biconnected_s = since(t0);
    long long needed = 0;
    std::vector<int> t3(3 * triplets.size() + 3), p3(3 * triplets.size() + 3);
    t0 = now();
    const int rc2 = pvlm_triplet::find_host(Fc, Pc, first.data(), second.data(), t3.data(), p3.data(), (long long)triplets.size(), &needed, nullptr);
    const double core_find_s = since(t0);
    p3.resize(trip_pairs.size());
    std::printf("bench {\"host_find_triplet_s\": %.6f, \"host_place_lookups_s\": %.6f, \"host_filter_by_triplet_s\": %.6f, \"host_largest_biconnected_s\": %.6f, "
                "\"host_filter_without_biconnected_s\": %.6f, \"core_host_find_s\": %.6f, \"core_host_filter_s\": %.6f, \"triplets\": %zu, \"same_triplet_pairs\": %d, "
                "\"same_filter_list\": %d, \"n_uncertain\": %lld}\n", find_s, place_s, filter_all_s, biconnected_s, filter_all_s - biconnected_s, core_find_s, core_filter_s,
                triplets.size(), rc2 == 0 && needed == (long long)triplets.size() && p3 == trip_pairs ? 1 : 0, rc == 0 && again.size() == filtered.size() ? 1 : 0, st.n_uncertain);
    return 0;
  }
  if (mode == "l1") {
    if (argc < 5) return 2;
    std::vector<Vector3d> t((size_t)F, Vector3d{0, 0, 0});
    pvlm_translp_summary s{0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
    const bool ok = TranslationAveragingL1(pairs, t, 0, host, &s, std::atoi(argv[4]) != 0);
    std::printf("ok %d\nsummary %.17g %.17g %.17g %.17g %.17g %d %d %d %d %d\n", ok ? 1 : 0, s.gamma, s.dual_objective, s.gap, s.primal_residual, s.dual_residual, s.iterations,
                s.bumps, s.n_components, s.n_loose, s.termination);
    for (int i = 0; i < F; ++i) std::printf("t %d %.17g %.17g %.17g\n", i, t[(size_t)i][0], t[(size_t)i][1], t[(size_t)i][2]);
    return 0;
  }
  return 2;
}
