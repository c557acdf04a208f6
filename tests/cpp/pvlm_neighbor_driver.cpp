// Test driver of the host mirror's SelectNeighborSFM / SelectNeighborViews (K49; panovlm_amd/host/pvlm_host_neighbor.hpp).
//   pvlm_neighbor_driver sfm   <host|device> <scene file> <neighbor_size> <sq_distance_threshold>
//   pvlm_neighbor_driver views <host|device> <scene file> <neighbor_size> <method> <min_distance>
// Scene file: F, then per frame "valid R_wc (9, row-major) t_wc (3)"; T, then per track "x y z n (image feature) x n".
// Output: "ok 0|1", "stats n_candidates n_contributions n_repeat_tracks n_uncertain" (sfm), and per frame "row r n" followed per neighbour by the id, the 12 floats of
// R_nr / t_nr and (sfm) the score, every float as the hexadecimal of its bits.  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: pvlm_neighbor_driver sfm|views host|device scene neighbor_size ...\n"); return 2; }
  const std::string mode = argv[1], route = argv[2];
  const bool host = route == "host";
  std::ifstream in(argv[3]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  auto num = [&in]() { std::string w; in >> w; return std::strtod(w.c_str(), nullptr); };
  size_t F = 0, T = 0;
  in >> F;
  std::vector<pvlm::Frame> frames(F);
  for (size_t f = 0; f < F; ++f) {
    int valid = 0;
    in >> valid;
    frames[f].id = (int)f; frames[f].pose_valid = valid != 0;
    for (int k = 0; k < 9; ++k) frames[f].R_wc[k] = num();
    for (int k = 0; k < 3; ++k) frames[f].t_wc[k] = num();
  }
  in >> T;
  std::vector<pvlm::PointTrack> structure(T);
  for (size_t t = 0; t < T; ++t) {
    structure[t].id = (uint32_t)t;
    for (int k = 0; k < 3; ++k) structure[t].point_3d[k] = num();
    size_t n = 0;
    in >> n;
    for (size_t k = 0; k < n; ++k) { uint32_t image = 0, feature = 0; in >> image >> feature; structure[t].feature_pairs.insert({image, feature}); }
  }
  if (!in) { std::fprintf(stderr, "short scene file\n"); return 2; }
  const int neighbor_size = std::atoi(argv[4]);
  std::vector<std::vector<pvlm::NeighborInfo>> neighbors;
  std::vector<std::vector<float>> scores;
  bool ok = false;
  if (mode == "sfm") {
    pvlm_neighbor_sfm_stats st{0, 0, 0, 0};
    ok = pvlm::SelectNeighborSFM(frames, structure, neighbor_size, (float)std::strtod(argv[5], nullptr), neighbors, host, &st, &scores);
    std::printf("stats %lld %lld %lld %lld\n", st.n_candidates, st.n_contributions, st.n_repeat_tracks, st.n_uncertain);
  } else if (mode == "views" && argc >= 7) {
    ok = pvlm::SelectNeighborViews(frames, structure, neighbor_size, std::atoi(argv[5]), (float)std::strtod(argv[6], nullptr), neighbors, host);
  } else {
    return 2;
  }
  std::printf("ok %d\n", ok ? 1 : 0);
  for (size_t r = 0; r < neighbors.size(); ++r) {
    std::printf("row %zu %zu", r, neighbors[r].size());
    for (size_t k = 0; k < neighbors[r].size(); ++k) {
      const pvlm::NeighborInfo& x = neighbors[r][k];
      std::printf(" %zu", x.id);
      for (float v : x.R_nr) std::printf(" %08x", bits(v));
      for (float v : x.t_nr) std::printf(" %08x", bits(v));
      if (mode == "sfm") std::printf(" %08x", bits(scores[r][k]));
    }
    std::printf("\n");
  }
  return 0;
}
