// pvlm_host_neighbor.cpp — part of the C++ host mirror (pvlm_host.hpp): MVS::SelectNeighborSFM and MVS::SelectNeighborViews (mvs/MVS.cpp:66-79, :248-332).
// The score matrix and the selection are pvlm_mvs_select_neighbors_sfm's (K49); the host route is the literal loop of csrc/pvlm_neighbor_sfm_core.h.
#include "pvlm_host_internal.hpp"
#include "../csrc/pvlm_neighbor_sfm_core.h"

namespace pvlm {

bool SelectNeighborSFM(const std::vector<Frame>& frames, const std::vector<PointTrack>& structure, int neighbor_size, float sq_distance_threshold,
                       std::vector<std::vector<NeighborInfo>>& neighbors, const bool host, pvlm_neighbor_sfm_stats* stats, std::vector<std::vector<float>>* scores) {
  namespace ns = pvlm_neighbor_sfm;
  neighbors.assign(frames.size(), {});
  if (scores) scores->assign(frames.size(), {});
  if (structure.empty()) return false;                                          // :250-254
  if (neighbor_size < 0 || frames.size() > (size_t)INT_MAX || structure.size() > (size_t)INT_MAX) return false;
  const int F = (int)frames.size(), T = (int)structure.size();
  std::vector<double> T_wc(12 * (size_t)F + 1);
  std::vector<unsigned char> valid((size_t)F + 1);
  for (int f = 0; f < F; ++f) {
    const Frame& fr = frames[(size_t)f];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T_wc[12 * (size_t)f + 4 * r + c] = fr.R_wc[3 * r + c]; T_wc[12 * (size_t)f + 4 * r + 3] = fr.t_wc[r]; }
    valid[(size_t)f] = fr.IsPoseValid() ? 1 : 0;
  }
  std::vector<int64_t> off((size_t)T + 1, 0);
  std::vector<int> views;
  std::vector<double> points(3 * (size_t)T);
  for (int t = 0; t < T; ++t) {
    for (const std::pair<uint32_t, uint32_t>& p : structure[(size_t)t].feature_pairs) {            // the set's order: image ascending
      if (p.first >= (uint32_t)F) return false;
      views.push_back((int)p.first);
    }
    off[(size_t)t + 1] = (int64_t)views.size();
    for (int k = 0; k < 3; ++k) points[3 * (size_t)t + k] = structure[(size_t)t].point_3d[k];
  }
  views.push_back(0);                                                           // never empty
  if (ns::check_args(F, T_wc.data(), valid.data(), T, off.data(), views.data(), points.data(), neighbor_size, (double)sq_distance_threshold)) return false;
  const size_t slots = (size_t)F * (size_t)neighbor_size;
  std::vector<int> n((size_t)F), ids(slots + 1);
  std::vector<float> R(9 * slots + 1), tt(3 * slots + 1), sc(slots + 1);
  pvlm_neighbor_sfm_stats st{0, 0, 0, 0};
  if (host) {
    ns::Stats hs{0, 0, 0, 0};
    if (ns::select_host(F, T_wc.data(), valid.data(), T, off.data(), views.data(), points.data(), neighbor_size, (double)sq_distance_threshold, n.data(), ids.data(),
                        R.data(), tt.data(), sc.data(), &hs))
      return false;
    st = {hs.n_candidates, hs.n_contributions, hs.n_repeat_tracks, hs.n_uncertain};
  } else {
    Engine& e = Engine::Default();
    e.Check(pvlm_mvs_select_neighbors_sfm(e.ctx(), F, T_wc.data(), valid.data(), T, off.data(), views.data(), points.data(), neighbor_size,
                                          (double)sq_distance_threshold, n.data(), ids.data(), R.data(), tt.data(), sc.data(), &st),
            "pvlm_mvs_select_neighbors_sfm");
  }
  if (stats) *stats = st;
  for (int row = 0; row < F; ++row)
    for (int k = 0; k < n[(size_t)row]; ++k) {
      const size_t at = (size_t)row * neighbor_size + k;
      NeighborInfo info;
      info.id = (size_t)ids[at];
      std::copy(R.begin() + 9 * at, R.begin() + 9 * at + 9, info.R_nr.begin());
      std::copy(tt.begin() + 3 * at, tt.begin() + 3 * at + 3, info.t_nr.begin());
      neighbors[(size_t)row].push_back(info);
      if (scores) (*scores)[(size_t)row].push_back(sc[at]);
    }
  return true;
}

bool SelectNeighborViews(const std::vector<Frame>& frames, const std::vector<PointTrack>& structure, int neighbor_size, int method, float min_distance,
                         std::vector<std::vector<NeighborInfo>>& neighbors, const bool host) {
  neighbors.clear();
  neighbors.resize(frames.size());
  const float sq = min_distance * min_distance;                                 // Square(min_distance)
  if (method == NeighborSelection::NEAREST_NEIGHBOR) { neighbors = SelectNeighborKNN(frames, neighbor_size, sq); return true; }
  if (method == NeighborSelection::SFM_POINTS) return SelectNeighborSFM(frames, structure, neighbor_size, sq, neighbors, host);
  return false;                                                                 // "Unknown neighbor selection method"
}

}  // namespace pvlm
