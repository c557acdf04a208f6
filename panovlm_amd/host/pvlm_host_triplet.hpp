// K48 in the host mirror: PoseGraph::FindTriplet and SfM::FilterByTriplet through pvlm_triplets_find / pvlm_triplets_filter (see pvlm.h for the definition), beside
// the std::set / std::map walks FindTriplet and FilterByTriplet, which stay as they are and are what these two are compared with.  Included at the end of
// pvlm_host.hpp; defined in pvlm_host_sfm.cpp.  host = true runs the host compile of csrc/pvlm_triplet_core.h (no device) in place of the library call.
#pragma once

namespace pvlm {

// FindTriplet's list, triplet for triplet.  edges: first < second in every edge (what every caller in the mirror has checked; an empty list comes back otherwise,
// where upstream's walk would emit triplets under other names).  The cameras are 0 .. the largest id.  triplet_pairs, when given, receives per triplet the positions
// of (i,j), (j,k), (i,k) in the set's order: what TranslationAveragingL1 builds with three std::map lookups per triplet, in pvlm_transavg_l1's layout.
std::vector<Triplet> FindTripletDevice(const std::set<std::pair<size_t, size_t>>& edges, std::vector<int>* triplet_pairs = nullptr, const bool host = false);

// FilterByTriplet's list.  A pair named twice is handled as the mirror handles it: the last rotation wins (upstream's map assignment), and every list entry of a kept
// pair survives; then the host's LargestBiconnectedGraph.  stats: the call's, when given.  An empty list for a pair with first >= second (upstream asserts).
std::vector<RelativePair> FilterByTripletDevice(const std::vector<RelativePair>& init_pairs, const double angle_threshold, std::set<size_t>& covered_frames,
                                                const bool host = false, pvlm_triplet_stats* stats = nullptr);

}  // namespace pvlm
