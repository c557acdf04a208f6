// pvlm_host_tracks.hpp — util/Tracks.h:34-107 (UnionFind) and util/Tracks.cpp:14-162 (TrackBuilder for point tracks): what the line tracks of
// LidarLineMatch::GenerateTracks and the feature tracks of TriangulateTracks share.  Standard library only, so that a host check
// (tests/cpp/structure_core_check.cpp) compiles it without the device library.  Not installed; not part of the interface.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <numeric>
#include <set>
#include <utility>
#include <vector>

namespace pvlm {

// union by rank, path compression in Find (m_cc_parent / m_cc_rank / m_cc_size upstream)
struct UnionFind {
  std::vector<unsigned> parent, rank, size;
  void Init(unsigned n) { size.assign(n, 1); parent.resize(n); std::iota(parent.begin(), parent.end(), 0u); rank.assign(n, 0); }
  unsigned Find(unsigned i) { if (parent[i] != i) parent[i] = Find(parent[i]); return parent[i]; }
  void Union(unsigned i, unsigned j) {
    i = Find(i); j = Find(j);
    if (i == j) return;
    if (rank[i] < rank[j]) { parent[i] = j; size[j] += size[i]; }
    else { parent[j] = i; size[i] += size[j]; if (rank[i] == rank[j]) ++rank[i]; }
  }
};

// TrackBuilder(allow_multiple_map = false) as TriangulateTracks uses it: Build, Filter(3), ExportTracks.  A feature is (image, keypoint); its
// index is its position in the sorted set of all features that occur in a match.  The order of events is upstream's: Build unions in match
// order; Filter path-compresses every feature through Find, marks the tracks that visit an image twice or span fewer than `length` images
// and resets them (parent = max, size of the root = 1); ExportTracks then reads the parent array directly: the track id is the root index.
class TrackBuilder {
 public:
  typedef std::pair<uint32_t, uint32_t> Feature;
  explicit TrackBuilder(bool allow_multiple_map = false) : allow_multiple_map_(allow_multiple_map) {}
  // matches[i]: (queryIdx, trainIdx) of image_pairs[i] = (image of the query keypoint, image of the train keypoint)
  bool Build(const std::vector<std::pair<size_t, size_t>>& image_pairs, const std::vector<std::vector<std::pair<int, int>>>& matches) {
    std::set<Feature> all_features;
    for (size_t i = 0; i < image_pairs.size(); i++)
      for (const std::pair<int, int>& m : matches[i]) {
        all_features.emplace((uint32_t)image_pairs[i].first, (uint32_t)m.first);
        all_features.emplace((uint32_t)image_pairs[i].second, (uint32_t)m.second);
      }
    uint32_t count = 0;
    for (const Feature& f : all_features) { feature_to_index_.emplace(f, count); index_to_feature_.push_back(f); count++; }
    max_id_ = (uint32_t)(count - 1);                            // uint32_t arithmetic, as upstream: no feature at all gives 2^32 - 1
    uf_.Init((unsigned)feature_to_index_.size());
    for (size_t i = 0; i < image_pairs.size(); i++)
      for (const std::pair<int, int>& m : matches[i])
        uf_.Union(feature_to_index_[Feature((uint32_t)image_pairs[i].first, (uint32_t)m.first)],
                  feature_to_index_[Feature((uint32_t)image_pairs[i].second, (uint32_t)m.second)]);
    return true;
  }
  bool Filter(uint32_t length) {
    std::map<uint32_t, std::set<uint32_t>> tracks;              // track id -> images
    std::set<uint32_t> problematic;
    for (size_t i = 0; i < feature_to_index_.size(); i++) {
      const uint32_t track_id = uf_.Find((unsigned)i);
      if (tracks[track_id].insert(index_to_feature_[i].first).second == false && !allow_multiple_map_) problematic.insert(track_id);
    }
    for (const auto& val : tracks)
      if (val.second.size() < length) problematic.insert(val.first);
    for (unsigned& root_index : uf_.parent)
      if (problematic.count(root_index) > 0) { uf_.size[root_index] = 1; root_index = std::numeric_limits<uint32_t>::max(); }
    return true;
  }
  bool ExportTracks(std::map<uint32_t, std::set<Feature>>& tracks) const {
    tracks.clear();
    for (uint32_t i = 0; i < feature_to_index_.size(); i++) {
      const uint32_t track_id = uf_.parent[i];
      if (track_id != std::numeric_limits<uint32_t>::max() && uf_.size[track_id] > 1) tracks[track_id].insert(index_to_feature_[i]);
    }
    return tracks.size() > 0;
  }
  // "the largest id a track can have": the index of the last feature.  TriangulateTracks visits track_idx < GetMaxID(), strictly.
  size_t GetMaxID() const { return max_id_; }

 private:
  std::map<Feature, uint32_t> feature_to_index_;
  std::vector<Feature> index_to_feature_;
  UnionFind uf_;
  size_t max_id_ = 0;
  bool allow_multiple_map_;
};

}  // namespace pvlm
