// Dispatch order of the block-form fused kernel on a point table (k_eval_fused, pvlm_resset::point_table): which work-list slot the workgroup at grid
// position i evaluates.  The work-list entries (pair, chunk) whose pairs share the neighbour scan and whose chunk number is the same read the same slice
// of that scan's point table.  Workgroups are dealt round-robin over the 8 XCDs in the order of their grid position, and every XCD has an L2 of its
// own: a slice is fetched once per XCD that touches it, and stays cheap only while its readers run at about the same time.  So the members of a group get
// positions with the same residue modulo 8, eight apart: groups are taken eight at a time, one per residue, and laid out column by column,
//     position = tile base + 8 * (member number) + (group number inside the tile).
// A tile is as tall as its largest group; a shorter group leaves padding positions (-1: the workgroup returns at once).  Groups are tiled in order of
// falling size (stable), so that a tile's groups are of nearly the same size and the padding stays below 8 x the largest group over the whole list.
// Placement is speed only: the partial sums are written at the SLOT, and everything behind the kernel reads them by slot.
// Host only (no device code); compiled into libpvlm.so and, alone, into tests/cpp/dispatch_order_driver.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

namespace pvlm_dispatch {

constexpr int kXcds = 8;

// key[s]: the group of slot s (any value; equal keys = one group).  pos: slot of every grid position, -1 = padding.  Every slot appears exactly once.
inline void build_order(int n_slots, const int64_t* key, std::vector<int>& pos) {
  pos.clear();
  if (n_slots <= 0) return;
  std::map<int64_t, std::vector<int>> by_key;
  for (int s = 0; s < n_slots; ++s) by_key[key[s]].push_back(s);
  std::vector<const std::vector<int>*> groups;
  groups.reserve(by_key.size());
  for (const auto& g : by_key) groups.push_back(&g.second);
  std::stable_sort(groups.begin(), groups.end(), [](const std::vector<int>* a, const std::vector<int>* b) { return a->size() > b->size(); });
  for (size_t t = 0; t < groups.size(); t += kXcds) {
    const size_t rows = groups[t]->size();                       // the tile's largest group (sorted)
    for (size_t r = 0; r < rows; ++r)
      for (size_t k = 0; k < (size_t)kXcds; ++k) {
        const bool has = t + k < groups.size() && r < groups[t + k]->size();
        pos.push_back(has ? (*groups[t + k])[r] : -1);
      }
  }
}

// the group key of a work-list entry: neighbour scan and chunk number
inline int64_t group_key(int nei, int chunk) { return ((int64_t)nei << 32) | (uint32_t)chunk; }

inline void identity_order(int n_slots, std::vector<int>& pos) {
  pos.resize((size_t)std::max(n_slots, 0));
  for (int s = 0; s < n_slots; ++s) pos[(size_t)s] = s;
}

}  // namespace pvlm_dispatch
