// Host compile of panovlm_amd/csrc/pvlm_dispatch_core.h (the dispatch order of the fused kernel on a point table) for tests/test_dispatch_order_cpu.py, which loads it
// as a shared object and checks the order of random pair lists.  TEST INFRASTRUCTURE ONLY.  With -DDISPATCH_ORDER_MAIN it is a stand-alone program that draws pair lists
// itself and checks the same properties (for a build with -fsanitize=address,undefined): exit code 0 when all hold.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_dispatch_core.h"

// Work list of a pair list as pvlm_i_resset_finalize lays it out: pair p has blocks[p] consecutive slots, chunk 0, 1, ...; its group key is (nei[p], chunk).
// pos: capacity cap entries.  Returns the number of grid positions, or -1 when cap is too small.
extern "C" int chk_dispatch_order(int n_pairs, const int* nei, const int* blocks, int* pos, int cap) {
  std::vector<int64_t> key;
  for (int p = 0; p < n_pairs; ++p)
    for (int c = 0; c < blocks[p]; ++c) key.push_back(pvlm_dispatch::group_key(nei[p], c));
  std::vector<int> order;
  pvlm_dispatch::build_order((int)key.size(), key.data(), order);
  if ((int)order.size() > cap) return -1;
  if (!order.empty()) std::memcpy(pos, order.data(), order.size() * sizeof(int));
  return (int)order.size();
}

#if defined(DISPATCH_ORDER_MAIN)
static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
  int failures = 0;
  for (int trial = 0; trial < 400; ++trial) {
    const int n_nei = 1 + (int)(rnd() % 12);
    std::vector<int> nei, blocks;
    for (int n = 0; n < n_nei; ++n) {
      const int shared = 1 + (int)(rnd() % 8);                       // 1 - 8 pairs per neighbour
      for (int s = 0; s < shared; ++s) { nei.push_back(n * 7 + 3); blocks.push_back((int)(rnd() % 10)); }   // 0 - 9 blocks per pair
    }
    for (size_t i = nei.size(); i > 1; --i) { const size_t j = rnd() % i; std::swap(nei[i - 1], nei[j]); std::swap(blocks[i - 1], blocks[j]); }
    int slots = 0;
    for (int b : blocks) slots += b;
    std::vector<int> pos((size_t)slots * 8 + 64, -7);
    const int n_pos = chk_dispatch_order((int)nei.size(), nei.data(), blocks.data(), pos.data(), (int)pos.size());
    std::vector<int> seen((size_t)slots, 0), residue((size_t)slots, -1);
    bool ok = n_pos >= slots;
    for (int i = 0; i < n_pos && ok; ++i) {
      if (pos[(size_t)i] == -1) continue;
      if (pos[(size_t)i] < 0 || pos[(size_t)i] >= slots) { ok = false; break; }
      ++seen[(size_t)pos[(size_t)i]]; residue[(size_t)pos[(size_t)i]] = i % 8;
    }
    for (int s = 0; s < slots && ok; ++s) ok = seen[(size_t)s] == 1;
    // members of a group share the residue
    int s0 = 0;
    std::vector<std::pair<int64_t, int>> first;
    for (size_t p = 0; p < nei.size() && ok; ++p)
      for (int c = 0; c < blocks[p] && ok; ++c, ++s0) {
        const int64_t k = pvlm_dispatch::group_key(nei[p], c);
        bool found = false;
        for (auto& f : first) if (f.first == k) { found = true; ok = f.second == residue[(size_t)s0]; }
        if (!found) first.emplace_back(k, residue[(size_t)s0]);
      }
    if (!ok) { ++failures; std::fprintf(stderr, "trial %d failed (%d slots, %d positions)\n", trial, slots, n_pos); }
  }
  std::printf("dispatch order: 400 random pair lists, %d failures\n", failures);
  return failures ? 1 : 0;
}
#endif
