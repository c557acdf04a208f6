// pvlm_host_match.hpp — K33 on the host: MatchSIFT (util/SIFT.cpp:130-162) on two descriptor arrays and the loop of SfM::MatchImagePairs
// (sfm/SfM.cpp:253-286) over a pair list, both on the host compile of csrc/pvlm_match_core.h, the pairs spread over the worker pool.  It serves
// pvlm::MatchSIFT (a handful of rows on the host), pvlm::MatchImagePairsHost (the baseline tools/match_bench.py times) and the tests' reference
// (tests/cpp/match_core_check.cpp).  Not installed; not part of the interface.
#pragma once
#include <atomic>
#include <vector>

#include "../csrc/pvlm_match_core.h"
#include "../csrc/pvlm_workers.h"

namespace pvlm {
namespace match_detail {

using pvlm_matching::Match;

// the ratio-test matches of descriptor rows A (n1 x 128) against B (n2 x 128), in query order; none when a side is empty or B has one row
inline std::vector<Match> MatchRows(const float* A, int n1, const float* B, int n2, float ratio) {
  std::vector<Match> m;
  if (n1 <= 0 || n2 <= 0) return m;
  std::vector<pvlm_matching::Knn2> k((size_t)n1);
  pvlm_matching::knn2_rows(A, 0, n1, B, n2, k.data());
  for (int i = 0; i < n1; ++i) { float d; if (pvlm_matching::ratio_keep(k[(size_t)i], ratio, &d)) m.push_back(Match{i, k[(size_t)i].idx[0], d}); }
  return m;
}

// every pair: MatchRows, then the pair filter.  keep[p] and matches[p] (empty for a dropped pair), in the order of the list.  -1 (PVLM_ERR_ARG) for a negative
// threshold or a frame index outside [0, n_frames), 0 otherwise.
inline int MatchPairsHost(int n_frames, const float* const* desc, const int* rows, int n_pairs, const int* src, const int* tgt, float ratio, int matches_threshold,
                          size_t n_threads, std::vector<unsigned char>& keep, std::vector<std::vector<Match>>& matches) {
  if (matches_threshold < 0) return -1;
  for (int p = 0; p < n_pairs; ++p) if (src[p] < 0 || src[p] >= n_frames || tgt[p] < 0 || tgt[p] >= n_frames) return -1;
  keep.assign((size_t)n_pairs, 0); matches.assign((size_t)n_pairs, std::vector<Match>());
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min(n_threads, (size_t)std::max(n_pairs, 1))), [&]() {
    for (int p = next++; p < n_pairs; p = next++) {
      std::vector<Match> m = MatchRows(desc[src[p]], rows[src[p]], desc[tgt[p]], rows[tgt[p]], ratio);
      keep[(size_t)p] = pvlm_matching::pair_filter(m, matches_threshold) ? 1 : 0;
      matches[(size_t)p].swap(m);
    }
  });
  return 0;
}

}  // namespace match_detail
}  // namespace pvlm
