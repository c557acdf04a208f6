// pvlm_host_essential.hpp — K34 on the host: the loop body of SfM::FilterImagePairs (sfm/SfM.cpp:298-480, up to RefineRelativePose) over a pair list, on the
// host compile of csrc/pvlm_essential_core.h, the pairs spread over the worker pool.  It serves pvlm::ComputeEssential / DecomposeEssential /
// FindEssentialACRANSAC / CheckRT / FilterImagePairsHost (the baseline tools/essential_bench.py times) and the tests' reference
// (tests/cpp/essential_core_check.cpp).  Not installed; not part of the interface.
#pragma once
#include <atomic>
#include <vector>

#include "../csrc/pvlm_essential_core.h"
#include "../csrc/pvlm_workers.h"

namespace pvlm {
namespace essential_detail {

using pvlm_essential::Match;
using pvlm_essential::PairResult;

// -1 (PVLM_ERR_ARG) for what the entry points refuse: bad parameters, a pair or a match that names what is not there
inline int CheckArgs(int n_frames, const int* rows, int n_pairs, const int* src, const int* tgt, const long long* off, const Match* m, int n_runs, int max_iterations) {
  if (n_runs < 1 || max_iterations < 1 || max_iterations > (1 << 24)) return -1;
  if (n_pairs > 0 && off[0] != 0) return -1;
  for (int p = 0; p < n_pairs; ++p) {
    if (src[p] < 0 || src[p] >= n_frames || tgt[p] < 0 || tgt[p] >= n_frames || off[p + 1] < off[p] || off[p + 1] - off[p] > pvlm_essential::kMaxMatches) return -1;
    for (long long i = off[p]; i < off[p + 1]; ++i)
      if (m[i].query < 0 || m[i].query >= rows[src[p]] || m[i].train < 0 || m[i].train >= rows[tgt[p]]) return -1;
  }
  return 0;
}

// the 3-degree threshold of CheckRT from this process's acos; false when the libm is not monotone there
inline bool CosReject(double* c) { static bool mono = false; static const double v = pvlm_essential::angle_threshold(&mono); *c = v; return mono; }

// the raw per-run result of every pair: E (zero = no model), nfa (+inf for a pair below 9 matches), the chain's inliers one chain after the other.
// stats4: chains, hypotheses, 0, 0.
inline int ACRansacHost(int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt, const long long* off, const Match* m,
                        int n_runs, int max_iterations, unsigned long long seed, unsigned flags, size_t n_threads, double* E, double* nfa, long long* offsets, int* inliers,
                        long long* stats4) {
  if (CheckArgs(n_frames, rows, n_pairs, src, tgt, off, m, n_runs, max_iterations)) return -1;
  std::vector<pvlm_essential::ChainResult> ch((size_t)n_pairs * (size_t)n_runs);
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min(n_threads, (size_t)std::max(n_pairs, 1))), [&]() {
    for (int p = next++; p < n_pairs; p = next++) {
      const int n = (int)(off[p + 1] - off[p]);
      std::vector<double> tab(2 + 2 * ((size_t)std::max(n, 9) + 1));
      if (n > pvlm_essential::kMinSample) pvlm_essential::nfa_tables(n, tab.data());
      for (int r = 0; r < n_runs; ++r) {
        pvlm_essential::ChainResult& c = ch[(size_t)p * (size_t)n_runs + (size_t)r];
        if (n > pvlm_essential::kMinSample) pvlm_essential::run_chain(bearings[src[p]], bearings[tgt[p]], m + off[p], n, tab.data(), seed, src[p], tgt[p], r, max_iterations, flags, c);
        else { for (double& e : c.E) e = 0.0; c.nfa = pvlm_essential::inf_d(); c.iterations = -1; }
      }
    }
  });
  offsets[0] = 0; stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
  for (size_t c = 0; c < ch.size(); ++c) {
    for (int i = 0; i < 9; ++i) E[9 * c + (size_t)i] = ch[c].E[i];
    nfa[c] = ch[c].nfa;
    for (size_t i = 0; i < ch[c].inliers.size(); ++i) inliers[offsets[c] + (long long)i] = ch[c].inliers[i];
    offsets[c + 1] = offsets[c] + (long long)ch[c].inliers.size();
    if (ch[c].iterations >= 0) { stats4[0] += 1; stats4[1] += ch[c].iterations; }
  }
  return 0;
}

inline int FilterPairsHost(int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt, const long long* off, const Match* m,
                           int n_runs, int max_iterations, int triangulation_num_threshold, unsigned long long seed, unsigned flags, size_t n_threads,
                           std::vector<PairResult>& res) {
  if (CheckArgs(n_frames, rows, n_pairs, src, tgt, off, m, n_runs, max_iterations)) return -1;
  double cos_reject;
  if (!CosReject(&cos_reject)) return -3;
  res.assign((size_t)n_pairs, PairResult());
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min(n_threads, (size_t)std::max(n_pairs, 1))), [&]() {
    for (int p = next++; p < n_pairs; p = next++)
      pvlm_essential::filter_pair(bearings[src[p]], bearings[tgt[p]], m + off[p], (int)(off[p + 1] - off[p]), src[p], tgt[p], n_runs, max_iterations,
                                  triangulation_num_threshold, seed, flags, cos_reject, res[(size_t)p]);
  });
  return 0;
}

}  // namespace essential_detail
}  // namespace pvlm
