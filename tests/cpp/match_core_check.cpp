// Host-compiled check of K33: the definition of panovlm_amd/csrc/pvlm_match_core.h (2-NN by the fmaf chain, ratio test, pair filter, screening value and
// bound) and the host loop of panovlm_amd/host/pvlm_host_match.hpp.  tests/test_match_cpu.py compares them with tests/match_ref.py without a GPU;
// tests/test_match_gpu.py compares the device calls with them bit for bit.  TEST INFRASTRUCTURE ONLY.  Built with -ffp-contract=off.
#include <cstring>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_match.hpp"

using namespace pvlm_matching;

extern "C" {

// knnMatch(A, B, 2): idx n1 x 2 (-1 where absent), dist n1 x 2 (+inf where absent)
void chk_match_knn2(const float* A, int n1, const float* B, int n2, int* idx, float* dist) {
  std::vector<Knn2> k((size_t)n1);
  knn2_rows(A, 0, n1, B, n2, k.data());
  for (int i = 0; i < n1; ++i)
    for (int c = 0; c < 2; ++c) { idx[2 * i + c] = k[(size_t)i].idx[c]; dist[2 * i + c] = sqrt_f(k[(size_t)i].d2[c]); }
}

// the plain per-row statement (no eight-row blocking), for the check that the blocked host loop equals it
void chk_match_knn2_plain(const float* A, int n1, const float* B, int n2, int* idx, float* dist) {
  for (int i = 0; i < n1; ++i) {
    const Knn2 k = knn2_row(A + (size_t)i * kDim, B, n2);
    for (int c = 0; c < 2; ++c) { idx[2 * i + c] = k.idx[c]; dist[2 * i + c] = sqrt_f(k.d2[c]); }
  }
}

// MatchSIFT: records (query, train, distance) into out (capacity n1); returns their number
int chk_match_sift(const float* A, int n1, const float* B, int n2, float ratio, Match* out) {
  const std::vector<Match> m = pvlm::match_detail::MatchRows(A, n1, B, n2, ratio);
  if (!m.empty()) std::memcpy(out, m.data(), m.size() * sizeof(Match));
  return (int)m.size();
}

// the pair filter on n records, in place; returns the number left, -1 for a dropped pair
int chk_pair_filter(Match* m, int n, int matches_threshold) {
  std::vector<Match> v(m, m + n);
  if (!pair_filter(v, matches_threshold)) return -1;
  if (!v.empty()) std::memcpy(m, v.data(), v.size() * sizeof(Match));
  return (int)v.size();
}

// the host loop over a pair list.  desc: the frames' rows one frame after the other.  keep: n_pairs; offsets: n_pairs + 1; out: capacity sum of the query rows.
// Returns 0, or -1 (PVLM_ERR_ARG).
int chk_match_pairs(int n_frames, const int* rows, const float* desc, int n_pairs, const int* src, const int* tgt, float ratio, int matches_threshold, int n_threads,
                    unsigned char* keep, long long* offsets, Match* out) {
  std::vector<const float*> ptr((size_t)n_frames);
  size_t at = 0;
  for (int f = 0; f < n_frames; ++f) { ptr[(size_t)f] = desc + at * kDim; at += (size_t)rows[f]; }
  std::vector<unsigned char> k; std::vector<std::vector<Match>> m;
  const int rc = pvlm::match_detail::MatchPairsHost(n_frames, ptr.data(), rows, n_pairs, src, tgt, ratio, matches_threshold, (size_t)n_threads, k, m);
  if (rc) return rc;
  offsets[0] = 0;
  for (int p = 0; p < n_pairs; ++p) {
    keep[p] = k[(size_t)p];
    if (!m[(size_t)p].empty()) std::memcpy(out + offsets[p], m[(size_t)p].data(), m[(size_t)p].size() * sizeof(Match));
    offsets[p + 1] = offsets[p] + (long long)m[(size_t)p].size();
  }
  return 0;
}

// the screening value of (a, b) with the dot product as an fmaf chain in index order, its bound E = screen_bound(norm2(a), norm2(b)), and the definition's d2
void chk_screen(const float* a, const float* b, float* s, float* E, float* d2) {
  float dot = 0.0f;
  for (int k = 0; k < kDim; ++k) dot = fma_f(a[k], b[k], dot);
  const float na = norm2(a), nb = norm2(b);
  *s = screen_value(na, nb, dot); *E = screen_bound(na, nb); *d2 = d2_exact(a, b);
}

int chk_certified(float s_c, float E, float d2_second) { return certified(s_c, E, d2_second) ? 1 : 0; }

}  // extern "C"
