// Host-compiled check of K34: the definition of panovlm_amd/csrc/pvlm_essential_core.h (asin / log10 without libm, the Philox sampler, ComputeEssential, the
// AC-RANSAC chain, DecomposeEssential, CheckRT, the selection over the runs) and the host loop of panovlm_amd/host/pvlm_host_essential.hpp.
// tests/test_essential_cpu.py compares them with tests/essential_ref.py without a GPU; tests/test_essential_gpu.py compares the device calls with them bit
// for bit.  With -DESSENTIAL_CHECK_MAIN it is a stand-alone program (the sanitizer build: 9, 120 and N_LDS + 1 matches).  TEST INFRASTRUCTURE ONLY.
// Built with -ffp-contract=off.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host_essential.hpp"

using namespace pvlm_essential;

extern "C" {

void chk_ess_asin(const double* x, int n, double* y) { for (int i = 0; i < n; ++i) y[i] = asin_d(x[i]); }
void chk_ess_log10(const double* x, int n, double* y) { for (int i = 0; i < n; ++i) y[i] = log10_d(x[i]); }
void chk_ess_sample8(unsigned long long seed, int src, int tgt, int run, int k, int m, int* out) { sample8(chain_key(seed, src, tgt, run), k, m, out); }
void chk_ess_compute(const float* p1, const float* p2, int n, double* E, double* sv) { compute_essential(p1, p2, n, E, sv); }
void chk_ess_decompose(const double* E, double* R, double* t) { decompose(E, R, t); }
int chk_ess_nfa_tables(int n, double* tab) { nfa_tables(n, tab); return 2 + 2 * (n + 1); }
double chk_ess_angle_threshold(int* monotone) { bool m; const double c = angle_threshold(&m); *monotone = m ? 1 : 0; return c; }

// one chain.  inliers: n ints; betters: (iteration, nfa) pairs, capacity max_iterations.  Returns the number of inliers; *n_better the number of "better" hypotheses.
int chk_ess_chain(const float* b1, const float* b2, const Match* m, int n, unsigned long long seed, int src, int tgt, int run, int max_iterations, unsigned flags,
                  double* E, double* nfa, int* iterations, int* inliers, int* better_iter, double* better_nfa, int* n_better) {
  std::vector<double> tab(2 + 2 * ((size_t)n + 1));
  nfa_tables(n, tab.data());
  ChainResult ch;
  run_chain(b1, b2, m, n, tab.data(), seed, src, tgt, run, max_iterations, flags, ch);
  std::memcpy(E, ch.E, sizeof ch.E); *nfa = ch.nfa; *iterations = ch.iterations;
  for (size_t i = 0; i < ch.inliers.size(); ++i) inliers[i] = ch.inliers[i];
  *n_better = (int)ch.betters.size();
  for (size_t i = 0; i < ch.betters.size(); ++i) { better_iter[i] = ch.betters[i].first; better_nfa[i] = ch.betters[i].second; }
  return (int)ch.inliers.size();
}

// the host loops over a pair list.  bearings: the frames' rows one frame after the other.  Returns 0, or -1 (PVLM_ERR_ARG).
// raw: E n_pairs * n_runs * 9, nfa n_pairs * n_runs, offsets n_pairs * n_runs + 1, inliers capacity sum(n) * n_runs
int chk_ess_acransac(int n_frames, const int* rows, const float* bearings, int n_pairs, const int* src, const int* tgt, const long long* match_offsets, const Match* matches,
                     int n_runs, int max_iterations, unsigned long long seed, unsigned flags, int n_threads, double* E, double* nfa, long long* offsets, int* inliers,
                     long long* stats4) {
  std::vector<const float*> ptr((size_t)n_frames);
  size_t at = 0;
  for (int f = 0; f < n_frames; ++f) { ptr[(size_t)f] = bearings + 3 * at; at += (size_t)rows[f]; }
  return pvlm::essential_detail::ACRansacHost(n_frames, ptr.data(), rows, n_pairs, src, tgt, match_offsets, matches, n_runs, max_iterations, seed, flags, (size_t)n_threads,
                                              E, nfa, offsets, inliers, stats4);
}
// filter: keep n_pairs, R n_pairs * 9, t n_pairs * 3, offsets n_pairs + 1, inlier_idx / triangulated capacity sum(n)
int chk_ess_filter(int n_frames, const int* rows, const float* bearings, int n_pairs, const int* src, const int* tgt, const long long* match_offsets, const Match* matches,
                   int n_runs, int max_iterations, int tri_threshold, unsigned long long seed, unsigned flags, int n_threads, unsigned char* keep, double* R, double* t,
                   long long* offsets, int* inlier_idx, double* triangulated, long long* stats4) {
  std::vector<const float*> ptr((size_t)n_frames);
  size_t at = 0;
  for (int f = 0; f < n_frames; ++f) { ptr[(size_t)f] = bearings + 3 * at; at += (size_t)rows[f]; }
  std::vector<PairResult> res;
  const int rc = pvlm::essential_detail::FilterPairsHost(n_frames, ptr.data(), rows, n_pairs, src, tgt, match_offsets, matches, n_runs, max_iterations, tri_threshold, seed, flags,
                                                         (size_t)n_threads, res);
  if (rc) return rc;
  offsets[0] = 0; stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const PairResult& r = res[(size_t)p];
    keep[p] = r.keep; std::memcpy(R + 9 * p, r.R, sizeof r.R); std::memcpy(t + 3 * p, r.t, sizeof r.t);
    for (size_t i = 0; i < r.inlier_idx.size(); ++i) inlier_idx[offsets[p] + (long long)i] = r.inlier_idx[i];
    if (!r.triangulated.empty()) std::memcpy(triangulated + 3 * offsets[p], r.triangulated.data(), r.triangulated.size() * sizeof(double));
    offsets[p + 1] = offsets[p] + (long long)r.inlier_idx.size();
    stats4[0] += r.chains; stats4[1] += r.hypotheses;
  }
  return 0;
}

}  // extern "C"

#ifdef ESSENTIAL_CHECK_MAIN
// a two-view scene of n matches (30 % gross outliers) through the host loop; prints keep and the inlier count
static int scene(int n) {
  std::vector<float> b1((size_t)3 * n), b2((size_t)3 * n);
  std::vector<Match> m((size_t)n);
  uint32_t s = 12345u + (uint32_t)n;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; };
  const double ang = 0.2, c = std::cos(ang), sn = std::sin(ang), t[3] = {1.0, 0.1, 0.05};
  for (int i = 0; i < n; ++i) {
    double X[3] = {8 * rnd() - 4, 8 * rnd() - 4, 8 * rnd() - 4};
    double Y[3] = {c * X[0] - sn * X[1] + t[0], sn * X[0] + c * X[1] + t[1], X[2] + t[2]};
    if (i % 10 < 3) { Y[0] = rnd() - 0.5; Y[1] = rnd() - 0.5; Y[2] = rnd() - 0.5; }
    const double nx = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), ny = std::sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
    for (int k = 0; k < 3; ++k) { b1[(size_t)3 * i + k] = (float)(X[k] / nx); b2[(size_t)3 * i + k] = (float)(Y[k] / ny); }
    m[(size_t)i] = Match{i, i, 0.0f};
  }
  const int rows[2] = {n, n}, src = 0, tgt = 1;
  const float* ptr[2] = {b1.data(), b2.data()};
  const long long off[2] = {0, n};
  std::vector<PairResult> res;
  const int rc = pvlm::essential_detail::FilterPairsHost(2, ptr, rows, 1, &src, &tgt, off, m.data(), 3, 40, 5, 7ull, 0u, 2, res);
  std::printf("n = %d: rc %d keep %d inliers %zu hypotheses %lld\n", n, rc, rc ? -1 : (int)res[0].keep, rc ? (size_t)0 : res[0].inlier_idx.size(), rc ? 0ll : res[0].hypotheses);
  return rc;
}
int main() {
  int rc = scene(9);
  rc |= scene(120);
  rc |= scene(kNLds + 1);
  return rc;
}
#endif
