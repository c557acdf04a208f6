// Host-compiled check of K49: the definition of panovlm_amd/csrc/pvlm_neighbor_sfm_core.h with its literal host loops in place of the kernels of
// pvlm_neighbor_sfm.hip.  tests/test_neighbor_sfm_cpu.py compares it with tests/neighbor_sfm_ref.py without a GPU.  With -DNEIGHBOR_SFM_CHECK_MAIN it is a stand-alone
// program (the sanitizer build).  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_neighbor_sfm_core.h"

namespace ns = pvlm_neighbor_sfm;

extern "C" {

// the two products of one (i, j): out2 = p12, p21
void chk_ns_pair_terms(const double* X, const double* C1, const double* C2, double* out2) { ns::pair_terms(X, C1, C2, &out2[0], &out2[1]); }
float chk_ns_add_to_cell(float cell, double product) { return ns::add_to_cell(cell, product); }
double chk_ns_bound(float score, int n) { return ns::bound(score, n); }
double chk_ns_norm_band() { return ns::kNormBand; }

// pvlm_mvs_select_neighbors_sfm's contract by the literal loop: 0 or -1 (PVLM_ERR_ARG, nothing written); stats4: n_candidates, n_contributions, n_repeat_tracks, n_uncertain
int chk_ns_select(int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets, const int* view_ids, const double* points,
                  int neighbor_size, double threshold, int* n_neighbors, int* ids, float* R_nr, float* t_nr, float* scores, long long* stats4) {
  if (!stats4) return -1;
  ns::Stats s{0, 0, 0, 0};
  const int rc = ns::select_host(F, T_wc, pose_valid, T, track_offsets, view_ids, points, neighbor_size, threshold, n_neighbors, ids, R_nr, t_nr, scores, &s);
  if (rc) return rc;
  stats4[0] = s.n_candidates; stats4[1] = s.n_contributions; stats4[2] = s.n_repeat_tracks; stats4[3] = s.n_uncertain;
  return 0;
}

// one row of the score matrix through the view -> track index (what the device's fall-back runs): scores[F], counts[F]
int chk_ns_row(int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets, const int* view_ids, const double* points, int row,
               float* scores, int* counts) {
  if (ns::check_args(F, T_wc, pose_valid, T, track_offsets, view_ids, points, 0, 0.0) || row < 0 || row >= F) return -1;
  ns::Index ix;
  ix.build(F, T, track_offsets, view_ids);
  ns::row_host(ix, F, T_wc, track_offsets, view_ids, points, row, scores, counts);
  return 0;
}

}  // extern "C"

#ifdef NEIGHBOR_SFM_CHECK_MAIN
// n views on a circle looking at points above it; every track is seen by `len` consecutive views (one of them twice when `repeat`).  Checks that the row form equals
// the dense loop's rows through the selection, the counts against the closed form, the guard words and the refusal of an invalid view.
static int ring(int n, int len, bool repeat) {
  std::vector<double> T_wc(12 * (size_t)n, 0.0), points;
  std::vector<unsigned char> valid((size_t)n, 1);
  for (int v = 0; v < n; ++v) {
    const double a = 6.283185307179586 * v / n;
    double* p = &T_wc[12 * (size_t)v];
    p[0] = std::cos(a); p[1] = -std::sin(a); p[4] = std::sin(a); p[5] = std::cos(a); p[10] = 1;
    p[3] = 10 * std::cos(a); p[7] = 10 * std::sin(a); p[11] = 0.1 * v;
  }
  std::vector<int64_t> off{0};
  std::vector<int> views;
  for (int t = 0; t + len <= n; ++t) {
    for (int k = 0; k < len; ++k) { views.push_back(t + k); if (repeat && k == 1 && (t % 3) == 0) views.push_back(t + k); }
    off.push_back((int64_t)views.size());
    points.push_back(3.0 * std::cos(0.3 * t)); points.push_back(2.0 * std::sin(0.7 * t)); points.push_back(4.0 + 0.01 * t);
  }
  const int T = (int)off.size() - 1, K = 4;
  std::vector<int> nn((size_t)n + 1, -7), ids((size_t)n * K + 1, -7);
  std::vector<float> R(9 * (size_t)n * K + 1, -7.f), tt(3 * (size_t)n * K + 1, -7.f), sc((size_t)n * K + 1, -7.f);
  ns::Stats st{0, 0, 0, 0};
  int bad = ns::select_host(n, T_wc.data(), valid.data(), T, off.data(), views.data(), points.data(), K, 0.5, nn.data(), ids.data(), R.data(), tt.data(), sc.data(), &st);
  bad |= nn[(size_t)n] != -7 || ids[(size_t)n * K] != -7 || R[9 * (size_t)n * K] != -7.f || tt[3 * (size_t)n * K] != -7.f || sc[(size_t)n * K] != -7.f;
  ns::Index ix;
  ix.build(n, T, off.data(), views.data());
  long long contributions = 0, candidates = 0;
  for (int t = 0; t < T; ++t) { const long long l = off[(size_t)t + 1] - off[(size_t)t]; contributions += l * (l - 1); }
  bad |= contributions != st.n_contributions || ix.n_contributions != contributions || ix.n_repeat_tracks != st.n_repeat_tracks;
  std::vector<float> row((size_t)n);
  std::vector<int> cnt((size_t)n);
  for (int v = 0; v < n; ++v) {
    ns::row_host(ix, n, T_wc.data(), off.data(), views.data(), points.data(), v, row.data(), cnt.data());
    const ns::RowResult r = ns::select_row_host(n, T_wc.data(), v, row.data(), K, 0.5);
    candidates += r.n_candidates;
    bad |= r.n != nn[(size_t)v];
    for (int k = 0; k < r.n; ++k) bad |= r.ids[(size_t)k] != ids[(size_t)v * K + k] || r.scores[(size_t)k] != sc[(size_t)v * K + k];
    for (int k = 1; k < r.n; ++k) bad |= !(r.scores[(size_t)k - 1] > r.scores[(size_t)k] || (r.scores[(size_t)k - 1] == r.scores[(size_t)k] && r.ids[(size_t)k - 1] > r.ids[(size_t)k]));
  }
  bad |= candidates != st.n_candidates;
  valid[(size_t)n / 2] = 0;
  const char* why = nullptr;
  bad |= ns::select_host(n, T_wc.data(), valid.data(), T, off.data(), views.data(), points.data(), K, 0.5, nn.data(), ids.data(), R.data(), tt.data(), sc.data(), &st, &why) != -1 || !why;
  std::printf("n = %d len %d repeat %d: tracks %d contributions %lld candidates %lld repeat tracks %lld bad %d\n", n, len, (int)repeat, T, contributions, candidates,
              st.n_repeat_tracks, bad);
  return bad;
}
int main() { return ring(5, 2, false) | ring(9, 3, true) | ring(70, 9, false) | ring(70, 70, true) | ring(200, 7, true); }
#endif
