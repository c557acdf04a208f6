// Host-compiled check of K48: the definition of panovlm_amd/csrc/pvlm_triplet_core.h with its host loops in place of the kernels of pvlm_triplet.hip.
// tests/test_triplet_cpu.py compares it with find_triplet_ref / filter_by_triplet_ref of tests/rotavg_ref.py without a GPU; tests/test_triplet_gpu.py compares
// pvlm_triplets_find / pvlm_triplets_filter with the same references.  With -DTRIPLET_CHECK_MAIN it is a stand-alone program (the sanitizer build).
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_triplet_core.h"

namespace tr = pvlm_triplet;

extern "C" {

int chk_triplet_group_size() { return tr::kGroup; }
double chk_triplet_band() { return tr::kBand; }

// pvlm_triplets_find's contract: 0, -1 (PVLM_ERR_ARG, nothing written) or -5 (PVLM_ERR_CAPACITY)
int chk_triplets_find(int F, int P, const int* first, const int* second, int* triplets, int* triplet_pairs, long long capacity, long long* needed, long long* pair_counts) {
  return tr::find_host(F, P, first, second, triplets, triplet_pairs, capacity, needed, pair_counts);
}

// pvlm_triplets_filter's contract; stats4: n_triplets, n_kept_triplets, n_uncertain, n_kept_pairs
int chk_triplets_filter(int F, int P, const int* first, const int* second, const double* R21, double angle_threshold, unsigned char* keep, long long* stats4) {
  if (!stats4) return -1;
  tr::Stats s{0, 0, 0, 0};
  const int rc = tr::filter_host(F, P, first, second, R21, angle_threshold, keep, &s);
  if (rc) return rc;
  stats4[0] = s.n_triplets; stats4[1] = s.n_kept_triplets; stats4[2] = s.n_uncertain; stats4[3] = s.n_kept_pairs;
  return 0;
}

// the loop measure and both decisions of one triplet: out3 = c, the verdict of classify against cut_for(threshold), the literal test
void chk_triplet_measure(const double* R_21, const double* R_32, const double* R_31, double angle_threshold, double* out3) {
  const double c = tr::loop_cos(R_21, R_32, R_31);
  out3[0] = c; out3[1] = (double)tr::classify(c, tr::cut_for(angle_threshold)); out3[2] = tr::keep_literal(c, angle_threshold) ? 1.0 : 0.0;
}

}  // extern "C"

#ifdef TRIPLET_CHECK_MAIN
// n cameras, every camera paired with its next `reach`, the list reversed; rotations about z whose loop errors grow with the camera number.  Checks the count against
// the closed form, the order, the pair indices, the capacity rule with a guard word, and that the filter's kept triplets fall with the threshold.
static int chain(int n, int reach) {
  std::vector<int> first, second; std::vector<double> R;
  for (int a = n - 1; a >= 0; --a)
    for (int k = reach; k >= 1; --k) {
      if (a + k >= n) continue;
      first.push_back(a); second.push_back(a + k);
      const double d = 0.01 * k + 1e-4 * a * (k == 2), cd = std::cos(d), sd = std::sin(d);
      const double m[9] = {cd, -sd, 0, sd, cd, 0, 0, 0, 1};
      R.insert(R.end(), m, m + 9);
    }
  const int P = (int)first.size();
  first.push_back(0); second.push_back(0); R.resize(R.size() + 9);
  long long needed = -1;
  int bad = tr::find_host(n, P, first.data(), second.data(), nullptr, nullptr, 0, &needed, nullptr);
  std::vector<int> t(3 * (size_t)needed + 3, -7), tp(3 * (size_t)needed + 3, -7);
  std::vector<long long> pc((size_t)P + 1, -7);
  bad |= tr::find_host(n, P, first.data(), second.data(), t.data(), tp.data(), needed, &needed, pc.data());
  long long sum = 0;
  for (int p = 0; p < P; ++p) sum += pc[(size_t)p];
  bad |= sum != needed || t[3 * (size_t)needed] != -7 || tp[3 * (size_t)needed] != -7 || pc[(size_t)P] != -7;
  for (long long k = 0; k < needed; ++k) {
    const int* a = &t[3 * (size_t)k]; const int* q = &tp[3 * (size_t)k];
    bad |= !(a[0] < a[1] && a[1] < a[2]);
    bad |= first[(size_t)q[0]] != a[0] || second[(size_t)q[0]] != a[1] || first[(size_t)q[1]] != a[1] || second[(size_t)q[1]] != a[2] || first[(size_t)q[2]] != a[0] || second[(size_t)q[2]] != a[2];
    if (k) { const int* b = a - 3; bad |= !(b[0] < a[0] || (b[0] == a[0] && (b[1] < a[1] || (b[1] == a[1] && b[2] < a[2])))); }
  }
  if (needed > 0) {
    std::vector<int> small(3 * (size_t)(needed - 1) + 3, -7);
    long long again = -1;
    bad |= tr::find_host(n, P, first.data(), second.data(), small.data(), nullptr, needed - 1, &again, nullptr) != -5 || again != needed || small[3 * (size_t)(needed - 1)] != -7;
  }
  std::vector<unsigned char> keep((size_t)P + 1, 7);
  long long kept_before = -1;
  for (double thr : {0.0, 0.05, 0.5, 5.0, 200.0}) {
    tr::Stats s{0, 0, 0, 0};
    bad |= tr::filter_host(n, P, first.data(), second.data(), R.data(), thr, keep.data(), &s);
    bad |= s.n_triplets != needed || s.n_kept_triplets < kept_before || keep[(size_t)P] != 7;
    bad |= (thr == 0.0 && s.n_kept_triplets != 0) || (thr == 200.0 && s.n_kept_triplets != needed);
    kept_before = s.n_kept_triplets;
  }
  std::printf("n = %d reach %d: pairs %d triplets %lld kept at 5 degrees and above %lld bad %d\n", n, reach, P, needed, kept_before, bad);
  return bad;
}
int main() { return chain(1, 3) | chain(3, 2) | chain(9, 3) | chain(70, 69) | chain(300, 19); }
#endif
