// Host compile of csrc/pvlm_scale_core.h (K39) for the tests: one pair's SetTranslationScaleDepthMap with the lanes of the wave taken one after the other
// (pvlm_scale::HostTeam), built with -ffp-contract=off.  With -DSCALE_CHECK_MAIN it is a stand-alone program (the sanitizer build): scenes of 4 .. 700 points that take
// every exit, each compared bit for bit with relpose_detail::SetScaleOne.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_scale_core.h"
#include "../../panovlm_amd/host/pvlm_host_relpose.hpp"

extern "C" {

int chk_scale_lanes() { return pvlm_scale::kLanes; }

// t (3) and tri (3 n) in / out.  out6: points_with_depth, upper, lower (the three left as they come in when the core does not write them), exit, consistent points,
// whether both maps were there.  Returns ok.
int chk_scale_pair(int eq_rows, int eq_cols, int rows1, const uint16_t* d1, int d1_rows, int d1_cols, const uint16_t* d2, int d2_rows, int d2_cols, const double* R, double* t,
                   double* tri, int n, double* out6) {
  std::vector<double> cur(2 * (size_t)n + 1), keep(2 * (size_t)n + 1);
  pvlm_scale::Pair P;
  P.n = n; P.eq_rows = eq_rows; P.eq_cols = eq_cols; P.rows1 = rows1;
  P.d1 = pvlm_scale::Map{d1_rows > 0 ? d1 : nullptr, d1_rows, d1_cols}; P.d2 = pvlm_scale::Map{d2_rows > 0 ? d2 : nullptr, d2_rows, d2_cols};
  P.cur = cur.data(); P.keep = keep.data();
  pvlm_scale::HostTeam team;
  pvlm_scale::Result r;
  pvlm_scale::scale_pair(team, P, R, t, tri, &r);
  if (r.maps) out6[0] = r.points_with_depth;
  if (r.ok) { out6[1] = r.upper; out6[2] = r.lower; }
  out6[3] = r.exit; out6[4] = r.consistent; out6[5] = r.maps;
  return r.ok;
}

// relpose_detail::SetScaleOne, the host step, over a pair list on ONE thread (the baseline tools/scale_bench.py times): the arrays of pvlm_set_translation_scales
// with the maps as host pointers (null: the frame has none).  Returns the number of scaled pairs.
int chk_scale_list_host(int eq_rows, int eq_cols, const int* frame_rows, const uint16_t* const* maps, const int* map_rows, const int* map_cols, int n_pairs, const int* src,
                        const int* tgt, const long long* off, const double* R, double* t, double* tri, unsigned char* ok, int* pwd, double* upper, double* lower) {
  using namespace pvlm::relpose_detail;
  int scaled = 0;
  for (int p = 0; p < n_pairs; ++p) {
    TailPair tp;
    std::memcpy(tp.R, R + 9 * (size_t)p, sizeof tp.R); std::memcpy(tp.t, t + 3 * (size_t)p, sizeof tp.t);
    tp.tri.assign(tri + 3 * (size_t)off[p], tri + 3 * (size_t)off[p + 1]);
    tp.points_with_depth = pwd[p]; tp.upper_scale = upper[p]; tp.lower_scale = lower[p];
    DepthView a, b;
    a.data = maps[src[p]]; a.rows = map_rows[src[p]]; a.cols = map_cols[src[p]]; b.data = maps[tgt[p]]; b.rows = map_rows[tgt[p]]; b.cols = map_cols[tgt[p]];
    ok[p] = SetScaleOne(eq_rows, eq_cols, frame_rows[src[p]], a, b, tp) ? 1 : 0;
    scaled += ok[p];
    std::memcpy(t + 3 * (size_t)p, tp.t, sizeof tp.t);
    std::copy(tp.tri.begin(), tp.tri.end(), tri + 3 * (size_t)off[p]);
    pwd[p] = tp.points_with_depth; upper[p] = tp.upper_scale; lower[p] = tp.lower_scale;
  }
  return scaled;
}

}  // extern "C"

#ifdef SCALE_CHECK_MAIN
#include <cmath>

// n points in front of both cameras, two maps that hold scale x depth x factor at the pixels they round to; mode 0: every factor 1 (early break), 1: most factors near
// 1 and the rest spread over 0.5 .. 1.6 (histogram passes), 2: factors 1 .. 2 with the second map 15 % off (median for small n)
static int scene(int n, int mode, bool half) {
  using namespace pvlm::relpose_detail;
  const int rows = 96, cols = 192, k = half ? 2 : 1;
  const int mr = half ? (rows + 1) / 2 : rows, mc = half ? (cols + 1) / 2 : cols;
  std::vector<uint16_t> d1((size_t)mr * mc, 0), d2((size_t)mr * mc, 0);
  uint32_t s = 4242u + (uint32_t)n * 7u + (uint32_t)mode;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; };
  const double ang = 0.1, c = std::cos(ang), sn = std::sin(ang);
  const double R[9] = {c, 0, sn, 0, 1, 0, -sn, 0, c};
  double t[3] = {0.8, 0.1, -0.59};
  std::vector<double> tri(3 * (size_t)n + 3);
  for (int i = 0; i < n; ++i) {
    double* p = &tri[3 * (size_t)i];
    p[0] = -4 + 8 * rnd(); p[1] = -4 + 8 * rnd(); p[2] = 2 + 4 * rnd();
    double f = 1.0, f2 = 1.0;
    if (mode == 1) f = rnd() < 0.7 ? 0.97 + 0.06 * rnd() : 0.5 + 1.1 * rnd();
    if (mode == 2) { f = 1.0 + (n > 1 ? (double)i / (n - 1) : 0.0); f2 = 1.15; }
    double q[3];
    for (int r = 0; r < 3; ++r) q[r] = (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r];
    const double* cam[2] = {p, q};
    std::vector<uint16_t>* map[2] = {&d1, &d2};
    for (int w = 0; w < 2; ++w) {
      double px[2];
      CamToImaged(rows, cols, cam[w], px);
      const int row = (int)std::round(px[1] / k), col = (int)std::round(px[0] / k);
      if (row < 0 || row >= mr || col < 0 || col >= mc) continue;
      const double depth = std::sqrt(cam[w][0] * cam[w][0] + cam[w][1] * cam[w][1] + cam[w][2] * cam[w][2]);
      const double v = std::round(2.5 * f * (w ? f2 : 1.0) * depth * 256);
      (*map[w])[(size_t)row * mc + col] = (uint16_t)(v > 65535 ? 65535 : v);
    }
  }
  TailPair ref;
  std::memcpy(ref.R, R, sizeof R); std::memcpy(ref.t, t, sizeof t); ref.tri.assign(tri.begin(), tri.begin() + 3 * (std::ptrdiff_t)n);
  DepthView a, b;
  a.data = d1.data(); a.rows = mr; a.cols = mc; b.data = d2.data(); b.rows = mr; b.cols = mc;
  const bool ref_ok = SetScaleOne(rows, cols, rows, a, b, ref);
  double out[6] = {0, -1, -1, 0, 0, 0};
  const int ok = chk_scale_pair(rows, cols, rows, d1.data(), mr, mc, d2.data(), mr, mc, R, t, tri.data(), n, out);
  int bad = ok != (ref_ok ? 1 : 0) || (int)out[0] != ref.points_with_depth || std::memcmp(&out[1], &ref.upper_scale, 8) || std::memcmp(&out[2], &ref.lower_scale, 8) ||
            std::memcmp(t, ref.t, sizeof t) || (n > 0 && std::memcmp(tri.data(), ref.tri.data(), 24 * (size_t)n));
  std::printf("n %d mode %d half %d: ok %d exit %d consistent %d with_depth %d upper %.17g lower %.17g %s\n", n, mode, (int)half, ok, (int)out[3], (int)out[4], (int)out[0],
              out[1], out[2], bad ? "MISMATCH" : "equal");
  return bad ? 1 : 0;
}

int main() {
  int rc = 0;
  const int sizes[] = {0, 4, 5, 6, 63, 64, 65, 129, 200, 700};
  for (int n : sizes)
    for (int mode = 0; mode < 3; ++mode) { rc |= scene(n, mode, true); rc |= scene(n, mode, false); }
  return rc;
}
#endif
