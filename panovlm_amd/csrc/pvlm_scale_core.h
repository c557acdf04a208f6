// Statement of K39: SfM::SetTranslationScaleDepthMap(eq, pair) (sfm/SfM.cpp:487-603) for ONE pair, operation by operation what relpose_detail::SetScaleOne
// (host/pvlm_host_relpose.hpp) computes, its documented divergence included (a rounded pixel inside the image but outside the map it indexes skips the point).
// Host / device: csrc/pvlm_scale.hip runs scale_pair with one wave of kLanes lanes per pair; tests/cpp/scale_core_check.cpp and the host mirror run the same
// function with the lanes taken one after the other (HostTeam).  Compile with -ffp-contract=off.
//
// Every number is a function of the pair alone:
//   survivors   point i belongs to lane i mod kLanes of trip i / kLanes; a trip's survivors are placed behind the running count by ballot and popcount, so the list
//               holds (scale1, scale2) of the survivors in point order.
//   min, max    of positive numbers without a NaN among them: no order dependence (the wave butterfly on the device).
//   a pass      bin index (int)((s - min - 1e-8) / interval) clamped to 0 .. 9; the counts are popcounts of per-bin ballots; a bin stays when
//               (double)count > 0.1 * (double)num (strict); the new list is offset[bin] + (elements of the bin before this one): kept bins in bin order, each bin in
//               its previous list order.
//   mean        the list added from left to right starting at 0.0 (Team::ordered_sum: one order, whoever adds), divided by its length.
//   median      the value v of the preserved list with #(< v) <= k < #(<= v), k = size / 2: what nth_element leaves at position k.
// Two lists of 2 n doubles each serve all of it (2 x 16 B per point): the survivors go to `keep` (current and preserved list are equal until the first pass), pass 1
// reads keep and writes cur, pass 2 reads cur and writes keep -- the preserved list has no reader once pass 2 runs (the fall-back is decided before it).
// Conversions of a double that no int holds (a quotient by a zero or infinite interval: a point at the origin or beyond 1e154) take x86-64's answer, INT_MIN, on both
// sides.  A list that pass 2 leaves EMPTY (upstream dereferences end() there) gives a NaN scale here; the pair still reports ok.
#pragma once
#include <cmath>

#include "pvlm_equirect_core.h"

#ifndef PVLM_SC_HD
#if defined(__HIPCC__)
#define PVLM_SC_HD __host__ __device__ __forceinline__
#else
#define PVLM_SC_HD inline
#endif
#endif

namespace pvlm_scale {

constexpr int kLanes = 64;
constexpr int kBins = 10;
constexpr int kMinScales = 10;
enum Exit { kExitNone = 0, kExitMean = 1, kExitMedian = 2 };

struct Map { const unsigned short* data; int rows, cols; };               // rows x cols uint16 (depth x 256), row-major; empty: data null or a size <= 0
struct Pair {
  int n;                        // triangulated points
  int eq_rows, eq_cols;         // the one Equirectangular of all frames
  int rows1;                    // image rows of the pair's first frame (the half-size test)
  Map d1, d2;
  double* cur; double* keep;    // 2 n doubles each
};
struct Result {
  int ok;                       // scaled
  int maps;                     // both maps were there: points_with_depth is written (0 when not scaled)
  int exit;                     // Exit
  int points_with_depth;
  int consistent;               // points that gave a scale pair
  double upper, lower;          // written when ok
};

PVLM_SC_HD bool empty(const Map& m) { return !m.data || m.rows <= 0 || m.cols <= 0; }
PVLM_SC_HD int to_int(double q) { return (q >= 2147483648.0 || q <= -2147483649.0 || q != q) ? (-2147483647 - 1) : (int)q; }
PVLM_SC_HD int popc(unsigned long long m) { return (int)__builtin_popcountll(m); }
PVLM_SC_HD unsigned long long below(int lane) { return (1ull << lane) - 1ull; }

// the depth of the map at the pixel cam projects to, as the scale real depth / |cam|; false: the point is skipped
PVLM_SC_HD bool scale_at(const Pair& P, const Map& d, double div, const double* cam, double* scale) {
  double u, v;
  pvlm_equirect::cam_to_image_f64(P.eq_rows, P.eq_cols, cam[0], cam[1], cam[2], &u, &v);
  u = u / div; v = v / div;
  const int row = to_int(::round(v)), col = to_int(::round(u));
  if (!(col >= 0 && row >= 0 && col + 1 <= P.eq_cols && row + 1 <= P.eq_rows)) return false;       // Equirectangular::IsInside(cv::Point2i)
  if (row >= d.rows || col >= d.cols) return false;
  const double depth = sqrt(cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2]);
  const float real = (float)(d.data[(size_t)row * (size_t)d.cols + (size_t)col] / 256.0);
  if (real <= 0) return false;
  *scale = real / depth;
  return true;
}

PVLM_SC_HD bool point_scales(const Pair& P, double div, const double* R, const double* t, const double* p, double* s1, double* s2) {
  if (!scale_at(P, P.d1, div, p, s1)) return false;
  double q[3];
  for (int r = 0; r < 3; ++r) q[r] = (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r];
  if (!scale_at(P, P.d2, div, q, s2)) return false;
  const double a = *s1, b = *s2;
  const double d = a - b;
  return !((d < 0 ? -d : d) / (b < a ? b : a) > 0.2);
}

PVLM_SC_HD int bin_of(double s, double mn, double interval) {
  int b = to_int((s - mn - 1e-8) / interval);
  b = b < kBins - 1 ? b : kBins - 1;
  return b > 0 ? b : 0;
}

// A Team runs the kLanes lanes of a pair.
//   template <class F> unsigned long long vote(F&& f)              f(lane) -> bool for every lane; bit `lane` of the result is f's answer
//   template <class F> void each(F&& f)                             f(lane) for every lane
//   template <class F> void minmax(double* mn, double* mx, F&& f)   f(lane, lo, hi) with lo = +inf, hi = -inf; the minimum of the lo's and the maximum of the hi's
//   double* regs(lane), int* ireg(lane)                             two doubles and an int a lane keeps between a vote and the each behind it
//   double ordered_sum(const double* v, int m)                      ((0.0 + v[0]) + v[1]) + .. + v[m - 1]
//   void sync()                                                     what the lanes wrote to cur / keep is visible to all of them
// HostTeam: the lanes one after the other.  The device's team is in csrc/pvlm_scale.hip.
struct HostTeam {
  double r[kLanes][2]; int ir[kLanes];
  template <class F> unsigned long long vote(F&& f) { unsigned long long m = 0; for (int l = 0; l < kLanes; ++l) if (f(l)) m |= 1ull << l; return m; }
  template <class F> void each(F&& f) { for (int l = 0; l < kLanes; ++l) f(l); }
  template <class F> void minmax(double* mn, double* mx, F&& f) {
    double a = HUGE_VAL, b = -HUGE_VAL;
    for (int l = 0; l < kLanes; ++l) { double lo = HUGE_VAL, hi = -HUGE_VAL; f(l, lo, hi); a = lo < a ? lo : a; b = hi > b ? hi : b; }
    *mn = a; *mx = b;
  }
  double* regs(int lane) { return r[lane]; }
  int* ireg(int lane) { return &ir[lane]; }
  double ordered_sum(const double* v, int m) { double s = 0.0; for (int j = 0; j < m; ++j) s += v[j]; return s; }
  void sync() {}
};

template <class Team>
PVLM_SC_HD void list_minmax(Team& team, const double* v, int m, double* mn, double* mx) {
  team.minmax(mn, mx, [&](int lane, double& lo, double& hi) {
    for (int j = lane; j < m; j += kLanes) { const double s = v[j]; lo = s < lo ? s : lo; hi = s > hi ? s : hi; }
  });
}

// one histogram pass over src[0 .. m): the kept bins into dst, the new length returned
template <class Team>
PVLM_SC_HD int histo_pass(Team& team, const double* src, int m, double mn, double interval, double* dst) {
  int cnt[kBins], off[kBins], run[kBins];
  for (int b = 0; b < kBins; ++b) cnt[b] = 0;
  for (int base = 0; base < m; base += kLanes) {
    team.each([&](int lane) { const int j = base + lane; *team.ireg(lane) = j < m ? bin_of(src[j], mn, interval) : -1; });
    for (int b = 0; b < kBins; ++b) cnt[b] += popc(team.vote([&](int lane) { return *team.ireg(lane) == b; }));
  }
  int total = 0;
  for (int b = 0; b < kBins; ++b) {
    const bool stays = (double)cnt[b] > 0.1 * (double)m;
    off[b] = stays ? total : -1;
    if (stays) total += cnt[b];
    run[b] = 0;
  }
  for (int base = 0; base < m; base += kLanes) {
    team.each([&](int lane) {
      const int j = base + lane;
      const double s = j < m ? src[j] : 0.0;
      team.regs(lane)[0] = s; *team.ireg(lane) = j < m ? bin_of(s, mn, interval) : -1;
    });
    for (int b = 0; b < kBins; ++b) {
      const unsigned long long mask = team.vote([&](int lane) { return *team.ireg(lane) == b; });
      if (off[b] >= 0) team.each([&](int lane) { if ((mask >> lane) & 1ull) dst[off[b] + run[b] + popc(mask & below(lane))] = team.regs(lane)[0]; });
      run[b] += popc(mask);
    }
  }
  return total;
}

// the element of rank k of v[0 .. m)
template <class Team>
PVLM_SC_HD double rank_select(Team& team, const double* v, int m, int k) {
  for (int base = 0; base < m; base += kLanes) {
    const unsigned long long hit = team.vote([&](int lane) {
      const int c = base + lane;
      if (c >= m) return false;
      const double x = v[c];
      int lt = 0, le = 0;
      for (int j = 0; j < m; ++j) { const double y = v[j]; lt += y < x; le += y <= x; }
      team.regs(lane)[0] = x;
      return lt <= k && k < le;
    });
    if (hit) {
      double lo, hi;
      team.minmax(&lo, &hi, [&](int lane, double& a, double& b) { if ((hit >> lane) & 1ull) { a = team.regs(lane)[0]; b = a; } });
      return lo;                                       // every hit holds the same value
    }
  }
  return 0.0;                                          // not reached for m > 0 without a NaN
}

// One pair.  R (9, row-major) is read; t (3) and tri (3 n) are read and, when the pair is scaled, multiplied by the scale.  *res is written by every lane alike.
template <class Team>
PVLM_SC_HD void scale_pair(Team& team, const Pair& P, const double* R_in, double* t, double* tri, Result* res) {
  Result out = {0, 0, kExitNone, 0, 0, 0.0, 0.0};
  *res = out;
  if (empty(P.d1) || empty(P.d2)) return;
  out.maps = 1;
  const int n = P.n;
  const double div = 1.0 + (P.d1.rows == (P.rows1 + 1) / 2 ? 1.0 : 0.0);
  double R[9], t0[3];
  for (int k = 0; k < 9; ++k) R[k] = R_in[k];
  for (int k = 0; k < 3; ++k) t0[k] = t[k];
  int count = 0;
  for (int base = 0; base < n; base += kLanes) {
    const unsigned long long mask = team.vote([&](int lane) {
      const int i = base + lane;
      if (i >= n) return false;
      const double p[3] = {tri[3 * (size_t)i], tri[3 * (size_t)i + 1], tri[3 * (size_t)i + 2]};
      double s1 = 0.0, s2 = 0.0;
      const bool good = point_scales(P, div, R, t0, p, &s1, &s2);
      team.regs(lane)[0] = s1; team.regs(lane)[1] = s2;
      return good;
    });
    team.each([&](int lane) {
      if (!((mask >> lane) & 1ull)) return;
      const size_t pos = 2 * (size_t)(count + popc(mask & below(lane)));
      P.keep[pos] = team.regs(lane)[0]; P.keep[pos + 1] = team.regs(lane)[1];
    });
    count += popc(mask);
  }
  team.sync();
  out.consistent = count;
  const int m0 = 2 * count;
  if (m0 < kMinScales) { *res = out; return; }
  const double* list = P.keep;
  int m = m0;
  bool good = true;
  for (int iter = 0; iter < 2; ++iter) {
    if (m < kMinScales) { good = false; break; }
    double mn, mx;
    list_minmax(team, list, m, &mn, &mx);
    if (mx / mn < 1.2) break;
    const double interval = (mx - mn) / (double)kBins;
    double* dst = iter == 0 ? P.cur : P.keep;
    m = histo_pass(team, list, m, mn, interval, dst);
    list = dst;
    team.sync();
  }
  double final_scale;
  if (good) {
    final_scale = team.ordered_sum(list, m) / (double)m;
    out.points_with_depth = m / 2;
    list_minmax(team, list, m, &out.lower, &out.upper);
    out.exit = kExitMean;
  } else {
    final_scale = rank_select(team, P.keep, m0, m0 / 2);
    out.upper = 0.0; out.lower = 0.0;
    out.points_with_depth = m0 / 2;
    out.exit = kExitMedian;
  }
  out.ok = 1;
  team.each([&](int lane) {
    if (lane < 3) t[lane] = t0[lane] * final_scale;
    for (size_t j = (size_t)lane; j < 3 * (size_t)n; j += kLanes) tri[j] *= final_scale;
  });
  *res = out;
}

}  // namespace pvlm_scale
