// Statement of K37: DepthCompletion (util/DepthCompletion.cpp:154-316) and the uint16 conversion of SfM::ComputeDepthImage (sfm/SfM.cpp:170-226): the IP-Basic style
// chain that turns the sparse LiDAR depth image of ProjectLidar2PanoramaDepth into the dense map SetTranslationScaleDepthMap reads.  Host / device:
// csrc/pvlm_depthfill.hip wraps the per-pixel functions below in tiled kernels, the host mirror runs the whole-image host loop at the end of this file
// (DepthCompletion, ComputeDepthImageHost), and a host compile (tests/cpp/depthfill_core_check.cpp) is what the CPU tests compare with numpy and the GPU tests
// compare with bit for bit.  Compile with -ffp-contract=off.
//
// All images are fp32, rows x cols.  sel(m, b, a) = b where m, else a: upstream writes every blend as a.mul(1 - m) + b.mul(m) with m in {0, 1}, which is sel for
// finite values >= +0; that is why the entry points refuse an fp32 input with a sign bit or a non-finite value.  M = max_depth as float.
//   S0    s0 = sel(d <= M, d, 0)
//   masks near = s0 > 0.1 && s0 <= 15; med = s0 > 15 && s0 <= 30; far = s0 > 30; v = s0 > 0.1
//   S1    s1 = sel(v, M - s0, s0)
//   S2    df = dilate(sel(far, s1, 0), cross3), dm = dilate(sel(med, s1, 0), cross5), dn = dilate(sel(near, s1, 0), cross7);
//         s2 = s1, then s2 = sel(df > 0.1, df, s2), s2 = sel(dm > 0.1, dm, s2), s2 = sel(dn > 0.1, dn, s2)
//   S3    s3 = erode(dilate(s2, full5), full5)
//   S4    s4 = sel(s3 > 0.1, median5(s3), s3)
//   top 1 top[c] = first row with s4 > 0.1, 0 for a column without one; tm = row >= top[c]
//   S5    s5 = sel(!(s4 > 0.1) && tm, dilate(s4, full9), s4)
//   top 2 the same scan of s5 > 0.1: tm2
//   S7a   six times s7 = sel(s7 < 0.1 && tm2, dilate(s7, full5), s7), from s7 = s5 (0.1f itself is neither valid nor empty)
//   S7b   v = s7 > 0.1 && tm2; s7 = sel(v, median5(s7), s7)
//   S7c   s7 = sel(v, bilateral(s7), s7), v still that of S7b
//   S8    out = sel(s7 > 0.1, M - s7, s7)
//   u16   rint(out * 256.f) to nearest-even, saturated to [0, 65535] (ComputeDepthImage only)
// cross3/5/7: the centre row and the centre column; full5/9: all-ones squares; the anchor is the centre.  The squares are separable and max / min of finite
// values >= +0 do not depend on the order of the taps, so a row pass followed by a column pass gives the same bits as the square.
// Kept quirks: a valid depth d >= M - 0.1 turns "empty" from S2 on; values in (0, 0.1] pass through; max_depth = 5 only ever uses the near band.
//
// [recalled] OpenCV semantics the stages rest on (there is no OpenCV build to pin them against): dilate / erode use a constant border that never wins, so taps
// outside the image are ignored; medianBlur(.., 5) on CV_32F replicates the border and returns the 13th smallest of 25; minMaxLoc returns the first occurrence;
// convertTo(CV_16U) is saturate_cast<ushort>(cvRound(x)), half to even; bilateralFilter(src, dst, 5, 0.5, 2.0) has radius 2, the circular mask dy^2 + dx^2 <= 4
// (13 taps) and BORDER_REFLECT_101.
//
// Deliberate divergence, the bilateral filter.  OpenCV's fp32 bilateral takes its colour weight from a 4096-bin interpolated table scaled to the image's min / max,
// differently in 3.4 and 4.x: nothing to be bit-equal to.  Ours: the 13 taps in order dy ascending, then dx ascending; reflect-101 applied until the index is in
// range (a dimension of length 1 maps to 0); in fp64 D = (double)tap - (double)centre, w = WS[dy^2 + dx^2] * exp_neg(2 D^2), WS[0, 1, 2, 4] = 1, e^-0.125, e^-0.25,
// e^-0.5 as correctly rounded literals; out = (float)(sum w tap / sum w), both sums ascending in tap order.
// exp_neg(x), x >= 0: e^-x from IEEE + * / and integer bit operations only, so that host, device and numpy give the same bits: k = (long long)(x / ln 2 + 0.5),
// r = (k ln2_hi - x) + k ln2_lo (Cody-Waite, k ln2_hi exact), the degree-13 Taylor polynomial of e^r in Horner order, times 2^-k through the exponent field; exactly
// 0.0 for x >= 708.  Measured against math.exp(-x) (tests/test_depthfill_cpu.py): see DESIGN.md, K37.
#pragma once
#include <cstdint>
#include <cstring>
#if !defined(__HIPCC__)
#include <algorithm>
#include <atomic>
#include <vector>

#include "pvlm_equirect_core.h"
#include "pvlm_exact_math.h"
#include "pvlm_workers.h"
#endif

#if defined(__HIPCC__)
#define PVLM_DF_HD __host__ __device__ inline
#else
#define PVLM_DF_HD inline
#endif

namespace pvlm_depthfill {

constexpr float kValid = 0.1f, kNear = 15.f, kMed = 30.f;
// reach of the stages of the three phases the two column scans cut the chain into
constexpr int kReachA = 3 + 2 + 2 + 2, kReachB = 4, kReachC = 6 * 2 + 2 + 2, kFillRounds = 6;

PVLM_DF_HD float sel(bool m, float b, float a) { return m ? b : a; }
PVLM_DF_HD float max2(float a, float b) { return b > a ? b : a; }
PVLM_DF_HD float min2(float a, float b) { return b < a ? b : a; }
PVLM_DF_HD float from_u16(unsigned v) { return (float)v * 0.00390625f; }            // value / 256, exact
PVLM_DF_HD float s0_of(float d, float M) { return sel(d <= M, d, 0.f); }
PVLM_DF_HD float invert(float x, float M) { return sel(x > kValid, M - x, x); }     // S1 and S8
PVLM_DF_HD int band(float s0) { return !(s0 > kValid) ? 0 : s0 <= kNear ? 1 : s0 <= kMed ? 2 : 3; }
// an fp32 input the entry points take: finite and without a sign bit (-0.0 is refused with the negatives: max / min would have to order it)
PVLM_DF_HD bool input_ok(float d) { uint32_t b; __builtin_memcpy(&b, &d, 4); return b <= 0x7f7fffffu; }

// S2 of one pixel.  s0_at(dr, dc): s0 of the tap, 0.f outside the image (a masked 0 there never changes a maximum of values >= +0 that includes the centre).
template <class A> PVLM_DF_HD float s2_pixel(const A& s0_at, float M) {
  float dn = 0.f, dm = 0.f, df = 0.f;
  const float c = s0_at(0, 0);
#pragma unroll
  for (int k = 0; k <= 3; ++k) {
#pragma unroll
    for (int j = 0; j < (k == 0 ? 1 : 4); ++j) {
      const float t = j == 0 ? s0_at(-k, 0) : j == 1 ? s0_at(k, 0) : j == 2 ? s0_at(0, -k) : s0_at(0, k);
      const int b = band(t);
      const float s1 = invert(t, M);
      if (b == 1) dn = max2(dn, s1);                                                // cross7
      if (b == 2 && k <= 2) dm = max2(dm, s1);                                      // cross5
      if (b == 3 && k <= 1) df = max2(df, s1);                                      // cross3
    }
  }
  float s2 = invert(c, M);
  s2 = sel(df > kValid, df, s2);
  s2 = sel(dm > kValid, dm, s2);
  s2 = sel(dn > kValid, dn, s2);
  return s2;
}

// maximum / minimum of the 2 R + 1 taps at(-R) .. at(R); a tap outside the image is a value that never wins
template <int R, class A> PVLM_DF_HD float run_max(const A& at) { float m = at(-R); for (int k = -R + 1; k <= R; ++k) m = max2(m, at(k)); return m; }
template <int R, class A> PVLM_DF_HD float run_min(const A& at) { float m = at(-R); for (int k = -R + 1; k <= R; ++k) m = min2(m, at(k)); return m; }

// the 13th smallest of 25 finite values: a fixed selection network of 99 exchanges (N. Devillard, "Fast median search: an ANSI C implementation", 1998; checked on all
// 2^25 zero-one inputs), every index a constant so that the values stay in registers
#define PVLM_DF_X(a, b) { const float lo = min2(p[a], p[b]); p[b] = max2(p[a], p[b]); p[a] = lo; }
PVLM_DF_HD float median25(float* p) {
  PVLM_DF_X(0, 1) PVLM_DF_X(3, 4) PVLM_DF_X(2, 4) PVLM_DF_X(2, 3) PVLM_DF_X(6, 7) PVLM_DF_X(5, 7) PVLM_DF_X(5, 6) PVLM_DF_X(9, 10) PVLM_DF_X(8, 10)
  PVLM_DF_X(8, 9) PVLM_DF_X(12, 13) PVLM_DF_X(11, 13) PVLM_DF_X(11, 12) PVLM_DF_X(15, 16) PVLM_DF_X(14, 16) PVLM_DF_X(14, 15) PVLM_DF_X(18, 19) PVLM_DF_X(17, 19)
  PVLM_DF_X(17, 18) PVLM_DF_X(21, 22) PVLM_DF_X(20, 22) PVLM_DF_X(20, 21) PVLM_DF_X(23, 24) PVLM_DF_X(2, 5) PVLM_DF_X(3, 6) PVLM_DF_X(0, 6) PVLM_DF_X(0, 3)
  PVLM_DF_X(4, 7) PVLM_DF_X(1, 7) PVLM_DF_X(1, 4) PVLM_DF_X(11, 14) PVLM_DF_X(8, 14) PVLM_DF_X(8, 11) PVLM_DF_X(12, 15) PVLM_DF_X(9, 15) PVLM_DF_X(9, 12)
  PVLM_DF_X(13, 16) PVLM_DF_X(10, 16) PVLM_DF_X(10, 13) PVLM_DF_X(20, 23) PVLM_DF_X(17, 23) PVLM_DF_X(17, 20) PVLM_DF_X(21, 24) PVLM_DF_X(18, 24) PVLM_DF_X(18, 21)
  PVLM_DF_X(19, 22) PVLM_DF_X(8, 17) PVLM_DF_X(9, 18) PVLM_DF_X(0, 18) PVLM_DF_X(0, 9) PVLM_DF_X(10, 19) PVLM_DF_X(1, 19) PVLM_DF_X(1, 10) PVLM_DF_X(11, 20)
  PVLM_DF_X(2, 20) PVLM_DF_X(2, 11) PVLM_DF_X(12, 21) PVLM_DF_X(3, 21) PVLM_DF_X(3, 12) PVLM_DF_X(13, 22) PVLM_DF_X(4, 22) PVLM_DF_X(4, 13) PVLM_DF_X(14, 23)
  PVLM_DF_X(5, 23) PVLM_DF_X(5, 14) PVLM_DF_X(15, 24) PVLM_DF_X(6, 24) PVLM_DF_X(6, 15) PVLM_DF_X(7, 16) PVLM_DF_X(7, 19) PVLM_DF_X(13, 21) PVLM_DF_X(15, 23)
  PVLM_DF_X(7, 13) PVLM_DF_X(7, 15) PVLM_DF_X(1, 9) PVLM_DF_X(3, 11) PVLM_DF_X(5, 17) PVLM_DF_X(11, 17) PVLM_DF_X(9, 17) PVLM_DF_X(4, 10) PVLM_DF_X(6, 12)
  PVLM_DF_X(7, 14) PVLM_DF_X(4, 6) PVLM_DF_X(4, 7) PVLM_DF_X(12, 14) PVLM_DF_X(10, 14) PVLM_DF_X(6, 7) PVLM_DF_X(10, 12) PVLM_DF_X(6, 10) PVLM_DF_X(6, 17)
  PVLM_DF_X(12, 17) PVLM_DF_X(7, 17) PVLM_DF_X(7, 10) PVLM_DF_X(12, 18) PVLM_DF_X(7, 12) PVLM_DF_X(10, 18) PVLM_DF_X(12, 20) PVLM_DF_X(10, 20) PVLM_DF_X(10, 12)
  return p[12];
}
#undef PVLM_DF_X
// median5 of one pixel.  at(dr, dc): the tap with the border replicated
template <class A> PVLM_DF_HD float median5(const A& at) {
  float p[25];
#pragma unroll
  for (int dr = -2; dr <= 2; ++dr)
#pragma unroll
    for (int dc = -2; dc <= 2; ++dc) p[5 * (dr + 2) + dc + 2] = at(dr, dc);
  return median25(p);
}

PVLM_DF_HD int clampi(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }
PVLM_DF_HD int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

PVLM_DF_HD double exp_neg(double x) {
  if (x >= 708.0) return 0.0;
  const long long k = (long long)(x * 1.4426950408889634 + 0.5);
  const double kd = (double)k;
  const double r = (kd * 6.93147180369123816490e-01 - x) + kd * 1.90821492927058770002e-10;       // in [-ln2/2, ln2/2] up to rounding
  double p = 1.6059043836821613e-10;
  p = p * r + 2.08767569878681e-09;
  p = p * r + 2.505210838544172e-08;
  p = p * r + 2.755731922398589e-07;
  p = p * r + 2.7557319223985893e-06;
  p = p * r + 2.48015873015873e-05;
  p = p * r + 0.0001984126984126984;
  p = p * r + 0.001388888888888889;
  p = p * r + 0.008333333333333333;
  p = p * r + 0.041666666666666664;
  p = p * r + 0.16666666666666666;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const unsigned long long sb = (unsigned long long)(1023 - k) << 52;                               // k <= 1021: a normal number
  double s; __builtin_memcpy(&s, &sb, 8);
  return p * s;
}

// S7c of one pixel.  at(dy, dx): the tap with the border reflected (reflect101)
template <class A> PVLM_DF_HD float bilateral(const A& at) {
  const double c = (double)at(0, 0);
  double sw = 0.0, sv = 0.0;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int d2 = dy * dy + dx * dx;
      if (d2 > 4) continue;
      const double ws = d2 == 0 ? 1.0 : d2 == 1 ? 0.8824969025845955 : d2 == 2 ? 0.7788007830714049 : 0.6065306597126334;
      const double t = (double)at(dy, dx), dl = t - c;
      const double w = ws * exp_neg(2.0 * (dl * dl));
      sw = sw + w;
      sv = sv + w * t;
    }
  return (float)(sv / sw);
}

// rint(out * 256.f), half to even, saturated; out is finite and >= +0 (x + 2^23 - 2^23 rounds a float below 2^23 to the nearest integer, ties to even)
PVLM_DF_HD unsigned short to_u16(float out) {
  const float x = out * 256.f;
  if (!(x < 65535.f)) return (unsigned short)65535;
  const float r = (x + 8388608.f) - 8388608.f;
  return (unsigned short)(int)r;
}

#if !defined(__HIPCC__)
// ---- the whole-image host loop: the equality partner of the kernels and the timed baseline -------------------------------------------------------------
struct HostStats { long long valid_in = 0, valid_out = 0; };

inline void column_tops(int rows, int cols, const float* img, std::vector<int>& top) {
  top.assign((size_t)cols, 0);
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r) if (img[(size_t)r * cols + c] > kValid) { top[(size_t)c] = r; break; }
}

// d: rows x cols depths (an uint16 image already divided by 256); dense_or_null / u16_or_null: the two forms of the result
inline void complete_host(int rows, int cols, const float* d, float M, float* dense_or_null, unsigned short* u16_or_null, HostStats* stats_or_null = nullptr) {
  const size_t n = (size_t)rows * cols;
  std::vector<float> a(n), b(n), t(n);
  std::vector<int> top;
  const float inf = __builtin_inff();
  auto px = [&](const std::vector<float>& im, int r, int c, float outside) { return (r < 0 || r >= rows || c < 0 || c >= cols) ? outside : im[(size_t)r * cols + c]; };
  auto square = [&](const std::vector<float>& src, std::vector<float>& dst, int R, bool is_max) {     // dilate / erode by a (2 R + 1)^2 square: rows, then columns
    const float out = is_max ? -inf : inf;
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {
      float m = px(src, r, c - R, out);
      for (int k = -R + 1; k <= R; ++k) m = is_max ? max2(m, px(src, r, c + k, out)) : min2(m, px(src, r, c + k, out));
      t[(size_t)r * cols + c] = m;
    }
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {
      float m = px(t, r - R, c, out);
      for (int k = -R + 1; k <= R; ++k) m = is_max ? max2(m, px(t, r + k, c, out)) : min2(m, px(t, r + k, c, out));
      dst[(size_t)r * cols + c] = m;
    }
  };
  auto med = [&](const std::vector<float>& src, int r, int c) {
    return median5([&](int dr, int dc) { return src[(size_t)clampi(r + dr, rows) * cols + clampi(c + dc, cols)]; });
  };
  long long vin = 0, vout = 0;
  for (size_t i = 0; i < n; ++i) { a[i] = s0_of(d[i], M); vin += a[i] > kValid; }                    // S0
  for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c)                                       // S1, S2
    b[(size_t)r * cols + c] = s2_pixel([&](int dr, int dc) { return px(a, r + dr, c + dc, 0.f); }, M);
  square(b, a, 2, true);                                                                              // S3
  square(a, b, 2, false);
  for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {                                     // S4
    const float s3 = b[(size_t)r * cols + c];
    a[(size_t)r * cols + c] = sel(s3 > kValid, med(b, r, c), s3);
  }
  column_tops(rows, cols, a.data(), top);
  square(a, b, 4, true);                                                                              // S5
  for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {
    const size_t i = (size_t)r * cols + c;
    b[i] = sel(!(a[i] > kValid) && r >= top[(size_t)c], b[i], a[i]);
  }
  column_tops(rows, cols, b.data(), top);
  for (int round = 0; round < kFillRounds; ++round) {                                                 // S7a: b -> b
    square(b, a, 2, true);
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {
      const size_t i = (size_t)r * cols + c;
      b[i] = sel(b[i] < kValid && r >= top[(size_t)c], a[i], b[i]);
    }
  }
  for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {                                     // S7b: b -> a
    const size_t i = (size_t)r * cols + c;
    a[i] = sel(b[i] > kValid && r >= top[(size_t)c], med(b, r, c), b[i]);
  }
  for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {                                     // S7c, S8, u16
    const size_t i = (size_t)r * cols + c;
    const bool v = b[i] > kValid && r >= top[(size_t)c];
    float s7 = a[i];
    if (v) s7 = bilateral([&](int dy, int dx) { return a[(size_t)reflect101(r + dy, rows) * cols + reflect101(c + dx, cols)]; });
    const float out = invert(s7, M);
    vout += out > kValid;
    if (dense_or_null) dense_or_null[i] = out;
    if (u16_or_null) u16_or_null[i] = to_u16(out);
  }
  if (stats_or_null) { stats_or_null->valid_in = vin; stats_or_null->valid_out = vout; }
}

// ProjectLidar2PanoramaDepth (util/Visualization.h:407-441) on the host, statement by statement what k_depth_splat (csrc/pvlm_lines.hip) computes per point: the
// points painted in cloud order, so that the last point that covers a pixel wins.  img: rows x cols, zeroed by the caller.
inline void splat_host(int rows, int cols, long long n, const float* xyz, const double* T_cl, unsigned size, unsigned short* img) {
  const int half = (int)(size / 2);
  for (long long i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    float p[3];
    for (int r = 0; r < 3; ++r) p[r] = (float)(T_cl[4 * r] * (double)x + T_cl[4 * r + 1] * (double)y + T_cl[4 * r + 2] * (double)z + T_cl[4 * r + 3]);
    const float lon = pvlm_equirect::fast_atan2<float>(p[0], p[2]);
    const float lat = -pvlm_equirect::fast_atan2<float>(p[1], pvlm_exact::sqrt_via_double(p[0] * p[0] + p[2] * p[2]));
    const float px = (float)(cols * (0.5 + pvlm_exact::div_two_pi(lon)));
    const float py = (float)(rows * (0.5 - pvlm_exact::div_pi(lat)));
    const int rbx = (int)(ceilf(px) + (float)half), rby = (int)(ceilf(py) + (float)half);
    const int ltx = (int)(floorf(px) - (float)half), lty = (int)(floorf(py) - (float)half);
    if (!(rbx >= 0 && rby >= 0 && rbx + 1 <= cols && rby + 1 <= rows)) continue;
    if (!(ltx >= 0 && lty >= 0 && ltx + 1 <= cols && lty + 1 <= rows)) continue;
    const float depth = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const unsigned short rel = (unsigned short)(unsigned int)((double)depth * 256.0);
    for (int u = lty; u <= rby; ++u)
      for (int v = ltx; v <= rbx; ++v) img[(size_t)u * cols + v] = rel;
  }
}

// a batch of equal-sized images, the images spread over n_threads workers
inline void complete_host_batch(int rows, int cols, int n_images, const unsigned short* in_u16_or_null, const float* in_f32_or_null, float M, float* dense_or_null,
                                unsigned short* u16_or_null, size_t n_threads, HostStats* stats_or_null = nullptr) {
  const size_t n = (size_t)rows * cols;
  std::atomic<int> next{0};
  std::atomic<long long> vin{0}, vout{0};
  pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads, (size_t)std::max(n_images, 1))), [&]() {
    std::vector<float> tmp;
    for (int k = next.fetch_add(1); k < n_images; k = next.fetch_add(1)) {
      const float* d = in_f32_or_null ? in_f32_or_null + k * n : nullptr;
      if (!d) { tmp.resize(n); for (size_t i = 0; i < n; ++i) tmp[i] = from_u16(in_u16_or_null[k * n + i]); d = tmp.data(); }
      HostStats s;
      complete_host(rows, cols, d, M, dense_or_null ? dense_or_null + k * n : nullptr, u16_or_null ? u16_or_null + k * n : nullptr, &s);
      vin += s.valid_in; vout += s.valid_out;
    }
  });
  if (stats_or_null) { stats_or_null->valid_in = vin.load(); stats_or_null->valid_out = vout.load(); }
}

// the loop body of SfM::ComputeDepthImage for every scan on the host: splat_host, complete_host, x 256, uint16; the scans spread over n_threads workers
inline void depth_images_host(int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl, unsigned size, float M,
                              unsigned short* depth_u16, size_t n_threads) {
  const size_t n = (size_t)rows * cols;
  std::atomic<int> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads, (size_t)std::max(n_scans, 1))), [&]() {
    std::vector<unsigned short> sparse(n);
    std::vector<float> d(n);
    for (int k = next.fetch_add(1); k < n_scans; k = next.fetch_add(1)) {
      std::fill(sparse.begin(), sparse.end(), (unsigned short)0);
      splat_host(rows, cols, first_point[k + 1] - first_point[k], xyz + 3 * (size_t)first_point[k], T_cl, size, sparse.data());
      for (size_t i = 0; i < n; ++i) d[i] = from_u16(sparse[i]);
      complete_host(rows, cols, d.data(), M, nullptr, depth_u16 + k * n);
    }
  });
}
#endif

}  // namespace pvlm_depthfill
