// Statement of K41: SIFT keypoints and (Root)SIFT descriptors as upstream takes them (util/SIFT.cpp:10-128: cv::xfeatures2d::SIFT::create(nfeatures), detect with a
// mask, compute; RootSIFT :10-21).  Host / device: csrc/pvlm_sift.hip wraps the per-pixel, per-candidate and per-keypoint functions below in kernels; the whole-image
// host loop at the end of this file (extract_host: ExtractSIFTHost and tests/cpp/sift_core_check.cpp) is what the CPU tests compare with numpy and the GPU tests
// compare with bit for bit.  Compile with -ffp-contract=off.  The full text of the definition, with what is [recalled] from OpenCV and the deliberate divergences,
// is the K41 comment of include/pvlm.h; this header keeps the operation orders.
//
// Everything is fp32 in the written order unless a double is named.  rint(x) is round-half-to-even (cvRound).
//   blur      dst(y, x) = column pass over row pass; a pass is s = 0, then s = s + c[k] * src(reflect101(p + k - taps / 2)) for k = 0 .. taps - 1 ascending
//   doubled   (d + 0.5) / 2 - 0.5 with a replicated border: weights 0.75 / 0.25, exact in fp32 for 8-bit input
//   atan2_deg octant reduction, a = min / max, a degree-11 odd polynomial in Horner order, the octant folded back, * 180 / pi; in [0, 360]
//   exp       (float)pvlm_depthfill::exp_neg((double)x) for x >= 0 (K37's e^-x)
//   sincos    of degrees, in double: the quadrant split off, Taylor series of sin and cos to x^23 / x^22 in Horner order
//   2^t       (float)(4 * exp_neg((2 - t) ln 2)) for t < 2
// Orientation and descriptor histograms are summed in a wave's shape so that 64 lanes can do it: sample j of the window (row-major, the skipped ones counted)
// belongs to lane j % 64; a lane adds its samples in ascending j into its own bins; a bin's total is the sum of the 64 lanes' values in ascending lane order.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <vector>

#include "pvlm_depthfill_core.h"

#if defined(__HIPCC__)
#define PVLM_SIFT_HD __host__ __device__ inline
#else
#define PVLM_SIFT_HD inline
#endif

namespace pvlm_sift {

constexpr int kLayers = 3, kGauss = kLayers + 3, kDog = kLayers + 2, kBorder = 5, kMaxTaps = 27, kMaxRadius = kMaxTaps / 2;
constexpr int kOriBins = 36, kMaxPeaks = 18, kLanes = 64, kDescBins = 128, kMaxSteps = 5, kMinSide = 8, kMaxOctaves = 24;
constexpr double kSigma = 1.6, kK = 1.2599210498948732;            // 2^(1/3) as a literal
constexpr float kContrast = 0.04f, kEdge = 10.f, kDetectThr = 1.f;   // floor(0.5 * 0.04 / 3 * 255) = 1
constexpr float kFltEps = 1.1920929e-07f;
enum { kKeep = 0, kRejectMoves = 1, kRejectContrast = 2, kRejectEdge = 3 };

struct Kernel { int taps; float c[kMaxTaps]; };
struct Keypoint { float x, y, size, angle, response; int octave; };          // pvlm_sift_keypoint
struct Cand { int octave, layer, r, c; float x, y, size, response; int word, det_layer, det_r, det_c; };   // a refined extremum, in its octave's pixels

PVLM_SIFT_HD int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}
PVLM_SIFT_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
PVLM_SIFT_HD float absf(float v) { return v < 0.f ? -v : v; }
// round half to even for |x| < 2^22
PVLM_SIFT_HD float rintf_even(float x) { const float a = (absf(x) + 8388608.f) - 8388608.f; return x < 0.f ? -a : a; }
PVLM_SIFT_HD float floorf_small(float x) { const float t = (float)(int)x; return t > x ? t - 1.f : t; }

// pixel (y, x) of the doubled image (2 rows x 2 cols)
PVLM_SIFT_HD float doubled_at(const unsigned char* img, int rows, int cols, int y, int x) {
  const int y0 = (y >> 1) - ((y & 1) ? 0 : 1), x0 = (x >> 1) - ((x & 1) ? 0 : 1);
  const float fy = (y & 1) ? 0.25f : 0.75f, fx = (x & 1) ? 0.25f : 0.75f;
  const int ya = clampi(y0, 0, rows - 1), yb = clampi(y0 + 1, 0, rows - 1), xa = clampi(x0, 0, cols - 1), xb = clampi(x0 + 1, 0, cols - 1);
  const float top = (float)img[(size_t)ya * cols + xa] * (1.f - fx) + (float)img[(size_t)ya * cols + xb] * fx;
  const float bot = (float)img[(size_t)yb * cols + xa] * (1.f - fx) + (float)img[(size_t)yb * cols + xb] * fx;
  return top * (1.f - fy) + bot * fy;
}

// one pass of the blur at position p of a line: at(q) is the line's value at an index already folded into the image
template <class A> PVLM_SIFT_HD float blur_tap_sum(const Kernel& K, const A& at, int p, int n) {
  const int r = K.taps / 2;
  float s = 0.f;
  for (int k = 0; k < K.taps; ++k) s = s + K.c[k] * at(reflect101(p + k - r, n));
  return s;
}

PVLM_SIFT_HD int octave_count(int base_rows, int base_cols) {
  const long long m = base_rows < base_cols ? base_rows : base_cols;
  int e = 0;
  while ((2ll << e) <= m) ++e;                                   // 2^e <= m < 2^(e + 1)
  const int lg = e + ((m * m >= (2ll << (2 * e))) ? 1 : 0);      // round(log2 m): up when m >= 2^(e + 0.5)
  const int n = lg - 2 + 1;
  return n < 1 ? 1 : n > kMaxOctaves ? kMaxOctaves : n;
}

PVLM_SIFT_HD float atan2_deg(float y, float x) {
  const float ax = absf(x), ay = absf(y);
  const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  if (mx == 0.f) return 0.f;
  const float a = mn / mx, s = a * a;
  float p = -0.01172120f;
  p = p * s + 0.05265332f;
  p = p * s + -0.11643287f;
  p = p * s + 0.19354346f;
  p = p * s + -0.33262347f;
  p = p * s + 0.99997726f;
  float r = p * a;
  if (ay > ax) r = 1.57079637f - r;
  if (x < 0.f) r = 3.14159274f - r;
  if (y < 0.f) r = 6.28318548f - r;
  return r * 57.2957802f;
}

PVLM_SIFT_HD float exp_neg_f(float x) { return (float)pvlm_depthfill::exp_neg((double)x); }
PVLM_SIFT_HD float pow2_f(float t) { return (float)(4.0 * pvlm_depthfill::exp_neg((2.0 - (double)t) * 0.6931471805599453)); }

// sin and cos of an angle in degrees, deg in [0, 360]
PVLM_SIFT_HD void sincos_deg(float deg, double* sn, double* cs) {
  const double a = (double)deg;
  int q = (int)(a / 90.0);
  if (q > 3) q = 3;
  const double x = (a - 90.0 * (double)q) * 0.017453292519943295, x2 = x * x;
  double s = -3.8681701706306835e-23;      // -1 / 23!
  s = s * x2 + 1.9572941063391263e-20;     //  1 / 21!
  s = s * x2 + -8.22063524662433e-18;      // -1 / 19!
  s = s * x2 + 2.8114572543455206e-15;     //  1 / 17!
  s = s * x2 + -7.647163731819816e-13;     // -1 / 15!
  s = s * x2 + 1.6059043836821613e-10;     //  1 / 13!
  s = s * x2 + -2.505210838544172e-08;     // -1 / 11!
  s = s * x2 + 2.7557319223985893e-06;     //  1 / 9!
  s = s * x2 + -0.0001984126984126984;     // -1 / 7!
  s = s * x2 + 0.008333333333333333;       //  1 / 5!
  s = s * x2 + -0.16666666666666666;       // -1 / 3!
  s = s * x2 + 1.0;
  s = s * x;
  double c = -8.896791392450574e-22;       // -1 / 22!
  c = c * x2 + 4.110317623312165e-19;      //  1 / 20!
  c = c * x2 + -1.5619206968586225e-16;    // -1 / 18!
  c = c * x2 + 4.779477332387385e-14;      //  1 / 16!
  c = c * x2 + -1.1470745597729725e-11;    // -1 / 14!
  c = c * x2 + 2.08767569878681e-09;       //  1 / 12!
  c = c * x2 + -2.755731922398589e-07;     // -1 / 10!
  c = c * x2 + 2.48015873015873e-05;       //  1 / 8!
  c = c * x2 + -0.001388888888888889;      // -1 / 6!
  c = c * x2 + 0.041666666666666664;       //  1 / 4!
  c = c * x2 + -0.5;                       // -1 / 2!
  c = c * x2 + 1.0;
  *sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  *cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// ---- extrema ------------------------------------------------------------------------------------------------------------------------------------------------
// D: the five difference layers of an octave, rows x cols each.  (layer, r, c): 1 <= layer <= 3, kBorder <= r < rows - kBorder, kBorder <= c < cols - kBorder.
PVLM_SIFT_HD bool is_extremum(const float* const* D, int cols, int layer, int r, int c) {
  const float* cur = D[layer]; const float* prv = D[layer - 1]; const float* nxt = D[layer + 1];
  const float v = cur[(size_t)r * cols + c];
  if (!(absf(v) > kDetectThr)) return false;
  bool ge = true, le = true;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const size_t o = (size_t)(r + dy) * cols + (c + dx);
      const float a = prv[o], b = cur[o], d = nxt[o];
      ge = ge && v >= a && v >= b && v >= d;
      le = le && v <= a && v <= b && v <= d;
    }
  return v > 0.f ? ge : le;
}

// the Newton steps, the contrast and the edge test of a detected extremum; *moved: the position changed at least once.  Returns kKeep or the rule that rejected.
PVLM_SIFT_HD int refine(const float* const* D, int rows, int cols, int octave, int layer, int r, int c, Cand* out, int* moved) {
  const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
  const int det_layer = layer, det_r = r, det_c = c;
  float xi = 0.f, xr = 0.f, xc = 0.f;
  int step = 0;
  *moved = 0;
  for (; step < kMaxSteps; ++step) {
    const float* img = D[layer]; const float* prv = D[layer - 1]; const float* nxt = D[layer + 1];
    const size_t o = (size_t)r * cols + c;
    const float g0 = (img[o + 1] - img[o - 1]) * deriv_scale, g1 = (img[o + cols] - img[o - cols]) * deriv_scale, g2 = (nxt[o] - prv[o]) * deriv_scale;
    const float v2 = img[o] * 2.f;
    const float dxx = (img[o + 1] + img[o - 1] - v2) * second_scale, dyy = (img[o + cols] + img[o - cols] - v2) * second_scale, dss = (nxt[o] + prv[o] - v2) * second_scale;
    const float dxy = (img[o + cols + 1] - img[o + cols - 1] - img[o - cols + 1] + img[o - cols - 1]) * cross_scale;
    const float dxs = (nxt[o + 1] - nxt[o - 1] - prv[o + 1] + prv[o - 1]) * cross_scale;
    const float dys = (nxt[o + cols] - nxt[o - cols] - prv[o + cols] + prv[o - cols]) * cross_scale;
    // H X = g by cofactors, H symmetric
    const float c00 = dyy * dss - dys * dys, c01 = dxs * dys - dxy * dss, c02 = dxy * dys - dxs * dyy;
    const float c11 = dxx * dss - dxs * dxs, c12 = dxs * dxy - dxx * dys, c22 = dxx * dyy - dxy * dxy;
    const float det = dxx * c00 + dxy * c01 + dxs * c02;
    if (det == 0.f) return kRejectMoves;
    const float inv = 1.f / det;
    const float X0 = (c00 * g0 + c01 * g1 + c02 * g2) * inv, X1 = (c01 * g0 + c11 * g1 + c12 * g2) * inv, X2 = (c02 * g0 + c12 * g1 + c22 * g2) * inv;
    xc = -X0; xr = -X1; xi = -X2;
    if (absf(xi) < 0.5f && absf(xr) < 0.5f && absf(xc) < 0.5f) break;
    if (!(absf(xi) < 1e6f) || !(absf(xr) < 1e6f) || !(absf(xc) < 1e6f)) return kRejectMoves;
    c += (int)rintf_even(xc); r += (int)rintf_even(xr); layer += (int)rintf_even(xi);
    *moved = 1;
    if (layer < 1 || layer > kLayers || c < kBorder || c >= cols - kBorder || r < kBorder || r >= rows - kBorder) return kRejectMoves;
  }
  if (step >= kMaxSteps) return kRejectMoves;
  {
    const float* img = D[layer]; const float* prv = D[layer - 1]; const float* nxt = D[layer + 1];
    const size_t o = (size_t)r * cols + c;
    const float g0 = (img[o + 1] - img[o - 1]) * deriv_scale, g1 = (img[o + cols] - img[o - cols]) * deriv_scale, g2 = (nxt[o] - prv[o]) * deriv_scale;
    const float t = g0 * xc + g1 * xr + g2 * xi;
    const float contr = img[o] * img_scale + t * 0.5f;
    if (absf(contr) * (float)kLayers < kContrast) return kRejectContrast;
    const float v2 = img[o] * 2.f;
    const float dxx = (img[o + 1] + img[o - 1] - v2) * second_scale, dyy = (img[o + cols] + img[o - cols] - v2) * second_scale;
    const float dxy = (img[o + cols + 1] - img[o + cols - 1] - img[o - cols + 1] + img[o - cols - 1]) * cross_scale;
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.f || tr * tr * kEdge >= (kEdge + 1.f) * (kEdge + 1.f) * det) return kRejectEdge;
    const float oct_scale = (float)(1 << octave);
    out->octave = octave; out->layer = layer; out->r = r; out->c = c;
    out->x = ((float)c + xc) * oct_scale; out->y = ((float)r + xr) * oct_scale;
    out->size = (float)kSigma * pow2_f(((float)layer + xi) / (float)kLayers) * oct_scale * 2.f;
    out->response = absf(contr);
    out->word = octave + (layer << 8) + ((int)rintf_even((xi + 0.5f) * 255.f) << 16);
    out->det_layer = det_layer; out->det_r = det_r; out->det_c = det_c;
  }
  return kKeep;
}

// ---- orientation --------------------------------------------------------------------------------------------------------------------------------------------
struct OriWindow { int r0, c0, radius, side, count; float inv2s2; };
PVLM_SIFT_HD OriWindow ori_window(const Cand& k) {
  OriWindow w;
  const float scl = k.size * 0.5f / (float)(1 << k.octave);
  w.r0 = k.r; w.c0 = k.c;
  w.radius = (int)rintf_even(3.f * 1.5f * scl);
  w.side = 2 * w.radius + 1; w.count = w.side * w.side;
  const float sg = 1.5f * scl;
  w.inv2s2 = 1.f / (2.f * (sg * sg));
  return w;
}
// sample j of the window on Gaussian layer G: false when the pixel is skipped
PVLM_SIFT_HD bool ori_sample(const float* G, int rows, int cols, const OriWindow& w, int j, int* bin, float* val) {
  const int i = j / w.side - w.radius, jj = j % w.side - w.radius;
  const int y = w.r0 + i, x = w.c0 + jj;
  if (y <= 0 || y >= rows - 1 || x <= 0 || x >= cols - 1) return false;
  const size_t o = (size_t)y * cols + x;
  const float dx = G[o + 1] - G[o - 1], dy = G[o - cols] - G[o + cols];
  const float wgt = exp_neg_f((float)(i * i + jj * jj) * w.inv2s2);
  const float mag = sqrtf(dx * dx + dy * dy);
  int b = (int)rintf_even((float)kOriBins / 360.f * atan2_deg(dy, dx));
  if (b >= kOriBins) b -= kOriBins;
  if (b < 0) b += kOriBins;
  *bin = b; *val = wgt * mag;
  return true;
}
// the raw histogram -> the keypoint angles (at most kMaxPeaks), ascending bin
PVLM_SIFT_HD int ori_peaks(const float* raw, float* angles) {
  float h[kOriBins];
  float mx = 0.f;
  for (int i = 0; i < kOriBins; ++i) {
    const float m2 = raw[(i + kOriBins - 2) % kOriBins], m1 = raw[(i + kOriBins - 1) % kOriBins], p1 = raw[(i + 1) % kOriBins], p2 = raw[(i + 2) % kOriBins];
    h[i] = (m2 + p2) * (1.f / 16.f) + (m1 + p1) * (4.f / 16.f) + raw[i] * (6.f / 16.f);
    if (i == 0 || h[i] > mx) mx = h[i];
  }
  const float thr = mx * 0.8f;
  int n = 0;
  for (int j = 0; j < kOriBins; ++j) {
    const float l = h[(j + kOriBins - 1) % kOriBins], r = h[(j + 1) % kOriBins];
    if (h[j] > l && h[j] > r && h[j] >= thr && n < kMaxPeaks) {
      float bin = (float)j + 0.5f * (l - r) / (l - 2.f * h[j] + r);
      bin = bin < 0.f ? (float)kOriBins + bin : bin >= (float)kOriBins ? bin - (float)kOriBins : bin;
      float ang = 360.f - (360.f / (float)kOriBins) * bin;
      if (absf(ang - 360.f) < kFltEps) ang = 0.f;
      angles[n++] = ang;
    }
  }
  return n;
}

// ---- descriptor ---------------------------------------------------------------------------------------------------------------------------------------------
struct DescWindow { int octave_index, layer, r0, c0, radius, side, count; float ori, cos_t, sin_t; };
// from a finished keypoint (first octave -1 applied): the layer it reads and the rotated window
PVLM_SIFT_HD DescWindow desc_window(const Keypoint& k, int rows, int cols /* of the layer */) {
  DescWindow w;
  int oc = k.octave & 255;
  w.layer = (k.octave >> 8) & 255;
  oc = oc < 128 ? oc : (-128 | oc);
  const float scale = oc >= 0 ? 1.f / (float)(1 << oc) : (float)(1 << -oc);
  w.octave_index = oc + 1;
  const float size = k.size * scale, px = k.x * scale, py = k.y * scale;
  float ang = 360.f - k.angle;
  if (absf(ang - 360.f) < kFltEps) ang = 0.f;
  w.ori = ang;
  w.c0 = (int)rintf_even(px); w.r0 = (int)rintf_even(py);
  double sn, cs;
  sincos_deg(ang, &sn, &cs);
  const float hist_width = 3.f * (size * 0.5f);
  int radius = (int)rintf_even(hist_width * 1.4142135623730951f * 5.f * 0.5f);
  const int diag = (int)sqrt((double)cols * (double)cols + (double)rows * (double)rows);
  w.radius = radius < diag ? radius : diag;
  w.side = 2 * w.radius + 1; w.count = w.side * w.side;
  w.cos_t = (float)cs / hist_width; w.sin_t = (float)sn / hist_width;
  return w;
}
// sample j: up to 8 (bin, value) contributions; returns how many (0 when skipped)
PVLM_SIFT_HD int desc_sample(const float* G, int rows, int cols, const DescWindow& w, int j, int* bins, float* vals) {
  const int i = j / w.side - w.radius, jj = j % w.side - w.radius;
  const float c_rot = (float)jj * w.cos_t - (float)i * w.sin_t, r_rot = (float)jj * w.sin_t + (float)i * w.cos_t;
  float rbin = r_rot + 2.f - 0.5f, cbin = c_rot + 2.f - 0.5f;
  const int r = w.r0 + i, c = w.c0 + jj;
  if (!(rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && r > 0 && r < rows - 1 && c > 0 && c < cols - 1)) return 0;
  const size_t o = (size_t)r * cols + c;
  const float dx = G[o + 1] - G[o - 1], dy = G[o - cols] - G[o + cols];
  const float wgt = exp_neg_f((c_rot * c_rot + r_rot * r_rot) * (1.f / 8.f));
  const float mag = sqrtf(dx * dx + dy * dy) * wgt;
  float obin = (atan2_deg(dy, dx) - w.ori) * (8.f / 360.f);
  const float r0f = floorf_small(rbin), c0f = floorf_small(cbin), o0f = floorf_small(obin);
  rbin -= r0f; cbin -= c0f; obin -= o0f;
  const int r0 = (int)r0f, c0 = (int)c0f;
  int o0 = (int)o0f;
  if (o0 < 0) o0 += 8;
  if (o0 >= 8) o0 -= 8;
  const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
  const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
  const float v111 = v_rc11 * obin, v110 = v_rc11 - v111, v101 = v_rc10 * obin, v100 = v_rc10 - v101;
  const float v011 = v_rc01 * obin, v010 = v_rc01 - v011, v001 = v_rc00 * obin, v000 = v_rc00 - v001;
  const float v[8] = {v000, v001, v010, v011, v100, v101, v110, v111};
  const int o1 = (o0 + 1) & 7;
  int n = 0;
  for (int k = 0; k < 8; ++k) {                       // k = 4 dr + 2 dc + do
    const int rr = r0 + (k >> 2), cc = c0 + ((k >> 1) & 1);
    if (rr < 0 || rr > 3 || cc < 0 || cc > 3) continue;
    bins[n] = (rr * 4 + cc) * 8 + ((k & 1) ? o1 : o0); vals[n] = v[k]; ++n;
  }
  return n;
}
// the 128 sums -> the stored row
PVLM_SIFT_HD void desc_finish(const float* hist, bool root, float* out) {
  float n2 = 0.f;
  for (int k = 0; k < kDescBins; ++k) n2 = n2 + hist[k] * hist[k];
  const float thr = sqrtf(n2) * 0.2f;
  n2 = 0.f;
  for (int k = 0; k < kDescBins; ++k) { const float v = hist[k] < thr ? hist[k] : thr; n2 = n2 + v * v; }
  const float nr = sqrtf(n2);
  const float f = 512.f / (nr > kFltEps ? nr : kFltEps);
  float l1 = 0.f;
  for (int k = 0; k < kDescBins; ++k) {
    const float v = (hist[k] < thr ? hist[k] : thr) * f;
    const float q = !(v > 0.f) ? 0.f : v >= 255.f ? 255.f : rintf_even(v);
    out[k] = q; l1 = l1 + q;
  }
  if (!root || l1 == 0.f) return;                      // a zero row stays zero
  for (int k = 0; k < kDescBins; ++k) out[k] = sqrtf(out[k] / l1) * 512.f;
}

// ---- host side of both compiles: kernels, sizes, selection ----------------------------------------------------------------------------------------------------
// kernel 0: the base blur; kernel i >= 1: layer i from layer i - 1
inline void make_kernels(Kernel* K) {
  double sig[kGauss];
  sig[0] = std::sqrt(std::max(kSigma * kSigma - 1.0, 0.01));
  double prev = kSigma;
  for (int i = 1; i < kGauss; ++i) { const double tot = prev * kK; sig[i] = std::sqrt(tot * tot - prev * prev); prev = tot; }
  for (int i = 0; i < kGauss; ++i) {
    const int taps = (int)std::floor(8.0 * sig[i] + 1.0 + 0.5) | 1;
    const int r = taps / 2;
    double e[kMaxTaps], sum = 0.0;
    for (int k = 0; k < taps; ++k) { const double x = (double)(k - r); e[k] = pvlm_depthfill::exp_neg(x * x / (2.0 * sig[i] * sig[i])); sum = sum + e[k]; }
    K[i].taps = taps;
    for (int k = 0; k < kMaxTaps; ++k) K[i].c[k] = k < taps ? (float)(e[k] / sum) : 0.f;
  }
}

struct Sizes { int n_oct; int rows[kMaxOctaves], cols[kMaxOctaves]; };
inline Sizes octave_sizes(int rows, int cols) {
  Sizes s;
  s.n_oct = octave_count(2 * rows, 2 * cols);
  int r = 2 * rows, c = 2 * cols;
  for (int o = 0; o < s.n_oct; ++o) { s.rows[o] = r; s.cols[o] = c; r /= 2; c /= 2; if (r < 1 || c < 1) { s.n_oct = o + 1; break; } }
  return s;
}

// duplicates, retainBest, first octave -1, mask: a stable filter of `kps`
inline void select(std::vector<Keypoint>& kps, int nfeatures, int rows, int cols, const unsigned char* mask) {
  const size_t n = kps.size();
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = i;
  auto less4 = [&](size_t a, size_t b) {
    const Keypoint &p = kps[a], &q = kps[b];
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    if (p.size != q.size) return p.size < q.size;
    return p.angle < q.angle;
  };
  std::stable_sort(idx.begin(), idx.end(), less4);
  std::vector<unsigned char> keep(n, 1);
  for (size_t i = 1; i < n; ++i) if (!less4(idx[i - 1], idx[i])) keep[idx[i]] = 0;          // equal to its predecessor: the first in order stays
  std::vector<Keypoint> a;
  for (size_t i = 0; i < n; ++i) if (keep[i]) a.push_back(kps[i]);
  if ((size_t)nfeatures < a.size()) {
    std::vector<float> resp(a.size());
    for (size_t i = 0; i < a.size(); ++i) resp[i] = a[i].response;
    std::nth_element(resp.begin(), resp.begin() + (nfeatures - 1), resp.end(), [](float p, float q) { return p > q; });
    const float thr = resp[(size_t)nfeatures - 1];
    std::vector<Keypoint> b;
    for (const Keypoint& k : a) if (k.response >= thr) b.push_back(k);
    a.swap(b);
  }
  kps.clear();
  for (Keypoint k : a) {
    k.octave = (k.octave & ~255) | ((k.octave - 1) & 255);
    k.x *= 0.5f; k.y *= 0.5f; k.size *= 0.5f;
    if (mask) {
      const int my = clampi((int)rintf_even(k.y), 0, rows - 1), mx = clampi((int)rintf_even(k.x), 0, cols - 1);
      if (mask[(size_t)my * cols + mx] == 0) continue;
    }
    kps.push_back(k);
  }
}

inline Keypoint keypoint_of(const Cand& c, float angle) { return Keypoint{c.x, c.y, c.size, angle, c.response, c.word}; }

#if !defined(__HIPCC__)
// ---- the whole-image host loop: the equality partner of the kernels and the timed baseline -------------------------------------------------------------------
struct Pyramid {
  Sizes sz;
  std::vector<std::vector<float>> G, D;               // n_oct * kGauss, n_oct * kDog
  const float* g(int o, int l) const { return G[(size_t)o * kGauss + l].data(); }
  const float* d(int o, int l) const { return D[(size_t)o * kDog + l].data(); }
};
struct Counters { long long extrema = 0, moved = 0, reject_moves = 0, reject_contrast = 0, reject_edge = 0, candidates = 0, multi_peak = 0, keypoints = 0; };

template <class Src> inline void blur_host(const Src& src, int rows, int cols, const Kernel& K, std::vector<float>& tmp, float* dst, size_t threads) {
  tmp.resize((size_t)rows * cols);
  std::atomic<int> next{0};
  pvlm_run_workers(threads, [&]() {
    for (int y = next++; y < rows; y = next++)
      for (int x = 0; x < cols; ++x) tmp[(size_t)y * cols + x] = blur_tap_sum(K, [&](int q) { return src(y, q); }, x, cols);
  });
  next = 0;
  pvlm_run_workers(threads, [&]() {
    for (int y = next++; y < rows; y = next++)
      for (int x = 0; x < cols; ++x) dst[(size_t)y * cols + x] = blur_tap_sum(K, [&](int q) { return tmp[(size_t)q * cols + x]; }, y, rows);
  });
}

inline void build_pyramid(const unsigned char* img, int rows, int cols, Pyramid& P, size_t threads = 1) {
  Kernel K[kGauss];
  make_kernels(K);
  P.sz = octave_sizes(rows, cols);
  P.G.assign((size_t)P.sz.n_oct * kGauss, {}); P.D.assign((size_t)P.sz.n_oct * kDog, {});
  std::vector<float> tmp;
  for (int o = 0; o < P.sz.n_oct; ++o) {
    const int R = P.sz.rows[o], Cc = P.sz.cols[o];
    for (int l = 0; l < kGauss; ++l) P.G[(size_t)o * kGauss + l].resize((size_t)R * Cc);
    for (int l = 0; l < kDog; ++l) P.D[(size_t)o * kDog + l].resize((size_t)R * Cc);
    float* g0 = P.G[(size_t)o * kGauss].data();
    if (o == 0) {
      blur_host([&](int y, int x) { return doubled_at(img, rows, cols, y, x); }, R, Cc, K[0], tmp, g0, threads);
    } else {
      const float* up = P.g(o - 1, kLayers); const int uc = P.sz.cols[o - 1];
      for (int y = 0; y < R; ++y) for (int x = 0; x < Cc; ++x) g0[(size_t)y * Cc + x] = up[(size_t)(2 * y) * uc + 2 * x];
    }
    for (int l = 1; l < kGauss; ++l) {
      const float* a = P.g(o, l - 1);
      float* b = P.G[(size_t)o * kGauss + l].data();
      blur_host([&](int y, int x) { return a[(size_t)y * Cc + x]; }, R, Cc, K[l], tmp, b, threads);
      float* d = P.D[(size_t)o * kDog + l - 1].data();
      for (size_t i = 0; i < (size_t)R * Cc; ++i) d[i] = b[i] - a[i];
    }
  }
}

inline int orientation_host(const float* G, int rows, int cols, const Cand& k, float* angles) {
  const OriWindow w = ori_window(k);
  static thread_local float part[kLanes][kOriBins];
  std::memset(part, 0, sizeof(part));
  for (int lane = 0; lane < kLanes; ++lane)
    for (int j = lane; j < w.count; j += kLanes) { int b; float v; if (ori_sample(G, rows, cols, w, j, &b, &v)) part[lane][b] = part[lane][b] + v; }
  float raw[kOriBins];
  for (int b = 0; b < kOriBins; ++b) { float s = 0.f; for (int lane = 0; lane < kLanes; ++lane) s = s + part[lane][b]; raw[b] = s; }
  return ori_peaks(raw, angles);
}

inline void descriptor_host(const float* G, int rows, int cols, const Keypoint& k, bool root, float* out) {
  const DescWindow w = desc_window(k, rows, cols);
  static thread_local float part[kLanes][kDescBins];
  std::memset(part, 0, sizeof(part));
  for (int lane = 0; lane < kLanes; ++lane)
    for (int j = lane; j < w.count; j += kLanes) {
      int b[8]; float v[8];
      const int n = desc_sample(G, rows, cols, w, j, b, v);
      for (int q = 0; q < n; ++q) part[lane][b[q]] = part[lane][b[q]] + v[q];
    }
  float hist[kDescBins];
  for (int b = 0; b < kDescBins; ++b) { float s = 0.f; for (int lane = 0; lane < kLanes; ++lane) s = s + part[lane][b]; hist[b] = s; }
  desc_finish(hist, root, out);
}

// candidates in (octave, layer, row, column) order of the detection and their keypoints (ascending bin) before the selection
inline void detect_host(const Pyramid& P, std::vector<Cand>& cands, std::vector<Keypoint>& kps, Counters* ct, size_t threads = 1) {
  struct Row { std::vector<Cand> cands; std::vector<Keypoint> kps; Counters ct; };
  for (int o = 0; o < P.sz.n_oct; ++o) {
    const int R = P.sz.rows[o], Cc = P.sz.cols[o];
    if (R <= 2 * kBorder || Cc <= 2 * kBorder) continue;
    const float* D[kDog];
    for (int l = 0; l < kDog; ++l) D[l] = P.d(o, l);
    for (int l = 1; l <= kLayers; ++l) {
      std::vector<Row> rows((size_t)(R - 2 * kBorder));                  // the rows are independent; their results are joined in row order
      std::atomic<int> next{kBorder};
      pvlm_run_workers(std::max<size_t>(1, threads), [&]() {
        for (int r = next++; r < R - kBorder; r = next++) {
          Row& out = rows[(size_t)(r - kBorder)];
          for (int c = kBorder; c < Cc - kBorder; ++c) {
            if (!is_extremum(D, Cc, l, r, c)) continue;
            Cand k; int moved;
            const int code = refine(D, R, Cc, o, l, r, c, &k, &moved);
            out.ct.extrema++; out.ct.moved += moved; out.ct.reject_moves += code == kRejectMoves; out.ct.reject_contrast += code == kRejectContrast;
            out.ct.reject_edge += code == kRejectEdge;
            if (code != kKeep) continue;
            float ang[kMaxPeaks];
            const int n = orientation_host(P.g(o, k.layer), R, Cc, k, ang);
            out.cands.push_back(k);
            for (int q = 0; q < n; ++q) out.kps.push_back(keypoint_of(k, ang[q]));
            out.ct.candidates++; out.ct.multi_peak += n > 1; out.ct.keypoints += n;
          }
        }
      });
      for (const Row& row : rows) {
        cands.insert(cands.end(), row.cands.begin(), row.cands.end());
        kps.insert(kps.end(), row.kps.begin(), row.kps.end());
        if (ct) {
          ct->extrema += row.ct.extrema; ct->moved += row.ct.moved; ct->reject_moves += row.ct.reject_moves; ct->reject_contrast += row.ct.reject_contrast;
          ct->reject_edge += row.ct.reject_edge; ct->candidates += row.ct.candidates; ct->multi_peak += row.ct.multi_peak; ct->keypoints += row.ct.keypoints;
        }
      }
    }
  }
}

inline void describe_host(const Pyramid& P, const std::vector<Keypoint>& kps, bool root, float* out, size_t threads = 1) {
  std::atomic<size_t> next{0};
  pvlm_run_workers(std::max<size_t>(1, threads), [&]() {
    for (size_t i = next++; i < kps.size(); i = next++) {
      const DescWindow w = desc_window(kps[i], 1, 1);
      const int o = clampi(w.octave_index, 0, P.sz.n_oct - 1), l = clampi(w.layer, 0, kGauss - 1);
      descriptor_host(P.g(o, l), P.sz.rows[o], P.sz.cols[o], kps[i], root, out + i * kDescBins);
    }
  });
}

// one image end to end
inline void extract_host(const unsigned char* img, int rows, int cols, const unsigned char* mask, int nfeatures, bool root, std::vector<Keypoint>& kps,
                         std::vector<float>& desc, size_t threads = 1, Counters* ct = nullptr) {
  Pyramid P;
  build_pyramid(img, rows, cols, P, threads);
  std::vector<Cand> cands;
  kps.clear();
  detect_host(P, cands, kps, ct, threads);
  select(kps, nfeatures, rows, cols, mask);
  desc.assign(kps.size() * kDescBins, 0.f);
  describe_host(P, kps, root, desc.data(), threads);
}
#endif

}  // namespace pvlm_sift
