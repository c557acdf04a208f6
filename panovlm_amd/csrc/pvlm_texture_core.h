// The per-point statement of Texture::ColorizeLidarPointCloud (mvs/Texture.cpp:46-76) for one (scan, frame) pair:
//   const double distance = pt_raw.x * pt_raw.x + pt_raw.y * pt_raw.y + pt_raw.z * pt_raw.z;   // float arithmetic, then promoted
//   if (distance < min_dist_sq || distance > max_dist_sq) continue;                              // a NaN distance passes
//   point = (T_cl * point.homogeneous()).hnormalized();                                          // double; T_cl = T_wc^-1 T_wl
//   cv::Point2i pt_pixel(round(px.x()), round(px.y()));  if (!eq.IsInside(pt_pixel)) continue;  // px = eq.CamToImage(point), double
//   hsv = img_hsv.at<cv::Vec3b>(pt_pixel);  skip when h in [100, 124], s in [43, 200], v in [150, 255]
//   PointXYZRGB{pt_raw.x, pt_raw.y, pt_raw.z, bgr of the pixel}
// host/device; compiled with -ffp-contract=off like the reference's x86-64 build (no FMA in the float distance, none in the double transform).
//
// The image test is cv::cvtColor(CV_BGR2HSV) on 8-bit input, OpenCV's integer RGB2HSV_b (hsv_shift = 12, the sdiv / hdiv180 tables), NOT the float
// BGR2HSV of util/Visualization.cpp that FuseDepthImages uses (pvlm_mvs_core.h).  It is recalled from OpenCV's color_hsv sources and not pinned against an
// OpenCV build; the tables' quotients never lie on a half, so cvRound's ties-to-even and the round-half-up of the integer form below agree.
#pragma once
#include <climits>
#include <cmath>

#include "pvlm_equirect_core.h"

#ifndef PVLM_UD
#if defined(__HIPCC__)
#define PVLM_UD __host__ __device__ inline
#else
#define PVLM_UD inline
#endif
#endif

namespace pvlm_texture {

// the range test (Texture.cpp:48-50): (x*x + y*y) + z*z in float
PVLM_UD bool in_range(float x, float y, float z, double sq_min, double sq_max) {
  const float xx = x * x, yy = y * y, zz = z * z;
  const float d = (xx + yy) + zz;
  const double distance = (double)d;
  return !(distance < sq_min || distance > sq_max);
}

// (T_cl * (x, y, z, 1)).hnormalized() with T_cl = rows 0..2 of a rigid transform (12 doubles; its last row is exactly 0 0 0 1): per row
// ((m0 x + m1 y) + m2 z) + m3, w the same sum over the last row (1, or NaN for a non-finite point), each coordinate divided by w
PVLM_UD void to_camera(const double* T, float x, float y, float z, double* p) {
  const double X = (double)x, Y = (double)y, Z = (double)z;
  const double w = ((0.0 * X + 0.0 * Y) + 0.0 * Z) + 1.0;
  for (int r = 0; r < 3; ++r) p[r] = (((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3]) / w;
}

// int(std::round(v)) as the reference's x86-64 build converts it (cvttsd2si): half away from zero, then NaN and values outside int's range become INT_MIN.
// A plain device conversion would give 0 for NaN and colour such a point from pixel (0, 0).
PVLM_UD int round_to_int(double v) {
  const double r = round(v);
  return (r >= -2147483648.0 && r < 2147483648.0) ? (int)r : INT_MIN;
}

// Equirectangular::IsInside(cv::Point2i) (sensors/Equirectangular.h:184-187)
PVLM_UD bool is_inside(int x, int y, int rows, int cols) { return x >= 0 && y >= 0 && (long long)x + 1 <= cols && (long long)y + 1 <= rows; }

// range test, transform, CamToImage, round, IsInside: true and the pixel when the point reaches the image
PVLM_UD bool project(const double* T, int rows, int cols, float x, float y, float z, double sq_min, double sq_max, int* px, int* py) {
  if (!in_range(x, y, z, sq_min, sq_max)) return false;
  double p[3], u, v;
  to_camera(T, x, y, z, p);
  pvlm_equirect::cam_to_image_f64(rows, cols, p[0], p[1], p[2], &u, &v);
  const int ix = round_to_int(u), iy = round_to_int(v);
  if (!is_inside(ix, iy, rows, cols)) return false;
  *px = ix; *py = iy;
  return true;
}

// OpenCV's RGB2HSV_b, hrange 180: sdiv[v] = round((255 << 12) / v), hdiv180[d] = round((180 << 12) / (6 d)), index 0 -> 0
PVLM_UD void bgr2hsv_u8(int b, int g, int r, int* h_out, int* s_out, int* v_out) {
  const int hsv_shift = 12;
  int v = b, vmin = b;
  v = v > g ? v : g; v = v > r ? v : r;
  vmin = vmin < g ? vmin : g; vmin = vmin < r ? vmin : r;
  const int diff = v - vmin;
  const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
  const int sdiv = v ? (2 * (255 << hsv_shift) + v) / (2 * v) : 0;
  const int hdiv = diff ? (2 * ((180 << hsv_shift) / 6) + diff) / (2 * diff) : 0;
  const int s = (diff * sdiv + (1 << (hsv_shift - 1))) >> hsv_shift;
  int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
  h = (h * hdiv + (1 << (hsv_shift - 1))) >> hsv_shift;
  h += h < 0 ? 180 : 0;
  *h_out = h; *s_out = s; *v_out = v;
}

// the sky test of Texture.cpp:67-68
PVLM_UD bool is_sky(int h, int s, int v) { return h >= 100 && h <= 124 && s >= 43 && s <= 200 && v >= 150 && v <= 255; }

// pcl::PointXYZRGB's colour word (b | g << 8 | r << 16 | 255 << 24; never 0), or 0 when the pixel's colour is sky
PVLM_UD unsigned colour_word(int b, int g, int r) {
  int h, s, v;
  bgr2hsv_u8(b, g, r, &h, &s, &v);
  if (is_sky(h, s, v)) return 0u;
  return (unsigned)b | ((unsigned)g << 8) | ((unsigned)r << 16) | (255u << 24);
}

}  // namespace pvlm_texture
