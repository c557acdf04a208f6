// Per-track statement of K31's filters after a global bundle adjustment: FilterTracksPixelResidual and FilterTracksAngleResidual
// (sfm/Structure.cpp:121-193), called by SfM::GlobalBundleAdjustment (sfm/SfM.cpp:1362-1383).  One call decides one track: it survives
// when none of its observations rejects it.  Host / device: csrc/pvlm_sfm_filter.hip wraps it in a kernel, a host compile
// (tests/cpp/sfm_ba_math_check.cpp) is what the CPU tests compare with numpy bit for bit.  Compile with -ffp-contract=off.
#pragma once
#include <cmath>

#include "pvlm_equirect_core.h"

namespace pvlm_sfm_filter {

// eq.ImageToCam(kp.pt) binds to ImageToCam(const cv::Point2i&) (Equirectangular.h:158-166): saturate_cast<int> rounds half to even,
// then ImageToCam(cv::Point2f(pixel), 1.f) un-projects in float; the mirror's Equirect::ImageToCam<float> takes sin / cos in double and
// rounds them to float.
PVLM_EQ_UD void image_to_cam_point2i(int rows, int cols, float kx, float ky, float* cam) {
  const float px = (float)(int)rintf(kx), py = (float)(int)rintf(ky);
  const float sx = (float)((double)(2 * px / cols - 1) * 3.14159265358979323846);
  const float sy = (float)((0.5 - (double)(py / rows)) * 3.14159265358979323846);
  const float cy = (float)cos((double)sy);
  cam[0] = 1.f * cy * (float)sin((double)sx);
  cam[1] = -1.f * (float)sin((double)sy);
  cam[2] = 1.f * cy * (float)cos((double)sx);
}

// (T_cw * X.homogeneous()).head(3) with T_cw = [R | t] row-major 3 x 4
PVLM_EQ_UD void transform(const double* T, const double* X, double* p) {
  for (int r = 0; r < 3; ++r) p[r] = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3];
}

// the value keep_track compares with: Square(threshold) of FilterTracksPixelResidual, +inf when threshold < 0 (its early return: nothing is
// filtered; sq > inf is never true), or cos(threshold * M_PI / 180.0) of FilterTracksAngleResidual
PVLM_EQ_UD double filter_threshold(int mode, double threshold) {
  if (mode == 0) return threshold < 0 ? (double)INFINITY : threshold * threshold;
  return cos(threshold * 3.14159265358979323846 / 180.0);
}

// mode 0 (pixel): thr = threshold^2, reject when the squared pixel distance exceeds it (+inf: keep everything).
// mode 1 (angle): thr = cos(threshold pi / 180), reject when the cosine is below it (NaN never rejects).
// Returns 1 = keep.
PVLM_EQ_UD unsigned char keep_track(int mode, int rows, int cols, long long o0, long long o1, const int* frame_ids, const float* kp, const double* X,
                                    const double* T_cw, double thr) {
  for (long long i = o0; i < o1; ++i) {
    double p[3];
    transform(T_cw + 12 * (long long)frame_ids[i], X, p);
    const float kx = kp[2 * i], ky = kp[2 * i + 1];
    if (mode == 0) {
      double u, v;
      pvlm_equirect::cam_to_image_f64(rows, cols, p[0], p[1], p[2], &u, &v);
      const double dx = (double)kx - u, dy = (double)ky - v;
      const double sq = dx * dx + dy * dy;
      if (sq > thr) return 0;
    } else {
      float ray[3];
      image_to_cam_point2i(rows, cols, kx, ky, ray);
      const double dot = p[0] * ray[0] + p[1] * ray[1] + p[2] * ray[2];
      const double np = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
      // cv::norm(Point3f): sqrt((double)x*x + (double)y*y + (double)z*z), recalled from OpenCV, not pinned
      const double nr = sqrt((double)ray[0] * ray[0] + (double)ray[1] * ray[1] + (double)ray[2] * ray[2]);
      const double c = dot / np / nr;
      if (c < thr) return 0;
    }
  }
  return 1;
}

}  // namespace pvlm_sfm_filter
