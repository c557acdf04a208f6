// FastAtan2 (base/Math.h:15-29) and the double-precision Equirectangular::CamToImage (sensors/Equirectangular.h:64-69, :84-85 with USE_FAST_ATAN2),
// host/device: K7's double path (pvlm_cam_to_image_f64, csrc/pvlm_lines.hip) and K30's projection (csrc/pvlm_texture_core.h) call the same code, and a
// host compile of it (tests/cpp/texture_core_check.cpp) is what the CPU tests compare with numpy.  Compile with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>

#ifndef PVLM_EQ_UD
#if defined(__HIPCC__)
#define PVLM_EQ_UD __host__ __device__ __forceinline__
#else
#define PVLM_EQ_UD inline
#endif
#endif

namespace pvlm_equirect {

// For T = float the polynomial is evaluated in double (double literals) and rounded to float on assignment, as are M_PI_2 - r and M_PI - r.
template <typename T>
PVLM_EQ_UD T fast_atan2(T y, T x) {
  const T ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;  // std::abs
  const T mn = ay < ax ? ay : ax, mxv = ax < ay ? ay : ax;  // std::min(ax, ay), std::max(ax, ay)
  const T a = mn / (mxv + (T)DBL_EPSILON);
  const T s = a * a;
  T r = ((-0.04432655554792128 * s + 0.1555786518463281) * s - 0.3258083974640975) * s * a + 0.9997878412794807 * a;
  if (ay > ax) r = 1.57079632679489661923 - r;
  if (x < 0) r = 3.14159265358979323846 - r;
  if (y < 0) r = -r;
  return r;
}

// Equirectangular::CamToImage(Eigen::Vector3d): CamToSphere (FastAtan2(x, z), -FastAtan2(y, sqrt(x*x + z*z))), then SphereToImage
// (cols * (0.5 + lon / (2 pi)), rows * (0.5 - lat / pi)), all in double
PVLM_EQ_UD void cam_to_image_f64(int rows, int cols, double x, double y, double z, double* u, double* v) {
  const double lon = fast_atan2<double>(x, z);
  const double lat = -fast_atan2<double>(y, (double)sqrt((double)(x * x + z * z)));
  *u = cols * (0.5 + lon / (2.0 * 3.14159265358979323846));
  *v = rows * (0.5 - lat / 3.14159265358979323846);
}

}  // namespace pvlm_equirect
