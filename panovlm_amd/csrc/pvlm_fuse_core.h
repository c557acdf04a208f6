// The per-point statement of LidarOdometry::FuseLidar (lidar_mapping/LidarOdometry.cpp:323-348; CameraLidarOptimizer::FuseLidar,
// joint_optimization/CameraLidarOptimizer.cpp:777-802, has the same body):
//   double range = pt.x * pt.x + pt.y * pt.z + pt.z * pt.z;       // float arithmetic, then promoted; y * z is upstream's (kept)
//   if (range > sq_max_range || range < sq_min_range) continue;    // NaN ranges are kept: both comparisons are false
//   pcl::transformPointCloud(kept, kept, GetPose());               // Matrix4d: per coordinate float(((m0 x + m1 y) + m2 z) + m3) in double
// host/device; compiled with -ffp-contract=off like the reference's x86-64 build (no FMA in the float range, none in the double transform).
// f32 subnormals are kept on both sides (hipcc's default kernel mode): a flush would change decisions near min_range ~ 1e-20.
#pragma once

#ifndef PVLM_UD
#if defined(__HIPCC__)
#define PVLM_UD __host__ __device__ inline
#else
#define PVLM_UD inline
#endif
#endif

namespace pvlm_fuse {

// the range test (LidarOdometry.cpp:336-338)
PVLM_UD bool keep_point(float x, float y, float z, double sq_min, double sq_max) {
  const float xx = x * x, yz = y * z, zz = z * z;
  const float r = (xx + yz) + zz;
  const double range = (double)r;
  return !(range > sq_max || range < sq_min);
}

// T: the first three rows of the row-major 4x4 world <- sensor pose (12 doubles)
PVLM_UD void transform_point(const double* T, float x, float y, float z, float* out) {
  const double X = (double)x, Y = (double)y, Z = (double)z;
  for (int r = 0; r < 3; ++r) out[r] = (float)(((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3]);
}

}  // namespace pvlm_fuse
