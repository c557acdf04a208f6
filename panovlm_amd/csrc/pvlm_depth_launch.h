// The splat launch of ProjectLidar2PanoramaDepth (k_depth_splat, pvlm_lines.hip), shared by pvlm_project_lidar_depth and K37 (pvlm_depthfill.hip).
#pragma once
#include "pvlm_internal.h"

namespace pvlm_depth_launch {

// Queues the splat of one cloud on the context's stream: every one of the n points of d_xyz (device, n x 3 floats, LiDAR frame) atomically maximises
// (point index + 1) << 16 | depth16 over its window in d_img (device, rows x cols words, zeroed by the caller), so that a pixel ends with the depth of the last point
// that covers it in its low 16 bits and stays 0 without one.  d_T: 16 doubles on the device.  n == 0 queues nothing.  Checks the launch.
pvlm_status splat(pvlm_ctx* ctx, const char* who, int rows, int cols, long long n, const float* d_xyz, const double* d_T, unsigned size, unsigned long long* d_img);

}  // namespace pvlm_depth_launch
