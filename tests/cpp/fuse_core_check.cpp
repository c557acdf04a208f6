// Host-compiled check of the per-point statement of K29 (panovlm_amd/csrc/pvlm_fuse_core.h: the range test and the world transform of
// LidarOdometry::FuseLidar), the functions k_fuse_count / k_fuse_scatter call, driven over caller-given points so that tests/test_fuse_cpu.py can compare
// them with a numpy restatement bit for bit on a machine without a GPU.  TEST INFRASTRUCTURE ONLY — libpvlm.so has no host path.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared
#include "../../panovlm_amd/csrc/pvlm_fuse_core.h"

extern "C" {
// pts: n x 4 (x, y, z, intensity); T: 16 doubles row-major; keep[i]: the range test; out: n x 3, the transform of every point (kept or not)
void chk_fuse(const float* pts, long long n, const double* T, double min_range, double max_range, unsigned char* keep, float* out) {
  const double sq_min = min_range * min_range, sq_max = max_range * max_range;
  for (long long i = 0; i < n; ++i) {
    const float* p = pts + 4 * i;
    keep[i] = pvlm_fuse::keep_point(p[0], p[1], p[2], sq_min, sq_max) ? 1 : 0;
    pvlm_fuse::transform_point(T, p[0], p[1], p[2], out + 3 * i);
  }
}
}
