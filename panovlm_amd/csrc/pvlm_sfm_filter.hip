// K31's track filter after a global bundle adjustment (FilterTracksPixelResidual / FilterTracksAngleResidual, sfm/Structure.cpp:121-193):
// one thread per track, all-of over its observations, a uint8 keep mask; the host compacts the tracks in their order.  The per-track
// statement is pvlm_sfm_filter_core.h.  Built with -ffp-contract=off: the threshold decisions must equal a non-FMA x86-64 build.
#include <cmath>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_sfm_filter_core.h"

__global__ void __launch_bounds__(256) k_filter_tracks(int mode, int rows, int cols, int n_points, const long long* __restrict__ off,
                                                       const int* __restrict__ frame_ids, const float* __restrict__ kp, const double* __restrict__ X,
                                                       const double* __restrict__ T_cw, double thr, unsigned char* __restrict__ keep) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_points) return;
  keep[t] = pvlm_sfm_filter::keep_track(mode, rows, cols, off[t], off[t + 1], frame_ids, kp, X + 3 * (size_t)t, T_cw, thr);
}

extern "C" pvlm_status pvlm_filter_tracks(pvlm_ctx* ctx, pvlm_filter_mode mode, int rows, int cols, int n_points, const int64_t* point_offsets,
                                          const int* frame_ids, const float* keypoints_f32, const double* points, int n_frames, const double* T_cw_3x4,
                                          double threshold, unsigned char* keep) {
  if (!ctx || n_points < 0 || n_frames < 0 || (mode != PVLM_FILTER_PIXEL && mode != PVLM_FILTER_ANGLE) || rows <= 0 || cols <= 0) return PVLM_ERR_ARG;
  if (n_points == 0) return PVLM_OK;
  if (!point_offsets || !points || !keep) return PVLM_ERR_ARG;
  pvlm_call c(ctx, "pvlm_filter_tracks");
  if (c.enter()) return c.st;
  if (point_offsets[0] != 0) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: point_offsets must start at 0"); return PVLM_ERR_ARG; }
  for (int t = 0; t < n_points; ++t)
    if (point_offsets[t + 1] < point_offsets[t]) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: point_offsets must be non-decreasing"); return PVLM_ERR_ARG; }
  const int64_t n_obs = point_offsets[n_points];
  if ((n_obs > 0 && (!frame_ids || !keypoints_f32)) || (n_frames > 0 && !T_cw_3x4)) return PVLM_ERR_ARG;
  for (int64_t i = 0; i < n_obs; ++i)
    if (frame_ids[i] < 0 || frame_ids[i] >= n_frames) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: frame id %d at observation %lld out of range", frame_ids[i], (long long)i); return PVLM_ERR_ARG; }
  const double thr = pvlm_sfm_filter::filter_threshold((int)mode, threshold);     // on the host: one cos, the reference's value
  const std::vector<long long> off(point_offsets, point_offsets + n_points + 1);
  long long* d_off = c.upload(off.data(), off.size());
  int* d_fid = c.upload(frame_ids, (size_t)n_obs);
  float* d_kp = c.upload(keypoints_f32, (size_t)n_obs * 2);
  double* d_X = c.upload(points, (size_t)n_points * 3);
  double* d_T = c.upload(T_cw_3x4, n_obs ? (size_t)n_frames * 12 : 0);
  unsigned char* d_keep = c.alloc<unsigned char>((size_t)n_points);
  c.launch(k_filter_tracks, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (int)mode, rows, cols, n_points, d_off, d_fid, d_kp, d_X, d_T, thr, d_keep);
  c.check_launches();
  c.d2h(keep, d_keep, (size_t)n_points);
  return c.sync();
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first pvlm_filter_tracks (see pvlm_ba.hip)
__global__ void k_preload_sfm_filter() {}
void pvlm_i_preload_sfm_filter(hipStream_t s) { hipLaunchKernelGGL(k_preload_sfm_filter, dim3(1), dim3(1), 0, s); }
