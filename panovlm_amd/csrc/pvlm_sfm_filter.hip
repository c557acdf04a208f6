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
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (point_offsets[0] != 0) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: point_offsets must start at 0"); return PVLM_ERR_ARG; }
  for (int t = 0; t < n_points; ++t)
    if (point_offsets[t + 1] < point_offsets[t]) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: point_offsets must be non-decreasing"); return PVLM_ERR_ARG; }
  const int64_t n_obs = point_offsets[n_points];
  if ((n_obs > 0 && (!frame_ids || !keypoints_f32)) || (n_frames > 0 && !T_cw_3x4)) return PVLM_ERR_ARG;
  for (int64_t i = 0; i < n_obs; ++i)
    if (frame_ids[i] < 0 || frame_ids[i] >= n_frames) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: frame id %d at observation %lld out of range", frame_ids[i], (long long)i); return PVLM_ERR_ARG; }
  const double thr = pvlm_sfm_filter::filter_threshold((int)mode, threshold);     // on the host: one cos, the reference's value
  std::vector<long long> off(point_offsets, point_offsets + n_points + 1);
  long long* d_off = nullptr; int* d_fid = nullptr; float* d_kp = nullptr; double* d_X = nullptr; double* d_T = nullptr; unsigned char* d_keep = nullptr;
  pvlm_status st = PVLM_OK;
  if (!st) st = pvlm_i_alloc(ctx, &d_off, off.size());
  if (!st) st = pvlm_i_alloc(ctx, &d_fid, (size_t)std::max<int64_t>(n_obs, 1));
  if (!st) st = pvlm_i_alloc(ctx, &d_kp, (size_t)std::max<int64_t>(n_obs, 1) * 2);
  if (!st) st = pvlm_i_alloc(ctx, &d_X, (size_t)n_points * 3);
  if (!st) st = pvlm_i_alloc(ctx, &d_T, (size_t)std::max(n_frames, 1) * 12);
  if (!st) st = pvlm_i_alloc(ctx, &d_keep, (size_t)n_points);
  if (!st) st = pvlm_i_h2d_q(ctx, d_off, off.data(), off.size() * sizeof(long long));
  if (!st && n_obs) st = pvlm_i_h2d_q(ctx, d_fid, frame_ids, (size_t)n_obs * sizeof(int));
  if (!st && n_obs) st = pvlm_i_h2d_q(ctx, d_kp, keypoints_f32, (size_t)n_obs * 2 * sizeof(float));
  if (!st) st = pvlm_i_h2d_q(ctx, d_X, points, (size_t)n_points * 3 * sizeof(double));
  if (!st && n_frames && n_obs) st = pvlm_i_h2d_q(ctx, d_T, T_cw_3x4, (size_t)n_frames * 12 * sizeof(double));
  if (!st) {
    hipLaunchKernelGGL(k_filter_tracks, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, ctx->stream, (int)mode, rows, cols, n_points, d_off, d_fid,
                       d_kp, d_X, d_T, thr, d_keep);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_filter_tracks: %s", hipGetErrorString(e)); st = PVLM_ERR_HIP; }
  }
  if (!st) st = pvlm_i_d2h_q(ctx, keep, d_keep, (size_t)n_points);
  { const pvlm_status s2 = pvlm_i_sync(ctx); if (!st) st = s2; }
  pvlm_i_free(ctx, d_off); pvlm_i_free(ctx, d_fid); pvlm_i_free(ctx, d_kp); pvlm_i_free(ctx, d_X); pvlm_i_free(ctx, d_T); pvlm_i_free(ctx, d_keep);
  return st;
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first pvlm_filter_tracks (see pvlm_ba.hip)
__global__ void k_preload_sfm_filter() {}
void pvlm_i_preload_sfm_filter(hipStream_t s) { hipLaunchKernelGGL(k_preload_sfm_filter, dim3(1), dim3(1), 0, s); }
