// K32: structure from tracks.  pvlm_triangulate_tracks is the loop body of TriangulateTracks (sfm/Structure.cpp:36-62) and
// pvlm_filter_tracks_far is FilterTracksToFar (:87-119): one lane per track, a point and a status byte / a keep byte per track, the host
// compacts the tracks in their order.  The per-track statement is pvlm_triangulate_core.h.  Built with -ffp-contract=off: the points must
// equal a non-FMA x86-64 build of the core bit for bit.
//
// Launch shape: blocks of one wave.  A wave waits for its longest track (2 to a few dozen observations, then up to 12 Jacobi sweeps), so
// a block of several waves would also hold its finished waves' registers until the slowest one ends.  A track's result depends on its
// own observations only: neither on its neighbours nor on the launch shape, no atomics, the same bits on every run.  The pose table
// (96 B per frame) is read through the cache: every lane of a wave gathers other frames, the table of a Room (44 KB) stays in L2.
#include <cmath>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_triangulate_core.h"

__global__ void __launch_bounds__(64) k_triangulate_tracks(int rows, int cols, int n_tracks, const long long* __restrict__ off, const int* __restrict__ frame_ids,
                                                           const float* __restrict__ kp, const float* __restrict__ bearings, const double* __restrict__ T_cw,
                                                           const unsigned char* __restrict__ frame_valid, double* __restrict__ X,
                                                           unsigned char* __restrict__ status) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tracks) return;
  double p[3];
  status[t] = (unsigned char)pvlm_triangulate::triangulate_track(rows, cols, off[t], off[t + 1], frame_ids, kp, bearings, T_cw, frame_valid, p);
  X[3 * (size_t)t] = p[0]; X[3 * (size_t)t + 1] = p[1]; X[3 * (size_t)t + 2] = p[2];
}

__global__ void __launch_bounds__(64) k_filter_tracks_far(int n_tracks, const long long* __restrict__ off, const int* __restrict__ frame_ids,
                                                          const double* __restrict__ X, const double* __restrict__ t_wc,
                                                          const unsigned char* __restrict__ frame_valid, double threshold, unsigned char* __restrict__ keep) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tracks) return;
  keep[t] = pvlm_triangulate::keep_track_far(off[t], off[t + 1], frame_ids, X + 3 * (size_t)t, t_wc, frame_valid, threshold);
}

// the kernels index with long long, the ABI hands int64_t: the same 8 bytes, uploaded as they are
static_assert(sizeof(long long) == sizeof(int64_t), "track offsets are uploaded without a copy");

// the CSR checks both entry points share: offsets start at 0 and do not decrease, every frame id indexes the frame tables
static pvlm_status check_tracks(pvlm_ctx* ctx, const char* who, int n_tracks, const int64_t* track_offsets, const int* frame_ids, int n_frames) {
  if (track_offsets[0] != 0) { PVLM_SET_ERR(ctx, "%s: track_offsets must start at 0", who); return PVLM_ERR_ARG; }
  for (int t = 0; t < n_tracks; ++t)
    if (track_offsets[t + 1] < track_offsets[t]) { PVLM_SET_ERR(ctx, "%s: track_offsets must be non-decreasing", who); return PVLM_ERR_ARG; }
  const int64_t n_obs = track_offsets[n_tracks];
  if (n_obs > 0 && !frame_ids) return PVLM_ERR_ARG;
  for (int64_t i = 0; i < n_obs; ++i)
    if (frame_ids[i] < 0 || frame_ids[i] >= n_frames) { PVLM_SET_ERR(ctx, "%s: frame id %d at observation %lld out of range", who, frame_ids[i], (long long)i); return PVLM_ERR_ARG; }
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_triangulate_tracks(pvlm_ctx* ctx, int rows, int cols, int n_tracks, const int64_t* track_offsets, const int* frame_ids,
                                               const float* keypoints_f32, const float* bearings_f32, int n_frames, const double* T_cw_3x4,
                                               const unsigned char* frame_valid, double* points, unsigned char* status) {
  if (!ctx || n_tracks < 0 || n_frames < 0 || (keypoints_f32 != nullptr) == (bearings_f32 != nullptr)) return PVLM_ERR_ARG;
  if (keypoints_f32 && (rows <= 0 || cols <= 0)) return PVLM_ERR_ARG;
  if (n_tracks == 0) return PVLM_OK;
  if (!track_offsets || !points || !status || (n_frames > 0 && !T_cw_3x4)) return PVLM_ERR_ARG;
  pvlm_call c(ctx, "pvlm_triangulate_tracks");
  if (c.enter() || (c.st = check_tracks(ctx, c.who, n_tracks, track_offsets, frame_ids, n_frames))) return c.st;
  const size_t n_obs = (size_t)track_offsets[n_tracks];
  const int per = keypoints_f32 ? 2 : 3;                                  // floats per observation
  long long* d_off = c.upload(reinterpret_cast<const long long*>(track_offsets), (size_t)n_tracks + 1);
  int* d_fid = c.upload(frame_ids, n_obs);
  float* d_obs = c.upload(keypoints_f32 ? keypoints_f32 : bearings_f32, n_obs * per);
  double* d_T = c.upload(T_cw_3x4, (size_t)n_frames * 12);
  unsigned char* d_valid = frame_valid ? c.upload(frame_valid, (size_t)n_frames) : nullptr;
  double* d_X = c.alloc<double>((size_t)n_tracks * 3);
  unsigned char* d_status = c.alloc<unsigned char>((size_t)n_tracks);
  c.launch(k_triangulate_tracks, dim3((unsigned)((n_tracks + 63) / 64)), dim3(64), 0, rows, cols, n_tracks, d_off, d_fid, keypoints_f32 ? d_obs : nullptr,
           bearings_f32 ? d_obs : nullptr, d_T, d_valid, d_X, d_status);
  c.check_launches();
  c.d2h(points, d_X, (size_t)n_tracks * 3 * sizeof(double));
  c.d2h(status, d_status, (size_t)n_tracks);
  return c.sync();
}

extern "C" pvlm_status pvlm_filter_tracks_far(pvlm_ctx* ctx, int n_tracks, const int64_t* track_offsets, const int* frame_ids, const double* points,
                                              int n_frames, const double* t_wc, const unsigned char* frame_valid, double threshold, unsigned char* keep) {
  if (!ctx || n_tracks < 0 || n_frames < 0) return PVLM_ERR_ARG;
  if (n_tracks == 0) return PVLM_OK;
  if (!track_offsets || !points || !keep || (n_frames > 0 && !t_wc)) return PVLM_ERR_ARG;
  pvlm_call c(ctx, "pvlm_filter_tracks_far");
  if (c.enter() || (c.st = check_tracks(ctx, c.who, n_tracks, track_offsets, frame_ids, n_frames))) return c.st;
  long long* d_off = c.upload(reinterpret_cast<const long long*>(track_offsets), (size_t)n_tracks + 1);
  int* d_fid = c.upload(frame_ids, (size_t)track_offsets[n_tracks]);
  double* d_X = c.upload(points, (size_t)n_tracks * 3);
  double* d_t = c.upload(t_wc, (size_t)n_frames * 3);
  unsigned char* d_valid = frame_valid ? c.upload(frame_valid, (size_t)n_frames) : nullptr;
  unsigned char* d_keep = c.alloc<unsigned char>((size_t)n_tracks);
  c.launch(k_filter_tracks_far, dim3((unsigned)((n_tracks + 63) / 64)), dim3(64), 0, n_tracks, d_off, d_fid, d_X, d_t, d_valid, threshold, d_keep);
  c.check_launches();
  c.d2h(keep, d_keep, (size_t)n_tracks);
  return c.sync();
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first pvlm_triangulate_tracks (see pvlm_ba.hip)
__global__ void k_preload_triangulate() {}
void pvlm_i_preload_triangulate(hipStream_t s) { hipLaunchKernelGGL(k_preload_triangulate, dim3(1), dim3(1), 0, s); }
