// Reprojection ("bundle") blocks of CameraLidarOptimizer::Optimize: PanoramaReprojResidual_1Angle
// (base/CostFunction.h:218-247) added by AddCameraResidual (util/Optimization.cpp:172-222).  Three parameter
// blocks per observation (aa_cw, t_cw, point_3d): the 3-D points are eliminated on the GPU (Schur complement,
// what Ceres' *_SCHUR solvers do for this problem, util/Optimization.cpp:608-634) so that the host LM driver
// only ever sees the 6x6 camera blocks in the same packed layout the LiDAR terms use.
//
// Layout in HBM: observations sorted by point (CSR), AoS 3-vectors (the set is 1e5..1e6 blocks — latency, not
// bandwidth, bound); one thread per point for the 3x3 work, one thread per observation for its row of the
// reduced system, fp64 hardware atomics into the packed buffer (summation order is not fixed: results are
// reproducible to rounding, ~1e-16 relative, not bit for bit).  gfx950 only.
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "pvlm_internal.h"

#define PVLM_HD __host__ __device__
#include "pvlm_ba_core.h"

struct pvlm_baset {
  int n_points = 0, n_cams = 0, n_upairs = 0;
  int64_t n_obs = 0;
  double weight = 1.0;
  int kind = 0;                     // pvlm_ba_kind: 0 PanoramaReprojResidual_1Angle, 1 _2Angle, 2 _Pixel (K31)
  pvlm_ba::Geo geo{0.0, 0.0};       // image rows / cols of the pixel kind
  std::vector<int> ui, uj;
  std::vector<int2> h_cpl;          // staging of the couple lists during pvlm_ba_create
  long long* d_pt_off = nullptr;
  int* d_cam = nullptr;
  int* d_obs_pt = nullptr;
  double* d_s = nullptr;            // n_obs x 3 unit bearings (kind 0) or n_obs x 2 observations
  double* d_X = nullptr;
  double* d_Xc = nullptr;
  double* d_scale = nullptr;
  double* d_Vinv = nullptr;
  double* d_gp = nullptr;
  int* d_adj_off = nullptr;
  int* d_adj_cam = nullptr;
  int* d_adj_slot = nullptr;
  unsigned char* d_frozen = nullptr;   // null = every point is free
  double* d_packed = nullptr;   // packed_size doubles
  double* d_dcam = nullptr;     // n_cams x 6
  double* d_small = nullptr;    // 4 doubles of scalar results
  long long* d_cpl_off = nullptr;   // n_cams + n_upairs + 1: couples of block s (diagonal blocks first, then the pairs in (ui, uj) order)
  int2* d_cpl = nullptr;            // (i, j) observation couples, block after block
  double* d_cost_cam = nullptr;     // n_cams partial costs (summed in camera order: reproducible)
  double* d_partials = nullptr;     // per-workgroup partial sums of k_ba_step (3 x) / k_ba_cost
  bool scaled = false;          // Jacobi scaling of the point columns initialised
  bool reduced = false;         // Vinv / gp valid for the current points
  uint64_t reduced_epoch = ~0ull;
  std::vector<double> reduced_poses;   // the host poses of the reduce (ctx->host_poses), when they were set from host memory
  bool reduced_poses_known = false;
  bool have_candidate = false;
};

static pvlm_ba::View make_view(const pvlm_baset* s, int loss, double a) {
  pvlm_ba::View v;
  v.n_points = s->n_points; v.n_cams = s->n_cams; v.n_upairs = s->n_upairs; v.n_obs = s->n_obs;
  v.pt_off = s->d_pt_off; v.cam = s->d_cam; v.obs_pt = s->d_obs_pt; v.s = s->d_s; v.X = s->d_X; v.Xc = s->d_Xc;
  v.scale = s->d_scale; v.Vinv = s->d_Vinv; v.gp = s->d_gp; v.adj_off = s->d_adj_off; v.adj_cam = s->d_adj_cam; v.adj_slot = s->d_adj_slot; v.frozen = s->d_frozen;
  v.w = s->weight; v.loss = loss; v.a = a;
  return v;
}

__device__ inline double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

__global__ void __launch_bounds__(128) k_ba_points(pvlm_ba::View v, const double* __restrict__ pose_tab, int init_scale, double radius, double min_diag, double max_diag,
                            double* gmax) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < v.n_points) pvlm_ba::point_pass(v, pose_tab, p, init_scale, radius, min_diag, max_diag, gmax);
}

// Round 1's scatter of every observation's rank-one blocks with fp64 atomics: 9.1 ms against 0.64 ms for the gather below at Room
// scale, and not bit-reproducible (profiles/r1_bundle_bench.json).  Kept out of the default library; a library
// built with -DPVLM_MEASURED_VARIANTS=1 (python -m panovlm_amd.build --variant measured -DPVLM_MEASURED_VARIANTS=1) selects it
// with PVLM_BA_ATOMICS=1.
#ifndef PVLM_MEASURED_VARIANTS
#define PVLM_MEASURED_VARIANTS 0
#endif
#if PVLM_MEASURED_VARIANTS
__global__ void __launch_bounds__(128) k_ba_obs(pvlm_ba::View v, const double* __restrict__ pose_tab, double* packed, double* cost) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double c = 0.0;
  if (i < v.n_obs) c = pvlm_ba::obs_pass(v, pose_tab, i, packed);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c != 0.0) unsafeAtomicAdd(cost, c);
}
#endif

// Pass B, gather form: wave s sums the couples of block s (s < n_cams: diagonal block of camera s + its g / Udiag / gcam /
// cost share; otherwise pair s - n_cams) — lane-strided partial sums, then a fixed shuffle tree: no atomics, bit-reproducible.
// couple(i, j, acc, vec) adds one couple (pvlm_ba::couple_pass, or couple_pass2 of a two-row kind).
template <typename Couple>
__device__ __forceinline__ void blocks_body(const pvlm_ba::View& v, const long long* __restrict__ cpl_off, const int2* __restrict__ cpl,
                                            double* __restrict__ packed, double* __restrict__ cost_cam, Couple couple) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= v.n_cams + v.n_upairs) return;
  double acc[36], vec[19];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 19; ++k) vec[k] = 0.0;
  for (long long q = cpl_off[s] + lane; q < cpl_off[s + 1]; q += 64) {
    const int2 c = cpl[q];
    couple(c.x, c.y, acc, vec);
  }
#pragma unroll
  for (int k = 0; k < 36; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  const bool diag = s < v.n_cams;
  if (diag) {
#pragma unroll
    for (int k = 0; k < 19; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) vec[k] += __shfl_xor(vec[k], off, 64);
  }
  if (lane != 0) return;
  double* dst = diag ? packed + (size_t)s * 36 : packed + (size_t)v.n_cams * 36 + (size_t)(s - v.n_cams) * 36;
#pragma unroll
  for (int k = 0; k < 36; ++k) dst[k] = acc[k];
  if (diag) {
    double* g = packed + (size_t)v.n_cams * 36 + (size_t)v.n_upairs * 36 + (size_t)s * 6;
    double* Ud = packed + (size_t)v.n_cams * 36 + (size_t)v.n_upairs * 36 + (size_t)v.n_cams * 6 + 1 + (size_t)s * 6;
    double* gc = Ud + (size_t)v.n_cams * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) { g[k] = vec[k]; Ud[k] = vec[6 + k]; gc[k] = vec[12 + k]; }
    cost_cam[s] = vec[18];
  }
}

__global__ void __launch_bounds__(256) k_ba_blocks(pvlm_ba::View v, const double* __restrict__ pose_tab, const long long* __restrict__ cpl_off,
                                                   const int2* __restrict__ cpl, double* __restrict__ packed, double* __restrict__ cost_cam) {
  blocks_body(v, cpl_off, cpl, packed, cost_cam,
              [&](long long i, long long j, double* acc, double* vec) { pvlm_ba::couple_pass(v, pose_tab, i, j, acc, vec); });
}
__global__ void k_ba_cost_sum(int n_cams, const double* __restrict__ cost_cam, double* __restrict__ cost) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { double c = 0.0; for (int k = 0; k < n_cams; ++k) c += cost_cam[k]; *cost = c; }
}

// Scalar results (model decrease, step norms, cost) are summed reproducibly: per-workgroup partials (waves in order), then
// one thread adds the partials in workgroup order (k_ba_sum_partials) — round 1 used one atomic per wave, whose order moved
// the last bits of the cost and with them the LM driver's borderline decisions from run to run.
__device__ inline void block_partial(double x, double* __restrict__ partial_out) {    // partial_out: this workgroup's slot
  __shared__ double ws[4];
  const double s = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0.0; for (unsigned w = 0; w < (blockDim.x >> 6); ++w) t += ws[w]; *partial_out = t; }
}
__global__ void k_ba_sum_partials(int n_partials, int n_out, const double* __restrict__ partials, double* __restrict__ out) {
  const int k = threadIdx.x;       // output k sums partials[k * n_partials ...]
  if (k >= n_out || blockIdx.x != 0) return;
  double t = 0.0;
  for (int q = 0; q < n_partials; ++q) t += partials[(size_t)k * n_partials + q];
  out[k] = t;
}
__global__ void __launch_bounds__(128) k_ba_step(pvlm_ba::View v, const double* __restrict__ pose_tab, const double* __restrict__ dcam, double* __restrict__ partials) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  double o[3] = {0.0, 0.0, 0.0};
  if (p < v.n_points) pvlm_ba::step_point(v, pose_tab, p, dcam, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) block_partial(o[k], &partials[(size_t)k * gridDim.x + blockIdx.x]);
}

__global__ void __launch_bounds__(256) k_ba_cost(pvlm_ba::View v, const double* __restrict__ pose_tab, int candidate, double* __restrict__ partials) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double c = 0.0;
  if (i < v.n_obs) c = pvlm_ba::cost_obs(v, pose_tab, i, candidate);
  block_partial(c, &partials[blockIdx.x]);
}

// materialise r and the 1x9 Jacobian rows [aa_cw | t_cw | X] (Ceres-feeding / parity mode)
__global__ void __launch_bounds__(256) k_ba_eval(pvlm_ba::View v, const double* __restrict__ pose_tab, double* __restrict__ r, double* __restrict__ J) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.n_obs) return;
  double rr, Jc[6], Jp[3];
  pvlm_reproj::eval_obs(pose_tab + (size_t)v.cam[i] * PVLM_BA_POSE_TAB, v.X + 3 * (size_t)v.obs_pt[i], v.s + 3 * i, v.w, &rr, Jc, Jp);
  r[i] = rr;
  if (J) {
    double* o = J + 9 * i;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = Jc[k];
    o[6] = Jp[0]; o[7] = Jp[1]; o[8] = Jp[2];
  }
}

// ---- K31: the two-row kinds (PanoramaReprojResidual_2Angle / _Pixel).  Same launch shapes, same gather order and the same reproducible
// sums as the 1Angle kernels above; the image size rides along as an extra argument so that the 1Angle kernels' arguments do not change.
template <int KIND>
__global__ void __launch_bounds__(128) k_ba2_points(pvlm_ba::View v, pvlm_ba::Geo geo, const double* __restrict__ pose_tab, int init_scale, double radius,
                                                    double min_diag, double max_diag, double* gmax) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < v.n_points) pvlm_ba::point_pass2<KIND>(v, geo, pose_tab, p, init_scale, radius, min_diag, max_diag, gmax);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_ba2_blocks(pvlm_ba::View v, pvlm_ba::Geo geo, const double* __restrict__ pose_tab, const long long* __restrict__ cpl_off,
                                                    const int2* __restrict__ cpl, double* __restrict__ packed, double* __restrict__ cost_cam) {
  blocks_body(v, cpl_off, cpl, packed, cost_cam,
              [&](long long i, long long j, double* acc, double* vec) { pvlm_ba::couple_pass2<KIND>(v, geo, pose_tab, i, j, acc, vec); });
}

template <int KIND>
__global__ void __launch_bounds__(128) k_ba2_step(pvlm_ba::View v, pvlm_ba::Geo geo, const double* __restrict__ pose_tab, const double* __restrict__ dcam,
                                                  double* __restrict__ partials) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  double o[3] = {0.0, 0.0, 0.0};
  if (p < v.n_points) pvlm_ba::step_point2<KIND>(v, geo, pose_tab, p, dcam, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) block_partial(o[k], &partials[(size_t)k * gridDim.x + blockIdx.x]);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_ba2_cost(pvlm_ba::View v, pvlm_ba::Geo geo, const double* __restrict__ pose_tab, int candidate, double* __restrict__ partials) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double c = 0.0;
  if (i < v.n_obs) c = pvlm_ba::cost_obs2<KIND>(v, geo, pose_tab, i, candidate);
  block_partial(c, &partials[blockIdx.x]);
}

// materialise the two rows r (2 per observation) and their 1 x 9 Jacobian rows [aa_cw | t_cw | X]
template <int KIND>
__global__ void __launch_bounds__(256) k_ba2_eval(pvlm_ba::View v, pvlm_ba::Geo geo, const double* __restrict__ pose_tab, double* __restrict__ r, double* __restrict__ J) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.n_obs) return;
  double rr[2], Jc[12], Jp[6];
  pvlm_reproj::eval_obs2<KIND>(pose_tab + (size_t)v.cam[i] * PVLM_BA_POSE_TAB, v.X + 3 * (size_t)v.obs_pt[i], v.s + 2 * i, v.w, geo.rows, geo.cols, rr, Jc, Jp);
  r[2 * i] = rr[0]; r[2 * i + 1] = rr[1];
  if (J) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double* o = J + 9 * (2 * i + k);
#pragma unroll
      for (int c = 0; c < 6; ++c) o[c] = Jc[6 * k + c];
      o[6] = Jp[3 * k]; o[7] = Jp[3 * k + 1]; o[8] = Jp[3 * k + 2];
    }
  }
}

// launches the kind's instance of a two-row kernel: BA2_LAUNCH(set, k_ba2_x, grid, block, args...)
#define BA2_LAUNCH(set, kern, grid, block, ...)                                                                        \
  do {                                                                                                                 \
    if ((set)->kind == pvlm_reproj::kPixel) hipLaunchKernelGGL(kern<pvlm_reproj::kPixel>, grid, block, 0, ctx->stream, __VA_ARGS__);   \
    else hipLaunchKernelGGL(kern<pvlm_reproj::kAngle2>, grid, block, 0, ctx->stream, __VA_ARGS__);                     \
  } while (0)

static pvlm_status ba_free(pvlm_ctx* ctx, pvlm_baset* s) {
  pvlm_i_free(ctx, s->d_pt_off); pvlm_i_free(ctx, s->d_cam); pvlm_i_free(ctx, s->d_obs_pt); pvlm_i_free(ctx, s->d_s); pvlm_i_free(ctx, s->d_X); pvlm_i_free(ctx, s->d_Xc); pvlm_i_free(ctx, s->d_scale);
  pvlm_i_free(ctx, s->d_Vinv); pvlm_i_free(ctx, s->d_gp); pvlm_i_free(ctx, s->d_adj_off); pvlm_i_free(ctx, s->d_adj_cam); pvlm_i_free(ctx, s->d_adj_slot); pvlm_i_free(ctx, s->d_packed);
  pvlm_i_free(ctx, s->d_dcam); pvlm_i_free(ctx, s->d_small); pvlm_i_free(ctx, s->d_frozen);
  pvlm_i_free(ctx, s->d_cpl_off); pvlm_i_free(ctx, s->d_cpl); pvlm_i_free(ctx, s->d_cost_cam); pvlm_i_free(ctx, s->d_partials);
  delete s;
  return PVLM_OK;
}

static pvlm_status ba_ready(pvlm_ctx* ctx, const pvlm_baset* s) {
  if (!ctx->poses_set) { PVLM_SET_ERR(ctx, "pvlm_set_poses (camera poses) must be called before the reprojection set is evaluated"); return PVLM_ERR_STATE; }
  if (ctx->n_poses < s->n_cams) { PVLM_SET_ERR(ctx, "the reprojection set references camera %d but only %d poses are set", s->n_cams - 1, ctx->n_poses); return PVLM_ERR_STATE; }
  return PVLM_OK;
}

template <typename T>
static pvlm_status h2d(pvlm_ctx* ctx, T* dst, const T* src, size_t n) {
  return n ? pvlm_i_h2d_q(ctx, dst, src, n * sizeof(T)) : PVLM_OK;     // through the pinned staging arena
}

extern "C" {

pvlm_status pvlm_ba_create_kind(pvlm_ctx* ctx, pvlm_ba_kind kind, int rows, int cols, int n_points, int64_t n_obs, const int64_t* point_offsets,
                                const int* cam_ids, const double* obs, const double* points, double weight, pvlm_baset** out) {
  if (!ctx || !out || n_points < 0 || n_obs < 0 || (n_points > 0 && (!point_offsets || !points)) || (n_obs > 0 && (!cam_ids || !obs)))
    return PVLM_ERR_ARG;
  if (kind != PVLM_BA_ANGLE1 && kind != PVLM_BA_ANGLE2 && kind != PVLM_BA_PIXEL) return PVLM_ERR_ARG;
  if (kind == PVLM_BA_PIXEL && (rows <= 0 || cols <= 0)) return PVLM_ERR_ARG;
  *out = nullptr;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (n_points > 0 && (point_offsets[0] != 0 || point_offsets[n_points] != n_obs)) { PVLM_SET_ERR(ctx, "point_offsets must run from 0 to n_obs"); return PVLM_ERR_ARG; }
  int n_cams = 0;
  for (int64_t i = 0; i < n_obs; ++i) {
    if (cam_ids[i] < 0) { PVLM_SET_ERR(ctx, "negative camera id at observation %lld", (long long)i); return PVLM_ERR_ARG; }
    n_cams = std::max(n_cams, cam_ids[i] + 1);
  }
  if (n_obs >= (1ll << 31)) { PVLM_SET_ERR(ctx, "more than 2^31 observations"); return PVLM_ERR_ARG; }
  std::vector<int> obs_pt((size_t)n_obs);
  std::vector<long long> off((size_t)n_points + 1, 0);
  // co-visible camera pairs as sorted unique 64-bit keys (ui << 32 | uj) — round 1 inserted 2 M couples into a std::set.
  // Up to 4096 cameras the pairs are marked in an n_cams x n_cams table (later the pair -> block lookup); beyond, sorted keys.
  std::vector<unsigned long long> keys;
  const bool table = n_cams <= 4096;
  std::vector<int> pair_slot;                       // (ci, cj), ci < cj -> index of the pair, -1 = not co-visible
  if (table) pair_slot.assign((size_t)n_cams * n_cams, -1);
  for (int p = 0; p < n_points; ++p) {
    if (point_offsets[p + 1] < point_offsets[p]) { PVLM_SET_ERR(ctx, "point_offsets must be non-decreasing"); return PVLM_ERR_ARG; }
    off[p] = point_offsets[p]; off[p + 1] = point_offsets[p + 1];
    for (int64_t i = point_offsets[p]; i < point_offsets[p + 1]; ++i) {
      obs_pt[(size_t)i] = p;
      for (int64_t j = i + 1; j < point_offsets[p + 1]; ++j)
        if (cam_ids[i] != cam_ids[j]) {
          const int lo = std::min(cam_ids[i], cam_ids[j]), hi = std::max(cam_ids[i], cam_ids[j]);
          if (table) pair_slot[(size_t)lo * n_cams + hi] = 0;
          else keys.push_back(((unsigned long long)lo << 32) | (unsigned)hi);
        }
    }
  }
  if (table) {
    for (int lo = 0; lo < n_cams; ++lo)
      for (int hi = lo + 1; hi < n_cams; ++hi)
        if (pair_slot[(size_t)lo * n_cams + hi] == 0) { pair_slot[(size_t)lo * n_cams + hi] = (int)keys.size(); keys.push_back(((unsigned long long)lo << 32) | (unsigned)hi); }
  } else {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  }
  const int od = kind == PVLM_BA_ANGLE1 ? 3 : 2;     // doubles per observation
  std::vector<double> s((size_t)n_obs * od);
  if (kind == PVLM_BA_ANGLE1) {
    // unit bearings: point_sphere.normalize() of the functor's constructor (CostFunction.h:227-230)
    for (int64_t i = 0; i < n_obs; ++i) {
      const double* b = obs + 3 * i;
      const double n = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      for (int k = 0; k < 3; ++k) s[(size_t)i * 3 + k] = n > 0.0 ? b[k] / n : b[k];
    }
  } else {
    for (int64_t i = 0; i < n_obs; ++i) {
      s[(size_t)i * 2] = obs[2 * i]; s[(size_t)i * 2 + 1] = obs[2 * i + 1];
      // PanoramaReprojResidual_2Angle's constructor (CostFunction.h:185-189): x += 2 pi if x < 0, in double
      if (kind == PVLM_BA_ANGLE2 && s[(size_t)i * 2] < 0) s[(size_t)i * 2] += 2 * M_PI;
    }
  }
  pvlm_baset* bs = new pvlm_baset();
  bs->n_points = n_points; bs->n_obs = n_obs; bs->n_cams = n_cams; bs->weight = weight;
  bs->kind = (int)kind; bs->geo = pvlm_ba::Geo{(double)rows, (double)cols};
  std::vector<int> adj_off((size_t)n_cams + 1, 0), adj_cam, adj_slot;
  for (unsigned long long k : keys) { bs->ui.push_back((int)(k >> 32)); bs->uj.push_back((int)(k & 0xFFFFFFFFu)); }   // sorted by (ui, uj): CSR order
  bs->n_upairs = (int)bs->ui.size();
  for (int u = 0; u < bs->n_upairs; ++u) { adj_off[(size_t)bs->ui[u] + 1]++; adj_cam.push_back(bs->uj[u]); adj_slot.push_back(u); }
  for (int c = 0; c < n_cams; ++c) adj_off[(size_t)c + 1] += adj_off[c];
  // couples of every block: (i, j) with cam[i] < cam[j] for the pair blocks (the block of (ci, cj) is rows ci x columns cj),
  // every ordered (i, j) with cam[i] == cam[j] — normally just (i, i) — for the diagonal blocks; counting sort by block
  const int n_slots = n_cams + bs->n_upairs;
  auto slot_of = [&](int ci, int cj) {          // ci < cj
    if (table) return n_cams + pair_slot[(size_t)ci * n_cams + cj];
    const unsigned long long k = ((unsigned long long)ci << 32) | (unsigned)cj;
    return n_cams + (int)(std::lower_bound(keys.begin(), keys.end(), k) - keys.begin());
  };
  std::vector<long long> cpl_off((size_t)n_slots + 1, 0);
  {
    std::vector<int> slot_seq;               // block of every couple, in visiting order (pass 0 finds it, pass 1 replays it)
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<long long> cursor;
      if (pass == 1) {
        for (int q = 0; q < n_slots; ++q) cpl_off[(size_t)q + 1] += cpl_off[q];
        cursor.assign(cpl_off.begin(), cpl_off.end() - 1);
        bs->h_cpl.resize((size_t)cpl_off[n_slots]);
      }
      size_t seq = 0;
      for (int p = 0; p < n_points; ++p)
        for (int64_t i = point_offsets[p]; i < point_offsets[p + 1]; ++i)
          for (int64_t j = point_offsets[p]; j < point_offsets[p + 1]; ++j) {
            const int ci = cam_ids[i], cj = cam_ids[j];
            if (cj < ci) continue;
            if (pass == 0) { const int q = ci == cj ? ci : slot_of(ci, cj); slot_seq.push_back(q); cpl_off[(size_t)q + 1]++; }
            else bs->h_cpl[(size_t)cursor[slot_seq[seq++]]++] = make_int2((int)i, (int)j);
          }
    }
  }
  const size_t psz = (size_t)pvlm_ba::packed_size(n_cams, bs->n_upairs);
  pvlm_status st = PVLM_OK;
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_pt_off, (size_t)n_points + 1);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_cam, (size_t)n_obs);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_obs_pt, (size_t)n_obs);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_s, (size_t)n_obs * od);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_X, (size_t)n_points * 3);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_Xc, (size_t)n_points * 3);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_scale, (size_t)n_points * 3);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_Vinv, (size_t)n_points * 6);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_gp, (size_t)n_points * 3);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_adj_off, (size_t)n_cams + 1);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_adj_cam, adj_cam.size());
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_adj_slot, adj_slot.size());
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_packed, psz);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_dcam, (size_t)n_cams * 6);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_small, (size_t)4);
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_cpl_off, cpl_off.size());
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_cpl, std::max<size_t>(bs->h_cpl.size(), 1));
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_cost_cam, (size_t)std::max(n_cams, 1));
  if (!st) st = pvlm_i_alloc(ctx, &bs->d_partials, std::max<size_t>(3 * (((size_t)n_points + 127) / 128), ((size_t)n_obs + 255) / 256) + 4);
  if (!st) st = h2d(ctx, bs->d_cpl_off, cpl_off.data(), cpl_off.size());
  if (!st) st = h2d(ctx, bs->d_cpl, bs->h_cpl.data(), bs->h_cpl.size());
  if (!st) st = h2d(ctx, bs->d_pt_off, off.data(), off.size());
  if (!st) st = h2d(ctx, bs->d_cam, cam_ids, (size_t)n_obs);
  if (!st) st = h2d(ctx, bs->d_obs_pt, obs_pt.data(), obs_pt.size());
  if (!st) st = h2d(ctx, bs->d_s, s.data(), s.size());
  if (!st) st = h2d(ctx, bs->d_X, points, (size_t)n_points * 3);
  if (!st) st = h2d(ctx, bs->d_Xc, points, (size_t)n_points * 3);
  if (!st) st = h2d(ctx, bs->d_adj_off, adj_off.data(), adj_off.size());
  if (!st) st = h2d(ctx, bs->d_adj_cam, adj_cam.data(), adj_cam.size());
  if (!st) st = h2d(ctx, bs->d_adj_slot, adj_slot.data(), adj_slot.size());
  if (!st && hipStreamSynchronize(ctx->stream) != hipSuccess) { PVLM_SET_ERR(ctx, "reprojection set upload failed"); st = PVLM_ERR_HIP; }
  bs->h_cpl.clear(); bs->h_cpl.shrink_to_fit();
  if (st) { ba_free(ctx, bs); return st; }
  *out = bs;
  return PVLM_OK;
}

pvlm_status pvlm_ba_create(pvlm_ctx* ctx, int n_points, int64_t n_obs, const int64_t* point_offsets, const int* cam_ids, const double* bearings,
                           const double* points, double weight, pvlm_baset** out) {
  return pvlm_ba_create_kind(ctx, PVLM_BA_ANGLE1, 0, 0, n_points, n_obs, point_offsets, cam_ids, bearings, points, weight, out);
}

pvlm_status pvlm_ba_info(const pvlm_baset* set, pvlm_ba_kind* kind, int* rows, int* cols, int* rows_per_obs) {
  if (!set) return PVLM_ERR_ARG;
  if (kind) *kind = (pvlm_ba_kind)set->kind;
  if (rows) *rows = (int)set->geo.rows;
  if (cols) *cols = (int)set->geo.cols;
  if (rows_per_obs) *rows_per_obs = set->kind == PVLM_BA_ANGLE1 ? 1 : 2;
  return PVLM_OK;
}

pvlm_status pvlm_ba_destroy(pvlm_ctx* ctx, pvlm_baset* set) {
  if (!ctx || !set) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  hipStreamSynchronize(ctx->stream);
  return ba_free(ctx, set);
}

pvlm_status pvlm_ba_structure(const pvlm_baset* set, int* n_points, int64_t* n_obs, int* n_cams, int* n_upairs, int* ui, int* uj) {
  if (!set) return PVLM_ERR_ARG;
  if (n_points) *n_points = set->n_points;
  if (n_obs) *n_obs = set->n_obs;
  if (n_cams) *n_cams = set->n_cams;
  if (n_upairs) *n_upairs = set->n_upairs;
  if (ui) std::copy(set->ui.begin(), set->ui.end(), ui);
  if (uj) std::copy(set->uj.begin(), set->uj.end(), uj);
  return PVLM_OK;
}

int64_t pvlm_ba_packed_size(const pvlm_baset* set) { return set ? (int64_t)pvlm_ba::packed_size(set->n_cams, set->n_upairs) : 0; }

pvlm_status pvlm_ba_get_points(pvlm_ctx* ctx, const pvlm_baset* set, int candidate, double* points) {
  if (!ctx || !set || !points) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (set->n_points) { const pvlm_status st = pvlm_i_d2h_q(ctx, points, candidate ? set->d_Xc : set->d_X, (size_t)set->n_points * 24); if (st) return st; }
  return pvlm_i_sync(ctx);
}

pvlm_status pvlm_ba_set_points(pvlm_ctx* ctx, pvlm_baset* set, const double* points) {
  if (!ctx || !set || !points) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_status st = h2d(ctx, set->d_X, points, (size_t)set->n_points * 3);
  if (st) return st;
  PVLM_TRY_SYNC(ctx);
  set->reduced = false; set->have_candidate = false;
  return PVLM_OK;
}

pvlm_status pvlm_ba_set_constant(pvlm_ctx* ctx, pvlm_baset* set, const unsigned char* mask) {
  if (!ctx || !set) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  PVLM_TRY_SYNC(ctx);
  if (!mask) { pvlm_i_free(ctx, set->d_frozen); set->d_frozen = nullptr; }
  else {
    pvlm_status st;
    if (!set->d_frozen && (st = pvlm_i_alloc(ctx, &set->d_frozen, (size_t)set->n_points))) return st;
    if ((st = h2d(ctx, set->d_frozen, mask, (size_t)set->n_points))) return st;
    PVLM_TRY_SYNC(ctx);
  }
  set->reduced = false;
  return PVLM_OK;
}

pvlm_status pvlm_ba_eval(pvlm_ctx* ctx, const pvlm_baset* set, double* r, double* J) {
  if (!ctx || !set || !r) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_status st = ba_ready(ctx, set);
  if (st) return st;
  if (set->n_obs == 0) return PVLM_OK;
  const size_t nr = (size_t)set->n_obs * (set->kind == PVLM_BA_ANGLE1 ? 1 : 2);    // residual rows
  double *d_r = nullptr, *d_J = nullptr;
  if ((st = pvlm_i_alloc(ctx, &d_r, nr))) return st;
  if (J && (st = pvlm_i_alloc(ctx, &d_J, nr * 9))) { pvlm_i_free(ctx, d_r); return st; }
  const pvlm_ba::View v = make_view(set, 0, 0.0);
  if (set->kind == PVLM_BA_ANGLE1)
    hipLaunchKernelGGL(k_ba_eval, dim3((unsigned)((set->n_obs + 255) / 256)), dim3(256), 0, ctx->stream, v, ctx->d_pose_tab, d_r, d_J);
  else
    BA2_LAUNCH(set, k_ba2_eval, dim3((unsigned)((set->n_obs + 255) / 256)), dim3(256), v, set->geo, ctx->d_pose_tab, d_r, d_J);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_ba_eval: %s", hipGetErrorString(e)); st = PVLM_ERR_HIP; }
  if (!st) st = pvlm_i_d2h_q(ctx, r, d_r, nr * 8);
  if (!st && J) st = pvlm_i_d2h_q(ctx, J, d_J, nr * 72);
  { const pvlm_status s2 = pvlm_i_sync(ctx); if (!st) st = s2; }
  pvlm_i_free(ctx, d_r); pvlm_i_free(ctx, d_J);
  return st;
}

pvlm_status pvlm_ba_reduce(pvlm_ctx* ctx, pvlm_baset* set, pvlm_loss loss, double a, int init_scale, double radius, double min_diag,
                           double max_diag, double* packed) {
  if (!ctx || !set || !packed || !(radius > 0.0)) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_status st = ba_ready(ctx, set);
  if (st) return st;
  if (!init_scale && !set->scaled) { PVLM_SET_ERR(ctx, "pvlm_ba_reduce: the first call must initialise the point scaling (init_scale = 1)"); return PVLM_ERR_STATE; }
  const size_t psz = (size_t)pvlm_ba::packed_size(set->n_cams, set->n_upairs);
  PVLM_HIP(ctx, hipMemsetAsync(set->d_packed, 0, psz * 8, ctx->stream));
  const pvlm_ba::View v = make_view(set, (int)loss, a);
  double* d_cost = set->d_packed + (size_t)set->n_cams * 42 + (size_t)set->n_upairs * 36;
  double* d_gmax = set->d_packed + psz - 1;
  const bool two = set->kind != PVLM_BA_ANGLE1;
  if (set->n_points) {
    if (two)
      BA2_LAUNCH(set, k_ba2_points, dim3((unsigned)((set->n_points + 127) / 128)), dim3(128), v, set->geo, ctx->d_pose_tab, init_scale, radius,
                 min_diag, max_diag, d_gmax);
    else
      hipLaunchKernelGGL(k_ba_points, dim3((unsigned)((set->n_points + 127) / 128)), dim3(128), 0, ctx->stream, v, ctx->d_pose_tab, init_scale, radius,
                         min_diag, max_diag, d_gmax);
    PVLM_HIP(ctx, hipGetLastError());
  }
  {
#if PVLM_MEASURED_VARIANTS
    static const bool scatter = getenv("PVLM_BA_ATOMICS") != nullptr;   // round 1's scatter with fp64 atomics (k_ba_obs)
    if (scatter && !two) {
      if (set->n_obs) hipLaunchKernelGGL(k_ba_obs, dim3((unsigned)((set->n_obs + 127) / 128)), dim3(128), 0, ctx->stream, v, ctx->d_pose_tab, set->d_packed, d_cost);
    } else
#endif
    {
      const int n_slots = set->n_cams + set->n_upairs;
      if (n_slots && two)
        BA2_LAUNCH(set, k_ba2_blocks, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), v, set->geo, ctx->d_pose_tab, set->d_cpl_off, set->d_cpl, set->d_packed,
                   set->d_cost_cam);
      else if (n_slots) hipLaunchKernelGGL(k_ba_blocks, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, ctx->stream, v, ctx->d_pose_tab, set->d_cpl_off, set->d_cpl, set->d_packed,
                                      set->d_cost_cam);
      hipLaunchKernelGGL(k_ba_cost_sum, dim3(1), dim3(64), 0, ctx->stream, set->n_cams, set->d_cost_cam, d_cost);
    }
    PVLM_HIP(ctx, hipGetLastError());
  }
  if ((st = pvlm_i_d2h(ctx, packed, set->d_packed, psz * 8))) return st;      // 1.2 MB at Room scale, every LM step: pinned arena, not a pageable copy
  if (init_scale) set->scaled = true;
  set->reduced = true; set->reduced_epoch = ctx->pose_epoch;
  set->reduced_poses_known = ctx->host_poses_known;
  if (ctx->host_poses_known) set->reduced_poses = ctx->host_poses;
  return PVLM_OK;
}

pvlm_status pvlm_ba_step(pvlm_ctx* ctx, pvlm_baset* set, pvlm_loss loss, double a, const double* dcam, double* out3) {
  if (!ctx || !set || !dcam || !out3) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_status st = ba_ready(ctx, set);
  if (st) return st;
  // the same poses: no pvlm_set_poses since the reduce, or the same values set again from host memory (a caller with several sets
  // reloads each set's poses before its step)
  const bool same_poses = set->reduced_epoch == ctx->pose_epoch ||
                          (set->reduced_poses_known && ctx->host_poses_known && set->reduced_poses == ctx->host_poses);
  if (!set->reduced || !same_poses) {
    PVLM_SET_ERR(ctx, "pvlm_ba_step needs pvlm_ba_reduce at the same camera poses and points first");
    return PVLM_ERR_STATE;
  }
  if ((st = h2d(ctx, set->d_dcam, dcam, (size_t)set->n_cams * 6))) return st;
  PVLM_HIP(ctx, hipMemsetAsync(set->d_small, 0, 32, ctx->stream));
  const pvlm_ba::View v = make_view(set, (int)loss, a);
  if (set->n_points) {
    const int nb = (set->n_points + 127) / 128;
    if (set->kind != PVLM_BA_ANGLE1) BA2_LAUNCH(set, k_ba2_step, dim3((unsigned)nb), dim3(128), v, set->geo, ctx->d_pose_tab, set->d_dcam, set->d_partials);
    else hipLaunchKernelGGL(k_ba_step, dim3((unsigned)nb), dim3(128), 0, ctx->stream, v, ctx->d_pose_tab, set->d_dcam, set->d_partials);
    hipLaunchKernelGGL(k_ba_sum_partials, dim3(1), dim3(64), 0, ctx->stream, nb, 3, set->d_partials, set->d_small);
    PVLM_HIP(ctx, hipGetLastError());
  }
  if ((st = pvlm_i_d2h(ctx, out3, set->d_small, 24))) return st;
  set->have_candidate = true;
  return PVLM_OK;
}

pvlm_status pvlm_ba_cost(pvlm_ctx* ctx, const pvlm_baset* set, pvlm_loss loss, double a, int candidate, double* cost) {
  if (!ctx || !set || !cost) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_status st = ba_ready(ctx, set);
  if (st) return st;
  if (candidate && !set->have_candidate) { PVLM_SET_ERR(ctx, "pvlm_ba_cost(candidate): no candidate points (call pvlm_ba_step first)"); return PVLM_ERR_STATE; }
  PVLM_HIP(ctx, hipMemsetAsync(set->d_small, 0, 32, ctx->stream));
  const pvlm_ba::View v = make_view(set, (int)loss, a);
  if (set->n_obs) {
    const int nb = (int)((set->n_obs + 255) / 256);
    if (set->kind != PVLM_BA_ANGLE1) BA2_LAUNCH(set, k_ba2_cost, dim3((unsigned)nb), dim3(256), v, set->geo, ctx->d_pose_tab, candidate, set->d_partials);
    else hipLaunchKernelGGL(k_ba_cost, dim3((unsigned)nb), dim3(256), 0, ctx->stream, v, ctx->d_pose_tab, candidate, set->d_partials);
    hipLaunchKernelGGL(k_ba_sum_partials, dim3(1), dim3(64), 0, ctx->stream, nb, 1, set->d_partials, set->d_small);
    PVLM_HIP(ctx, hipGetLastError());
  }
  return pvlm_i_d2h(ctx, cost, set->d_small, 8);
}

pvlm_status pvlm_ba_accept(pvlm_ctx* ctx, pvlm_baset* set) {
  if (!ctx || !set) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (!set->have_candidate) { PVLM_SET_ERR(ctx, "pvlm_ba_accept: no candidate points"); return PVLM_ERR_STATE; }
  std::swap(set->d_X, set->d_Xc);
  set->reduced = false; set->have_candidate = false;
  return PVLM_OK;
}

}  // extern "C"

// pvlm_preload: HIP loads the code object of a translation unit at the first launch of one of its kernels (15 ms for the larger ones) — an empty launch from here
// moves that out of the first call that needs this file's kernels
__global__ void k_preload_ba() {}
void pvlm_i_preload_ba(hipStream_t s) { hipLaunchKernelGGL(k_preload_ba, dim3(1), dim3(1), 0, s); }
