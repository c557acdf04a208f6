// K36: SfM::RefineRelativePose (sfm/SfM.cpp:482-485, SfMLocalBA util/Optimization.cpp:84-170) for a whole pair list, on the definition of pvlm_relpose_core.h.
//
// The unit of parallelism is the PAIR: k_relpose runs pvlm_relpose::refine_pair with one workgroup of ONE wave (kLanes = 64) per pair, the pair's points strided
// over the lanes, the whole Levenberg-Marquardt loop inside the kernel.  A lane only ever reads and writes the scratch of its own points, the sums over the points
// are the xor butterfly of the wave (the tree the header fixes), and the 6 x 6 solve and the accept / reject decision are computed by every lane from the same
// reduced numbers: they are uniform without a broadcast, a barrier or a byte of LDS beyond the three pose tables.  A workgroup never waits for another one; every
// loop is bounded by N or by max_num_iterations.  Per-point state (X, the candidate, the Jacobi scale, Vinv, g_p: 144 B per inlier) lives in a global scratch
// sized by the batch's inlier total, component-major so that the lanes of a trip read neighbouring doubles.
// The host side gathers the observations (two keypoints per inlier through the match records, pvlm_relpose::make_obs) while it validates the indices, so the kernel
// indexes nothing but [pair base + i], i < n.  Vector stores and plain C++ only.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_relpose_core.h"

namespace {

namespace rp = pvlm_relpose;

constexpr int kBatchPairs = 1 << 14;
constexpr long long kBatchPoints = 1ll << 21;        // 2 M inliers: 302 MB of scratch, 64 MB of observations

struct PairDesc { long long pt0; int n, kind; double rows1, cols1, rows2, cols2; };

struct WaveTeam {
  double* mem;
  template <class F> __device__ __forceinline__ void lanes(int n_sum, int n_max, double* out, F&& f) {
    double part[rp::kLinAll];
    const int nv = n_sum + n_max;
#pragma unroll
    for (int k = 0; k < rp::kLinAll; ++k) part[k] = 0.0;
    f((int)threadIdx.x, part);
#pragma unroll
    for (int k = 0; k < rp::kLinAll; ++k) {
      if (k < nv) {
        double v = part[k];
        for (int m = 1; m < rp::kLanes; m <<= 1) { const double o = __shfl_xor(v, m, rp::kLanes); v = k < n_sum ? v + o : fmax(v, o); }
        out[k] = v;
      }
    }
  }
  __device__ __forceinline__ double* shared() { return mem; }
  __device__ __forceinline__ bool leader() const { return threadIdx.x == 0; }
};

__global__ __launch_bounds__(rp::kLanes) void k_relpose(const PairDesc* __restrict__ pairs, int n_pairs, const double* __restrict__ obs, double* __restrict__ scr,
                                                        rp::Options opt, double* __restrict__ R, double* __restrict__ t, double* __restrict__ tri,
                                                        unsigned char* __restrict__ ok, rp::Summary* __restrict__ sums) {
  __shared__ double tabs[rp::kSharedDoubles + 1];
  const int p = (int)blockIdx.x;
  if (p >= n_pairs) return;
  const PairDesc d = pairs[p];
  rp::Pair P;
  P.n = d.n; P.kind = d.kind; P.rows1 = d.rows1; P.cols1 = d.cols1; P.rows2 = d.rows2; P.cols2 = d.cols2;
  P.obs = obs + 4 * (size_t)d.pt0; P.scr = scr + (size_t)rp::kScratchPerPoint * (size_t)d.pt0;
  WaveTeam team{tabs};
  rp::refine_pair(team, P, opt, R + 9 * (size_t)p, t + 3 * (size_t)p, tri + 3 * (size_t)d.pt0, ok + p, sums + p);
}

bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

}  // namespace

extern "C" pvlm_status pvlm_refine_relative_poses(pvlm_ctx* ctx, int n_frames, const float* const* keypoints, const int* rows_kp, const int* img_rows, const int* img_cols,
                                                  int n_pairs, const int* src, const int* tgt, const long long* match_offsets, const pvlm_match* matches,
                                                  const long long* inlier_offsets, const int* inlier_idx, double* R_21, double* t_21, double* triangulated,
                                                  const pvlm_relpose_params* params, unsigned char* ok, pvlm_relpose_summary* summaries) {
  static_assert(sizeof(rp::Summary) == sizeof(pvlm_relpose_summary), "pvlm_relpose_summary is the core's Summary");
  const char* who = "pvlm_refine_relative_poses";
  if (!ctx) return PVLM_ERR_ARG;
  if (n_frames < 0 || n_pairs < 0 || !params || (n_frames > 0 && (!keypoints || !rows_kp || !img_rows || !img_cols)) ||
      (n_pairs > 0 && (!src || !tgt || !match_offsets || !inlier_offsets || !R_21 || !t_21 || !ok))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (params->kind != PVLM_BA_PIXEL && params->kind != PVLM_BA_ANGLE2) { PVLM_SET_ERR(ctx, "%s: kind must be PVLM_BA_PIXEL or PVLM_BA_ANGLE2", who); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0", who); return PVLM_ERR_ARG; }
  if (n_pairs == 0) return PVLM_OK;
  if (match_offsets[0] != 0 || inlier_offsets[0] != 0) { PVLM_SET_ERR(ctx, "%s: offsets must start at 0", who); return PVLM_ERR_ARG; }
  for (int p = 0; p < n_pairs; ++p) {
    if (src[p] < 0 || src[p] >= n_frames || tgt[p] < 0 || tgt[p] >= n_frames) { PVLM_SET_ERR(ctx, "%s: pair %d names a frame that is not there", who, p); return PVLM_ERR_ARG; }
    const long long nm = match_offsets[p + 1] - match_offsets[p], ni = inlier_offsets[p + 1] - inlier_offsets[p];
    if (nm < 0 || ni < 0 || ni > 0x7fffffffll / rp::kScratchPerPoint) { PVLM_SET_ERR(ctx, "%s: offsets of pair %d", who, p); return PVLM_ERR_ARG; }
  }
  const long long total = inlier_offsets[n_pairs];
  if (total > 0 && (!matches || !inlier_idx || !triangulated)) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  // the observations of every inlier, gathered while the indices are checked
  const int kind = (int)params->kind;
  std::vector<double> h_obs(4 * (size_t)total);
  for (int p = 0; p < n_pairs; ++p) {
    const int f1 = src[p], f2 = tgt[p];
    const long long i0 = inlier_offsets[p], i1 = inlier_offsets[p + 1], nm = match_offsets[p + 1] - match_offsets[p];
    if (i1 > i0 && (img_rows[f1] <= 0 || img_cols[f1] <= 0 || img_rows[f2] <= 0 || img_cols[f2] <= 0 || !keypoints[f1] || !keypoints[f2])) {
      PVLM_SET_ERR(ctx, "%s: pair %d names a frame without keypoints or image size", who, p); return PVLM_ERR_ARG;
    }
    for (long long i = i0; i < i1; ++i) {
      const int j = inlier_idx[i];
      if (j < 0 || j >= nm) { PVLM_SET_ERR(ctx, "%s: inlier %lld of pair %d is not a match of the pair", who, i - i0, p); return PVLM_ERR_ARG; }
      const pvlm_match m = matches[match_offsets[p] + j];
      if (m.query < 0 || m.query >= rows_kp[f1] || m.train < 0 || m.train >= rows_kp[f2]) {
        PVLM_SET_ERR(ctx, "%s: match %d of pair %d names a keypoint that is not there", who, j, p); return PVLM_ERR_ARG;
      }
      rp::make_obs(kind, keypoints[f1][2 * (size_t)m.query], keypoints[f1][2 * (size_t)m.query + 1], img_rows[f1], img_cols[f1], &h_obs[4 * (size_t)i]);
      rp::make_obs(kind, keypoints[f2][2 * (size_t)m.train], keypoints[f2][2 * (size_t)m.train + 1], img_rows[f2], img_cols[f2], &h_obs[4 * (size_t)i + 2]);
    }
  }
  if (!finite_all(R_21, 9 * (size_t)n_pairs) || !finite_all(t_21, 3 * (size_t)n_pairs) || !finite_all(triangulated, 3 * (size_t)total) || !finite_all(h_obs.data(), h_obs.size())) {
    PVLM_SET_ERR(ctx, "%s: a pose, a point or a keypoint is not finite", who); return PVLM_ERR_ARG;
  }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const int pair_limit = (int)pvlm_i_env_limit("PVLM_RELPOSE_BATCH_PAIRS", kBatchPairs);
  rp::Options opt;
  opt.max_num_iterations = params->max_num_iterations;
  std::vector<PairDesc> pd;
  std::vector<rp::Summary> h_sum;
  for (int p0 = 0; p0 < n_pairs;) {
    int np = 0; long long pts = 0;
    while (p0 + np < n_pairs && np < pair_limit) {
      const long long ni = inlier_offsets[p0 + np + 1] - inlier_offsets[p0 + np];
      if (np > 0 && pts + ni > kBatchPoints) break;
      pts += ni; ++np;
    }
    const long long base = inlier_offsets[p0];
    pd.resize((size_t)np);
    for (int k = 0; k < np; ++k) {
      const int p = p0 + k;
      pd[(size_t)k] = PairDesc{inlier_offsets[p] - base, (int)(inlier_offsets[p + 1] - inlier_offsets[p]), kind, (double)img_rows[src[p]], (double)img_cols[src[p]],
                               (double)img_rows[tgt[p]], (double)img_cols[tgt[p]]};
    }
    pvlm_call::batch bs(c);                                  // this batch's scratch
    PairDesc* d_pairs = c.upload(pd.data(), (size_t)np);
    double* d_obs = c.upload(h_obs.data() + 4 * (size_t)base, 4 * (size_t)pts);
    double* d_tri = c.upload(triangulated + 3 * (size_t)base, 3 * (size_t)pts);
    double* d_R = c.upload(R_21 + 9 * (size_t)p0, 9 * (size_t)np);
    double* d_t = c.upload(t_21 + 3 * (size_t)p0, 3 * (size_t)np);
    double* d_scr = c.alloc<double>((size_t)rp::kScratchPerPoint * (size_t)pts);
    unsigned char* d_ok = c.alloc<unsigned char>((size_t)np);
    rp::Summary* d_sum = c.alloc<rp::Summary>((size_t)np);
    c.launch(k_relpose, dim3((unsigned)np), dim3(rp::kLanes), 0, d_pairs, np, d_obs, d_scr, opt, d_R, d_t, d_tri, d_ok, d_sum);
    c.check_launches();
    h_sum.resize((size_t)np);
    c.d2h(R_21 + 9 * (size_t)p0, d_R, 9 * (size_t)np * sizeof(double));
    c.d2h(t_21 + 3 * (size_t)p0, d_t, 3 * (size_t)np * sizeof(double));
    c.d2h(triangulated + 3 * (size_t)base, d_tri, 3 * (size_t)pts * sizeof(double));
    c.d2h(ok + p0, d_ok, (size_t)np);
    c.d2h(h_sum.data(), d_sum, (size_t)np * sizeof(rp::Summary));
    if (c.sync()) break;
    if (summaries) std::memcpy(summaries + p0, h_sum.data(), (size_t)np * sizeof(rp::Summary));
    p0 += np;
  }
  return c.st;
}

extern "C" int pvlm_relpose_workgroup_size(void) { return rp::kLanes; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_relpose() {}
void pvlm_i_preload_relpose(hipStream_t s) { hipLaunchKernelGGL(k_preload_relpose, dim3(1), dim3(1), 0, s); }
