// K39: SfM::SetTranslationScaleDepthMap(eq, pair) (sfm/SfM.cpp:487-603) for a whole pair list, on the depth maps of a pvlm_depthset, on the definition of
// pvlm_scale_core.h.
//
// The unit of parallelism is the PAIR, as in K36: k_scale runs pvlm_scale::scale_pair with one workgroup of ONE wave (kLanes = 64) per pair, the pair's points
// strided over the lanes.  A trip's survivors are placed behind a running count by ballot and popcount (point order kept); the two lists of a pair (current,
// preserved: 2 x 16 B per point) live in a global scratch sized by the batch's point total -- a pair has a median of 210 points but no upper bound, so neither
// registers nor LDS can hold them --, written by the lanes of the wave and read back by them behind a workgroup barrier (one wave: a wait for its own stores).
// Minimum and maximum are the wave butterfly, the histogram is ten ballots per trip, the mean is added in list order by every lane alike from values handed round
// the wave, the median is found by counting ranks.  Every decision is taken by every lane from the same numbers: uniform control flow without a broadcast.  A
// workgroup never waits for another one; every loop is bounded by the pair's point count.  Vector stores and plain C++ only.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_depthset.h"
#include "pvlm_internal.h"
#include "pvlm_scale_core.h"

namespace {

namespace sc = pvlm_scale;

constexpr int kBatchPairs = 1 << 14;
constexpr long long kBatchPoints = 1ll << 21;        // 2 M points: 64 MB of lists, 48 MB of points

struct PairDesc { long long pt0; int n, f1, f2, rows1; };
struct PairOut { double upper, lower; int ok, maps, exit, points_with_depth, consistent, pad; };

struct WaveTeam {
  double r[2]; int ir;
  template <class F> __device__ __forceinline__ unsigned long long vote(F&& f) { return __ballot(f((int)threadIdx.x) ? 1 : 0); }
  template <class F> __device__ __forceinline__ void each(F&& f) { f((int)threadIdx.x); }
  template <class F> __device__ __forceinline__ void minmax(double* mn, double* mx, F&& f) {
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    f((int)threadIdx.x, lo, hi);
    for (int m = 1; m < sc::kLanes; m <<= 1) {
      const double a = __shfl_xor(lo, m, sc::kLanes), b = __shfl_xor(hi, m, sc::kLanes);
      lo = a < lo ? a : lo; hi = b > hi ? b : hi;
    }
    *mn = lo; *mx = hi;
  }
  __device__ __forceinline__ double* regs(int) { return r; }
  __device__ __forceinline__ int* ireg(int) { return &ir; }
  // every lane adds the same values in the same order: a trip of 64 loaded side by side, then handed round lane by lane
  __device__ __forceinline__ double ordered_sum(const double* v, int m) {
    double s = 0.0;
    for (int base = 0; base < m; base += sc::kLanes) {
      const int j = base + (int)threadIdx.x, cnt = m - base < sc::kLanes ? m - base : sc::kLanes;
      const double x = j < m ? v[j] : 0.0;
      for (int l = 0; l < cnt; ++l) s += __shfl(x, l, sc::kLanes);
    }
    return s;
  }
  __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(sc::kLanes) void k_scale(const PairDesc* __restrict__ pairs, int n_pairs, const sc::Map* __restrict__ maps, int eq_rows, int eq_cols,
                                                      const double* __restrict__ R, double* __restrict__ t, double* __restrict__ tri, double* __restrict__ lists,
                                                      PairOut* __restrict__ out) {
  const int p = (int)blockIdx.x;
  if (p >= n_pairs) return;
  const PairDesc d = pairs[p];
  sc::Pair P;
  P.n = d.n; P.eq_rows = eq_rows; P.eq_cols = eq_cols; P.rows1 = d.rows1;
  P.d1 = maps[d.f1]; P.d2 = maps[d.f2];
  P.cur = lists + 4 * (size_t)d.pt0; P.keep = P.cur + 2 * (size_t)d.n;
  WaveTeam team;
  sc::Result res;
  sc::scale_pair(team, P, R + 9 * (size_t)p, t + 3 * (size_t)p, tri + 3 * (size_t)d.pt0, &res);
  if (threadIdx.x == 0) out[p] = PairOut{res.upper, res.lower, res.ok, res.maps, res.exit, res.points_with_depth, res.consistent, 0};
}

bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

}  // namespace

extern "C" pvlm_status pvlm_set_translation_scales(pvlm_ctx* ctx, const pvlm_depthset* set, int eq_rows, int eq_cols, const int* frame_rows, int n_pairs, const int* src,
                                                   const int* tgt, const long long* point_offsets, const double* R_21, double* t_21, double* triangulated, unsigned char* ok,
                                                   int* points_with_depth, double* upper_scale, double* lower_scale, pvlm_scale_stats* stats) {
  const char* who = "pvlm_set_translation_scales";
  if (!ctx) return PVLM_ERR_ARG;
  if (!set) { PVLM_SET_ERR(ctx, "%s: null set", who); return PVLM_ERR_ARG; }
  if (set->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the set belongs to another context", who); return PVLM_ERR_ARG; }
  if (eq_rows <= 0 || eq_cols <= 0 || n_pairs < 0) { PVLM_SET_ERR(ctx, "%s: eq_rows, eq_cols or n_pairs", who); return PVLM_ERR_ARG; }
  if ((set->n_frames > 0 && !frame_rows) ||
      (n_pairs > 0 && (!src || !tgt || !point_offsets || !R_21 || !t_21 || !ok || !points_with_depth || !upper_scale || !lower_scale))) {
    PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG;
  }
  if (stats) *stats = pvlm_scale_stats{0, 0, 0, 0, 0, 0};
  if (n_pairs == 0) return PVLM_OK;
  if (point_offsets[0] != 0) { PVLM_SET_ERR(ctx, "%s: point_offsets must start at 0", who); return PVLM_ERR_ARG; }
  for (int p = 0; p < n_pairs; ++p) {
    if (src[p] < 0 || src[p] >= set->n_frames || tgt[p] < 0 || tgt[p] >= set->n_frames) { PVLM_SET_ERR(ctx, "%s: pair %d names a frame that is not in the set", who, p); return PVLM_ERR_ARG; }
    const long long n = point_offsets[p + 1] - point_offsets[p];
    if (n < 0 || n > 0x7fffffffll / 4) { PVLM_SET_ERR(ctx, "%s: point_offsets of pair %d", who, p); return PVLM_ERR_ARG; }
  }
  const long long total = point_offsets[n_pairs];
  if (total > 0 && !triangulated) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (!finite_all(R_21, 9 * (size_t)n_pairs) || !finite_all(t_21, 3 * (size_t)n_pairs) || !finite_all(triangulated, 3 * (size_t)total)) {
    PVLM_SET_ERR(ctx, "%s: a pose or a point is not finite", who); return PVLM_ERR_ARG;
  }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const int pair_limit = (int)pvlm_i_env_limit("PVLM_SCALE_BATCH_PAIRS", kBatchPairs);
  std::vector<sc::Map> h_maps((size_t)set->n_frames);
  for (int f = 0; f < set->n_frames; ++f) h_maps[(size_t)f] = sc::Map{set->d_map[(size_t)f], set->rows[(size_t)f], set->cols[(size_t)f]};
  sc::Map* d_maps = c.upload(h_maps.data(), h_maps.size());
  std::vector<PairDesc> pd;
  std::vector<PairOut> h_out;
  for (int p0 = 0; p0 < n_pairs;) {
    int np = 0; long long pts = 0;
    while (p0 + np < n_pairs && np < pair_limit) {
      const long long n = point_offsets[p0 + np + 1] - point_offsets[p0 + np];
      if (np > 0 && pts + n > kBatchPoints) break;
      pts += n; ++np;
    }
    const long long base = point_offsets[p0];
    pd.resize((size_t)np);
    for (int k = 0; k < np; ++k) {
      const int p = p0 + k;
      pd[(size_t)k] = PairDesc{point_offsets[p] - base, (int)(point_offsets[p + 1] - point_offsets[p]), src[p], tgt[p], frame_rows[src[p]]};
    }
    pvlm_call::batch bs(c);                                  // this batch's scratch
    PairDesc* d_pairs = c.upload(pd.data(), (size_t)np);
    double* d_tri = c.upload(triangulated + 3 * (size_t)base, 3 * (size_t)pts);
    double* d_R = c.upload(R_21 + 9 * (size_t)p0, 9 * (size_t)np);
    double* d_t = c.upload(t_21 + 3 * (size_t)p0, 3 * (size_t)np);
    double* d_lists = c.alloc<double>(4 * (size_t)pts);
    PairOut* d_out = c.alloc<PairOut>((size_t)np);
    c.launch(k_scale, dim3((unsigned)np), dim3(sc::kLanes), 0, d_pairs, np, d_maps, eq_rows, eq_cols, d_R, d_t, d_tri, d_lists, d_out);
    c.check_launches();
    h_out.resize((size_t)np);
    c.d2h(t_21 + 3 * (size_t)p0, d_t, 3 * (size_t)np * sizeof(double));
    c.d2h(triangulated + 3 * (size_t)base, d_tri, 3 * (size_t)pts * sizeof(double));
    c.d2h(h_out.data(), d_out, (size_t)np * sizeof(PairOut));
    if (c.sync()) break;
    for (int k = 0; k < np; ++k) {
      const PairOut& o = h_out[(size_t)k];
      const int p = p0 + k;
      ok[p] = o.ok ? 1 : 0;
      if (o.maps) points_with_depth[p] = o.points_with_depth;
      if (o.ok) { upper_scale[p] = o.upper; lower_scale[p] = o.lower; }
      if (stats) {
        stats->pairs_mean += o.exit == sc::kExitMean; stats->pairs_median += o.exit == sc::kExitMedian; stats->pairs_unscaled += o.exit == sc::kExitNone;
        if (o.maps) stats->points_tested += pd[(size_t)k].n;
        stats->points_scaled += o.consistent;
      }
    }
    if (stats) stats->batches += 1;
    p0 += np;
  }
  return c.st;
}

extern "C" int pvlm_scale_workgroup_size(void) { return sc::kLanes; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_scale() {}
void pvlm_i_preload_scale(hipStream_t s) { hipLaunchKernelGGL(k_preload_scale, dim3(1), dim3(1), 0, s); }
