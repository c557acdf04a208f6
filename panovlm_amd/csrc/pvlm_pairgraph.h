// The device half of the pair-graph layer (pvlm_pairgraph_core.h) under K40 (pvlm_rotavg.hip), K42 (pvlm_transavg.hip), K44 (pvlm_bata.hip), K45
// (pvlm_rotstart.hip), K46 (pvlm_transdir.hip) and K47 (pvlm_translp.hip); included after pvlm_internal.h.
//   k_pg_tree       one node level of the fixed reduction tree (kChunk leaves per workgroup, halved in LDS), launched level by level until one number is left;
//   camera_gather   the skeleton of every per-camera gather: kGroup lanes per camera walk its CSR row, an xor butterfly over the group adds the partial sums, lane 0
//                   writes.  The stage gives the lane function and the epilogue;
//   k_pg_gather_lm  the gather of an LM linearisation: the two-sided kCam-number record into the camera's gather and its diagonal block of the solver's list;
//   k_pg_cam_step   a lane per camera: the candidate of a 3-vector per camera and its terms;
//   k_pg_lm_cost, k_pg_lm_pairs, k_pg_lm_step   a lane per pair around the three methods of a pair model (pvlm_pairgraph_core.h, at lm_solve): the cost term, the
//                   linearisation into the pair's record and the solver's block list, the candidate scale and the pair's terms.
// On the host's side: the pair list, its CSR and the tree's partials on the device (DeviceGraph), the call of the library's block-sparse SPD solver (solve_cameras),
// what every LM backend keeps on top of the graph (LmDevice) and the LM backend of a pair model (LmPairDevice), which K40's L2 stage, K42 and K46 instantiate.
// The six includers are separate code objects in one library: everything here sits in an unnamed namespace, so each has its own kernels and host stubs.
// Vector stores and plain C++ only.
#pragma once
#include <chrono>
#include <cmath>
#include <vector>

#include "pvlm_pairgraph_core.h"

namespace {

namespace pg = pvlm_pairgraph;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;           // the kernels stride past kMaxBlocks workgroups

// the xor butterfly of a group of LANES lanes over N numbers: every lane ends with the group's sums
template <int N, int LANES> __device__ __forceinline__ void group_sum(double* part) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double v = part[k];
    for (int m = 1; m < LANES; m <<= 1) v += __shfl_xor(v, m, LANES);
    part[k] = v;
  }
}

// lane_fn(e0, e1, lane, part): the lane's N partial sums over the row ent[e0 .. e1); tail(c, part): what lane 0 of a live camera does with the sums
template <int N, class LaneFn, class Tail> __device__ __forceinline__ void camera_gather(int F, const int* __restrict__ row_off, LaneFn lane_fn, Tail tail) {
  const int lane = (int)threadIdx.x % pg::kGroup, per_block = kThreads / pg::kGroup;
  // the trip count is uniform over the workgroup: every lane of a group takes part in the butterfly, a group past F with an empty row
  for (long long c0 = (long long)blockIdx.x * per_block; c0 < F; c0 += (long long)gridDim.x * per_block) {
    const long long c = c0 + (int)threadIdx.x / pg::kGroup;
    const bool live = c < F;
    double part[N];
    lane_fn(live ? row_off[c] : 0, live ? row_off[c + 1] : 0, lane, part);
    group_sum<N, pg::kGroup>(part);
    if (live && lane == 0) tail(c, part);
  }
}

__global__ __launch_bounds__(kThreads) void k_pg_gather_lm(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                           double* __restrict__ cam, double* __restrict__ diag_blocks) {
  camera_gather<pg::kCam>(F, row_off, [&](int e0, int e1, int lane, double* part) { pg::gather_lane(rec, P, ent, e0, e1, lane, part); },
                          [&](long long c, const double* part) {
                            for (int k = 0; k < pg::kCam; ++k) cam[pg::kCam * c + k] = part[k];
                            pg::diagonal_block(part, diag_blocks + 36 * c);
                          });
}

// out[col * out_stride + b] = the node over in[col * in_stride + b * kChunk ..]
template <bool MAX> __global__ __launch_bounds__(pg::kChunk) void k_pg_tree(const double* __restrict__ in, long long n, long long in_stride, double* __restrict__ out,
                                                                             long long out_stride) {
  __shared__ double buf[pg::kChunk];
  const long long j = (long long)blockIdx.x * pg::kChunk + threadIdx.x;
  buf[threadIdx.x] = j < n ? in[(long long)blockIdx.y * in_stride + j] : 0.0;
  __syncthreads();
  for (int s = pg::kChunk / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) buf[threadIdx.x] = pg::tree_op<MAX>(buf[threadIdx.x], buf[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(long long)blockIdx.y * out_stride + blockIdx.x] = buf[0];
}

// the candidate x + step of every camera's 3-vector and the cameras' terms: [0] = |step|^2, [1] = |x|^2
__global__ __launch_bounds__(kThreads) void k_pg_cam_step(int F, const double* __restrict__ t, const double* __restrict__ step, double* __restrict__ t_cand,
                                                          double* __restrict__ cterms) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    const double x = t[3 * c], y = t[3 * c + 1], z = t[3 * c + 2], dx = step[3 * c], dy = step[3 * c + 1], dz = step[3 * c + 2];
    t_cand[3 * c] = x + dx; t_cand[3 * c + 1] = y + dy; t_cand[3 * c + 2] = z + dz;
    cterms[c] = (dx * dx + dy * dy) + dz * dz; cterms[F + c] = (x * x + y * y) + z * z;
  }
}

// wall clock of the stages of a call, each of which ends in a wait for the stream: `kernels` = the evaluations, gathers, steps and reductions with their copies,
// `solve` = the camera system (plan, assembly, factorisation, substitution), `form_g` = the dense inverse of K40's L1 stage (zero everywhere else).  Every entry
// point prints them as one profile line on stderr when its stage's variable is set — PVLM_ROTAVG_PROFILE (K40, K45), PVLM_TRANSAVG_PROFILE, PVLM_BATA_PROFILE,
// PVLM_TRANSDIR_PROFILE, PVLM_TRANSLP_PROFILE — and the stage's tools/*_bench.py parses that line.
struct StageClock {
  double kernels_ms = 0, solve_ms = 0, form_g_ms = 0; int solves = 0;
  std::chrono::steady_clock::time_point t0;
  void start() { t0 = std::chrono::steady_clock::now(); }
  double stop() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

unsigned grid_for(long long n, int per_block, long long limit) { const long long g = (n + per_block - 1) / per_block; return (unsigned)(g < 1 ? 1 : (g > limit ? limit : g)); }

// the pair list and its CSR on the device, the partials of the reduction tree.  limit_env: the variable that may lower the workgroup limit
struct DeviceGraph {
  pvlm_call& c; int F, P; long long blocks_limit;
  int *d_first = nullptr, *d_second = nullptr, *d_off = nullptr, *d_ent = nullptr;
  double *d_R21 = nullptr, *d_part[2] = {nullptr, nullptr};
  StageClock clock;

  DeviceGraph(pvlm_call& call, const char* limit_env, int F_, int P_) : c(call), F(F_), P(P_) { blocks_limit = pvlm_i_env_limit(limit_env, kMaxBlocks); }
  void setup(const int* first, const int* second, const double* R21, int max_cols) {
    std::vector<int> off, ent;
    pg::build_csr(F, P, first, second, &off, &ent);
    d_first = c.upload(first, (size_t)P); d_second = c.upload(second, (size_t)P);
    d_off = c.upload(off.data(), off.size()); d_ent = c.upload(ent.data(), ent.size());
    d_R21 = R21 ? c.upload(R21, 9 * (size_t)P) : nullptr;        // a stage whose pairs carry no rotation (K44) passes none
    const long long most = P > F ? P : F, stride = (most + pg::kChunk - 1) / pg::kChunk;
    for (int k = 0; k < 2; ++k) d_part[k] = c.alloc<double>((size_t)max_cols * (size_t)stride);
  }
  bool failed() const { return c.st != PVLM_OK; }
  unsigned pair_grid() const { return grid_for(P, kThreads, blocks_limit); }
  unsigned camera_grid() const { return grid_for(F, kThreads, blocks_limit); }
  unsigned group_grid() const { return grid_for(F, kThreads / pg::kGroup, blocks_limit); }
  // the roots of `cols` trees over in[col * in_stride + 0 .. n) land in out[0 .. cols) at the next sync
  template <bool MAX> void reduce(const double* in, long long n, long long in_stride, int cols, double* out) {
    int k = 0;
    for (;;) {
      const long long m = (n + pg::kChunk - 1) / pg::kChunk;
      c.launch(k_pg_tree<MAX>, dim3((unsigned)m, (unsigned)cols), dim3(pg::kChunk), 0, in, n, in_stride, d_part[k], m);
      in = d_part[k]; in_stride = m; n = m; k ^= 1;
      if (m == 1) break;
    }
    c.check_launches();
    c.d2h(out, in, (size_t)cols * sizeof(double));
  }
};

// sys (prepared) through the library's block-sparse SPD solver, the block list factorised in place; the solution replaces sys.rhs.  false: a device error (c.st)
bool solve_cameras(pvlm_call& c, pg::CameraSystem& sys, double* d_blocks, int n_blocks, StageClock& clock, int* info) {
  clock.start();
  const pvlm_status st = pvlm_i_spd_solve_blocks(c.ctx, sys.n, n_blocks, sys.rows.data(), sys.cols.data(), sys.mirror.data(), d_blocks, true, sys.sigma.data(),
                                                 sys.diag.data(), sys.rhs.data(), info);
  clock.solve_ms += clock.stop(); ++clock.solves;
  if (st) c.st = st;
  return !st;
}

// What an LM backend (pg::lm_solve) keeps on top of the graph, whatever its pair model: the camera system and its block list ([F diagonal | P off-diagonal]), the
// gather, the step.
struct LmDevice : DeviceGraph {
  pg::Options opt;
  pg::CameraSystem sys;
  double *d_blocks = nullptr, *d_cam = nullptr, *d_step = nullptr, *d_cterms = nullptr;
  std::vector<double> cam, step;

  LmDevice(pvlm_call& call, const char* limit_env, const pg::Options& o, int F_, int P_) : DeviceGraph(call, limit_env, F_, P_), opt(o) {}
  void setup(const int* first, const int* second, const double* R21, int max_cols, int origin) {
    DeviceGraph::setup(first, second, R21, max_cols);
    sys.init(F, P, first, second, origin);
    d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P)); d_cam = c.alloc<double>((size_t)pg::kCam * (size_t)F);
    d_step = c.alloc<double>(3 * (size_t)F); d_cterms = c.alloc<double>(2 * (size_t)F);
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
    cam.assign((size_t)pg::kCam * (size_t)F, 0.0);
  }
  double* off_blocks() const { return d_blocks + 36 * (size_t)F; }
  // the end of a linearisation: the gather of the pair records, its download and the wait.  false: a device error
  bool gather(const double* d_rec) {
    c.launch(k_pg_gather_lm, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_rec, d_cam, d_blocks);
    c.check_launches();
    c.d2h(cam.data(), d_cam, cam.size() * sizeof(double));
    return c.sync() == PVLM_OK;
  }
  // info of the factorisation in *info_out when given
  bool solve(double radius, bool damped, int* info_out) {
    if (failed()) return false;
    sys.prepare(cam.data(), damped, radius, opt);
    int info = 0;
    if (!solve_cameras(c, sys, d_blocks, F + P, clock, &info)) return false;
    if (info_out) *info_out = info;
    if (info != 0) return false;
    sys.expand(&step);
    c.h2d(d_step, step.data(), step.size() * sizeof(double));
    return !failed();
  }
  // the camera half of a candidate: x_cand = x + step and the cameras' terms, which camera_terms reduces
  void step_cameras(const double* d_x, double* d_x_cand) { c.launch(k_pg_cam_step, dim3(camera_grid()), dim3(kThreads), 0, F, d_x, d_step, d_x_cand, d_cterms); }
  void camera_terms(double* ct) { reduce<false>(d_cterms, F, F, 2, ct); }
};

// The three per-pair kernels of a pair model M (pvlm_pairgraph_core.h, at lm_solve): a lane per pair reads its cameras' vectors by first / second (strided) and, where
// M::kScale, its scale; the record and the terms are component-major, so the lanes of a wave store side by side.  s, sigma, gs_abs and s_cand are null without kScale.
template <class M> __global__ __launch_bounds__(kThreads) void k_pg_lm_cost(M m, int P, const int* __restrict__ first, const int* __restrict__ second,
                                                                            const double* __restrict__ x, const double* __restrict__ s, double a, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double xi[3], xj[3];
    for (int k = 0; k < 3; ++k) { xi[k] = x[3 * (long long)first[p] + k]; xj[k] = x[3 * (long long)second[p] + k]; }
    terms[p] = m.cost(p, xi, xj, pg::pair_scale<M>(s, p), a);
  }
}

template <class M> __global__ __launch_bounds__(kThreads) void k_pg_lm_pairs(M m, int P, const int* __restrict__ first, const int* __restrict__ second,
                                                                             const double* __restrict__ x, const double* __restrict__ s, double a, double radius,
                                                                             double min_diag, double max_diag, int first_time, double* __restrict__ sigma,
                                                                             double* __restrict__ rec, double* __restrict__ off_blocks, double* __restrict__ gs_abs) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double xi[3], xj[3];
    for (int k = 0; k < 3; ++k) { xi[k] = x[3 * (long long)first[p] + k]; xj[k] = x[3 * (long long)second[p] + k]; }
    m.linearise(p, xi, xj, pg::pair_scale<M>(s, p), a, radius, min_diag, max_diag, first_time != 0, pg::pair_slot<M>(sigma, p), rec + p, P, off_blocks + 36 * p);
    if constexpr (M::kScale) gs_abs[p] = fabs(rec[(long long)M::kGs * P + p]);
  }
}

template <class M> __global__ __launch_bounds__(kThreads) void k_pg_lm_step(M m, int P, const int* __restrict__ first, const int* __restrict__ second,
                                                                            const double* __restrict__ rec, const double* __restrict__ step,
                                                                            const double* __restrict__ x_cand, const double* __restrict__ s, double a,
                                                                            double* __restrict__ s_cand, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    const long long i = first[p], j = second[p];
    double di[3], dj[3], ci[3], cj[3], sc = 0.0;
    for (int k = 0; k < 3; ++k) { di[k] = step[3 * i + k]; dj[k] = step[3 * j + k]; ci[k] = x_cand[3 * i + k]; cj[k] = x_cand[3 * j + k]; }
    m.step(p, rec + p, P, di, dj, ci, cj, pg::pair_scale<M>(s, p), a, M::kScale ? &sc : nullptr, terms + p, P);
    if constexpr (M::kScale) s_cand[p] = sc;
  }
}

// The LM backend of a pair model M.  The state (x: 3 numbers per camera; where M::kScale, s and the Jacobi scale sigma: one per pair), its candidate and the pair
// records stay on the device for the whole call; per iteration the host reads the gather, hands the solver its right-hand side and LM diagonal, sends the camera step
// back and reads the roots of the terms.  limit_env: the stage's PVLM_*_MAX_BLOCKS.  After setup() the stage sets `model` (its inputs uploaded through c; d_R21 is the
// graph's) and may clear `damped`: no LM diagonal and no Jacobi scaling of the cameras, one plain solve of the linearisation (K42's DLT).
template <class M> struct LmPairDevice : LmDevice {
  M model{};
  bool damped = true;
  double *d_x[2] = {nullptr, nullptr}, *d_s[2] = {nullptr, nullptr}, *d_sigma = nullptr, *d_gs = nullptr, *d_rec = nullptr, *d_terms = nullptr;
  int cur = 0;

  LmPairDevice(pvlm_call& call, const char* limit_env, const pg::Options& o, int F_, int P_) : LmDevice(call, limit_env, o, F_, P_) {}

  // x0: 3 F; s0: P where M::kScale, else unread; R21: see DeviceGraph
  void setup(const int* first, const int* second, const double* R21, const double* x0, const double* s0, int origin) {
    LmDevice::setup(first, second, R21, M::kTerms, origin);
    d_x[0] = c.upload(x0, 3 * (size_t)F); d_x[1] = c.alloc<double>(3 * (size_t)F);
    if constexpr (M::kScale) {
      d_s[0] = c.upload(s0, (size_t)P); d_s[1] = c.alloc<double>((size_t)P);
      d_sigma = c.alloc<double>((size_t)P); d_gs = c.alloc<double>((size_t)P);
    }
    d_rec = c.alloc<double>((size_t)M::kSlots * (size_t)P); d_terms = c.alloc<double>((size_t)M::kTerms * (size_t)P);
  }
  // the current state, for the entry point's download
  const double* x() const { return d_x[cur]; }
  const double* s() const { return d_s[cur]; }

  double initial_cost() {
    double cost = 0.0;
    clock.start();
    c.launch(k_pg_lm_cost<M>, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_x[cur], d_s[cur], opt.loss_a, d_terms);
    reduce<false>(d_terms, P, P, 1, &cost);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    return bad ? std::nan("") : cost;
  }
  double linearise(double radius, bool first) {
    double gs_max = 0.0;
    clock.start();
    c.launch(k_pg_lm_pairs<M>, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_x[cur], d_s[cur], opt.loss_a, radius, opt.min_lm_diagonal,
             opt.max_lm_diagonal, first ? 1 : 0, d_sigma, d_rec, off_blocks(), d_gs);
    if constexpr (M::kScale) reduce<true>(d_gs, P, P, 1, &gs_max);
    const bool ok = gather(d_rec);
    clock.kernels_ms += clock.stop();
    if (!ok) return 0.0;
    if (first && damped) sys.set_sigma(cam.data());
    const double g_max = sys.gradient_max(cam.data());
    return M::kScale ? std::fmax(gs_max, g_max) : g_max;
  }
  bool solve(double radius, int* info_out = nullptr) { return LmDevice::solve(radius, damped, info_out); }
  pg::Scalars candidate() {
    double pt[4] = {0, 0, 0, 0}, ct[2] = {0, 0};
    clock.start();
    step_cameras(d_x[cur], d_x[cur ^ 1]);
    c.launch(k_pg_lm_step<M>, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_rec, d_step, d_x[cur ^ 1], d_s[cur], opt.loss_a, d_s[cur ^ 1], d_terms);
    reduce<false>(d_terms, P, P, M::kTerms, pt);          // the staged copy of the roots is ordered on the stream before the next tree reuses the partials
    camera_terms(ct);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return pg::Scalars{std::nan(""), 0, 0, 0};
    if constexpr (M::kScale) return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], pt[pg::kTermStep2] + ct[0], pt[pg::kTermX2] + ct[1]};
    else return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], ct[0], ct[1]};
  }
  void accept() { cur ^= 1; }
};

}  // namespace
