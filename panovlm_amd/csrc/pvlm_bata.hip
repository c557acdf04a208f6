// K44: BATA translation averaging (sfm/BATA.cpp:36-237; the wrapper sfm/TranslationAveraging.cpp:483-525 is the host mirror's) on the definition of pvlm_bata_core.h.
//
// Both stages are sequences of re-weighted Laplacian solves over the pair graph (init_iteration * 2 + (outer_iteration - 1) * inner_iteration of them); the unit of
// parallelism is the PAIR for everything that is per pair and the CAMERA for the gather:
//   k_bt_lud       a lane per pair: scale and weight at the current positions (or the start), the record (w, w s tij), the off-diagonal block -2 w I3 straight into
//                  the solver's block list;
//   k_bt_dots      a lane per pair: the pair's terms of c~^T x1 and c~^T x2;
//   k_bt_outer     a lane per pair: the robust weight Wvec of an outer iteration;
//   k_bt_inner     a lane per pair: the bilinear scale, the record (omega, (Wvec / S) tij), the off-diagonal block -omega I3, the not-a-number flag;
//   k_bt_gather    the pair-graph layer's gather skeleton (camera_gather) with the one-sided gather_lane<4> and its sign mask: sum of weights and the signed
//                  right-hand side per camera, the diagonal block written by its tail; k_bt_gather_c the same over the directions (c = At0^T vec(tij), once a call);
//   k_pg_tree      the layer's fixed reduction tree: the sum of the start scales, the two dot products, the maximum of the flags.
// No floating-point atomic of this file's own, one order per sum.  The directions, the scales, Wvec and the records stay on the device for the whole call; per solve
// the host reads the gather (4 numbers per camera), hands the layer's solve_cameras its right-hand side and sends the positions back (3 per camera).  Every loop is
// bounded by P, F, a CSR row or an iteration count of the parameters; every index is checked on the host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_bata_core.h"

namespace {

namespace bt = pvlm_bata;

// dir is component-major: component k of pair p at [k * P + p]
__device__ __forceinline__ void load_pair(long long p, long long P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                          const double* __restrict__ t, double* tij, double* ti, double* tj) {
  const long long i = first[p], j = second[p];
  for (int k = 0; k < 3; ++k) { tij[k] = dir[k * P + p]; ti[k] = t[3 * i + k]; tj[k] = t[3 * j + k]; }
}

__global__ __launch_bounds__(kThreads) void k_bt_lud(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                     const double* __restrict__ t, const double* __restrict__ s0, int first_time, double factor, double delta, int record,
                                                     double* __restrict__ s, double* __restrict__ rec, double* __restrict__ off_blocks) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double tij[3], ti[3], tj[3], sc, w = 1.0;
    load_pair(p, P, first, second, dir, t, tij, ti, tj);
    if (first_time) sc = s0[p] * factor;
    else bt::lud_update(tij, ti, tj, delta, &sc, &w);
    s[p] = sc;
    if (record) bt::lud_record(tij, sc, w, rec + p, P, off_blocks + 36 * p);
  }
}

__global__ __launch_bounds__(kThreads) void k_bt_dots(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                      const double* __restrict__ x1, const double* __restrict__ x2, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double tij[3], a[3], b[3], c[3], d[3];
    load_pair(p, P, first, second, dir, x1, tij, a, b);
    const long long i = first[p], j = second[p];
    for (int k = 0; k < 3; ++k) { c[k] = x2[3 * i + k]; d[k] = x2[3 * j + k]; }
    bt::dots_pair(tij, a, b, c, d, terms + p, P);
  }
}

__global__ __launch_bounds__(kThreads) void k_bt_outer(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                       const double* __restrict__ t, const double* __restrict__ s, double thr, double* __restrict__ wvec) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double tij[3], ti[3], tj[3];
    load_pair(p, P, first, second, dir, t, tij, ti, tj);
    wvec[p] = bt::outer_weight(tij, ti, tj, s[p], thr);
  }
}

__global__ __launch_bounds__(kThreads) void k_bt_inner(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                       const double* __restrict__ t, const double* __restrict__ wvec, double* __restrict__ s, double* __restrict__ rec,
                                                       double* __restrict__ off_blocks, double* __restrict__ flags) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double tij[3], ti[3], tj[3], sc;
    load_pair(p, P, first, second, dir, t, tij, ti, tj);
    flags[p] = bt::inner_record(tij, ti, tj, wvec[p], &sc, rec + p, P, off_blocks + 36 * p);
    s[p] = sc;
  }
}

// cam: kCam per camera (sum of weights, signed sum of the right-hand side vectors); the camera's diagonal block diag_factor * (sum of weights) I3
__global__ __launch_bounds__(kThreads) void k_bt_gather(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                        double diag_factor, double* __restrict__ cam, double* __restrict__ diag_blocks) {
  camera_gather<bt::kCam>(F, row_off, [&](int e0, int e1, int lane, double* part) { pg::gather_lane<bt::kCam>(rec, P, ent, e0, e1, lane, 0, 0xeu, part); },
                          [&](long long c, const double* part) {
                            for (int k = 0; k < bt::kCam; ++k) cam[bt::kCam * c + k] = part[k];
                            for (int k = 0; k < 3; ++k) diag_blocks[36 * c + 7 * k] = diag_factor * part[bt::kW];
                          });
}

// c = At0^T vec(tij): minus the signed gather of the directions
__global__ __launch_bounds__(kThreads) void k_bt_gather_c(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ dir,
                                                          double* __restrict__ cvec) {
  camera_gather<3>(F, row_off, [&](int e0, int e1, int lane, double* part) { pg::gather_lane<3>(dir, P, ent, e0, e1, lane, 0, 0x7u, part); },
                   [&](long long c, const double* part) { for (int k = 0; k < 3; ++k) cvec[3 * c + k] = -part[k]; });
}

// the backend of bt::run: the layer's graph, tree and camera solve; the directions, scales, weights, positions and records are its own
struct DeviceBackend : DeviceGraph {
  bt::Params prm;
  pg::CameraSystem sys;
  double *d_dir = nullptr, *d_s0 = nullptr, *d_s = nullptr, *d_wvec = nullptr, *d_t = nullptr, *d_x2 = nullptr, *d_rec = nullptr, *d_terms = nullptr, *d_cam = nullptr,
         *d_blocks = nullptr, *d_c = nullptr;
  std::vector<double> cam;

  DeviceBackend(pvlm_call& call, const bt::Params& p, int F_, int P_) : DeviceGraph(call, "PVLM_BATA_MAX_BLOCKS", F_, P_), prm(p) {}

  void setup(const int* first, const int* second, const double* dir, const double* scales0) {
    DeviceGraph::setup(first, second, nullptr, 2);
    sys.init(F, P, first, second, 0);
    std::vector<double> cm(3 * (size_t)P);
    for (int p = 0; p < P; ++p) for (int k = 0; k < 3; ++k) cm[(size_t)k * P + p] = dir[3 * (size_t)p + k];
    d_dir = c.upload(cm.data(), cm.size()); d_s0 = c.upload(scales0, (size_t)P);
    d_s = c.alloc<double>((size_t)P); d_wvec = c.alloc<double>((size_t)P); d_t = c.alloc<double>(3 * (size_t)F); d_x2 = c.alloc<double>(3 * (size_t)F);
    d_rec = c.alloc<double>((size_t)bt::kSlots * (size_t)P); d_terms = c.alloc<double>(2 * (size_t)P); d_cam = c.alloc<double>((size_t)bt::kCam * (size_t)F);
    d_c = c.alloc<double>(3 * (size_t)F); d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P));
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
    c.memset(d_t, 0, 3 * (size_t)F * sizeof(double));
    cam.assign((size_t)bt::kCam * (size_t)F, 0.0);
  }
  double* off_blocks() const { return d_blocks + 36 * (size_t)F; }

  double scale_sum() {
    double sum = 0.0;
    clock.start();
    reduce<false>(d_s0, P, P, 1, &sum);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    return bad ? std::nan("") : sum;
  }
  void gather_c(std::vector<double>* cv) {
    cv->assign(3 * (size_t)F, 0.0);
    clock.start();
    c.launch(k_bt_gather_c, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_dir, d_c);
    c.check_launches();
    c.d2h(cv->data(), d_c, cv->size() * sizeof(double));
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  // the gather of the record, its download and the wait
  void gather(double diag_factor) {
    c.launch(k_bt_gather, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_rec, diag_factor, d_cam, d_blocks);
    c.check_launches();
    c.d2h(cam.data(), d_cam, cam.size() * sizeof(double));
    c.sync();
  }
  void lud_pairs(bool first_time, double factor) {
    clock.start();
    c.launch(k_bt_lud, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_dir, d_t, d_s0, first_time ? 1 : 0, factor, prm.delta, 1, d_s, d_rec, off_blocks());
    gather(2.0);
    clock.kernels_ms += clock.stop();
  }
  void lud_scales() {
    clock.start();
    c.launch(k_bt_lud, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_dir, d_t, d_s0, 0, 1.0, prm.delta, 0, d_s, d_rec, off_blocks());
    c.check_launches();
    clock.kernels_ms += clock.stop();
  }
  int solve() {
    int info = 0;
    if (failed() || !solve_cameras(c, sys, d_blocks, F + P, clock, &info)) return -1;
    return info;
  }
  void dots(const std::vector<double>& x1, const std::vector<double>& x2, double* a) {
    clock.start();
    c.h2d(d_t, x1.data(), x1.size() * sizeof(double)); c.h2d(d_x2, x2.data(), x2.size() * sizeof(double));
    c.launch(k_bt_dots, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_dir, d_t, d_x2, d_terms);
    reduce<false>(d_terms, P, P, 2, a);
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  void set_t(const std::vector<double>& x) { c.h2d(d_t, x.data(), x.size() * sizeof(double)); }
  void outer(double thr) {
    clock.start();
    c.launch(k_bt_outer, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_dir, d_t, d_s, thr, d_wvec);
    c.check_launches();
    clock.kernels_ms += clock.stop();
  }
  double inner_pairs() {
    double bad = 0.0;
    clock.start();
    c.launch(k_bt_inner, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_dir, d_t, d_wvec, d_s, d_rec, off_blocks(), d_terms);
    reduce<true>(d_terms, P, P, 1, &bad);          // the staged copy of the root lands at the gather's wait
    gather(1.0);
    clock.kernels_ms += clock.stop();
    return bad;
  }
};

}  // namespace

extern "C" pvlm_status pvlm_transavg_bata(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir, const double* scales0,
                                          const pvlm_bata_params* params, double* centres, double* lud_centres_or_null, double* scales_out_or_null, int* info) {
  const char* who = "pvlm_transavg_bata";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !centres || !info) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  bt::Params prm;
  prm.delta = params->delta; prm.init_iteration = params->init_iteration; prm.inner_iteration = params->inner_iteration; prm.outer_iteration = params->outer_iteration;
  prm.robust_threshold = params->robust_threshold;
  int min_id = 0, F = 0;
  if (const char* bad = bt::check_args(n_cameras, n_pairs, first, second, dir, scales0, &prm, &min_id, &F)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int P = n_pairs;
  if (P == 0) { *info = bt::kInfoNoPairs; return PVLM_OK; }
  std::vector<int> fi((size_t)P), se((size_t)P);
  for (int p = 0; p < P; ++p) { fi[(size_t)p] = first[p] - min_id; se[(size_t)p] = second[p] - min_id; }
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  DeviceBackend be(c, prm, F, P);
  be.setup(fi.data(), se.data(), dir, scales0);
  std::vector<double> lud, out, s_out((size_t)P);
  const int inf = bt::run(be, prm, &lud, &out);
  if (inf == 0 && scales_out_or_null) c.d2h(s_out.data(), be.d_s, s_out.size() * sizeof(double));
  if (c.sync()) return c.st;
  if (inf == bt::kDeviceError) { PVLM_SET_ERR(ctx, "%s: the device failed", who); return PVLM_ERR_HIP; }
  *info = inf;
  if (inf == 0) {
    std::memcpy(centres, out.data(), out.size() * sizeof(double));
    if (lud_centres_or_null) std::memcpy(lud_centres_or_null, lud.data(), lud.size() * sizeof(double));
    if (scales_out_or_null) std::memcpy(scales_out_or_null, s_out.data(), s_out.size() * sizeof(double));
  }
  if (std::getenv("PVLM_BATA_PROFILE")) {
    const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count();
    std::fprintf(stderr, "pvlm_bata_profile {\"cameras\": %d, \"pairs\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, \"host_ms\": %.3f, \"solves\": %d}\n", F, P,
                 total, be.clock.kernels_ms, be.clock.solve_ms, total - be.clock.kernels_ms - be.clock.solve_ms, be.clock.solves);
  }
  return PVLM_OK;
}

extern "C" int pvlm_bata_group_size(void) { return pg::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_bata() {}
void pvlm_i_preload_bata(hipStream_t s) { hipLaunchKernelGGL(k_preload_bata, dim3(1), dim3(1), 0, s); }
