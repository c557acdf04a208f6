// K45: RotationAveragingLeastSquare (sfm/RotationAveraging.cpp:185-275), the start of the L2 rotation-averaging method, on the definition of pvlm_rotstart_core.h:
// shift-and-invert subspace iteration of width 3 with Rayleigh-Ritz on the block-sparse M = A^T A, in place of upstream's dense eigen-decomposition.
//
// The fourth consumer of the pair-graph layer; the unit of parallelism is the PAIR for the product M X and the CAMERA for everything else:
//   k_rs_blocks    a lane per block of the solver's list [F diagonal | P off-diagonal]: (deg + sigma) I3 from the CSR row, -R_21^T in the layout of K42's pairs; once a call;
//   k_rs_pair      a lane per pair: the two-sided record of M X, 9 numbers per side;
//   k_rs_gather    the layer's gather skeleton (camera_gather) over the two-sided record: (M X)_c, and by its tail the camera's terms of X^T (M X);
//   k_rs_gram      a lane per camera: its terms of X^T X;
//   k_rs_mul       a lane per camera: X <- X C;
//   k_rs_rotate    a lane per camera: X <- X S, M X <- (M X) S, its terms of |M x_k - theta_k x_k|^2;
//   k_rs_polar     a lane per camera: the polar factor of its block, the sign rule, the product with rot_0^T, the singular flag;
//   k_pg_tree      the layer's fixed reduction tree: the Gram and Rayleigh sums, the residual norms, the maximum of the flags.
// No floating-point atomic, one order per sum.  X, M X and the record stay on the device; per iteration the host reads X (9 per camera) for the three right-hand
// sides of the layer's solve_cameras and sends the three solutions back.  Every loop is bounded by P, F, a CSR row or max_iterations; every index is checked on the
// host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_rotstart_core.h"

namespace {

namespace rs = pvlm_rotstart;

struct Mat3 { double v[9]; };
struct Vec3 { double v[3]; };

__global__ __launch_bounds__(kThreads) void k_rs_blocks(int F, int P, const int* __restrict__ row_off, const double* __restrict__ R21, double sigma,
                                                        double* __restrict__ blocks) {
  const long long n = (long long)F + P;
  for (long long b = (long long)blockIdx.x * kThreads + threadIdx.x; b < n; b += (long long)gridDim.x * kThreads) {
    if (b < F) rs::diag_block((double)(row_off[b + 1] - row_off[b]), sigma, blocks + 36 * b);
    else rs::off_block(R21 + 9 * (b - F), blocks + 36 * b);
  }
}

__global__ __launch_bounds__(kThreads) void k_rs_pair(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R21,
                                                      const double* __restrict__ X, double* __restrict__ rec) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double R[9], xi[9], xj[9];
    const long long i = first[p], j = second[p];
    for (int k = 0; k < 9; ++k) { R[k] = R21[9 * p + k]; xi[k] = X[9 * i + k]; xj[k] = X[9 * j + k]; }
    rs::mx_pair(R, xi, xj, rec + p, P);
  }
}

// MX: 9 per camera; terms: the camera's part of X^T (M X), kSym columns of stride F
__global__ __launch_bounds__(kThreads) void k_rs_gather(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                        const double* __restrict__ X, double* __restrict__ MX, double* __restrict__ terms) {
  camera_gather<rs::kBlock>(F, row_off, [&](int e0, int e1, int lane, double* part) { rs::gather_lane(rec, P, ent, e0, e1, lane, part); },
                            [&](long long c, const double* part) {
                              double x[9];
                              for (int k = 0; k < 9; ++k) { MX[9 * c + k] = part[k]; x[k] = X[9 * c + k]; }
                              rs::sym_terms(x, part, terms + c, F);
                            });
}

__global__ __launch_bounds__(kThreads) void k_rs_gram(int F, const double* __restrict__ X, double* __restrict__ terms) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    double x[9];
    for (int k = 0; k < 9; ++k) x[k] = X[9 * c + k];
    rs::sym_terms(x, x, terms + c, F);
  }
}

__global__ __launch_bounds__(kThreads) void k_rs_mul(int F, Mat3 C, double* __restrict__ X) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    double x[9];
    for (int k = 0; k < 9; ++k) x[k] = X[9 * c + k];
    rs::mul_block(x, C.v);
    for (int k = 0; k < 9; ++k) X[9 * c + k] = x[k];
  }
}

__global__ __launch_bounds__(kThreads) void k_rs_rotate(int F, Mat3 S, Vec3 theta, double* __restrict__ X, double* __restrict__ MX, double* __restrict__ terms) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    double x[9], mx[9];
    for (int k = 0; k < 9; ++k) { x[k] = X[9 * c + k]; mx[k] = MX[9 * c + k]; }
    rs::mul_block(x, S.v); rs::mul_block(mx, S.v);
    for (int k = 0; k < 9; ++k) { X[9 * c + k] = x[k]; MX[9 * c + k] = mx[k]; }
    rs::residual_terms(x, mx, theta.v, terms + c, F);
  }
}

// out: 9 per camera, untouched where the flag is set
__global__ __launch_bounds__(kThreads) void k_rs_polar(int F, const double* __restrict__ X, double* __restrict__ out, double* __restrict__ flags) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    double x[9], x0[9], r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 9; ++k) { x[k] = X[9 * c + k]; x0[k] = X[k]; }
    flags[c] = rs::final_rotation(x, x0, r);
    for (int k = 0; k < 9; ++k) out[9 * c + k] = r[k];
  }
}

// the backend of rs::run: the layer's graph, tree and camera solve; X, M X, the record and the block list are its own
struct DeviceBackend : DeviceGraph {
  pg::CameraSystem sys;
  double *d_X = nullptr, *d_MX = nullptr, *d_rec = nullptr, *d_terms = nullptr, *d_blocks = nullptr, *d_out = nullptr;

  DeviceBackend(pvlm_call& call, int F_, int P_) : DeviceGraph(call, "PVLM_ROTAVG_MAX_BLOCKS", F_, P_) {}

  void setup(const int* first, const int* second, const double* R21) {
    DeviceGraph::setup(first, second, R21, rs::kSym);
    sys.init(F, P, first, second, -1);
    d_X = c.alloc<double>(9 * (size_t)F); d_MX = c.alloc<double>(9 * (size_t)F); d_out = c.alloc<double>(9 * (size_t)F);
    d_rec = c.alloc<double>((size_t)rs::kSlots * (size_t)P); d_terms = c.alloc<double>((size_t)rs::kSym * (size_t)F);
    d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P));
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
  }
  unsigned block_grid() const { return grid_for((long long)F + P, kThreads, blocks_limit); }

  void assemble(double sigma) {
    clock.start();
    c.launch(k_rs_blocks, dim3(block_grid()), dim3(kThreads), 0, F, P, d_off, d_R21, sigma, d_blocks);
    c.check_launches();
    clock.kernels_ms += clock.stop();
  }
  int solve() {
    int info = 0;
    if (failed() || !solve_cameras(c, sys, d_blocks, F + P, clock, &info)) return -1;
    return info;
  }
  void put(const std::vector<double>& x) { c.h2d(d_X, x.data(), x.size() * sizeof(double)); }
  void fetch(std::vector<double>* x) {
    clock.start();
    x->resize(9 * (size_t)F);
    c.d2h(x->data(), d_X, x->size() * sizeof(double));
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  void gram(double* g) {
    clock.start();
    c.launch(k_rs_gram, dim3(camera_grid()), dim3(kThreads), 0, F, d_X, d_terms);
    reduce<false>(d_terms, F, F, rs::kSym, g);
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  void mul(const double* C) {
    Mat3 m;
    std::memcpy(m.v, C, sizeof m.v);
    clock.start();
    c.launch(k_rs_mul, dim3(camera_grid()), dim3(kThreads), 0, F, m, d_X);
    c.check_launches();
    clock.kernels_ms += clock.stop();
  }
  void rayleigh(double* t) {
    clock.start();
    c.launch(k_rs_pair, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_R21, d_X, d_rec);
    c.launch(k_rs_gather, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_rec, d_X, d_MX, d_terms);
    reduce<false>(d_terms, F, F, rs::kSym, t);
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  void rotate(const double* S, const double* theta, double* r2, std::vector<double>* x) {
    Mat3 m; Vec3 th;
    std::memcpy(m.v, S, sizeof m.v); std::memcpy(th.v, theta, sizeof th.v);
    clock.start();
    c.launch(k_rs_rotate, dim3(camera_grid()), dim3(kThreads), 0, F, m, th, d_X, d_MX, d_terms);
    reduce<false>(d_terms, F, F, 3, r2);
    x->resize(9 * (size_t)F);
    c.d2h(x->data(), d_X, x->size() * sizeof(double));
    c.sync();
    clock.kernels_ms += clock.stop();
  }
  double polar(std::vector<double>* out) {
    double bad = 0.0;
    out->assign(9 * (size_t)F, 0.0);
    clock.start();
    c.launch(k_rs_polar, dim3(camera_grid()), dim3(kThreads), 0, F, d_X, d_out, d_terms);
    reduce<true>(d_terms, F, F, 1, &bad);
    c.d2h(out->data(), d_out, out->size() * sizeof(double));
    c.sync();
    clock.kernels_ms += clock.stop();
    return bad;
  }
};

}  // namespace

extern "C" pvlm_status pvlm_rotavg_least_square(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, double* rotations,
                                                const pvlm_rotavg_lsq_params* params, pvlm_rotavg_lsq_summary* summary) {
  static_assert(sizeof(rs::Summary) == sizeof(pvlm_rotavg_lsq_summary), "pvlm_rotavg_lsq_summary is the core's Summary");
  const char* who = "pvlm_rotavg_least_square";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  rs::Params prm;
  prm.shift_rel = params->shift_rel; prm.tol = params->tol; prm.max_iterations = params->max_iterations;
  if (const char* bad = rs::check_args(n_cameras, n_pairs, first, second, R_21, rotations, &prm)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  DeviceBackend be(c, F, P);
  be.setup(first, second, R_21);
  std::vector<double> out;
  rs::Summary s;
  const int inf = rs::run(be, prm, (double)rs::max_degree(F, P, first, second), rotations, &out, &s);
  if (c.sync()) return c.st;
  if (inf == rs::kDeviceError) { PVLM_SET_ERR(ctx, "%s: the device failed", who); return PVLM_ERR_HIP; }
  std::memcpy(summary, &s, sizeof s);
  if (inf == 0) std::memcpy(rotations, out.data(), out.size() * sizeof(double));
  if (std::getenv("PVLM_ROTAVG_PROFILE")) {
    const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count();
    std::fprintf(stderr, "pvlm_rotavg_profile {\"entry\": \"least_square\", \"cameras\": %d, \"pairs\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, "
                 "\"form_g_ms\": 0.000, \"host_ms\": %.3f, \"solves\": %d, \"iterations\": %d}\n", F, P, total, be.clock.kernels_ms, be.clock.solve_ms,
                 total - be.clock.kernels_ms - be.clock.solve_ms, be.clock.solves, s.iterations);
  }
  return PVLM_OK;
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_rotstart() {}
void pvlm_i_preload_rotstart(hipStream_t s) { hipLaunchKernelGGL(k_preload_rotstart, dim3(1), dim3(1), 0, s); }
