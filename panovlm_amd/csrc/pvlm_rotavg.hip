// K40: rotation averaging (RotationAveragingRefineL1 and RotationAveragingL2, sfm/RotationAveraging.cpp:317-374, :428-582) on the definition of pvlm_rotavg_core.h.
//
// The unit of parallelism is the PAIR for everything that is per pair, the CAMERA for the gathers and the ROW of G for the dense product:
//   k_ra_begin       a lane per pair: the pair error b, z = u = 0, w = b, |b|^2;
//   k_ra_gather_admm kGroup lanes per camera walk its CSR row (entry = 2 * pair + side, pair-list order) over w, z+ - z and u with the sign of the incidence, an xor
//                    butterfly adds the partial sums: the camera's right-hand side g = A^T (b + z - u) and its terms |A^T (z+ - z)|^2, |A^T u|^2.  No atomics;
//   k_ra_product     X = G g, three columns: one wave per row of G, lane l takes the columns l, l + kTile, ..., an xor butterfly over the wave.  G is read once per
//                    ADMM iteration, row by row, each row contiguous: the kernel is bound by that stream (8 (F - 1)^2 bytes);
//   k_ra_admm        a lane per pair: A x, the shrinkage, the u-update, the next w, z+ - z and the pair's three norm terms;
//   k_pg_tree        one node level of the pair-graph layer's fixed reduction tree (pvlm_pairgraph.h: kChunk leaves per workgroup, halved in LDS);
//   k_ra_update      a lane per camera: R <- R exp(x);
//   k_ra_irls        a lane per pair: b, the weights |A x_prev - b|^-1.5, weights * b, the off-diagonal block straight into the solver's block list;
//   k_ra_gather_irls the per-camera sums of the weights (the diagonal block) and of the signed weights * b (the right-hand side);
//   k_pg_lm_*        the L2 stage: the layer's LM backend (LmPairDevice of pvlm_pairgraph.h) over the pair model ra::L2Model — per-pair cost, linearisation and
//                    candidate terms, the gather (k_pg_gather_lm), the camera step (k_pg_cam_step) and the camera system.  The two gathers here share its
//                    skeleton (camera_gather).
// The rotations, b, z, u, x and the per-pair records stay on the device for the whole call.  G = (2 L)^-1 is formed ONCE per call by the library's dense SPD solver
// with the identity as right-hand sides (pvlm_spd_solve takes and returns host memory: 2 L goes up and G comes back and is sent up again, once per call).  Per ADMM
// iteration the host reads five scalars and decides convergence — every iteration, so the iterates and the count are those of the definition; per IRLS / LM iteration
// it reads the gather, hands the solver behind the layer's solve_cameras its right-hand side and sends the step back.  Every loop is bounded by P, F, a CSR row or an
// iteration cap; every index is checked on the host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_rotavg_core.h"

namespace {

namespace ra = pvlm_rotavg;

static_assert(ra::kTile == 64, "the dense product gives one wave of 64 lanes to a row");

__device__ __forceinline__ void load9(const double* __restrict__ p, double* v) { for (int k = 0; k < 9; ++k) v[k] = p[k]; }
// the component-major 3 x F table x at camera c
__device__ __forceinline__ void load_x(const double* __restrict__ x, long long F, long long c, double* v) { v[0] = x[c]; v[1] = x[F + c]; v[2] = x[2 * F + c]; }

__global__ __launch_bounds__(kThreads) void k_ra_begin(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R21,
                                                       const double* __restrict__ rot, double* __restrict__ rec, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double R1[9], R2[9], Rp[9], b2;
    load9(rot + 9 * (long long)first[p], R1); load9(rot + 9 * (long long)second[p], R2); load9(R21 + 9 * p, Rp);
    ra::admm_begin_pair(R1, R2, Rp, rec + p, P, &b2);
    terms[p] = b2;
  }
}

// g: component-major 3 x (F - 1) over the rows of G; cterms: [0 .. F) = |A^T (z+ - z)|^2, [F .. 2 F) = |A^T u|^2 per camera
__global__ __launch_bounds__(kThreads) void k_ra_gather_admm(int F, long long P, int start, const int* __restrict__ row_off, const int* __restrict__ ent,
                                                             const double* __restrict__ rec, double* __restrict__ g, double* __restrict__ cterms) {
  camera_gather<9>(F, row_off, [&](int e0, int e1, int lane, double* part) { pg::gather_lane<9>(rec, P, ent, e0, e1, lane, ra::kW, 0x1ffu, part); },
                   [&](long long c, const double* part) {
                     if (c == start) { cterms[c] = 0.0; cterms[F + c] = 0.0; return; }
                     double gc[3], s2, atu2;
                     ra::admm_camera(part, gc, &s2, &atu2);
                     const long long n = F - 1, row = c - (c > start);
                     g[row] = gc[0]; g[n + row] = gc[1]; g[2 * n + row] = gc[2];
                     cterms[c] = s2; cterms[F + c] = atu2;
                   });
}

// X (component-major 3 x F, the camera of row i is i + (i >= start); the entries of start stay zero) = G g
__global__ __launch_bounds__(kThreads) void k_ra_product(int n, int start, const double* __restrict__ G, const double* __restrict__ g, double* __restrict__ X) {
  const int lane = (int)threadIdx.x % ra::kTile, per_block = kThreads / ra::kTile;
  const long long F = (long long)n + 1;
  // the row is uniform over a wave: all its lanes take part in the butterfly, a wave past n with nothing to add
  for (long long i0 = (long long)blockIdx.x * per_block; i0 < n; i0 += (long long)gridDim.x * per_block) {
    const long long i = i0 + (int)threadIdx.x / ra::kTile;
    double acc[3] = {0.0, 0.0, 0.0};
    if (i < n) {
      const double* __restrict__ row = G + i * n;
      for (int j = lane; j < n; j += ra::kTile) { const double a = row[j]; acc[0] += a * g[j]; acc[1] += a * g[(long long)n + j]; acc[2] += a * g[2 * (long long)n + j]; }
    }
    group_sum<3, ra::kTile>(acc);
    if (i < n && lane == 0) { const long long c = i + (i >= start); X[c] = acc[0]; X[F + c] = acc[1]; X[2 * F + c] = acc[2]; }
  }
}

__global__ __launch_bounds__(kThreads) void k_ra_admm(int P, long long F, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ X,
                                                      double* __restrict__ rec, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double xi[3], xj[3];
    load_x(X, F, first[p], xi); load_x(X, F, second[p], xj);
    ra::admm_pair(xi, xj, rec + p, P, terms + p, P);
  }
}

__global__ __launch_bounds__(kThreads) void k_ra_update(int F, int start, const double* __restrict__ x, double* __restrict__ rot) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    if (c == start) continue;
    double R[9], xc[3];
    load9(rot + 9 * c, R); load_x(x, F, c, xc);
    ra::apply_update(R, xc);
    for (int k = 0; k < 9; ++k) rot[9 * c + k] = R[k];
  }
}

__global__ __launch_bounds__(kThreads) void k_ra_irls(int P, long long F, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R21,
                                                      const double* __restrict__ rot, const double* __restrict__ x_prev, double* __restrict__ rec,
                                                      double* __restrict__ off_blocks) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double R1[9], R2[9], Rp[9], xi[3], xj[3];
    load9(rot + 9 * (long long)first[p], R1); load9(rot + 9 * (long long)second[p], R2); load9(R21 + 9 * p, Rp);
    load_x(x_prev, F, first[p], xi); load_x(x_prev, F, second[p], xj);
    ra::irls_pair(R1, R2, Rp, xi, xj, rec + p, P, off_blocks + 36 * p);
  }
}

// cam: 6 per camera (sum of weights 3, signed sum of weights * b 3); the diagonal of the camera's block of A^T W A
__global__ __launch_bounds__(kThreads) void k_ra_gather_irls(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                             double* __restrict__ cam, double* __restrict__ diag_blocks) {
  camera_gather<6>(F, row_off, [&](int e0, int e1, int lane, double* part) { pg::gather_lane<6>(rec, P, ent, e0, e1, lane, ra::kIw, 0x38u, part); },
                   [&](long long c, const double* part) {
                     for (int k = 0; k < 6; ++k) cam[6 * c + k] = part[k];
                     for (int k = 0; k < 3; ++k) diag_blocks[36 * c + 7 * k] = 2.0 * part[k];
                   });
}

struct L1DeviceBackend : DeviceGraph {
  int start, n;
  pg::CameraSystem sys;
  double *d_rot = nullptr, *d_rec = nullptr, *d_G = nullptr, *d_g = nullptr, *d_X = nullptr, *d_terms = nullptr, *d_cterms = nullptr, *d_cam = nullptr, *d_blocks = nullptr,
         *d_xp = nullptr;
  std::vector<double> cam;
  int info_g = 0;

  L1DeviceBackend(pvlm_call& call, int F_, int P_, int start_) : DeviceGraph(call, "PVLM_ROTAVG_MAX_BLOCKS", F_, P_), start(start_), n(F_ - 1) {}

  void setup(const int* first, const int* second, const double* R21, const double* rotations) {
    DeviceGraph::setup(first, second, R21, ra::kL1Terms);
    sys.init(F, P, first, second, start);
    d_rot = c.upload(rotations, 9 * (size_t)F);
    d_rec = c.alloc<double>((size_t)ra::kL1Slots * (size_t)P); d_g = c.alloc<double>(3 * (size_t)n); d_X = c.alloc<double>(3 * (size_t)F); d_xp = c.alloc<double>(3 * (size_t)F);
    d_terms = c.alloc<double>((size_t)ra::kL1Terms * (size_t)P); d_cterms = c.alloc<double>(2 * (size_t)F); d_cam = c.alloc<double>(6 * (size_t)F);
    d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P)); d_G = c.alloc<double>((size_t)n * (size_t)n);
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
    c.memset(d_X, 0, 3 * (size_t)F * sizeof(double));
    cam.assign(6 * (size_t)F, 0.0);
    if (c.sync()) return;
    // G = (2 L)^-1: the library's dense SPD solver with the identity as right-hand sides; G[i * n ..] is the solution for the unit vector e_i
    clock.start();
    std::vector<double> A, G((size_t)n * (size_t)n, 0.0);
    ra::laplacian2(F, P, first, second, start, &A);
    for (int i = 0; i < n; ++i) G[(size_t)i * n + i] = 1.0;
    const pvlm_status st = pvlm_spd_solve(c.ctx, n, n, A.data(), G.data(), &info_g);
    if (st) { c.st = st; return; }
    if (info_g == 0) {
      c.copy_pinned(d_G, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice, c.ctx->stream);      // too large for the staging arena; waited for before G goes
      c.sync();
    }
    clock.form_g_ms = clock.stop();
  }

  void gather_admm() {
    c.launch(k_ra_gather_admm, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, start, d_off, d_ent, d_rec, d_g, d_cterms);
  }
  double admm_begin() {
    double b2 = 0.0;
    clock.start();
    c.launch(k_ra_begin, dim3(pair_grid()), dim3(kThreads), 0, P, d_first, d_second, d_R21, d_rot, d_rec, d_terms);
    gather_admm();
    reduce<false>(d_terms, P, P, 1, &b2);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    return bad ? std::nan("") : b2;
  }
  ra::AdmmNorms admm_iterate() {
    double pt[ra::kL1Terms] = {0, 0, 0}, ct[2] = {0, 0};
    clock.start();
    c.launch(k_ra_product, dim3(grid_for(n, kThreads / ra::kTile, blocks_limit)), dim3(kThreads), 0, n, start, d_G, d_g, d_X);
    c.launch(k_ra_admm, dim3(pair_grid()), dim3(kThreads), 0, P, (long long)F, d_first, d_second, d_X, d_rec, d_terms);
    gather_admm();
    reduce<false>(d_terms, P, P, ra::kL1Terms, pt);          // the staged copy of the roots is ordered on the stream before the next tree reuses the partials
    reduce<false>(d_cterms, F, F, 2, ct);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return ra::AdmmNorms{std::nan(""), 0, 0, 0, 0};
    return ra::AdmmNorms{pt[ra::kTermR2], pt[ra::kTermAx2], pt[ra::kTermZ2], ct[0], ct[1]};
  }
  void fetch_x(std::vector<double>* x) {
    x->assign(3 * (size_t)F, 0.0);
    c.d2h(x->data(), d_X, x->size() * sizeof(double));
    c.sync();
  }
  void apply_x() { c.launch(k_ra_update, dim3(camera_grid()), dim3(kThreads), 0, F, start, d_X, d_rot); c.check_launches(); }
  void apply(const std::vector<double>& x) {
    c.h2d(d_X, x.data(), x.size() * sizeof(double));
    apply_x();
  }
  int irls_solve(const std::vector<double>& x_prev, std::vector<double>* x) {
    clock.start();
    c.h2d(d_xp, x_prev.data(), x_prev.size() * sizeof(double));
    c.launch(k_ra_irls, dim3(pair_grid()), dim3(kThreads), 0, P, (long long)F, d_first, d_second, d_R21, d_rot, d_xp, d_rec, d_blocks + 36 * (size_t)F);
    c.launch(k_ra_gather_irls, dim3(group_grid()), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_rec, d_cam, d_blocks);
    c.check_launches();
    c.d2h(cam.data(), d_cam, cam.size() * sizeof(double));
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return -1;
    if (!ra::irls_prepare(&sys, cam.data())) return sys.n + 1;
    int info = 0;
    if (!solve_cameras(c, sys, d_blocks, F + P, clock, &info)) return -1;
    if (info != 0) return info;
    if (!pg::finite_all(sys.rhs.data(), sys.rhs.size())) return sys.n + 1;
    ra::irls_expand(sys, x);
    return 0;
  }
};

void print_profile(const char* entry, int F, int P, double total, const StageClock& k, int iterations) {
  std::fprintf(stderr, "pvlm_rotavg_profile {\"entry\": \"%s\", \"cameras\": %d, \"pairs\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, \"form_g_ms\": %.3f, "
               "\"host_ms\": %.3f, \"solves\": %d, \"iterations\": %d}\n", entry, F, P, total, k.kernels_ms, k.solve_ms, k.form_g_ms, total - k.kernels_ms - k.solve_ms - k.form_g_ms,
               k.solves, iterations);
}

}  // namespace

extern "C" pvlm_status pvlm_rotavg_l1(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, int start_idx, double* rotations,
                                      pvlm_rotavg_l1_summary* summary) {
  static_assert(sizeof(ra::L1Summary) == sizeof(pvlm_rotavg_l1_summary), "pvlm_rotavg_l1_summary is the core's L1Summary");
  const char* who = "pvlm_rotavg_l1";
  if (!ctx) return PVLM_ERR_ARG;
  if (!summary) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = ra::check_args(n_cameras, n_pairs, first, second, R_21, rotations, start_idx, true)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  ra::L1Summary s{0, 0, 0, 0};
  if (F == 1) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }           // the gauge camera alone: nothing to average
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  L1DeviceBackend be(c, F, P, start_idx);
  be.setup(first, second, R_21, rotations);
  if (c.st) return c.st;
  if (be.info_g != 0) s.info = be.info_g;
  else ra::l1_solve(be, F, P, &s);
  std::vector<double> out(9 * (size_t)F);
  c.d2h(out.data(), be.d_rot, out.size() * sizeof(double));
  if (c.sync()) return c.st;
  std::memcpy(rotations, out.data(), out.size() * sizeof(double));
  std::memcpy(summary, &s, sizeof s);
  if (std::getenv("PVLM_ROTAVG_PROFILE"))
    print_profile("l1", F, P, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count(), be.clock, s.admm_iterations);
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_rotavg_l2(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, double* rotations,
                                      const pvlm_rotavg_l2_params* params, pvlm_rotavg_l2_summary* summary) {
  static_assert(sizeof(pg::Summary) == sizeof(pvlm_rotavg_l2_summary), "pvlm_rotavg_l2_summary is the core's Summary");
  const char* who = "pvlm_rotavg_l2";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = ra::check_args(n_cameras, n_pairs, first, second, R_21, rotations, -1, false)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0 || !std::isfinite(params->loss_a)) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0 or loss_a not finite", who); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  const auto call_t0 = std::chrono::steady_clock::now();
  std::vector<double> aa(3 * (size_t)F);
  for (int k = 0; k < F; ++k) ra::log_rotation(rotations + 9 * (size_t)k, &aa[3 * (size_t)k]);
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  pg::Options opt;
  opt.loss_a = params->loss_a; opt.max_num_iterations = params->max_num_iterations;
  LmPairDevice<ra::L2Model> be(c, "PVLM_ROTAVG_MAX_BLOCKS", opt, F, P);
  be.setup(first, second, R_21, aa.data(), nullptr, -1);
  be.model = ra::L2Model{be.d_R21};
  pg::lm_solve(be, opt, &s);
  c.d2h(aa.data(), be.x(), aa.size() * sizeof(double));
  if (c.sync()) return c.st;
  if (pg::finite_all(aa.data(), aa.size())) for (int k = 0; k < F; ++k) ra::exp_rotation(&aa[3 * (size_t)k], rotations + 9 * (size_t)k);
  std::memcpy(summary, &s, sizeof s);
  if (std::getenv("PVLM_ROTAVG_PROFILE"))
    print_profile("l2", F, P, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count(), be.clock, s.successful_steps + s.unsuccessful_steps);
  return PVLM_OK;
}

extern "C" int pvlm_rotavg_group_size(void) { return pg::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_rotavg() {}
void pvlm_i_preload_rotavg(hipStream_t s) { hipLaunchKernelGGL(k_preload_rotavg, dim3(1), dim3(1), 0, s); }
