// K47: TranslationAveragingL1 (sfm/TranslationAveraging.cpp:277-417), the triplet minimax programme, by the interior-point iteration of pvlm_translp_core.h.
//
// The unit of parallelism is the TRIPLET for everything that is per row and the CAMERA / the PAIR for the two gathers:
//   k_lp_start      a lane per triplet: the start of its 19 rows (s = h - G x at t = 0, z = 1 / rows);
//   k_lp_assemble   a lane per triplet: w = z / s of its 19 rows, its lambda eliminated by the 1 x 1 pivot, the reduced 3 x 3 blocks, its part of the gamma column
//                   and of G^T z into the triplet's component-major record; its five terms (s^T z, gamma entries, residual maxima);
//   k_lp_gather_cam the layer's gather skeleton (camera_gather) over the CSR camera -> (triplet, slot): kGroup lanes per camera, an xor butterfly; the diagonal block
//                   into the solver's list.  k_lp_gather_pair is its per-pair twin over the CSR pair -> (triplet, slot): the off-diagonal block;
//   k_lp_rhs        a lane per triplet: the right-hand side of the predictor or the corrector, lambda eliminated; k_lp_gather_rhs gathers it per camera;
//   k_lp_direction  a lane per triplet: dlambda by back-substitution, ds and dz per row, the two step ratios (negated, for the tree's maximum);
//   k_lp_mu_aff     the predictor's complementarity at its step lengths; k_lp_update / k_lp_cam_update the step;
//   k_pg_tree       the layer's fixed reduction tree under every scalar.
// The state — 19 rows of (s, z) and of the direction per triplet, the lambdas, the translations — stays on the device for the whole call.  Per camera solve the host
// reads one gather (the matrix gather once per iteration: 12 numbers per camera; a right-hand side: 3) and sends the camera step back (3 per camera).  Three camera
// systems per iteration go through the layer's solve_cameras, each assembled and factorised on its own.  Every loop is bounded by T, F, P, a CSR row or
// max_iterations; every index is checked on the host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_translp_core.h"

namespace {

namespace lp = pvlm_translp;

// what every per-triplet kernel reads of the problem
struct TripIn { int T; const int* cam; const int* pair; const double* R21; const double* t21; const double* lo; };

__global__ __launch_bounds__(kThreads) void k_lp_start(TripIn in, const double* __restrict__ lam, double gam, double zval, double* __restrict__ s, double* __restrict__ z) {
  const long long T = in.T;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    lp::Trip tr; double sv[lp::kRows], zv[lp::kRows];
    lp::load_trip(t, in.pair, in.R21, in.t21, in.lo, &tr);
    lp::start_rows(tr, lam[t], gam, zval, sv, zv);
    lp::store_rows(s, T, t, sv); lp::store_rows(z, T, t, zv);
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_assemble(TripIn in, const double* __restrict__ x, const double* __restrict__ lam, double gam, const double* __restrict__ s,
                                                          const double* __restrict__ z, double* __restrict__ rec, double* __restrict__ terms) {
  const long long T = in.T;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], xc[3][3];
    lp::load_trip(t, in.pair, in.R21, in.t21, in.lo, &tr);
    lp::load_rows(s, T, t, sv); lp::load_rows(z, T, t, zv); lp::load_cams(x, in.cam, t, xc);
    lp::assemble_triplet(tr, xc, lam[t], gam, sv, zv, rec + t, T, terms + t, T);
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_rhs(TripIn in, int mode, const double* __restrict__ x, const double* __restrict__ lam, double gam, double sigma_mu,
                                                     const double* __restrict__ s, const double* __restrict__ z, const double* __restrict__ ds, const double* __restrict__ dz,
                                                     double* __restrict__ rec, double* __restrict__ terms) {
  const long long T = in.T;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows], xc[3][3];
    lp::load_trip(t, in.pair, in.R21, in.t21, in.lo, &tr);
    lp::load_rows(s, T, t, sv); lp::load_rows(z, T, t, zv); lp::load_rows(ds, T, t, dsv); lp::load_rows(dz, T, t, dzv); lp::load_cams(x, in.cam, t, xc);
    terms[t] = lp::rhs_triplet(mode, tr, xc, lam[t], gam, sv, zv, dsv, dzv, sigma_mu, rec + t, T);
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_direction(TripIn in, int mode, const double* __restrict__ x, const double* __restrict__ lam, double gam, double sigma_mu,
                                                           const double* __restrict__ s, const double* __restrict__ z, const double* __restrict__ dx, double dgam,
                                                           const double* __restrict__ rec, double* __restrict__ ds, double* __restrict__ dz, double* __restrict__ dlam,
                                                           double* __restrict__ terms) {
  const long long T = in.T;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    lp::Trip tr; double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows], xc[3][3], dxc[3][3], r[2], dl;
    lp::load_trip(t, in.pair, in.R21, in.t21, in.lo, &tr);
    lp::load_rows(s, T, t, sv); lp::load_rows(z, T, t, zv); lp::load_rows(ds, T, t, dsv); lp::load_rows(dz, T, t, dzv);
    lp::load_cams(x, in.cam, t, xc); lp::load_cams(dx, in.cam, t, dxc);
    lp::direction_triplet(mode, tr, xc, lam[t], gam, sv, zv, dxc, dgam, sigma_mu, rec + t, T, dsv, dzv, &dl, r);
    lp::store_rows(ds, T, t, dsv); lp::store_rows(dz, T, t, dzv);
    dlam[t] = dl; terms[t] = r[0]; terms[T + t] = r[1];
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_mu_aff(int T_, const double* __restrict__ s, const double* __restrict__ z, const double* __restrict__ ds,
                                                        const double* __restrict__ dz, double ap, double ad, double* __restrict__ terms) {
  const long long T = T_;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    double sv[lp::kRows], zv[lp::kRows], dsv[lp::kRows], dzv[lp::kRows];
    lp::load_rows(s, T, t, sv); lp::load_rows(z, T, t, zv); lp::load_rows(ds, T, t, dsv); lp::load_rows(dz, T, t, dzv);
    terms[t] = lp::mu_aff_triplet(sv, zv, dsv, dzv, ap, ad);
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_update(int T_, double ap, double ad, const double* __restrict__ ds, const double* __restrict__ dz,
                                                        const double* __restrict__ dlam, double* __restrict__ s, double* __restrict__ z, double* __restrict__ lam) {
  const long long T = T_, n = (long long)lp::kRows * T;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    s[i] += ap * ds[i]; z[i] += ad * dz[i];
    if (i < T) lam[i] += ap * dlam[i];
  }
}

__global__ __launch_bounds__(kThreads) void k_lp_cam_update(int F, double ap, const double* __restrict__ dx, double* __restrict__ x) {
  const long long n = 3 * (long long)F;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) x[i] += ap * dx[i];
}

__global__ __launch_bounds__(kThreads) void k_lp_gather_cam(int F, long long T, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                            double* __restrict__ cam, double* __restrict__ diag_blocks) {
  camera_gather<lp::kCamRec>(F, row_off, [&](int e0, int e1, int lane, double* part) { lp::gather_lane<lp::kCamRec>(rec, T, ent, e0, e1, lane, 0, lp::kCamRec, part); },
                             [&](long long c, const double* part) {
                               for (int k = 0; k < lp::kCamRec; ++k) cam[lp::kCamRec * c + k] = part[k];
                               pg::diagonal_block(part, diag_blocks + 36 * c);
                             });
}
// the per-pair twin: the rows of the skeleton are the pairs
__global__ __launch_bounds__(kThreads) void k_lp_gather_pair(int P, long long T, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                             double* __restrict__ off_blocks) {
  camera_gather<9>(P, row_off, [&](int e0, int e1, int lane, double* part) { lp::gather_lane<9>(rec, T, ent, e0, e1, lane, lp::kRecOff, 9, part); },
                   [&](long long p, const double* part) { lp::off_block(part, off_blocks + 36 * p); });
}
__global__ __launch_bounds__(kThreads) void k_lp_gather_rhs(int F, long long T, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                            double* __restrict__ cam_rhs) {
  camera_gather<3>(F, row_off, [&](int e0, int e1, int lane, double* part) { lp::gather_lane<3>(rec, T, ent, e0, e1, lane, lp::kRecRhs, 3, part); },
                   [&](long long c, const double* part) { for (int k = 0; k < 3; ++k) cam_rhs[3 * c + k] = part[k]; });
}

// the backend of lp::run: the layer's tree and camera solve; the state, the records and both CSRs are its own
struct DeviceBackend : DeviceGraph {
  lp::Problem& prob;
  int T;
  TripIn in{};
  int *d_cam_off = nullptr, *d_cam_ent = nullptr, *d_pair_off = nullptr, *d_pair_ent = nullptr;
  double *d_s = nullptr, *d_z = nullptr, *d_ds = nullptr, *d_dz = nullptr, *d_lam = nullptr, *d_dlam = nullptr, *d_x = nullptr, *d_dx = nullptr, *d_rec = nullptr,
         *d_terms = nullptr, *d_blocks = nullptr, *d_camv = nullptr, *d_camrhs = nullptr;
  std::vector<double> camv, camrhs;

  DeviceBackend(pvlm_call& call, lp::Problem& pr) : DeviceGraph(call, "PVLM_TRANSLP_MAX_BLOCKS", pr.F, pr.P), prob(pr), T(pr.T) {}

  void setup(const int* trip_pairs, const double* R21, const double* t21) {
    const size_t nT = (size_t)T, rows = (size_t)lp::kRows * nT;
    in.T = T;
    in.cam = c.upload(prob.trip_cam.data(), 3 * nT); in.pair = c.upload(trip_pairs, 3 * nT);
    in.R21 = c.upload(R21, 9 * (size_t)P); in.t21 = c.upload(t21, 3 * (size_t)P); in.lo = c.upload(prob.lo.data(), nT);
    d_cam_off = c.upload(prob.cam_off.data(), prob.cam_off.size()); d_cam_ent = c.upload(prob.cam_ent.data(), prob.cam_ent.size());
    d_pair_off = c.upload(prob.pair_off.data(), prob.pair_off.size()); d_pair_ent = c.upload(prob.pair_ent.data(), prob.pair_ent.size());
    d_s = c.alloc<double>(rows); d_z = c.alloc<double>(rows); d_lam = c.upload(prob.lam0.data(), nT);
    d_ds = c.alloc<double>(rows); d_dz = c.alloc<double>(rows); d_dlam = c.alloc<double>(nT);
    d_x = c.alloc<double>(3 * (size_t)F); d_dx = c.alloc<double>(3 * (size_t)F);
    d_rec = c.alloc<double>((size_t)lp::kRecSlots * nT); d_terms = c.alloc<double>((size_t)lp::kTerms * nT);
    d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P)); d_camv = c.alloc<double>((size_t)lp::kCamRec * (size_t)F); d_camrhs = c.alloc<double>(3 * (size_t)F);
    const size_t stride = (nT + pg::kChunk - 1) / pg::kChunk;
    for (int k = 0; k < 2; ++k) d_part[k] = c.alloc<double>((size_t)lp::kTerms * stride);
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
    c.memset(d_x, 0, 3 * (size_t)F * sizeof(double));
    c.memset(d_ds, 0, rows * sizeof(double)); c.memset(d_dz, 0, rows * sizeof(double));
    c.launch(k_lp_start, dim3(trip_grid()), dim3(kThreads), 0, in, (const double*)d_lam, prob.gamma0, prob.z0, d_s, d_z);
    c.check_launches();
    camv.assign((size_t)lp::kCamRec * (size_t)F, 0.0); camrhs.assign(3 * (size_t)F, 0.0);
  }
  const double* cam() const { return camv.data(); }
  const double* cam_rhs() const { return camrhs.data(); }
  unsigned trip_grid() const { return grid_for(T, kThreads, blocks_limit); }
  unsigned row_grid() const { return grid_for((long long)lp::kRows * T, kThreads, blocks_limit); }
  unsigned pair_group_grid() const { return grid_for(P, kThreads / pg::kGroup, blocks_limit); }
  bool wait() { const bool ok = c.sync() == PVLM_OK; clock.kernels_ms += clock.stop(); return ok; }

  bool evaluate(double gam, double* roots) {
    clock.start();
    c.launch(k_lp_assemble, dim3(trip_grid()), dim3(kThreads), 0, in, (const double*)d_x, (const double*)d_lam, gam, (const double*)d_s, (const double*)d_z, d_rec, d_terms);
    c.launch(k_lp_gather_cam, dim3(group_grid()), dim3(kThreads), 0, F, (long long)T, (const int*)d_cam_off, (const int*)d_cam_ent, (const double*)d_rec, d_camv, d_blocks);
    c.launch(k_lp_gather_pair, dim3(pair_group_grid()), dim3(kThreads), 0, P, (long long)T, (const int*)d_pair_off, (const int*)d_pair_ent, (const double*)d_rec,
             d_blocks + 36 * (size_t)F);
    c.check_launches();
    c.d2h(camv.data(), d_camv, camv.size() * sizeof(double));
    reduce<false>(d_terms, T, T, lp::kTermRp, roots);          // the staged copy of the roots is ordered on the stream before the next tree reuses the partials
    reduce<true>(d_terms + (size_t)lp::kTermRp * (size_t)T, T, T, lp::kTerms - lp::kTermRp, roots + lp::kTermRp);
    return wait();
  }
  bool rhs(int mode, double gam, double sigma_mu, double* gamma_share) {
    clock.start();
    c.launch(k_lp_rhs, dim3(trip_grid()), dim3(kThreads), 0, in, mode, (const double*)d_x, (const double*)d_lam, gam, sigma_mu, (const double*)d_s, (const double*)d_z,
             (const double*)d_ds, (const double*)d_dz, d_rec, d_terms);
    c.launch(k_lp_gather_rhs, dim3(group_grid()), dim3(kThreads), 0, F, (long long)T, (const int*)d_cam_off, (const int*)d_cam_ent, (const double*)d_rec, d_camrhs);
    c.check_launches();
    c.d2h(camrhs.data(), d_camrhs, camrhs.size() * sizeof(double));
    reduce<false>(d_terms, T, T, 1, gamma_share);
    return wait();
  }
  bool solve(int* info) { return !failed() && solve_cameras(c, prob.sys, d_blocks, F + P, clock, info); }
  bool direction(int mode, double gam, const std::vector<double>& dx, double dgam, double sigma_mu, double* ratio) {
    clock.start();
    c.h2d(d_dx, dx.data(), dx.size() * sizeof(double));
    c.launch(k_lp_direction, dim3(trip_grid()), dim3(kThreads), 0, in, mode, (const double*)d_x, (const double*)d_lam, gam, sigma_mu, (const double*)d_s, (const double*)d_z,
             (const double*)d_dx, dgam, (const double*)d_rec, d_ds, d_dz, d_dlam, d_terms);
    reduce<true>(d_terms, T, T, 2, ratio);
    return wait();
  }
  bool mu_aff(double ap, double ad, double* sum) {
    clock.start();
    c.launch(k_lp_mu_aff, dim3(trip_grid()), dim3(kThreads), 0, T, (const double*)d_s, (const double*)d_z, (const double*)d_ds, (const double*)d_dz, ap, ad, d_terms);
    reduce<false>(d_terms, T, T, 1, sum);
    return wait();
  }
  // d_dx holds dx since the corrector's direction
  bool update(double ap, double ad, const std::vector<double>&) {
    clock.start();
    c.launch(k_lp_update, dim3(row_grid()), dim3(kThreads), 0, T, ap, ad, (const double*)d_ds, (const double*)d_dz, (const double*)d_dlam, d_s, d_z, d_lam);
    c.launch(k_lp_cam_update, dim3(camera_grid()), dim3(kThreads), 0, F, ap, (const double*)d_dx, d_x);
    c.check_launches();
    clock.kernels_ms += clock.stop();
    return !failed();
  }
};

}  // namespace

extern "C" pvlm_status pvlm_transavg_l1(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, const double* t_21,
                                        int n_triplets, const int* triplet_pairs, int origin_idx, double* translations, double* duals, const pvlm_translp_params* params,
                                        pvlm_translp_summary* summary) {
  static_assert(sizeof(lp::Summary) == sizeof(pvlm_translp_summary), "pvlm_translp_summary is the core's Summary");
  static_assert(sizeof(lp::Params) == sizeof(pvlm_translp_params), "pvlm_translp_params is the core's Params");
  const char* who = "pvlm_transavg_l1";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary || !translations) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  lp::Params prm;
  prm.max_iterations = params->max_iterations; prm.gap_tol = params->gap_tol; prm.feas_tol = params->feas_tol;
  if (const char* bad = lp::check_args(n_cameras, n_pairs, first, second, R_21, t_21, n_triplets, triplet_pairs, origin_idx, translations, &prm)) {
    PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG;
  }
  const int F = n_cameras, P = n_pairs, T = n_triplets;
  lp::Summary s{0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, lp::kNoTriplets};
  if (T == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  const auto call_t0 = std::chrono::steady_clock::now();
  lp::Problem prob;
  prob.init(F, P, first, second, R_21, t_21, T, triplet_pairs, origin_idx);
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  DeviceBackend be(c, prob);
  be.setup(triplet_pairs, R_21, t_21);
  lp::run(be, prob, prm, &s);
  // the multipliers come back whole only for a caller that takes them; the dual objective needs the bound rows' alone
  std::vector<double> x_out(3 * (size_t)F), z_cm(duals ? (size_t)lp::kRows * (size_t)T : (size_t)T);
  const size_t z_from = duals ? 0 : (size_t)lp::kBound * (size_t)T;
  c.d2h(x_out.data(), be.d_x, x_out.size() * sizeof(double));
  c.d2h(z_cm.data(), be.d_z + z_from, z_cm.size() * sizeof(double));
  if (c.sync()) return c.st;
  if (s.termination < 0) { PVLM_SET_ERR(ctx, "%s: the device failed", who); return PVLM_ERR_HIP; }
  if (s.termination == lp::kConverged || s.termination == lp::kIterationLimit) {
    s.dual_objective = lp::dual_objective(prob, z_cm.data() + (duals ? (size_t)lp::kBound * (size_t)T : 0));
    std::memcpy(translations, x_out.data(), x_out.size() * sizeof(double));
    if (duals) for (int t = 0; t < T; ++t) for (int r = 0; r < lp::kRows; ++r) duals[(size_t)lp::kRows * t + r] = z_cm[(size_t)r * T + t];
  }
  std::memcpy(summary, &s, sizeof s);
  if (std::getenv("PVLM_TRANSLP_PROFILE")) {
    const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count();
    std::fprintf(stderr, "pvlm_translp_profile {\"cameras\": %d, \"pairs\": %d, \"triplets\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, \"host_ms\": %.3f, "
                 "\"solves\": %d, \"iterations\": %d}\n", F, P, T, total, be.clock.kernels_ms, be.clock.solve_ms, total - be.clock.kernels_ms - be.clock.solve_ms, be.clock.solves,
                 s.iterations);
  }
  return PVLM_OK;
}

extern "C" int pvlm_translp_group_size(void) { return pg::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_translp() {}
void pvlm_i_preload_translp(hipStream_t s) { hipLaunchKernelGGL(k_preload_translp, dim3(1), dim3(1), 0, s); }
