// K46: translation averaging on world-frame directions — TranslationAveragingL2Chordal and one solve of TranslationAveragingLUD (sfm/TranslationAveraging.cpp:206-274,
// :553-626) — on the definition of pvlm_transdir_core.h.  ONE backend serves both problems; the pair model (kChordal / kLud) is an argument of the per-pair kernels,
// uniform over a launch.  K42's backend is not shared: its pairs carry R_21 and a DLT mode that these problems do not have, and its record has other slots.
//
// The unit of parallelism is the PAIR for everything that is per pair and the CAMERA for the gather:
//   k_td_pairs     (a) a lane per pair: the residual, its Jacobian pieces and (kLud) the scale's pivot into the pair's component-major record, the off-diagonal
//                      3 x 3 straight into the solver's block list.  The centres are read by first / second (strided), the record is written component-major, so
//                      the lanes of a wave store side by side;
//   k_pg_gather_lm (b) the pair-graph layer's gather (pvlm_pairgraph.h): kGroup lanes per camera walk its CSR row, an xor butterfly adds the partial sums;
//   k_pg_tree      (c) the layer's fixed reduction tree;
//   k_td_step      (d) a lane per pair: (kLud) back-substitution of the scale step and the clamp onto the parameter bounds; the pair's terms (candidate cost, model
//                      decrease at the clamped step, squared step and squared parameter); k_pg_cam_step moves the cameras.
// The LM state stays on the device for the whole call; per iteration the host reads the gather (15 numbers per camera), hands the solver its right-hand side and LM
// diagonal, sends the camera step back and reads six scalars.  Every loop is bounded by P, F, a CSR row or max_num_iterations; every index is checked on the host
// before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_transdir_core.h"

namespace {

namespace td = pvlm_transdir;

// what a lane reads of its pair; bnd, w and s are null for kChordal
struct PairIn { double dir[3], bnd[4], w, s; };
__device__ __forceinline__ PairIn load_pair(long long p, const double* __restrict__ dir, const double* __restrict__ bnd, const double* __restrict__ w,
                                            const double* __restrict__ s) {
  PairIn in;
  for (int k = 0; k < 3; ++k) in.dir[k] = dir[3 * p + k];
  for (int k = 0; k < 4; ++k) in.bnd[k] = bnd ? bnd[4 * p + k] : 0.0;
  in.w = w ? w[p] : 1.0; in.s = s ? s[p] : 0.0;
  return in;
}

__global__ __launch_bounds__(kThreads) void k_td_pairs(int model, int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                       const double* __restrict__ bnd, const double* __restrict__ w, const double* __restrict__ c,
                                                       const double* __restrict__ s, double a, double radius, double min_diag, double max_diag, int first_time,
                                                       double* __restrict__ sigma, double* __restrict__ rec, double* __restrict__ off_blocks, double* __restrict__ gs_abs) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    const PairIn in = load_pair(p, dir, bnd, w, s);
    double ci[3], cj[3], sg = 0.0;
    for (int k = 0; k < 3; ++k) { ci[k] = c[3 * (long long)first[p] + k]; cj[k] = c[3 * (long long)second[p] + k]; }
    if (sigma && !first_time) sg = sigma[p];
    td::linearise_pair(model, in.dir, in.bnd, in.w, ci, cj, in.s, a, radius, min_diag, max_diag, first_time != 0, &sg, rec + p, P, off_blocks + 36 * p);
    if (sigma && first_time) sigma[p] = sg;
    gs_abs[p] = fabs(rec[(long long)td::kGs * P + p]);
  }
}

__global__ __launch_bounds__(kThreads) void k_td_cost(int model, int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                      const double* __restrict__ bnd, const double* __restrict__ w, const double* __restrict__ c,
                                                      const double* __restrict__ s, double a, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    const PairIn in = load_pair(p, dir, bnd, w, s);
    double ci[3], cj[3];
    for (int k = 0; k < 3; ++k) { ci[k] = c[3 * (long long)first[p] + k]; cj[k] = c[3 * (long long)second[p] + k]; }
    terms[p] = td::pair_cost(model, in.dir, in.bnd, in.w, ci, cj, in.s, a);
  }
}

__global__ __launch_bounds__(kThreads) void k_td_step(int model, int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ dir,
                                                      const double* __restrict__ bnd, const double* __restrict__ w, const double* __restrict__ rec,
                                                      const double* __restrict__ step, const double* __restrict__ c_cand, const double* __restrict__ s, double a,
                                                      double* __restrict__ s_cand, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    const PairIn in = load_pair(p, dir, bnd, w, s);
    const long long i = first[p], j = second[p];
    double di[3], dj[3], ci[3], cj[3], sc;
    for (int k = 0; k < 3; ++k) { di[k] = step[3 * i + k]; dj[k] = step[3 * j + k]; ci[k] = c_cand[3 * i + k]; cj[k] = c_cand[3 * j + k]; }
    td::step_pair(model, in.dir, in.bnd, in.w, rec + p, P, di, dj, ci, cj, in.s, a, &sc, terms + p, P);
    if (s_cand) s_cand[p] = sc;
  }
}

// the LM backend of both problems: the layer's graph, camera system and camera step; the centres, the scales (kLud) and the per-pair records are its own
struct DeviceBackend : LmDevice {
  int model;
  double *d_dir = nullptr, *d_bnd = nullptr, *d_w = nullptr, *d_sigma = nullptr, *d_rec = nullptr, *d_terms = nullptr, *d_gs = nullptr;
  double *d_c[2] = {nullptr, nullptr}, *d_s[2] = {nullptr, nullptr};
  int cur = 0;

  DeviceBackend(pvlm_call& call, int model_, const pg::Options& o, int F_, int P_) : LmDevice(call, "PVLM_TRANSDIR_MAX_BLOCKS", o, F_, P_), model(model_) {}

  // bnd, w and s0 are null for kChordal
  void setup(const int* first, const int* second, const double* dir, const double* bnd, const double* w, const double* c0, const double* s0, int origin) {
    LmDevice::setup(first, second, nullptr, td::kPairTerms, origin);
    d_dir = c.upload(dir, 3 * (size_t)P);
    d_c[0] = c.upload(c0, 3 * (size_t)F); d_c[1] = c.alloc<double>(3 * (size_t)F);
    if (model == td::kLud) {
      d_bnd = c.upload(bnd, 4 * (size_t)P); d_w = c.upload(w, (size_t)P);
      d_s[0] = c.upload(s0, (size_t)P); d_s[1] = c.alloc<double>((size_t)P);
      d_sigma = c.alloc<double>((size_t)P);
    }
    d_rec = c.alloc<double>((size_t)td::kPairSlots * (size_t)P);
    d_terms = c.alloc<double>((size_t)td::kPairTerms * (size_t)P); d_gs = c.alloc<double>((size_t)P);
  }

  double initial_cost() {
    double cost = 0.0;
    clock.start();
    c.launch(k_td_cost, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_dir, d_bnd, d_w, d_c[cur], d_s[cur], opt.loss_a, d_terms);
    reduce<false>(d_terms, P, P, 1, &cost);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    return bad ? std::nan("") : cost;
  }
  double linearise(double radius, bool first) {
    double gs_max = 0.0;
    clock.start();
    c.launch(k_td_pairs, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_dir, d_bnd, d_w, d_c[cur], d_s[cur], opt.loss_a, radius, opt.min_lm_diagonal,
             opt.max_lm_diagonal, first ? 1 : 0, d_sigma, d_rec, off_blocks(), d_gs);
    reduce<true>(d_gs, P, P, 1, &gs_max);
    const bool ok = gather(d_rec);
    clock.kernels_ms += clock.stop();
    if (!ok) return 0.0;
    if (first) sys.set_sigma(cam.data());
    return std::fmax(gs_max, sys.gradient_max(cam.data()));
  }
  bool solve(double radius) { return LmDevice::solve(radius, true, nullptr); }
  pg::Scalars candidate() {
    double pt[td::kPairTerms] = {0, 0, 0, 0}, ct[2] = {0, 0};
    clock.start();
    step_cameras(d_c[cur], d_c[cur ^ 1]);
    c.launch(k_td_step, dim3(pair_grid()), dim3(kThreads), 0, model, P, d_first, d_second, d_dir, d_bnd, d_w, d_rec, d_step, d_c[cur ^ 1], d_s[cur], opt.loss_a, d_s[cur ^ 1],
             d_terms);
    reduce<false>(d_terms, P, P, td::kPairTerms, pt);          // the staged copy of the roots is ordered on the stream before the next tree reuses the partials
    camera_terms(ct);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return pg::Scalars{std::nan(""), 0, 0, 0};
    return pg::Scalars{pt[pg::kTermCost], pt[pg::kTermModel], pt[td::kTermStep2] + ct[0], pt[td::kTermX2] + ct[1]};
  }
  void accept() { cur ^= 1; }
};

void profile_line(const char* who, int F, int P, const std::chrono::steady_clock::time_point& t0, const StageClock& clock, const pg::Summary& s) {
  if (!std::getenv("PVLM_TRANSDIR_PROFILE")) return;
  const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::fprintf(stderr, "pvlm_transdir_profile {\"call\": \"%s\", \"cameras\": %d, \"pairs\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, \"host_ms\": %.3f, "
               "\"solves\": %d, \"iterations\": %d}\n", who, F, P, total, clock.kernels_ms, clock.solve_ms, total - clock.kernels_ms - clock.solve_ms, clock.solves,
               s.successful_steps + s.unsuccessful_steps);
}

}  // namespace

extern "C" pvlm_status pvlm_transavg_chordal(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir, int origin_idx,
                                             double* centres, const pvlm_transdir_chordal_params* params, pvlm_transdir_summary* summary) {
  static_assert(sizeof(pg::Summary) == sizeof(pvlm_transdir_summary), "pvlm_transdir_summary is the core's Summary");
  const char* who = "pvlm_transavg_chordal";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary || !centres) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = td::check_pairs(n_cameras, n_pairs, first, second, dir)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (const char* bad = td::check_centres(n_cameras, origin_idx, centres)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0", who); return PVLM_ERR_ARG; }
  if (!std::isfinite(params->loss_a)) { PVLM_SET_ERR(ctx, "%s: a parameter is not finite", who); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const pg::Options opt = td::chordal_options(params->loss_a, params->max_num_iterations);
  DeviceBackend be(c, td::kChordal, opt, F, P);
  be.setup(first, second, dir, nullptr, nullptr, centres, nullptr, origin_idx);
  pg::lm_solve(be, opt, &s);
  std::vector<double> c_out(3 * (size_t)F);
  c.d2h(c_out.data(), be.d_c[be.cur], c_out.size() * sizeof(double));
  if (c.sync()) return c.st;
  if (s.termination != pg::kCostNotFinite) std::memcpy(centres, c_out.data(), c_out.size() * sizeof(double));
  std::memcpy(summary, &s, sizeof s);
  profile_line(who, F, P, call_t0, be.clock, s);
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_transavg_lud(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir, double* scales, double* weight,
                                         int origin_idx, double* centres, const pvlm_transdir_lud_params* params, double* sum_e, pvlm_transdir_summary* summary) {
  const char* who = "pvlm_transavg_lud";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary || !centres || !sum_e || (n_pairs > 0 && (!scales || !weight))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = td::check_pairs(n_cameras, n_pairs, first, second, dir)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (const char* bad = td::check_centres(n_cameras, origin_idx, centres)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0", who); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  if (!pg::finite_all(scales, (size_t)P) || !pg::finite_all(weight, (size_t)P) || !std::isfinite(params->upper_scale_ratio) || !std::isfinite(params->lower_scale_ratio)) {
    PVLM_SET_ERR(ctx, "%s: a scale, a weight or a parameter is not finite", who); return PVLM_ERR_ARG;
  }
  for (int p = 0; p < P; ++p) if (!(weight[p] > 0.0)) { PVLM_SET_ERR(ctx, "%s: a weight <= 0", who); return PVLM_ERR_ARG; }
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  std::vector<double> bnd(4 * (size_t)P);
  for (int p = 0; p < P; ++p) td::lud_bounds(scales[p], params->upper_scale_ratio, params->lower_scale_ratio, &bnd[4 * (size_t)p]);
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  pg::Options opt;
  opt.max_num_iterations = params->max_num_iterations;
  DeviceBackend be(c, td::kLud, opt, F, P);
  be.setup(first, second, dir, bnd.data(), weight, centres, scales, origin_idx);
  pg::lm_solve(be, opt, &s);
  std::vector<double> c_out(3 * (size_t)F), s_out((size_t)P), m((size_t)P);
  c.d2h(c_out.data(), be.d_c[be.cur], c_out.size() * sizeof(double));
  c.d2h(s_out.data(), be.d_s[be.cur], s_out.size() * sizeof(double));
  if (c.sync()) return c.st;
  if (s.termination != pg::kCostNotFinite) {
    std::memcpy(centres, c_out.data(), c_out.size() * sizeof(double));
    std::memcpy(scales, s_out.data(), s_out.size() * sizeof(double));
    for (int p = 0; p < P; ++p) weight[p] = td::final_weight(dir + 3 * (size_t)p, &c_out[3 * (size_t)first[p]], &c_out[3 * (size_t)second[p]], s_out[(size_t)p], &m[(size_t)p]);
    *sum_e = pg::tree_reduce_host<false>(m.data(), P);
  }
  std::memcpy(summary, &s, sizeof s);
  profile_line(who, F, P, call_t0, be.clock, s);
  return PVLM_OK;
}

extern "C" int pvlm_transdir_group_size(void) { return pg::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_transdir() {}
void pvlm_i_preload_transdir(hipStream_t s) { hipLaunchKernelGGL(k_preload_transdir, dim3(1), dim3(1), 0, s); }
