// K46: translation averaging on world-frame directions — TranslationAveragingL2Chordal and one solve of TranslationAveragingLUD (sfm/TranslationAveraging.cpp:206-274,
// :553-626) — on the definition of pvlm_transdir_core.h.  Both problems run on the pair-graph layer's LM backend (LmPairDevice of pvlm_pairgraph.h), each over its
// own pair model (td::Chordal, td::Lud).
//
// The unit of parallelism is the PAIR for everything that is per pair and the CAMERA for the gather:
//   k_pg_lm_pairs  (a) a lane per pair: the residual, its Jacobian pieces and (Lud) the scale's pivot into the pair's component-major record, the off-diagonal
//                      3 x 3 straight into the solver's block list;
//   k_pg_gather_lm (b) the layer's gather: kGroup lanes per camera walk its CSR row, an xor butterfly adds the partial sums;
//   k_pg_tree      (c) the layer's fixed reduction tree;
//   k_pg_lm_step   (d) a lane per pair: (Lud) back-substitution of the scale step and the clamp onto the parameter bounds; the pair's terms (candidate cost, model
//                      decrease at the clamped step and, for Lud, squared step and squared parameter); k_pg_cam_step moves the cameras.
// The LM state stays on the device for the whole call; per iteration the host reads the gather (15 numbers per camera), hands the solver its right-hand side and LM
// diagonal, sends the camera step back and reads four or six scalars.  Every loop is bounded by P, F, a CSR row or max_num_iterations; every index is checked on the
// host before the first launch.  Vector stores and plain C++ only.
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

const char* const kLimitEnv = "PVLM_TRANSDIR_MAX_BLOCKS";

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
  LmPairDevice<td::Chordal> be(c, kLimitEnv, opt, F, P);
  be.setup(first, second, nullptr, centres, nullptr, origin_idx);
  be.model = td::Chordal{c.upload(dir, 3 * (size_t)P)};
  pg::lm_solve(be, opt, &s);
  std::vector<double> c_out(3 * (size_t)F);
  c.d2h(c_out.data(), be.x(), c_out.size() * sizeof(double));
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
  LmPairDevice<td::Lud> be(c, kLimitEnv, opt, F, P);
  be.setup(first, second, nullptr, centres, scales, origin_idx);
  be.model = td::Lud{c.upload(dir, 3 * (size_t)P), c.upload(bnd.data(), 4 * (size_t)P), c.upload(weight, (size_t)P)};
  pg::lm_solve(be, opt, &s);
  std::vector<double> c_out(3 * (size_t)F), s_out((size_t)P), m((size_t)P);
  c.d2h(c_out.data(), be.x(), c_out.size() * sizeof(double));
  c.d2h(s_out.data(), be.s(), s_out.size() * sizeof(double));
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
