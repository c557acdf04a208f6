// K42: translation averaging (TranslationAveragingL2 / TranslationAveragingDLT, sfm/TranslationAveraging.cpp:31-169) on the definition of pvlm_transavg_core.h.
//
// The LM backend is the pair-graph layer's (LmPairDevice of pvlm_pairgraph.h) over the pair model ta::Model; the unit of parallelism is the PAIR for everything
// that is per pair and the CAMERA for the gather:
//   k_pg_lm_pairs  (a) a lane per pair: residual, rho', the scale's pivot, the two reduced diagonal pieces and gradient pieces into the pair's component-major record,
//                      the off-diagonal 3 x 3 straight into the solver's block list;
//   k_pg_gather_lm (b) the layer's gather: kGroup lanes per camera walk its CSR row, an xor butterfly adds the partial sums.  No floating-point atomic: one order
//                      per camera, whatever the degree;
//   k_pg_tree      (c) the layer's fixed reduction tree, launched level by level until one number is left;
//   k_pg_lm_step   (d) a lane per pair: back-substitution of the scale step, the clamp onto the parameter bounds, the candidate scale and the pair's terms
//                      (candidate cost, model decrease at the clamped step, squared step and squared parameter); k_pg_cam_step moves the cameras.
// The LM state (translations, scales, their candidates, the Jacobi scales of the scales, the pair records) stays on the device for the whole call; per iteration the
// host reads the gather (15 numbers per camera), hands the solver its right-hand side and LM diagonal, sends the camera step back and reads six scalars.  The camera
// system is factorised by the library's block-sparse SPD solver (pvlm_i_spd_solve_blocks, behind the layer's solve_cameras) from the block list in place: a 3 x 3
// block is a 6 x 6 block whose last three row and column indices are -1.  Every loop is bounded by P, F, a CSR row or max_num_iterations; every index is checked on
// the host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_pairgraph.h"
#include "pvlm_transavg_core.h"

namespace {

namespace ta = pvlm_transavg;

using Backend = LmPairDevice<ta::Model>;
const char* const kLimitEnv = "PVLM_TRANSAVG_MAX_BLOCKS";

// the graph and the state on the device, then the model over the uploaded inputs of the pairs
void setup(Backend& be, const int* first, const int* second, const double* R, const double* d, const double* bnd, const double* t0, const double* s0, int origin, bool dlt) {
  be.setup(first, second, R, t0, s0, origin);
  be.model = ta::Model{be.d_R21, be.c.upload(d, 3 * (size_t)be.P), be.c.upload(bnd, 4 * (size_t)be.P), dlt};
  be.damped = !dlt;
}

}  // namespace

extern "C" pvlm_status pvlm_transavg_dlt(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, const double* t_21,
                                         double* translations_out, int* info) {
  const char* who = "pvlm_transavg_dlt";
  if (!ctx) return PVLM_ERR_ARG;
  if (!info || (n_cameras > 0 && !translations_out)) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = ta::check_pairs(n_cameras, n_pairs, first, second, R_21, t_21)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  if (P == 0) {                                   // nothing ties the cameras: one camera is the gauge itself, more are undetermined
    *info = F <= 1 ? 0 : 1;
    if (F == 1) translations_out[0] = translations_out[1] = translations_out[2] = 0.0;
    return PVLM_OK;
  }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  pg::Options opt;
  Backend be(c, kLimitEnv, opt, F, P);
  const std::vector<double> zeros(3 * (size_t)F + 4 * (size_t)P, 0.0);
  setup(be, first, second, R_21, t_21, zeros.data(), zeros.data(), zeros.data(), 0, true);
  be.linearise(1.0, true);
  int inf = 0;
  const bool ok = be.solve(1.0, &inf);
  if (c.sync()) return c.st;
  *info = inf;
  if (ok) std::memcpy(translations_out, be.step.data(), 3 * (size_t)F * sizeof(double));
  return c.st;
}

extern "C" pvlm_status pvlm_transavg_solve(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, const double* t_21,
                                           double* scales, int origin_idx, double* translations, double* weight, const pvlm_transavg_params* params,
                                           pvlm_transavg_summary* summary) {
  static_assert(sizeof(pg::Summary) == sizeof(pvlm_transavg_summary), "pvlm_transavg_summary is the core's Summary");
  const char* who = "pvlm_transavg_solve";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary || !translations || (n_pairs > 0 && (!scales || !weight))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = ta::check_pairs(n_cameras, n_pairs, first, second, R_21, t_21)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  if (origin_idx < 0 || origin_idx >= F) { PVLM_SET_ERR(ctx, "%s: origin_idx names no camera", who); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0", who); return PVLM_ERR_ARG; }
  if (!pg::finite_all(translations, 3 * (size_t)F) || !pg::finite_all(scales, (size_t)P) || !std::isfinite(params->loss_a) || !std::isfinite(params->upper_scale_ratio) ||
      !std::isfinite(params->lower_scale_ratio)) { PVLM_SET_ERR(ctx, "%s: a translation, a scale or a parameter is not finite", who); return PVLM_ERR_ARG; }
  for (int k = 0; k < 3; ++k)
    if (translations[3 * (size_t)origin_idx + k] != 0.0) { PVLM_SET_ERR(ctx, "%s: the translation of the origin camera is not zero", who); return PVLM_ERR_ARG; }
  pg::Summary s{0.0, 0.0, 0, 0, pg::kNoPairs};
  if (P == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  std::vector<double> d(3 * (size_t)P), bnd(4 * (size_t)P);
  for (int p = 0; p < P; ++p) { ta::direction(t_21 + 3 * (size_t)p, &d[3 * (size_t)p]); ta::bounds(scales[p], params->upper_scale_ratio, params->lower_scale_ratio, &bnd[4 * (size_t)p]); }
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  pg::Options opt;
  opt.loss_a = params->loss_a; opt.max_num_iterations = params->max_num_iterations;
  Backend be(c, kLimitEnv, opt, F, P);
  setup(be, first, second, R_21, d.data(), bnd.data(), translations, scales, origin_idx, false);
  pg::lm_solve(be, opt, &s);
  std::vector<double> t_out(3 * (size_t)F), s_out((size_t)P);
  c.d2h(t_out.data(), be.x(), t_out.size() * sizeof(double));
  c.d2h(s_out.data(), be.s(), s_out.size() * sizeof(double));
  if (c.sync()) return c.st;
  std::memcpy(translations, t_out.data(), t_out.size() * sizeof(double));
  std::memcpy(scales, s_out.data(), s_out.size() * sizeof(double));
  for (int p = 0; p < P; ++p)
    weight[p] = ta::final_weight(R_21 + 9 * (size_t)p, t_21 + 3 * (size_t)p, &t_out[3 * (size_t)first[p]], &t_out[3 * (size_t)second[p]], s_out[(size_t)p]);
  std::memcpy(summary, &s, sizeof s);
  if (std::getenv("PVLM_TRANSAVG_PROFILE")) {
    const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call_t0).count();
    std::fprintf(stderr, "pvlm_transavg_profile {\"cameras\": %d, \"pairs\": %d, \"total_ms\": %.3f, \"kernels_ms\": %.3f, \"solve_ms\": %.3f, \"host_ms\": %.3f, \"solves\": %d}\n", F, P,
                 total, be.clock.kernels_ms, be.clock.solve_ms, total - be.clock.kernels_ms - be.clock.solve_ms, be.clock.solves);
  }
  return PVLM_OK;
}

extern "C" int pvlm_transavg_group_size(void) { return pg::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_transavg() {}
void pvlm_i_preload_transavg(hipStream_t s) { hipLaunchKernelGGL(k_preload_transavg, dim3(1), dim3(1), 0, s); }
