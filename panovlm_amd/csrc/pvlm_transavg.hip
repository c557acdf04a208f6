// K42: translation averaging (TranslationAveragingL2 / TranslationAveragingDLT, sfm/TranslationAveraging.cpp:31-169) on the definition of pvlm_transavg_core.h.
//
// The unit of parallelism is the PAIR for everything that is per pair and the CAMERA for the gather:
//   k_ta_pairs   (a) a lane per pair: residual, rho', the scale's pivot, the two reduced diagonal pieces and gradient pieces into the pair's component-major record,
//                    the off-diagonal 3 x 3 straight into the solver's block list;
//   k_ta_gather  (b) kGroup lanes per camera walk its CSR row (entry = 2 * pair + side, pair-list order), lane l takes the entries l, l + kGroup, ...; an xor butterfly
//                    over the group adds the partial sums.  A gather, no floating-point atomic: one order per camera, whatever the degree;
//   k_ta_tree    (c) one node level of the fixed reduction tree (kChunk leaves per workgroup, halved in LDS), launched level by level until one number is left;
//   k_ta_step    (d) a lane per pair: back-substitution of the scale step, the clamp onto the parameter bounds, the candidate scale and the pair's terms
//                    (candidate cost, model decrease at the clamped step, squared step and squared parameter); k_ta_cam_step moves the cameras.
// The LM state (translations, scales, their candidates, the Jacobi scales of the scales, the pair records) stays on the device for the whole call; per iteration the
// host reads the gather (15 numbers per camera), hands the solver its right-hand side and LM diagonal, sends the camera step back and reads six scalars.  The camera
// system is factorised by the library's block-sparse SPD solver (pvlm_i_spd_solve_blocks) from the block list in place: a 3 x 3 block is a 6 x 6 block whose last
// three row and column indices are -1.  Every loop is bounded by P, F, a CSR row or max_num_iterations; every index is checked on the host before the first launch.
// Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_transavg_core.h"

namespace {

namespace ta = pvlm_transavg;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;           // the per-pair kernels stride past kMaxBlocks * kThreads pairs

__global__ __launch_bounds__(kThreads) void k_ta_pairs(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R,
                                                       const double* __restrict__ d, const double* __restrict__ bnd, const double* __restrict__ t,
                                                       const double* __restrict__ s, double a, double radius, double min_diag, double max_diag, int first_time, int dlt,
                                                       double* __restrict__ sigma, double* __restrict__ rec, double* __restrict__ off_blocks, double* __restrict__ gs_abs) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double Rp[9], dp[3], bp[4], ti[3], tj[3];
    for (int k = 0; k < 9; ++k) Rp[k] = R[9 * p + k];
    for (int k = 0; k < 3; ++k) { dp[k] = d[3 * p + k]; ti[k] = t[3 * (long long)first[p] + k]; tj[k] = t[3 * (long long)second[p] + k]; }
    for (int k = 0; k < 4; ++k) bp[k] = bnd[4 * p + k];
    ta::linearise_pair(Rp, dp, bp, ti, tj, s[p], a, radius, min_diag, max_diag, first_time != 0, dlt != 0, sigma + p, rec + p, P, off_blocks + 36 * p);
    gs_abs[p] = fabs(rec[(long long)ta::kGs * P + p]);
  }
}

__global__ __launch_bounds__(kThreads) void k_ta_gather(int F, long long P, const int* __restrict__ row_off, const int* __restrict__ ent, const double* __restrict__ rec,
                                                        double* __restrict__ cam, double* __restrict__ diag_blocks) {
  const int lane = (int)threadIdx.x % ta::kGroup, per_block = kThreads / ta::kGroup;
  // the trip count is uniform over the workgroup: every lane of a group takes part in the butterfly, a group past F with an empty row
  for (long long c0 = (long long)blockIdx.x * per_block; c0 < F; c0 += (long long)gridDim.x * per_block) {
    const long long c = c0 + (int)threadIdx.x / ta::kGroup;
    const bool live = c < F;
    double part[ta::kCam];
    ta::gather_lane(rec, P, ent, live ? row_off[c] : 0, live ? row_off[c + 1] : 0, lane, part);
#pragma unroll
    for (int k = 0; k < ta::kCam; ++k) {
      double v = part[k];
      for (int m = 1; m < ta::kGroup; m <<= 1) v += __shfl_xor(v, m, ta::kGroup);
      part[k] = v;
    }
    if (live && lane == 0) {
      for (int k = 0; k < ta::kCam; ++k) cam[ta::kCam * c + k] = part[k];
      double* B = diag_blocks + 36 * c;
      B[0] = part[0]; B[1] = part[1]; B[2] = part[2]; B[6] = part[1]; B[7] = part[3]; B[8] = part[4]; B[12] = part[2]; B[13] = part[4]; B[14] = part[5];
    }
  }
}

// out[col * out_stride + b] = the node over in[col * in_stride + b * kChunk ..]
template <bool MAX> __global__ __launch_bounds__(ta::kChunk) void k_ta_tree(const double* __restrict__ in, long long n, long long in_stride, double* __restrict__ out,
                                                                             long long out_stride) {
  __shared__ double buf[ta::kChunk];
  const long long j = (long long)blockIdx.x * ta::kChunk + threadIdx.x;
  buf[threadIdx.x] = j < n ? in[(long long)blockIdx.y * in_stride + j] : 0.0;
  __syncthreads();
  for (int s = ta::kChunk / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) buf[threadIdx.x] = ta::tree_op<MAX>(buf[threadIdx.x], buf[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(long long)blockIdx.y * out_stride + blockIdx.x] = buf[0];
}

__global__ __launch_bounds__(kThreads) void k_ta_cost(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R,
                                                      const double* __restrict__ d, const double* __restrict__ bnd, const double* __restrict__ t,
                                                      const double* __restrict__ s, double a, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double Rp[9], dp[3], bp[4], ti[3], tj[3];
    for (int k = 0; k < 9; ++k) Rp[k] = R[9 * p + k];
    for (int k = 0; k < 3; ++k) { dp[k] = d[3 * p + k]; ti[k] = t[3 * (long long)first[p] + k]; tj[k] = t[3 * (long long)second[p] + k]; }
    for (int k = 0; k < 4; ++k) bp[k] = bnd[4 * p + k];
    terms[p] = ta::pair_cost(Rp, dp, bp, ti, tj, s[p], a);
  }
}

// candidate translations and the cameras' terms: [0] = |step|^2, [1] = |t|^2
__global__ __launch_bounds__(kThreads) void k_ta_cam_step(int F, const double* __restrict__ t, const double* __restrict__ step, double* __restrict__ t_cand,
                                                          double* __restrict__ cterms) {
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < F; c += (long long)gridDim.x * kThreads) {
    const double x = t[3 * c], y = t[3 * c + 1], z = t[3 * c + 2], dx = step[3 * c], dy = step[3 * c + 1], dz = step[3 * c + 2];
    t_cand[3 * c] = x + dx; t_cand[3 * c + 1] = y + dy; t_cand[3 * c + 2] = z + dz;
    cterms[c] = dx * dx + dy * dy + dz * dz; cterms[F + c] = x * x + y * y + z * z;
  }
}

__global__ __launch_bounds__(kThreads) void k_ta_step(int P, const int* __restrict__ first, const int* __restrict__ second, const double* __restrict__ R,
                                                      const double* __restrict__ d, const double* __restrict__ bnd, const double* __restrict__ rec,
                                                      const double* __restrict__ step, const double* __restrict__ t_cand, const double* __restrict__ s, double a,
                                                      double* __restrict__ s_cand, double* __restrict__ terms) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kThreads) {
    double Rp[9], dp[3], bp[4], di[3], dj[3], ci[3], cj[3], sc;
    const long long i = first[p], j = second[p];
    for (int k = 0; k < 9; ++k) Rp[k] = R[9 * p + k];
    for (int k = 0; k < 3; ++k) { dp[k] = d[3 * p + k]; di[k] = step[3 * i + k]; dj[k] = step[3 * j + k]; ci[k] = t_cand[3 * i + k]; cj[k] = t_cand[3 * j + k]; }
    for (int k = 0; k < 4; ++k) bp[k] = bnd[4 * p + k];
    ta::step_pair(Rp, dp, bp, rec + p, P, di, dj, ci, cj, s[p], a, &sc, terms + p, P);
    s_cand[p] = sc;
  }
}

// wall clock of the stages of a call, each of which ends in a wait for the stream: `kernels` = the evaluations, gathers, steps and reductions with their copies,
// `solve` = the camera system (plan, assembly, factorisation, substitution).  Printed on stderr when PVLM_TRANSAVG_PROFILE is set (tools/transavg_bench.py).
struct StageClock {
  double kernels_ms = 0, solve_ms = 0; int solves = 0;
  std::chrono::steady_clock::time_point t0;
  void start() { t0 = std::chrono::steady_clock::now(); }
  double stop() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

unsigned grid_for(long long n, int per_block, long long limit) { const long long g = (n + per_block - 1) / per_block; return (unsigned)(g < 1 ? 1 : (g > limit ? limit : g)); }

struct DeviceBackend {
  pvlm_call& c; ta::Options opt; int F, P; long long blocks_limit;
  ta::CameraSystem sys;
  int *d_first = nullptr, *d_second = nullptr, *d_off = nullptr, *d_ent = nullptr;
  double *d_R = nullptr, *d_d = nullptr, *d_bnd = nullptr, *d_sigma = nullptr, *d_rec = nullptr, *d_blocks = nullptr, *d_cam = nullptr, *d_step = nullptr, *d_terms = nullptr,
         *d_cterms = nullptr, *d_gs = nullptr, *d_part[2] = {nullptr, nullptr};
  double *d_t[2] = {nullptr, nullptr}, *d_s[2] = {nullptr, nullptr};
  int cur = 0; bool dlt = false;
  std::vector<double> cam, step;
  long long part_stride = 1;
  StageClock clock;

  DeviceBackend(pvlm_call& call, const ta::Options& o, int F_, int P_) : c(call), opt(o), F(F_), P(P_) { blocks_limit = pvlm_i_env_limit("PVLM_TRANSAVG_MAX_BLOCKS", kMaxBlocks); }

  void setup(const int* first, const int* second, const double* R, const double* d, const double* bnd, const double* t0, const double* s0, int origin) {
    std::vector<int> off, ent;
    ta::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, origin);
    d_first = c.upload(first, (size_t)P); d_second = c.upload(second, (size_t)P);
    d_off = c.upload(off.data(), off.size()); d_ent = c.upload(ent.data(), ent.size());
    d_R = c.upload(R, 9 * (size_t)P); d_d = c.upload(d, 3 * (size_t)P); d_bnd = c.upload(bnd, 4 * (size_t)P);
    d_t[0] = c.upload(t0, 3 * (size_t)F); d_t[1] = c.alloc<double>(3 * (size_t)F);
    d_s[0] = c.upload(s0, (size_t)P); d_s[1] = c.alloc<double>((size_t)P);
    d_sigma = c.alloc<double>((size_t)P); d_rec = c.alloc<double>((size_t)ta::kPairSlots * (size_t)P);
    d_blocks = c.alloc<double>(36 * ((size_t)F + (size_t)P)); d_cam = c.alloc<double>((size_t)ta::kCam * (size_t)F);
    d_step = c.alloc<double>(3 * (size_t)F); d_terms = c.alloc<double>((size_t)ta::kPairTerms * (size_t)P); d_cterms = c.alloc<double>(2 * (size_t)F);
    d_gs = c.alloc<double>((size_t)P);
    const long long most = P > F ? P : F;
    part_stride = (most + ta::kChunk - 1) / ta::kChunk;
    for (int k = 0; k < 2; ++k) d_part[k] = c.alloc<double>((size_t)ta::kPairTerms * (size_t)part_stride);
    c.memset(d_blocks, 0, 36 * ((size_t)F + (size_t)P) * sizeof(double));
    cam.assign((size_t)ta::kCam * (size_t)F, 0.0);
  }
  bool failed() const { return c.st != PVLM_OK; }

  // the roots of `cols` trees over in[col * in_stride + 0 .. n) land in out[0 .. cols) at the next sync
  template <bool MAX> void reduce(const double* in, long long n, long long in_stride, int cols, double* out) {
    int k = 0;
    for (;;) {
      const long long m = (n + ta::kChunk - 1) / ta::kChunk;
      c.launch(k_ta_tree<MAX>, dim3((unsigned)m, (unsigned)cols), dim3(ta::kChunk), 0, in, n, in_stride, d_part[k], m);
      in = d_part[k]; in_stride = m; n = m; k ^= 1;
      if (m == 1) break;
    }
    c.check_launches();
    c.d2h(out, in, (size_t)cols * sizeof(double));
  }

  double initial_cost() {
    double cost = 0.0;
    clock.start();
    c.launch(k_ta_cost, dim3(grid_for(P, kThreads, blocks_limit)), dim3(kThreads), 0, P, d_first, d_second, d_R, d_d, d_bnd, d_t[cur], d_s[cur], opt.loss_a, d_terms);
    reduce<false>(d_terms, P, P, 1, &cost);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    return bad ? std::nan("") : cost;
  }
  double linearise(double radius, bool first) {
    double gs_max = 0.0;
    clock.start();
    c.launch(k_ta_pairs, dim3(grid_for(P, kThreads, blocks_limit)), dim3(kThreads), 0, P, d_first, d_second, d_R, d_d, d_bnd, d_t[cur], d_s[cur], opt.loss_a, radius,
             opt.min_lm_diagonal, opt.max_lm_diagonal, first ? 1 : 0, dlt ? 1 : 0, d_sigma, d_rec, d_blocks + 36 * (size_t)F, d_gs);
    c.launch(k_ta_gather, dim3(grid_for(F, kThreads / ta::kGroup, blocks_limit)), dim3(kThreads), 0, F, (long long)P, d_off, d_ent, d_rec, d_cam, d_blocks);
    reduce<true>(d_gs, P, P, 1, &gs_max);
    c.d2h(cam.data(), d_cam, cam.size() * sizeof(double));
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return 0.0;
    if (first && !dlt) sys.set_sigma(cam.data());
    return std::fmax(gs_max, sys.gradient_max(cam.data()));
  }
  // info of the factorisation in *info_out when given
  bool solve(double radius, int* info_out = nullptr) {
    if (failed()) return false;
    sys.prepare(cam.data(), !dlt, radius, opt);
    int info = 0;
    clock.start();
    const pvlm_status st = pvlm_i_spd_solve_blocks(c.ctx, sys.n, F + P, sys.rows.data(), sys.cols.data(), sys.mirror.data(), d_blocks, true, sys.sigma.data(),
                                                   sys.diag.data(), sys.rhs.data(), &info);
    clock.solve_ms += clock.stop(); ++clock.solves;
    if (st) { c.st = st; return false; }
    if (info_out) *info_out = info;
    if (info != 0) return false;
    sys.expand(&step);
    c.h2d(d_step, step.data(), step.size() * sizeof(double));
    return !failed();
  }
  ta::Scalars candidate() {
    double pt[ta::kPairTerms] = {0, 0, 0, 0}, ct[2] = {0, 0};
    clock.start();
    c.launch(k_ta_cam_step, dim3(grid_for(F, kThreads, blocks_limit)), dim3(kThreads), 0, F, d_t[cur], d_step, d_t[cur ^ 1], d_cterms);
    c.launch(k_ta_step, dim3(grid_for(P, kThreads, blocks_limit)), dim3(kThreads), 0, P, d_first, d_second, d_R, d_d, d_bnd, d_rec, d_step, d_t[cur ^ 1], d_s[cur],
             opt.loss_a, d_s[cur ^ 1], d_terms);
    reduce<false>(d_terms, P, P, ta::kPairTerms, pt);          // the staged copy of the roots is ordered on the stream before the next tree reuses the partials
    reduce<false>(d_cterms, F, F, 2, ct);
    const bool bad = c.sync() != PVLM_OK;
    clock.kernels_ms += clock.stop();
    if (bad) return ta::Scalars{std::nan(""), 0, 0, 0};
    return ta::Scalars{pt[ta::kTermCost], pt[ta::kTermModel], pt[ta::kTermStep2] + ct[0], pt[ta::kTermX2] + ct[1]};
  }
  void accept() { cur ^= 1; }
};

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
  ta::Options opt;
  DeviceBackend be(c, opt, F, P);
  be.dlt = true;
  const std::vector<double> zeros(3 * (size_t)F + 4 * (size_t)P, 0.0);
  be.setup(first, second, R_21, t_21, zeros.data(), zeros.data(), zeros.data(), 0);
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
  static_assert(sizeof(ta::Summary) == sizeof(pvlm_transavg_summary), "pvlm_transavg_summary is the core's Summary");
  const char* who = "pvlm_transavg_solve";
  if (!ctx) return PVLM_ERR_ARG;
  if (!params || !summary || !translations || (n_pairs > 0 && (!scales || !weight))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = ta::check_pairs(n_cameras, n_pairs, first, second, R_21, t_21)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const int F = n_cameras, P = n_pairs;
  if (origin_idx < 0 || origin_idx >= F) { PVLM_SET_ERR(ctx, "%s: origin_idx names no camera", who); return PVLM_ERR_ARG; }
  if (params->max_num_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_num_iterations < 0", who); return PVLM_ERR_ARG; }
  if (!ta::finite_all(translations, 3 * (size_t)F) || !ta::finite_all(scales, (size_t)P) || !std::isfinite(params->loss_a) || !std::isfinite(params->upper_scale_ratio) ||
      !std::isfinite(params->lower_scale_ratio)) { PVLM_SET_ERR(ctx, "%s: a translation, a scale or a parameter is not finite", who); return PVLM_ERR_ARG; }
  for (int k = 0; k < 3; ++k)
    if (translations[3 * (size_t)origin_idx + k] != 0.0) { PVLM_SET_ERR(ctx, "%s: the translation of the origin camera is not zero", who); return PVLM_ERR_ARG; }
  ta::Summary s{0.0, 0.0, 0, 0, ta::kNoPairs};
  if (P == 0) { std::memcpy(summary, &s, sizeof s); return PVLM_OK; }
  std::vector<double> d(3 * (size_t)P), bnd(4 * (size_t)P);
  for (int p = 0; p < P; ++p) { ta::direction(t_21 + 3 * (size_t)p, &d[3 * (size_t)p]); ta::bounds(scales[p], params->upper_scale_ratio, params->lower_scale_ratio, &bnd[4 * (size_t)p]); }
  const auto call_t0 = std::chrono::steady_clock::now();
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  ta::Options opt;
  opt.loss_a = params->loss_a; opt.max_num_iterations = params->max_num_iterations;
  DeviceBackend be(c, opt, F, P);
  be.setup(first, second, R_21, d.data(), bnd.data(), translations, scales, origin_idx);
  ta::lm_solve(be, opt, &s);
  std::vector<double> t_out(3 * (size_t)F), s_out((size_t)P);
  c.d2h(t_out.data(), be.d_t[be.cur], t_out.size() * sizeof(double));
  c.d2h(s_out.data(), be.d_s[be.cur], s_out.size() * sizeof(double));
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

extern "C" int pvlm_transavg_group_size(void) { return ta::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_transavg() {}
void pvlm_i_preload_transavg(hipStream_t s) { hipLaunchKernelGGL(k_preload_transavg, dim3(1), dim3(1), 0, s); }
