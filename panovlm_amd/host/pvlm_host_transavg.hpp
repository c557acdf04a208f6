// K42 on the host: the definition of csrc/pvlm_transavg_core.h (translation averaging) behind a host backend that does what the kernels of csrc/pvlm_transavg.hip do —
// the per-pair linearisation, the per-camera gather over kGroup lanes and their butterfly, the fixed reduction tree, the back-substitution — with a dense host
// Cholesky of the camera system in place of the library's solver.  No device, no dependency on the rest of the host mirror: the equality partner of
// pvlm_transavg_solve / pvlm_transavg_dlt (tests/cpp/transavg_core_check.cpp) and the `host` route of EstimateGlobalTranslation (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_transavg_core.h"

namespace pvlm {
namespace transavg_detail {

namespace ta = pvlm_transavg;

struct HostBackend {
  ta::Options opt; int F, P; bool dlt = false;
  const int *first, *second; const double *R;
  std::vector<double> d, bnd, sigma, rec, blocks, cam, step, terms, cterms, gs;
  std::vector<double> t[2], s[2];
  std::vector<int> off, ent;
  ta::CameraSystem sys;
  int cur = 0, info = 0;

  HostBackend(const ta::Options& o, int F_, int P_, const int* fi, const int* se, const double* R_, const double* d_, const double* bnd_, const double* t0, const double* s0,
              int origin) : opt(o), F(F_), P(P_), first(fi), second(se), R(R_), d(d_, d_ + 3 * (size_t)P_), bnd(bnd_, bnd_ + 4 * (size_t)P_) {
    ta::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, origin);
    sigma.assign((size_t)P, 0.0); rec.assign((size_t)ta::kPairSlots * P, 0.0); blocks.assign(36 * ((size_t)F + P), 0.0); cam.assign((size_t)ta::kCam * F, 0.0);
    terms.assign((size_t)ta::kPairTerms * P, 0.0); cterms.assign(2 * (size_t)F, 0.0); gs.assign((size_t)P, 0.0);
    t[0].assign(t0, t0 + 3 * (size_t)F); t[1] = t[0]; s[0].assign(s0, s0 + (size_t)P); s[1] = s[0];
  }
  bool failed() const { return false; }
  double initial_cost() {
    for (int p = 0; p < P; ++p)
      terms[(size_t)p] = ta::pair_cost(R + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &t[cur][3 * (size_t)first[p]], &t[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a);
    return ta::tree_reduce_host<false>(terms.data(), P);
  }
  double linearise(double radius, bool first_time) {
    for (int p = 0; p < P; ++p) {
      ta::linearise_pair(R + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &t[cur][3 * (size_t)first[p]], &t[cur][3 * (size_t)second[p]], s[cur][(size_t)p], opt.loss_a,
                         radius, opt.min_lm_diagonal, opt.max_lm_diagonal, first_time, dlt, &sigma[(size_t)p], &rec[(size_t)p], P, &blocks[36 * ((size_t)F + p)]);
      gs[(size_t)p] = std::fabs(rec[(size_t)ta::kGs * P + p]);
    }
    for (int c = 0; c < F; ++c) {
      double part[ta::kGroup][ta::kCam], nxt[ta::kGroup][ta::kCam];
      for (int l = 0; l < ta::kGroup; ++l) ta::gather_lane(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, part[l]);
      for (int m = 1; m < ta::kGroup; m <<= 1) {                      // the xor butterfly of the lane group
        for (int l = 0; l < ta::kGroup; ++l) for (int k = 0; k < ta::kCam; ++k) nxt[l][k] = part[l][k] + part[l ^ m][k];
        std::memcpy(part, nxt, sizeof part);
      }
      const double* v = part[0];
      for (int k = 0; k < ta::kCam; ++k) cam[(size_t)ta::kCam * c + k] = v[k];
      double* B = &blocks[36 * (size_t)c];
      B[0] = v[0]; B[1] = v[1]; B[2] = v[2]; B[6] = v[1]; B[7] = v[3]; B[8] = v[4]; B[12] = v[2]; B[13] = v[4]; B[14] = v[5];
    }
    if (first_time && !dlt) sys.set_sigma(cam.data());
    return std::fmax(ta::tree_reduce_host<true>(gs.data(), P), sys.gradient_max(cam.data()));
  }
  // M = D (sum of blocks) D + diag, dense; Cholesky; the solution replaces sys.rhs
  bool solve(double radius) {
    sys.prepare(cam.data(), !dlt, radius, opt);
    const int n = sys.n;
    std::vector<double> M((size_t)n * n, 0.0);
    for (size_t b = 0; b < (size_t)F + P; ++b)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
          const int i = sys.rows[6 * b + r], j = sys.cols[6 * b + c];
          if (i < 0 || j < 0) continue;
          const double v = blocks[36 * b + 6 * r + c] * sys.sigma[(size_t)i] * sys.sigma[(size_t)j];
          M[(size_t)i * n + j] += v;
          if (sys.mirror[b]) M[(size_t)j * n + i] += v;
        }
    for (int i = 0; i < n; ++i) M[(size_t)i * n + i] += sys.diag[(size_t)i];
    info = 0;
    for (int j = 0; j < n; ++j) {
      double v = M[(size_t)j * n + j];
      for (int k = 0; k < j; ++k) v -= M[(size_t)j * n + k] * M[(size_t)j * n + k];
      if (!(v > 0.0)) { info = j + 1; return false; }
      const double l = std::sqrt(v);
      M[(size_t)j * n + j] = l;
      for (int i = j + 1; i < n; ++i) {
        double w = M[(size_t)i * n + j];
        for (int k = 0; k < j; ++k) w -= M[(size_t)i * n + k] * M[(size_t)j * n + k];
        M[(size_t)i * n + j] = w / l;
      }
    }
    std::vector<double>& x = sys.rhs;
    for (int i = 0; i < n; ++i) { double w = x[(size_t)i]; for (int k = 0; k < i; ++k) w -= M[(size_t)i * n + k] * x[(size_t)k]; x[(size_t)i] = w / M[(size_t)i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { double w = x[(size_t)i]; for (int k = i + 1; k < n; ++k) w -= M[(size_t)k * n + i] * x[(size_t)k]; x[(size_t)i] = w / M[(size_t)i * n + i]; }
    sys.expand(&step);
    return true;
  }
  ta::Scalars candidate() {
    std::vector<double>& tc = t[cur ^ 1]; const std::vector<double>& tn = t[cur];
    for (int c = 0; c < F; ++c) {
      const double x = tn[3 * (size_t)c], y = tn[3 * (size_t)c + 1], z = tn[3 * (size_t)c + 2], dx = step[3 * (size_t)c], dy = step[3 * (size_t)c + 1], dz = step[3 * (size_t)c + 2];
      tc[3 * (size_t)c] = x + dx; tc[3 * (size_t)c + 1] = y + dy; tc[3 * (size_t)c + 2] = z + dz;
      cterms[(size_t)c] = dx * dx + dy * dy + dz * dz; cterms[(size_t)F + c] = x * x + y * y + z * z;
    }
    for (int p = 0; p < P; ++p) {
      const size_t i = (size_t)first[p], j = (size_t)second[p];
      ta::step_pair(R + 9 * (size_t)p, &d[3 * (size_t)p], &bnd[4 * (size_t)p], &rec[(size_t)p], P, &step[3 * i], &step[3 * j], &tc[3 * i], &tc[3 * j], s[cur][(size_t)p], opt.loss_a,
                    &s[cur ^ 1][(size_t)p], &terms[(size_t)p], P);
    }
    double pt[ta::kPairTerms];
    for (int k = 0; k < ta::kPairTerms; ++k) pt[k] = ta::tree_reduce_host<false>(&terms[(size_t)k * P], P);
    const double c0 = ta::tree_reduce_host<false>(&cterms[0], F), c1 = ta::tree_reduce_host<false>(&cterms[(size_t)F], F);
    return ta::Scalars{pt[ta::kTermCost], pt[ta::kTermModel], pt[ta::kTermStep2] + c0, pt[ta::kTermX2] + c1};
  }
  void accept() { cur ^= 1; }
};


// pvlm_transavg_dlt on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, or k > 0 when the system is not positive definite (out untouched).
inline int DltHost(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* out, int* info) {
  if (!info || (F > 0 && !out) || ta::check_pairs(F, P, first, second, R, t21)) return -1;
  if (P == 0) { *info = F <= 1 ? 0 : 1; if (F == 1) out[0] = out[1] = out[2] = 0.0; return 0; }
  const std::vector<double> zeros(3 * (size_t)F + 4 * (size_t)P, 0.0);
  ta::Options opt;
  HostBackend be(opt, F, P, first, second, R, t21, zeros.data(), zeros.data(), zeros.data(), 0);
  be.dlt = true;
  be.linearise(1.0, true);
  const bool ok = be.solve(1.0);
  *info = be.info;
  if (ok) std::memcpy(out, be.step.data(), 3 * (size_t)F * sizeof(double));
  return 0;
}

// pvlm_transavg_solve on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.
inline int SolveHost(int F, int P, const int* first, const int* second, const double* R, const double* t21, double* scales, int origin, double* translations, double* weight,
                     double loss_a, double upper_ratio, double lower_ratio, int max_num_iterations, ta::Summary* summary) {
  if (!summary || !translations || (P > 0 && (!scales || !weight)) || ta::check_pairs(F, P, first, second, R, t21)) return -1;
  if (origin < 0 || origin >= F || max_num_iterations < 0) return -1;
  if (!ta::finite_all(translations, 3 * (size_t)F) || !ta::finite_all(scales, (size_t)P) || !std::isfinite(loss_a) || !std::isfinite(upper_ratio) || !std::isfinite(lower_ratio)) return -1;
  for (int k = 0; k < 3; ++k) if (translations[3 * (size_t)origin + k] != 0.0) return -1;
  ta::Summary s{0.0, 0.0, 0, 0, ta::kNoPairs};
  if (P > 0) {
    std::vector<double> d(3 * (size_t)P), bnd(4 * (size_t)P);
    for (int p = 0; p < P; ++p) { ta::direction(t21 + 3 * (size_t)p, &d[3 * (size_t)p]); ta::bounds(scales[p], upper_ratio, lower_ratio, &bnd[4 * (size_t)p]); }
    ta::Options opt;
    opt.loss_a = loss_a; opt.max_num_iterations = max_num_iterations;
    HostBackend be(opt, F, P, first, second, R, d.data(), bnd.data(), translations, scales, origin);
    ta::lm_solve(be, opt, &s);
    std::memcpy(translations, be.t[be.cur].data(), 3 * (size_t)F * sizeof(double));
    std::memcpy(scales, be.s[be.cur].data(), (size_t)P * sizeof(double));
    for (int p = 0; p < P; ++p)
      weight[p] = ta::final_weight(R + 9 * (size_t)p, t21 + 3 * (size_t)p, &translations[3 * (size_t)first[p]], &translations[3 * (size_t)second[p]], scales[p]);
  }
  *summary = s;
  return 0;
}

}  // namespace transavg_detail
}  // namespace pvlm
