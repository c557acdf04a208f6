// The pair-graph layer under the six stages that solve on a camera graph — K40 (rotation averaging), K42 (translation averaging), K44 (BATA), K45 (the L2 rotation
// start), K46 (chordal / LUD) and K47 (the L1 translation LP) — host and device.  The stages hang residual blocks on the pairs of a camera graph and solve for
// per-camera unknowns of three numbers; what they share is here and nothing in it knows what the unknowns are (K44, K45 and K47 take the CSR, the gather, the tree
// and the camera system, not the LM loop):
//   the CSR of the cameras' incident pairs (entry = 2 * pair + side, pair-list order) and its gather: kGroup lanes per camera, lane l takes the entries l, l + kGroup,
//     ..., an xor butterfly adds the partial sums.  One order per camera, whatever the degree, no floating-point atomics;
//   the fixed reduction tree of every scalar (cost, model decrease, norms): leaves in chunks of kChunk, a halving tree inside a chunk, the chunk sums reduced the same
//     way.  The tree depends on the count alone;
//   the camera system of one linearisation (CameraSystem: the index lists of the reduced 3 x 3 blocks, Jacobi scaling, LM diagonal) and the Levenberg-Marquardt
//     policy over a backend that evaluates, gathers, solves and steps (lm_solve).  Trust region: the constants and the policy of ceres_like::Solve
//     (host/pvlm_host.hpp Solver::Options): Jacobi scaling 1 / (1 + sqrt(H_kk)) from the first linearisation, radius / max(1/3, 1 - (2 rho - 1)^3) on success,
//     radius / 2, / 4, ... on failure, min_relative_decrease 1e-3 and the three tolerances;
//   the pair model: what one LM problem on the graph (K40's L2 stage, K42, K46's two) gives the one backend per side that lm_solve drives (see lm_solve);
//   SoftLOneLoss on a squared residual, the loss of K40's and K42's pair blocks, and HuberLoss beside it (K46's chordal blocks).
// The device half (kernels, buffers, the solver call, the LM backend) is pvlm_pairgraph.h, the host twin host/pvlm_host_pairgraph.hpp.
#pragma once
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define PVLM_PG_HD __host__ __device__ __forceinline__
#else
#define PVLM_PG_HD inline
#endif

namespace pvlm_pairgraph {

constexpr int kGroup = 8;            // lanes that share one camera's gather
constexpr int kChunk = 256;          // leaves under one node of the reduction tree
constexpr int kCam = 15;             // per camera: reduced diagonal block (6, upper triangle by rows), diagonal of the unreduced block (3), gradient (3), reduced gradient (3)
enum { kTermCost = 0, kTermModel = 1, kTermStep2 = 2, kTermX2 = 3 };      // the per-pair terms of a candidate; the last two only where the pairs have a scale
// termination codes on K36's numbering
enum { kMaxIterations = 0, kFunctionTol = 1, kGradientTol = 2, kParameterTol = 3, kRadiusCollapsed = 4, kCostNotFinite = 5, kNoPairs = 6 };

struct Options {
  double loss_a = 0.01;
  int max_num_iterations = 50;
  double initial_radius = 1e4, max_radius = 1e16, min_radius = 1e-32;
  double min_relative_decrease = 1e-3, function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
};
struct Summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; };

PVLM_PG_HD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// SoftLOneLoss(a) at s2 = |r|^2: rho(s) = 2 b (sqrt(1 + s / b) - 1), b = a^2, and rho'; none when a < 0
PVLM_PG_HD void loss(double a, double s2, double* rho, double* rho1) {
  if (a < 0) { *rho = s2; *rho1 = 1.0; return; }
  const double b = a * a, c = 1.0 / b, tmp = sqrt(1.0 + s2 * c);
  *rho = 2.0 * b * (tmp - 1.0); *rho1 = 1.0 / tmp;
}
// HuberLoss(a) at s2 = |r|^2: rho(s) = s up to a^2, 2 a sqrt(s) - a^2 past it, and rho' (K46's chordal blocks).  A NaN takes the outer branch and stays one.
PVLM_PG_HD void huber(double a, double s2, double* rho, double* rho1) {
  if (s2 <= a * a) { *rho = s2; *rho1 = 1.0; return; }
  const double r = sqrt(s2);
  *rho = 2.0 * a * r - a * a; *rho1 = a / r;
}

// lane `lane` of the kGroup lanes of one camera over a two-sided record (side 0 = first and side 1 = second as kCam numbers each, component k of pair p at
// [k * P + p]): its part of the row ent[e0 .. e1) (entry = 2 * pair + side), in list order
PVLM_PG_HD void gather_lane(const double* rec, long long P, const int* ent, int e0, int e1, int lane, double* part) {
  for (int k = 0; k < kCam; ++k) part[k] = 0.0;
  for (int e = e0 + lane; e < e1; e += kGroup) {
    const int p = ent[e] >> 1, side = ent[e] & 1;
    const double* s = rec + (long long)side * kCam * P + p;
    for (int k = 0; k < kCam; ++k) part[k] += s[(long long)k * P];
  }
}
// the same over a one-sided record: N consecutive slots from slot0; slot k takes the sign of the incidence (- for first, + for second) when bit k of signed_mask is set
template <int N> PVLM_PG_HD void gather_lane(const double* rec, long long P, const int* ent, int e0, int e1, int lane, int slot0, unsigned signed_mask, double* part) {
  for (int k = 0; k < N; ++k) part[k] = 0.0;
  for (int e = e0 + lane; e < e1; e += kGroup) {
    const int p = ent[e] >> 1, side = ent[e] & 1;
    const double* s = rec + (long long)slot0 * P + p;
    for (int k = 0; k < N; ++k) { const double v = s[(long long)k * P]; part[k] += ((signed_mask >> k) & 1u) && side == 0 ? -v : v; }
  }
}
// the first six numbers of a camera's gather (the reduced diagonal block, upper triangle by rows) into its 6 x 6 row-major block of the solver's list
PVLM_PG_HD void diagonal_block(const double* v, double* B) {
  B[0] = v[0]; B[1] = v[1]; B[2] = v[2]; B[6] = v[1]; B[7] = v[3]; B[8] = v[4]; B[12] = v[2]; B[13] = v[4]; B[14] = v[5];
}

// one node of the reduction tree: up to kChunk leaves, zero-padded, halved
template <bool MAX> PVLM_PG_HD double tree_op(double x, double y) { return MAX ? fmax(x, y) : x + y; }

// ---- host side: shared by the device entry points and by the host compile ----------------------------------------------------------------------------------

template <bool MAX> inline double tree_reduce_host(const double* v, long long n) {
  std::vector<double> cur(v, v + n), nxt;
  if (n <= 0) return 0.0;
  for (;;) {
    const long long m = ((long long)cur.size() + kChunk - 1) / kChunk;
    nxt.assign((size_t)m, 0.0);
    for (long long b = 0; b < m; ++b) {
      double buf[kChunk];
      for (int i = 0; i < kChunk; ++i) { const long long j = b * kChunk + i; buf[i] = j < (long long)cur.size() ? cur[(size_t)j] : 0.0; }
      for (int s = kChunk / 2; s > 0; s >>= 1) for (int i = 0; i < s; ++i) buf[i] = tree_op<MAX>(buf[i], buf[i + s]);
      nxt[(size_t)b] = buf[0];
    }
    cur.swap(nxt);
    if (cur.size() == 1) return cur[0];
  }
}

// the CSR of the cameras' incident pairs: entry = 2 * pair + side, in pair-list order
inline void build_csr(int F, int P, const int* first, const int* second, std::vector<int>* off, std::vector<int>* ent) {
  off->assign((size_t)F + 1, 0); ent->assign(2 * (size_t)P, 0);
  for (int p = 0; p < P; ++p) { ++(*off)[(size_t)first[p] + 1]; ++(*off)[(size_t)second[p] + 1]; }
  for (int c = 0; c < F; ++c) (*off)[(size_t)c + 1] += (*off)[(size_t)c];
  std::vector<int> at(off->begin(), off->end() - 1);
  for (int p = 0; p < P; ++p) { (*ent)[(size_t)at[(size_t)first[p]]++] = 2 * p; (*ent)[(size_t)at[(size_t)second[p]]++] = 2 * p + 1; }
}

inline bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// The camera system of one linearisation on the host's side: the index lists of the reduced blocks ([F diagonal | P off-diagonal], 6 x 6 with the last three
// indices -1), the Jacobi scale of the cameras and, per solve, the LM diagonal and the right-hand side.  cam: the gather (kCam numbers per camera).
struct CameraSystem {
  int F = 0, P = 0, origin = -1, n = 0;
  std::vector<int> rows, cols, mirror;
  std::vector<double> sigma, diag, rhs;
  int index(int c) const { return c == origin ? -1 : 3 * (c < origin || origin < 0 ? c : c - 1); }
  void init(int F_, int P_, const int* first, const int* second, int origin_) {
    F = F_; P = P_; origin = origin_; n = 3 * (origin >= 0 ? F - 1 : F);
    rows.assign(6 * ((size_t)F + P), -1); cols.assign(6 * ((size_t)F + P), -1); mirror.assign((size_t)F + P, 0);
    for (int c = 0; c < F; ++c) for (int k = 0; k < 3; ++k) if (index(c) >= 0) rows[6 * (size_t)c + k] = cols[6 * (size_t)c + k] = index(c) + k;
    for (int p = 0; p < P; ++p) {
      const size_t b = (size_t)F + p;
      mirror[b] = 1;
      for (int k = 0; k < 3; ++k) { if (index(first[p]) >= 0) rows[6 * b + k] = index(first[p]) + k; if (index(second[p]) >= 0) cols[6 * b + k] = index(second[p]) + k; }
    }
    sigma.assign((size_t)n, 1.0); diag.assign((size_t)n, 0.0); rhs.assign((size_t)n, 0.0);
  }
  void set_sigma(const double* cam) {
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) sigma[(size_t)index(c) + k] = 1.0 / (1.0 + std::sqrt(std::fmax(cam[(size_t)kCam * c + 6 + k], 0.0)));
  }
  // damped: the LM diagonal clip(sigma^2 H_kk) / radius; otherwise none (the DLT)
  void prepare(const double* cam, bool damped, double radius, const Options& o) {
    for (int c = 0; c < F; ++c) {
      if (index(c) < 0) continue;
      for (int k = 0; k < 3; ++k) {
        const size_t i = (size_t)index(c) + k; const double sg = sigma[i];
        diag[i] = damped ? clip(sg * sg * cam[(size_t)kCam * c + 6 + k], o.min_lm_diagonal, o.max_lm_diagonal) / radius : 0.0;
        rhs[i] = -sg * cam[(size_t)kCam * c + 12 + k];
      }
    }
  }
  // the solved rhs -> the step of every camera (3 F, zero at the origin)
  void expand(std::vector<double>* step) const {
    step->assign(3 * (size_t)F, 0.0);
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) (*step)[3 * (size_t)c + k] = sigma[(size_t)index(c) + k] * rhs[(size_t)index(c) + k];
  }
  double gradient_max(const double* cam) const {
    double g = 0;
    for (int c = 0; c < F; ++c) if (index(c) >= 0) for (int k = 0; k < 3; ++k) g = std::fmax(g, std::fabs(cam[(size_t)kCam * c + 9 + k]));
    return g;
  }
};

struct Scalars { double cost, model, step2, x2; };

// The LM loop.  Backend: double initial_cost(); double linearise(double radius, bool first) -> max |g|; bool solve(double radius) (false: no step);
// Scalars candidate(); void accept(); bool failed() (a device error: the loop stops).
//
// There is one backend per side, LmPairDevice (pvlm_pairgraph.h) and LmPairHost (host/pvlm_host_pairgraph.hpp), both templated on a PAIR MODEL: the definition of
// one LM problem on the graph.  A pair model is a small trivially copyable struct of the problem's per-pair input pointers and uniform scalars, passed by value to
// the kernels and used as it is by the host twin (whose pointers are host memory).  The state is one 3-vector x per camera and, where kScale, one scale s per pair.
//   static constexpr int kSlots, kTerms; static constexpr bool kScale;
//     kSlots: the numbers of a pair's record, component-major (component k of pair p at [k * P + p]): side 0 (first) and side 1 (second) as kCam numbers each, then
//       what step() needs of the linearisation.  kTerms: the per-pair terms of a candidate, 4 where kScale and 2 otherwise.
//     kScale: one private scale per pair — eliminated by a 1 x 1 pivot, Jacobi-scaled by a per-pair sigma, clamped at the candidate.  Its gradient sits in the
//       record's slot kGs (static constexpr int, only where kScale) and enters the gradient maximum; the terms kTermStep2 and kTermX2 exist iff kScale.
//   double cost(p, xi, xj, s, a): the cost term of pair p at its cameras' vectors and its scale; a = Options::loss_a;
//   void linearise(p, xi, xj, s, a, radius, min_diag, max_diag, first_time, sigma, rec, P, off): the record (rec points at the pair, stride P) and the 3 x 3 block
//     between first (rows) and second (columns) inside the 6 x 6 row-major block off.  first_time: the Jacobi scale of s is taken here (*sigma), else read;
//   void step(p, rec, P, di, dj, ci, cj, s, a, s_cand, terms, tstride): from the steps (di, dj) and the candidates (ci, cj) of its cameras the candidate scale
//     and the pair's terms: cost at the candidate, model decrease, and where kScale the squared scale step and the squared scale.
// Without kScale s is 0 and sigma and s_cand are null; a model ignores them and radius, min_diag, max_diag and first_time with them.  Every method is host /
// device, loads the pair's own inputs by p and leaves the arithmetic to its stage's core.  The models: pvlm_rotavg::L2Model, pvlm_transavg::Model,
// pvlm_transdir::Chordal and pvlm_transdir::Lud.
template <class M> PVLM_PG_HD double pair_scale(const double* s, long long p) { if constexpr (M::kScale) return s[p]; else return 0.0; }
template <class M> PVLM_PG_HD double* pair_slot(double* v, long long p) { if constexpr (M::kScale) return v + p; else return nullptr; }

template <class B> inline void lm_solve(B& be, const Options& o, Summary* out) {
  Summary s{0.0, 0.0, 0, 0, -1};
  double cost = be.initial_cost();
  s.initial_cost = cost;
  double radius = o.initial_radius, dec = 2.0;
  int it = 0;
  if (!std::isfinite(cost)) s.termination = kCostNotFinite;
  else if (o.max_num_iterations > 0 && be.linearise(radius, true) <= o.gradient_tolerance) s.termination = kGradientTol;
  while (s.termination < 0 && it < o.max_num_iterations && !be.failed()) {
    ++it;
    bool ok = be.solve(radius), accepted = false;
    Scalars c{0, 0, 0, 0};
    if (ok) { c = be.candidate(); ok = c.model > 0 && std::isfinite(c.model); }
    if (ok) {
      const double rho = (cost - c.cost) / c.model;
      if (std::isfinite(c.cost) && rho > o.min_relative_decrease) {
        accepted = true;
        const double change = cost - c.cost, prev = cost;
        be.accept();
        cost = c.cost;
        radius = std::fmin(o.max_radius, radius / std::fmax(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0)));
        dec = 2.0;
        ++s.successful_steps;
        if (std::fabs(change) <= o.function_tolerance * prev) s.termination = kFunctionTol;
        else if (be.linearise(radius, false) <= o.gradient_tolerance) s.termination = kGradientTol;
        else if (std::sqrt(c.step2) <= o.parameter_tolerance * (std::sqrt(c.x2) + o.parameter_tolerance)) s.termination = kParameterTol;
      }
    }
    if (!accepted) {
      ++s.unsuccessful_steps;
      radius /= dec; dec *= 2.0;
      if (radius < o.min_radius) s.termination = kRadiusCollapsed;
      else if (it < o.max_num_iterations) be.linearise(radius, false);
    }
  }
  if (s.termination < 0) s.termination = kMaxIterations;
  s.final_cost = cost;
  *out = s;
}

}  // namespace pvlm_pairgraph

// The LM summary and the group size were K42's before the layer existed.  The host compiles of K40 and K42 (tests/cpp/rotavg_core_check.cpp, transavg_core_check.cpp)
// name them there, and those two files must keep compiling as they stand against every later version of this header, so the names stay.
namespace pvlm_transavg {
using pvlm_pairgraph::kGroup;
using pvlm_pairgraph::Summary;
}
