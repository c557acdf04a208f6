// Host-compiled check of the per-query device bodies in panovlm_amd/csrc/pvlm_assoc_core.h (K2 exact k-NN in the voxel
// grid with row pruning, K3 plane fit + certified collinearity test): the same functions k_knn_pairs / k_fit_pairs call,
// driven serially over a grid built here the way pvlm_scan_upload_batch builds it (cell edge heuristic, dense table when
// the bounding box allows, hashed table otherwise), so that the search can be compared with brute force and the fits with
// the oracle on a machine without a GPU (tests/test_assoc_core_cpu.py).  TEST INFRASTRUCTURE ONLY — libpvlm.so has no
// host path.  Build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared
#include <algorithm>
#include <cmath>
#include <vector>

#define PVLM_HD inline
static long long g_candidates = 0, g_rows_visited = 0;
#define PVLM_ASSOC_STATS_CANDIDATE() (++g_candidates)
#define PVLM_ASSOC_STATS_ROW() (++g_rows_visited)
// lockstep statistics (chk_knn_lockstep): one record per scanned run = (row-loop iteration id, run length, candidates that beat the k-th key)
struct RunRecord { int iter, len, pass; };
static std::vector<RunRecord>* g_runs = nullptr;
static int g_iter_id = 0;
#define PVLM_ASSOC_STATS_COUNT_PASS 1
#define PVLM_ASSOC_STATS_ITER(r, dz, dy, part) (g_iter_id = (((r) * 64 + (dz) + 32) * 64 + (dy) + 32) * 2 + (part))
#define PVLM_ASSOC_STATS_RUN(len, pass) do { if (g_runs) g_runs->push_back(RunRecord{g_iter_id, (len), (pass)}); } while (0)
#include "../../panovlm_amd/csrc/pvlm_assoc_core.h"

using namespace pvlm_assoc;

namespace {
struct Grid {
  std::vector<Point4> sorted;
  std::vector<unsigned long long> keys;
  std::vector<int> start, count;
  CloudView view;
};

// cloud_plan + k_grid_count / k_grid_scan / k_grid_scatter of csrc/pvlm_assoc.hip, serial
void build_grid(const float* xyz, int n, float cell_override, int force_hash, int xf_want, Grid& g) {
  float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
  for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], xyz[3 * i + k]); mx[k] = std::max(mx[k], xyz[3 * i + k]); }
  float e[3];
  for (int k = 0; k < 3; ++k) e[k] = std::max(mx[k] - mn[k], 0.05f);
  const float area = 2.f * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]);
  float h = 0.65f * std::sqrt(4.f * area / (float)std::max(n, 1));
  if (cell_override > 0) h = cell_override;
  h = std::min(std::max(h, 0.02f), 4.0f);
  float origin[3];
  for (int k = 0; k < 3; ++k) origin[k] = mn[k] - h;
  const float inv_h = 1.0f / h;
  long long dims[3];
  for (int k = 0; k < 3; ++k) dims[k] = (long long)std::ceil((mx[k] - origin[k]) * inv_h) + 2;
  const long long ncells = dims[0] * dims[1] * dims[2];
  const bool dense = ncells <= std::max<long long>(64ll * n, 4096) && ncells <= (4ll << 20) && !force_hash;
  CloudView& v = g.view;
  v = CloudView();
  v.n = n; v.xyz = xyz; v.tag = nullptr; v.ox = origin[0]; v.oy = origin[1]; v.oz = origin[2]; v.h = h; v.inv_h = inv_h;
  int xf = 1;
  if (dense) {
    xf = std::min(std::max(xf_want, 1), 16);
    while (xf > 1 && !(ncells * xf <= std::max<long long>(64ll * n, 4096) && ncells * xf <= (4ll << 20))) --xf;
  }
  v.dense = dense ? 1 : 0; v.nx = (int)dims[0] * xf; v.ny = (int)dims[1]; v.nz = (int)dims[2]; v.xf = xf;
  std::vector<int> slot((size_t)n);
  long long T;
  if (dense) {
    T = ncells * xf + 1;
    g.count.assign((size_t)T, 0); g.start.assign((size_t)T, 0);
    for (int i = 0; i < n; ++i) {
      const int ix = std::min(std::max(cell_of(xyz[3 * i], v.ox, inv_h * (float)xf), 0), v.nx - 1), iy = std::min(std::max(cell_of(xyz[3 * i + 1], v.oy, inv_h), 0), v.ny - 1),
                iz = std::min(std::max(cell_of(xyz[3 * i + 2], v.oz, inv_h), 0), v.nz - 1);
      slot[(size_t)i] = (iz * v.ny + iy) * v.nx + ix;
      ++g.count[(size_t)slot[(size_t)i]];
    }
    v.mask = 0;
  } else {
    T = 1024; while (T < 2ll * n) T <<= 1;
    g.keys.assign((size_t)T, PVLM_EMPTY_KEY); g.count.assign((size_t)T, 0); g.start.assign((size_t)T, 0);
    const int mask = (int)T - 1;
    for (int i = 0; i < n; ++i) {
      const unsigned long long key = cell_key(cell_of(xyz[3 * i], v.ox, inv_h), cell_of(xyz[3 * i + 1], v.oy, inv_h), cell_of(xyz[3 * i + 2], v.oz, inv_h));
      int s = (int)(mix64(key) & (unsigned long long)mask);
      while (g.keys[(size_t)s] != PVLM_EMPTY_KEY && g.keys[(size_t)s] != key) s = (s + 1) & mask;
      g.keys[(size_t)s] = key;
      slot[(size_t)i] = s; ++g.count[(size_t)s];
    }
    v.mask = mask;
  }
  int run = 0;
  for (long long c = 0; c < T; ++c) { g.start[(size_t)c] = run; run += g.count[(size_t)c]; }
  std::vector<int> cursor((size_t)T, 0);
  g.sorted.resize((size_t)std::max(n, 1));
  // reverse insertion order inside a cell on purpose: the device's order is arbitrary (atomic cursor), the result must not depend on it
  for (int i = n - 1; i >= 0; --i) {
    const int s = slot[(size_t)i];
    Point4 p; p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2]; p.w = u2f((unsigned)i);
    g.sorted[(size_t)(g.start[(size_t)s] + cursor[(size_t)s]++)] = p;
  }
  v.sorted = g.sorted.data(); v.keys = g.keys.empty() ? nullptr : g.keys.data(); v.cell_start = g.start.data(); v.cell_count = g.count.data();
}
}  // namespace

extern "C" {

// k = 5 or 10; xf = refinement of the dense table along x (the library default is 4).  stats[0] = candidates scanned, stats[1] = (z, y) rows visited, stats[2] = 1 when the grid is dense
int chk_knn(const float* tgt, int n, const float* q, int nq, int k, float max_dist, float cell_override, int force_hash, int xf, int* idx, float* sqd, long long* stats) {
  Grid g;
  build_grid(tgt, n, cell_override, force_hash, xf, g);
  g_candidates = 0; g_rows_visited = 0;
  const float thr2 = max_dist * max_dist;
  for (int i = 0; i < nq; ++i) {
    if (k == 10) {
      TopK<10> tk;
      knn_search<10>(g.view, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, thr2, tk);
      for (int j = 0; j < 10; ++j) { idx[(size_t)i * 10 + j] = tk.index(j); sqd[(size_t)i * 10 + j] = tk.dist(j); }
    } else if (k == 5) {
      TopK<5> tk;
      knn_search<5>(g.view, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, thr2, tk);
      for (int j = 0; j < 5; ++j) { idx[(size_t)i * 5 + j] = tk.index(j); sqd[(size_t)i * 5 + j] = tk.dist(j); }
    } else {
      return -1;
    }
  }
  if (stats) { stats[0] = g_candidates; stats[1] = g_rows_visited; stats[2] = g.view.dense; }
  return 0;
}

// Divergence statistics of the search as a wave runs it: the queries of a wave (64 consecutive ones) walk the same (r, dz, dy) loop,
// each scanning its own run; a wave pays max-over-lanes per iteration.  Per query: out_n[i] records starting at out_off[i] in rec (iter, len, pass).
long long chk_knn_lockstep(const float* tgt, int n, const float* q, int nq, float max_dist, int* rec, long long cap, long long* out_off) {
  Grid g;
  build_grid(tgt, n, 0.f, 0, 4, g);
  std::vector<RunRecord> runs;
  g_runs = &runs;
  const float thr2 = max_dist * max_dist;
  long long total = 0;
  for (int i = 0; i < nq; ++i) {
    runs.clear();
    TopK<10> tk;
    knn_search<10>(g.view, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, thr2, tk);
    out_off[i] = total;
    for (const RunRecord& r : runs) { if (total < cap) { rec[3 * total] = r.iter; rec[3 * total + 1] = r.len; rec[3 * total + 2] = r.pass; } ++total; }
  }
  out_off[nq] = total;
  g_runs = nullptr;
  return total;
}

// pts: m x 10 x 3 (row-major).  plane_ok[m], plane[m x 4], line[m]: the two decisions of K3 for every 10-point set
void chk_fit(const double* pts, int m, double plane_tol, double line_tol, int* plane_ok, double* plane, int* line) {
  for (int s = 0; s < m; ++s) {
    double px[10], py[10], pz[10];
    for (int i = 0; i < 10; ++i) { px[i] = pts[(size_t)s * 30 + 3 * i]; py[i] = pts[(size_t)s * 30 + 3 * i + 1]; pz[i] = pts[(size_t)s * 30 + 3 * i + 2]; }
    plane_ok[s] = Fit10::form_plane(px, py, pz, plane_tol, plane + 4 * (size_t)s) ? 1 : 0;
    line[s] = Fit10::is_line(px, py, pz, line_tol) ? 1 : 0;
  }
}

// the closed-form screen alone on m symmetric matrices (a00 a01 a02 a11 a12 a22): decision (-1 = left to the exact loop) and the
// eigenvalues it computed — accuracy and fall-back rate for the test
void chk_line_screen(const double* A, int m, double tol, int* decision, double* eig) {
  for (int s = 0; s < m; ++s) decision[s] = Fit10::line_screen(A[6 * s], A[6 * s + 1], A[6 * s + 2], A[6 * s + 3], A[6 * s + 4], A[6 * s + 5], tol, eig + 3 * (size_t)s);
}

// how many Jacobi sweeps the certified test ran before deciding (statistics for DESIGN.md), -1 = ran to the oracle's termination
long long chk_line_sweeps(const double* pts, int m, double line_tol, int screen, int* hist13) {
  long long total = 0;
  for (int k = 0; k < 13; ++k) hist13[k] = 0;
  for (int s = 0; s < m; ++s) {
    double px[10], py[10], pz[10];
    for (int i = 0; i < 10; ++i) { px[i] = pts[(size_t)s * 30 + 3 * i]; py[i] = pts[(size_t)s * 30 + 3 * i + 1]; pz[i] = pts[(size_t)s * 30 + 3 * i + 2]; }
    int sweeps = 0;
    Fit10::is_line(px, py, pz, line_tol, &sweeps, screen != 0);
    ++hist13[std::min(sweeps, 12)];
    total += sweeps;
  }
  return total;
}

// the collinearity decision from the raw moments (Fit10::is_line_fast, the streaming kernel's form) next to the reference's (is_line): decided[s] = 1 / 0 / -1,
// exact[s] = 1 / 0.  Returns the number of decided sets that differ (must be 0).
long long chk_is_line_fast(const double* pts, int m, double tol, int* decided, int* exact) {
  long long wrong = 0;
  for (int s = 0; s < m; ++s) {
    double px[10], py[10], pz[10];
    for (int i = 0; i < 10; ++i) { px[i] = pts[(size_t)s * 30 + 3 * i]; py[i] = pts[(size_t)s * 30 + 3 * i + 1]; pz[i] = pts[(size_t)s * 30 + 3 * i + 2]; }
    decided[s] = Fit10::is_line_fast(px, py, pz, tol);
    exact[s] = Fit10::is_line(px, py, pz, tol) ? 1 : 0;
    if (decided[s] >= 0 && decided[s] != exact[s]) ++wrong;
  }
  return wrong;
}

// the certified fast fit (Fit10::form_plane_fast) against the exact path on m 10-point sets.  Per set, out8 = [decision of the fast fit (1 / 0 / -1),
// decision of form_plane, E (its bound on ||x - x_qr||), ||x - x_qr|| measured, ||x - x_ref|| and ||x_qr - x_ref|| against a __float128 solve of the
// normal equations (only when quad != 0; else 0), B (its bound on the distance), |max distance of the fast fit - max distance the exact path evaluates|].
// With quad, out8[2] / out8[6] are replaced by the two shares E_fast / E_qr of the bound.  Returns the number of sets where a DECIDED fast answer differs from form_plane's (must be 0).
long long chk_fit_fast(const double* pts, int m, double tol, int quad, double* out8, double* plane_fast) {
  long long wrong = 0;
  for (int s = 0; s < m; ++s) {
    double px[10], py[10], pz[10];
    for (int i = 0; i < 10; ++i) { px[i] = pts[(size_t)s * 30 + 3 * i]; py[i] = pts[(size_t)s * 30 + 3 * i + 1]; pz[i] = pts[(size_t)s * 30 + 3 * i + 2]; }
    double* o = out8 + 8 * (size_t)s;
    for (int k = 0; k < 8; ++k) o[k] = 0.0;
    double pf[4] = {0, 0, 0, 0}, pe[4], pall[4], diag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int fast = Fit10::form_plane_fast(px, py, pz, tol, pf, diag);
    const bool exact = Fit10::form_plane(px, py, pz, tol, pe);
    o[0] = fast; o[1] = exact ? 1 : 0;
    if (plane_fast) for (int k = 0; k < 4; ++k) plane_fast[4 * (size_t)s + k] = fast == 1 ? pf[k] : pe[k];
    if (fast >= 0 && fast != (exact ? 1 : 0)) ++wrong;
    if (fast < 0 && diag[3] == 0.0) continue;                               // refused before a solution existed
    Fit10::form_plane(px, py, pz, 1e300, pall);                             // the QR's plane whatever the tolerance: x_qr = n / d
    if (!(pall[3] > 0.0)) continue;
    const double xq[3] = {pall[0] / pall[3], pall[1] / pall[3], pall[2] / pall[3]};
    o[2] = diag[3];
    o[3] = std::sqrt((diag[0] - xq[0]) * (diag[0] - xq[0]) + (diag[1] - xq[1]) * (diag[1] - xq[1]) + (diag[2] - xq[2]) * (diag[2] - xq[2]));
    double dmax = 0.0;
    for (int i = 0; i < 10; ++i) dmax = std::max(dmax, std::fabs((pall[0] * px[i] + pall[1] * py[i]) + pall[2] * pz[i] + pall[3]));
    o[6] = diag[5]; o[7] = std::fabs(diag[4] - dmax);
    if (quad) {
      __float128 M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, sv[3] = {0, 0, 0};
      for (int i = 0; i < 10; ++i) {
        const __float128 p[3] = {px[i], py[i], pz[i]};
        for (int a = 0; a < 3; ++a) { sv[a] += p[a]; for (int b = 0; b < 3; ++b) M[a][b] += p[a] * p[b]; }
      }
      const __float128 c00 = M[1][1] * M[2][2] - M[1][2] * M[1][2], c01 = M[1][2] * M[0][2] - M[0][1] * M[2][2], c02 = M[0][1] * M[1][2] - M[1][1] * M[0][2];
      const __float128 c11 = M[0][0] * M[2][2] - M[0][2] * M[0][2], c12 = M[0][1] * M[0][2] - M[0][0] * M[1][2], c22 = M[0][0] * M[1][1] - M[0][1] * M[0][1];
      const __float128 det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
      const __float128 xr[3] = {-(c00 * sv[0] + c01 * sv[1] + c02 * sv[2]) / det, -(c01 * sv[0] + c11 * sv[1] + c12 * sv[2]) / det, -(c02 * sv[0] + c12 * sv[1] + c22 * sv[2]) / det};
      double a = 0.0, b = 0.0;
      for (int k = 0; k < 3; ++k) { const double d1 = (double)((__float128)diag[k] - xr[k]), d2 = (double)((__float128)xq[k] - xr[k]); a += d1 * d1; b += d2 * d2; }
      o[4] = std::sqrt(a); o[5] = std::sqrt(b); o[2] = diag[6]; o[6] = diag[7];
    }
  }
  return wrong;
}

// The RECORD of an accepted fast fit: decide() stores y = x - M^-1 rho, not the x whose residuals it certified.  Per set, out4 = [1 when the fast fit accepted (else the
// rest is 0), ||y - x_qr|| with y = n / d recovered from the stored plane, E (the bound the decision was certified under), ||y - x_ref|| against the __float128 solve of the
// normal equations (quad != 0) ] and, in out4[3] when quad == 0, E_fast (the share of E the derivation gives the fast side).  share[s] = E_fast always.
void chk_fit_fast_record(const double* pts, int m, double tol, int quad, double* out4, double* share) {
  for (int s = 0; s < m; ++s) {
    double px[10], py[10], pz[10];
    for (int i = 0; i < 10; ++i) { px[i] = pts[(size_t)s * 30 + 3 * i]; py[i] = pts[(size_t)s * 30 + 3 * i + 1]; pz[i] = pts[(size_t)s * 30 + 3 * i + 2]; }
    double* o = out4 + 4 * (size_t)s;
    o[0] = o[1] = o[2] = o[3] = 0.0; share[s] = 0.0;
    double pf[4] = {0, 0, 0, 0}, pall[4], diag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (Fit10::form_plane_fast(px, py, pz, tol, pf, diag) != 1) continue;
    Fit10::form_plane(px, py, pz, 1e300, pall);
    if (!(pall[3] > 0.0) || !(pf[3] > 0.0)) continue;
    const double y[3] = {pf[0] / pf[3], pf[1] / pf[3], pf[2] / pf[3]}, xq[3] = {pall[0] / pall[3], pall[1] / pall[3], pall[2] / pall[3]};
    o[0] = 1.0;
    o[1] = std::sqrt((y[0] - xq[0]) * (y[0] - xq[0]) + (y[1] - xq[1]) * (y[1] - xq[1]) + (y[2] - xq[2]) * (y[2] - xq[2]));
    o[2] = diag[3]; share[s] = diag[6];
    if (quad) {
      __float128 M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, sv[3] = {0, 0, 0};
      for (int i = 0; i < 10; ++i) {
        const __float128 p[3] = {px[i], py[i], pz[i]};
        for (int a = 0; a < 3; ++a) { sv[a] += p[a]; for (int b = 0; b < 3; ++b) M[a][b] += p[a] * p[b]; }
      }
      const __float128 c00 = M[1][1] * M[2][2] - M[1][2] * M[1][2], c01 = M[1][2] * M[0][2] - M[0][1] * M[2][2], c02 = M[0][1] * M[1][2] - M[1][1] * M[0][2];
      const __float128 c11 = M[0][0] * M[2][2] - M[0][2] * M[0][2], c12 = M[0][1] * M[0][2] - M[0][0] * M[1][2], c22 = M[0][0] * M[1][1] - M[0][1] * M[0][1];
      const __float128 det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
      const __float128 xr[3] = {-(c00 * sv[0] + c01 * sv[1] + c02 * sv[2]) / det, -(c01 * sv[0] + c11 * sv[1] + c12 * sv[2]) / det, -(c02 * sv[0] + c12 * sv[1] + c22 * sv[2]) / det};
      double a = 0.0;
      for (int k = 0; k < 3; ++k) { const double d1 = (double)((__float128)y[k] - xr[k]); a += d1 * d1; }
      o[3] = std::sqrt(a);
    }
  }
}

}  // extern "C"
