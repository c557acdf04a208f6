// Host-compiled check of K31's device bodies: the two-row reprojection kinds of panovlm_amd/csrc/pvlm_reproj.h / pvlm_ba_core.h
// (PanoramaReprojResidual_2Angle / _Pixel) and the per-track filter of pvlm_sfm_filter_core.h, driven by serial loops so that
// tests/test_sfm_ba_cpu.py can compare them with numpy restatements without a GPU.  TEST INFRASTRUCTURE ONLY — libpvlm.so has no
// host path.  Built with -ffp-contract=off (the filter's decisions are compared bit for bit).
#include <algorithm>
#include <cstring>
#include <vector>

#define PVLM_HD
#define PVLM_ATOMIC_ADD(ptr, v) (*(ptr) += (v))
#define PVLM_ATOMIC_MAXPOS(ptr, v) (*(ptr) = std::max(*(ptr), (v)))
#include "../../panovlm_amd/csrc/pvlm_ba_core.h"
#include "../../panovlm_amd/csrc/pvlm_sfm_filter_core.h"

extern "C" {

struct chk_view {
  int n_points, n_cams, n_upairs; long long n_obs;
  const long long* pt_off; const int* cam; const int* obs_pt; const double* s; const double* X; double* Xc; double* scale; double* Vinv; double* gp;
  const int* adj_off; const int* adj_cam; const int* adj_slot; const unsigned char* frozen; double w; int loss; double a;
};

static pvlm_ba::View to_view(const chk_view* c) {
  pvlm_ba::View v;
  v.n_points = c->n_points; v.n_cams = c->n_cams; v.n_upairs = c->n_upairs; v.n_obs = c->n_obs; v.pt_off = c->pt_off; v.cam = c->cam;
  v.obs_pt = c->obs_pt; v.s = c->s; v.X = c->X; v.Xc = c->Xc; v.scale = c->scale; v.Vinv = c->Vinv; v.gp = c->gp; v.adj_off = c->adj_off;
  v.adj_cam = c->adj_cam; v.adj_slot = c->adj_slot; v.frozen = c->frozen; v.w = c->w; v.loss = c->loss; v.a = c->a;
  return v;
}

// n observations, each with its own pose-table row (pose_tab: n x 21): r n x 2, J (n x 2) x 9
void chk2_eval(int kind, long long n, const double* pose_tab, const double* X, const double* o, double w, double rows, double cols, double* r, double* J) {
  for (long long i = 0; i < n; ++i) {
    double Jc[12], Jp[6];
    if (kind == 2) pvlm_reproj::eval_obs2<2>(pose_tab + 21 * i, X + 3 * i, o + 2 * i, w, rows, cols, r + 2 * i, Jc, Jp);
    else pvlm_reproj::eval_obs2<1>(pose_tab + 21 * i, X + 3 * i, o + 2 * i, w, rows, cols, r + 2 * i, Jc, Jp);
    for (int k = 0; k < 2; ++k) { std::memcpy(J + 9 * (2 * i + k), Jc + 6 * k, 48); std::memcpy(J + 9 * (2 * i + k) + 6, Jp + 3 * k, 24); }
  }
}

}  // extern "C"

template <int K>
static void reduce_k(const pvlm_ba::View& v, const pvlm_ba::Geo& geo, const double* pose_tab, int init_scale, double radius, double min_diag, double max_diag,
                     double* S, double* vecs, double* gmax) {
  const int F = v.n_cams;
  for (int p = 0; p < v.n_points; ++p) pvlm_ba::point_pass2<K>(v, geo, pose_tab, p, init_scale, radius, min_diag, max_diag, gmax);
  for (int p = 0; p < v.n_points; ++p)
    for (long long i = v.pt_off[p]; i < v.pt_off[p + 1]; ++i)
      for (long long j = v.pt_off[p]; j < v.pt_off[p + 1]; ++j) {
        const int ci = v.cam[i], cj = v.cam[j];
        if (cj < ci) continue;
        double acc[36] = {0}, vec[19] = {0};
        pvlm_ba::couple_pass2<K>(v, geo, pose_tab, i, j, acc, vec);
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) {
            S[(size_t)(6 * ci + a) * 6 * F + 6 * cj + b] += acc[a * 6 + b];
            if (cj != ci) S[(size_t)(6 * cj + b) * 6 * F + 6 * ci + a] += acc[a * 6 + b];
          }
        if (i == j) for (int k = 0; k < 19; ++k) vecs[19 * ci + k] += vec[k];
      }
}

extern "C" {

// dense reduced system S (6F x 6F, zeroed by the caller), per-camera [g 6 | Udiag 6 | gcam 6 | cost] (F x 19), gmax
void chk2_reduce(int kind, const chk_view* c, double rows, double cols, const double* pose_tab, int init_scale, double radius, double min_diag, double max_diag,
                 double* S, double* vecs, double* gmax) {
  const pvlm_ba::View v = to_view(c);
  const pvlm_ba::Geo geo{rows, cols};
  if (kind == 2) reduce_k<2>(v, geo, pose_tab, init_scale, radius, min_diag, max_diag, S, vecs, gmax);
  else reduce_k<1>(v, geo, pose_tab, init_scale, radius, min_diag, max_diag, S, vecs, gmax);
}

void chk2_step(int kind, const chk_view* c, double rows, double cols, const double* pose_tab, const double* dcam, double* out3) {
  const pvlm_ba::View v = to_view(c);
  const pvlm_ba::Geo geo{rows, cols};
  out3[0] = out3[1] = out3[2] = 0.0;
  for (int p = 0; p < v.n_points; ++p) {
    double o[3];
    if (kind == 2) pvlm_ba::step_point2<2>(v, geo, pose_tab, p, dcam, o); else pvlm_ba::step_point2<1>(v, geo, pose_tab, p, dcam, o);
    for (int k = 0; k < 3; ++k) out3[k] += o[k];
  }
}

double chk2_cost(int kind, const chk_view* c, double rows, double cols, const double* pose_tab, int candidate) {
  const pvlm_ba::View v = to_view(c);
  const pvlm_ba::Geo geo{rows, cols};
  double s = 0.0;
  for (long long i = 0; i < v.n_obs; ++i) s += kind == 2 ? pvlm_ba::cost_obs2<2>(v, geo, pose_tab, i, candidate) : pvlm_ba::cost_obs2<1>(v, geo, pose_tab, i, candidate);
  return s;
}

void chk_filter(int mode, int rows, int cols, int n_points, const long long* off, const int* frame_ids, const float* kp, const double* X, const double* T_cw,
                double thr, unsigned char* keep) {
  for (int t = 0; t < n_points; ++t) keep[t] = pvlm_sfm_filter::keep_track(mode, rows, cols, off[t], off[t + 1], frame_ids, kp, X + 3 * (size_t)t, T_cw, thr);
}

double chk_filter_threshold(int mode, double threshold) { return pvlm_sfm_filter::filter_threshold(mode, threshold); }

void chk_image_to_cam_point2i(int rows, int cols, long long n, const float* kp, float* cam) {
  for (long long i = 0; i < n; ++i) pvlm_sfm_filter::image_to_cam_point2i(rows, cols, kp[2 * i], kp[2 * i + 1], cam + 3 * i);
}

}  // extern "C"
