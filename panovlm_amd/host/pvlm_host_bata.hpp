// K44 on the host: the definition of csrc/pvlm_bata_core.h (BATA translation averaging) behind a host backend that does what the kernels of csrc/pvlm_bata.hip do —
// the per-pair records, the per-camera gather over kGroup lanes and their butterfly, the fixed reduction tree — on the host's pair-graph layer
// (pvlm_host_pairgraph.hpp), with its dense host Cholesky of the camera system in place of the library's solver.  No device, no dependency on the rest of the host
// mirror: the equality partner of pvlm_transavg_bata (tests/cpp/bata_core_check.cpp) and the `host` route of TranslationAveragingBATA (pvlm_host_sfm.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/pvlm_bata_core.h"
#include "pvlm_host_pairgraph.hpp"

namespace pvlm {
namespace bata_detail {

namespace bt = pvlm_bata;
namespace pg = pvlm_pairgraph;

// the backend of bt::run on the host's layer; the pivot test is the library's (d > 0 alone), which this twin exists to equal
struct HostBackend {
  int F, P; bt::Params prm;
  const int *first, *second;
  std::vector<double> dir, s0, s, wvec, t, rec, blocks, cam, terms;      // dir: component-major, as the device keeps it
  std::vector<int> off, ent;
  pg::CameraSystem sys;

  HostBackend(const bt::Params& p, int F_, int P_, const int* fi, const int* se, const double* dir_, const double* scales0) : F(F_), P(P_), prm(p), first(fi), second(se) {
    pg::build_csr(F, P, first, second, &off, &ent);
    sys.init(F, P, first, second, 0);
    dir.assign(3 * (size_t)P, 0.0);
    for (int q = 0; q < P; ++q) for (int k = 0; k < 3; ++k) dir[(size_t)k * P + q] = dir_[3 * (size_t)q + k];
    s0.assign(scales0, scales0 + (size_t)P); s.assign((size_t)P, 0.0); wvec.assign((size_t)P, 0.0); t.assign(3 * (size_t)F, 0.0);
    rec.assign((size_t)bt::kSlots * P, 0.0); blocks.assign(36 * ((size_t)F + P), 0.0); cam.assign((size_t)bt::kCam * F, 0.0); terms.assign(2 * (size_t)P, 0.0);
  }
  bool failed() const { return false; }
  void tij(int q, double* v) const { for (int k = 0; k < 3; ++k) v[k] = dir[(size_t)k * P + q]; }
  double* off_block(int q) { return &blocks[36 * ((size_t)F + q)]; }
  double scale_sum() { return pg::tree_reduce_host<false>(s0.data(), P); }
  // per camera: kGroup lanes over the one-sided record, their butterfly; the diagonal block diag_factor * (sum of weights) I3
  void gather(double diag_factor) {
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][bt::kCam];
      for (int l = 0; l < pg::kGroup; ++l) pg::gather_lane<bt::kCam>(rec.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, 0, 0xeu, part[l]);
      pairgraph_detail::butterfly<pg::kGroup, bt::kCam>(part);
      for (int k = 0; k < bt::kCam; ++k) cam[(size_t)bt::kCam * c + k] = part[0][k];
      for (int k = 0; k < 3; ++k) blocks[36 * (size_t)c + 7 * k] = diag_factor * part[0][bt::kW];
    }
  }
  void gather_c(std::vector<double>* cv) {
    cv->assign(3 * (size_t)F, 0.0);
    for (int c = 0; c < F; ++c) {
      double part[pg::kGroup][3];
      for (int l = 0; l < pg::kGroup; ++l) pg::gather_lane<3>(dir.data(), P, ent.data(), off[(size_t)c], off[(size_t)c + 1], l, 0, 0x7u, part[l]);
      pairgraph_detail::butterfly<pg::kGroup, 3>(part);
      for (int k = 0; k < 3; ++k) (*cv)[3 * (size_t)c + k] = -part[0][k];
    }
  }
  void lud_pairs(bool first_time, double factor) {
    for (int q = 0; q < P; ++q) {
      double v[3], w = 1.0;
      tij(q, v);
      if (first_time) s[(size_t)q] = s0[(size_t)q] * factor;
      else bt::lud_update(v, &t[3 * (size_t)first[q]], &t[3 * (size_t)second[q]], prm.delta, &s[(size_t)q], &w);
      bt::lud_record(v, s[(size_t)q], w, &rec[(size_t)q], P, off_block(q));
    }
    gather(2.0);
  }
  void lud_scales() {
    for (int q = 0; q < P; ++q) { double v[3], w; tij(q, v); bt::lud_update(v, &t[3 * (size_t)first[q]], &t[3 * (size_t)second[q]], prm.delta, &s[(size_t)q], &w); }
  }
  int solve() { return pairgraph_detail::solve_camera_system(&sys, blocks, false); }
  void dots(const std::vector<double>& x1, const std::vector<double>& x2, double* a) {
    for (int q = 0; q < P; ++q) {
      double v[3];
      tij(q, v);
      const size_t i = 3 * (size_t)first[q], j = 3 * (size_t)second[q];
      bt::dots_pair(v, &x1[i], &x1[j], &x2[i], &x2[j], &terms[(size_t)q], P);
    }
    a[0] = pg::tree_reduce_host<false>(terms.data(), P); a[1] = pg::tree_reduce_host<false>(&terms[(size_t)P], P);
  }
  void set_t(const std::vector<double>& x) { t = x; }
  void outer(double thr) {
    for (int q = 0; q < P; ++q) { double v[3]; tij(q, v); wvec[(size_t)q] = bt::outer_weight(v, &t[3 * (size_t)first[q]], &t[3 * (size_t)second[q]], s[(size_t)q], thr); }
  }
  double inner_pairs() {
    for (int q = 0; q < P; ++q) {
      double v[3];
      tij(q, v);
      terms[(size_t)q] = bt::inner_record(v, &t[3 * (size_t)first[q]], &t[3 * (size_t)second[q]], wvec[(size_t)q], &s[(size_t)q], &rec[(size_t)q], P, off_block(q));
    }
    gather(1.0);
    return pg::tree_reduce_host<true>(terms.data(), P);
  }
};

// pvlm_transavg_bata on the host.  Returns 0, or -1 (PVLM_ERR_ARG) with nothing written.  info: 0, k > 0 (not positive definite), -1 (not finite), -2 (no pairs); the
// outputs are written only when info is 0: centres and lud_centres (3 per camera of F = max_id - min_id + 1, the ids shifted by min_id), scales_out (P).
inline int SolveHost(int n_cameras, int P, const int* first, const int* second, const double* dir, const double* scales0, const bt::Params* prm, double* centres,
                     double* lud_centres, double* scales_out, int* info) {
  int min_id = 0, F = 0;
  if (!info || !centres || bt::check_args(n_cameras, P, first, second, dir, scales0, prm, &min_id, &F)) return -1;
  if (P == 0) { *info = bt::kInfoNoPairs; return 0; }
  std::vector<int> fi((size_t)P), se((size_t)P);
  for (int p = 0; p < P; ++p) { fi[(size_t)p] = first[p] - min_id; se[(size_t)p] = second[p] - min_id; }
  HostBackend be(*prm, F, P, fi.data(), se.data(), dir, scales0);
  std::vector<double> lud, out;
  *info = bt::run(be, *prm, &lud, &out);
  if (*info == 0) {
    std::memcpy(centres, out.data(), out.size() * sizeof(double));
    if (lud_centres) std::memcpy(lud_centres, lud.data(), lud.size() * sizeof(double));
    if (scales_out) std::memcpy(scales_out, be.s.data(), (size_t)P * sizeof(double));
  }
  return 0;
}

}  // namespace bata_detail
}  // namespace pvlm
