// Per-track statement of K32: TriangulateNView (sfm/Triangulate.cpp:8-28, :117-139, :198-226) as TriangulateTracks calls it
// (sfm/Structure.cpp:8-69), its inf skip rule (:56-57), and FilterTracksToFar (:87-119) with FurthestPoints (base/Geometry.hpp:594-617).
// One call decides one track.  Host / device: csrc/pvlm_triangulate.hip wraps it in two kernels, the host mirror compiles it for
// Triangulate2View / TriangulateNView on host vectors, and a host compile (tests/cpp/structure_core_check.cpp) is what the CPU tests
// compare with numpy and the GPU tests compare with bit for bit.  Compile with -ffp-contract=off.  Only + - * / sqrt from here on: the
// bearing of a keypoint (sin / cos) is pvlm_sfm_filter::image_to_cam_point2i, taken before the core is entered.
//
// What is recalled from Eigen and not pinned against a build of it:
//   - fixed-size products and dot products sum their three terms in index order, (a0 b0 + a1 b1) + a2 b2;
//   - Matrix2d::inverse() is the adjugate times 1 / det, det = a00 a11 - a10 a01;
//   - normalized() divides by sqrt(squaredNorm) when the squared norm is > 0 and returns the vector unchanged otherwise.
// Parity by tolerance, not in bits: upstream's SelfAdjointEigenSolver<Matrix4d> is a tridiagonal QL; here the eigenvector of the smallest
// eigenvalue comes from a cyclic Jacobi in fp64 with the fixed rotation order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) and at most 12 sweeps
// (a sweep with every off-diagonal entry exactly zero rotates nothing, so stopping there changes no bit).  The two agree to rounding
// (Davis-Kahan: 64 eps lambda_max / (lambda_1 - lambda_0) on the unit eigenvector, see tests/test_structure_cpu.py); host and device
// builds of THIS code agree bit for bit.  info() is always Success for Jacobi.  Among equal smallest eigenvalues the first index wins.
#pragma once
#include <cmath>

#include "pvlm_sfm_filter_core.h"

// the 4 x 4 arrays of the Jacobi must stay in registers: every loop over them is unrolled, so that every index is static
#if defined(__HIPCC__)
#define PVLM_TRI_UNROLL _Pragma("unroll")
#else
#define PVLM_TRI_UNROLL
#endif

namespace pvlm_triangulate {

enum { STATUS_OK = 0, STATUS_INF = 1, STATUS_INVALID_FRAME = 2 };

PVLM_EQ_UD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Triangulate2View(R_21, t_21, p1, p2) (:8-28): the midpoint of the two rays in camera 1's frame.  R_21 row-major.
PVLM_EQ_UD void triangulate_2view(const double* R_21, const double* t_21, const float* p1, const float* p2, double* P) {
  const double point1[3] = {(double)p1[0], (double)p1[1], (double)p1[2]}, point2[3] = {(double)p2[0], (double)p2[1], (double)p2[2]};
  double trans_12[3], b2[3];
  for (int r = 0; r < 3; ++r) {                      // -R_21^T t_21 and R_21^T p2: column r of R_21
    trans_12[r] = ((-R_21[r]) * t_21[0] + (-R_21[3 + r]) * t_21[1]) + (-R_21[6 + r]) * t_21[2];
    b2[r] = (R_21[r] * point2[0] + R_21[3 + r] * point2[1]) + R_21[6 + r] * point2[2];
  }
  const double a00 = dot3(point1, point1), a10 = dot3(b2, point1), a01 = -dot3(point1, b2), a11 = -dot3(b2, b2);
  const double rhs0 = dot3(point1, trans_12), rhs1 = dot3(b2, trans_12);
  const double invdet = 1.0 / (a00 * a11 - a10 * a01);          // parallel rays: det = 0, IEEE runs its course
  const double i00 = a11 * invdet, i01 = -a01 * invdet, i10 = -a10 * invdet, i11 = a00 * invdet;
  const double l0 = i00 * rhs0 + i01 * rhs1, l1 = i10 * rhs0 + i11 * rhs1;
  for (int r = 0; r < 3; ++r) P[r] = (l0 * point1[r] + (l1 * b2[r] + trans_12[r])) / 2.0;
}

// TriangulateNView's two-view branch (:204-211) on two [R | t] rows (row-major 3 x 4) and two bearings
PVLM_EQ_UD void triangulate_pair(const double* T1, const double* T2, const float* p1, const float* p2, double* X) {
  double R_21[9], t_21[3], P[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R_21[3 * i + j] = (T2[4 * i] * T1[4 * j] + T2[4 * i + 1] * T1[4 * j + 1]) + T2[4 * i + 2] * T1[4 * j + 2];   // R_2w R_1w^T
  for (int i = 0; i < 3; ++i) t_21[i] = T2[4 * i + 3] - ((R_21[3 * i] * T1[3] + R_21[3 * i + 1] * T1[7]) + R_21[3 * i + 2] * T1[11]);
  triangulate_2view(R_21, t_21, p1, p2, P);
  for (int r = 0; r < 3; ++r) {                      // R_1w^T P + (-R_1w^T t_1w)
    const double t_w1 = ((-T1[r]) * T1[3] + (-T1[4 + r]) * T1[7]) + (-T1[8 + r]) * T1[11];
    X[r] = ((T1[r] * P[0] + T1[4 + r] * P[1]) + T1[8 + r] * P[2]) + t_w1;
  }
}

// the 10 distinct entries of the symmetric AtA, row by row: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
// AtA += cost^T cost, cost = P - (n n^T) P, n = bearing.normalized(), P = [R | t]   (:126-130)
PVLM_EQ_UD void ata_add(const double* T, const float* bearing, double* ata) {
  double n[3] = {(double)bearing[0], (double)bearing[1], (double)bearing[2]};
  const double z = dot3(n, n);
  if (z > 0.0) { const double s = sqrt(z); n[0] = n[0] / s; n[1] = n[1] / s; n[2] = n[2] / s; }
  double cost[12];
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 4; ++c) cost[4 * i + c] = T[4 * i + c] - (((n[i] * n[0]) * T[c] + (n[i] * n[1]) * T[4 + c]) + (n[i] * n[2]) * T[8 + c]);
  int k = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++k) ata[k] = ata[k] + ((cost[a] * cost[b] + cost[4 + a] * cost[4 + b]) + cost[8 + a] * cost[8 + b]);
}

template <int P, int Q>
PVLM_EQ_UD void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] = a[P][P] - t * apq; a[Q][Q] = a[Q][Q] + t * apq; a[P][Q] = 0.0; a[Q][P] = 0.0;
PVLM_TRI_UNROLL
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = a[r][P], arq = a[r][Q];
      a[r][P] = c * arp - s * arq; a[P][r] = a[r][P];
      a[r][Q] = s * arp + c * arq; a[Q][r] = a[r][Q];
    }
    const double vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = c * vrp - s * vrq; v[r][Q] = s * vrp + c * vrq;
  }
}

// eigenvector (unit up to rounding, sign as the rotations leave it) of the smallest eigenvalue of the symmetric 4 x 4 with the 10
// entries `ata`; w (optional): the four eigenvalues in the order of the diagonal
PVLM_EQ_UD void eig4_smallest(const double* ata, double* vec, double* w = nullptr) {
  double a[4][4], v[4][4];
  {
    int k = 0;
PVLM_TRI_UNROLL
    for (int r = 0; r < 4; ++r)
PVLM_TRI_UNROLL
      for (int c = r; c < 4; ++c, ++k) { a[r][c] = ata[k]; a[c][r] = ata[k]; }
PVLM_TRI_UNROLL
    for (int r = 0; r < 4; ++r)
PVLM_TRI_UNROLL
      for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 12; ++sweep) {
    const bool done = a[0][1] == 0.0 && a[0][2] == 0.0 && a[0][3] == 0.0 && a[1][2] == 0.0 && a[1][3] == 0.0 && a[2][3] == 0.0;
    if (done) break;
    jacobi_rotate<0, 1>(a, v); jacobi_rotate<0, 2>(a, v); jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v); jacobi_rotate<1, 3>(a, v); jacobi_rotate<2, 3>(a, v);
  }
  double best = a[0][0];
  vec[0] = v[0][0]; vec[1] = v[1][0]; vec[2] = v[2][0]; vec[3] = v[3][0];
  if (a[1][1] < best) { best = a[1][1]; vec[0] = v[0][1]; vec[1] = v[1][1]; vec[2] = v[2][1]; vec[3] = v[3][1]; }
  if (a[2][2] < best) { best = a[2][2]; vec[0] = v[0][2]; vec[1] = v[1][2]; vec[2] = v[2][2]; vec[3] = v[3][2]; }
  if (a[3][3] < best) { best = a[3][3]; vec[0] = v[0][3]; vec[1] = v[1][3]; vec[2] = v[2][3]; vec[3] = v[3][3]; }
  if (w) { w[0] = a[0][0]; w[1] = a[1][1]; w[2] = a[2][2]; w[3] = a[3][3]; }
}

// One track of TriangulateTracks: observations [o0, o1) in their order, frame_ids[i] into T_cw (row-major 3 x 4 per frame) and frame_valid
// (NULL = every frame valid).  The bearing of observation i is bearings + 3 i when bearings is given, else eq.ImageToCam(kp.pt) of
// keypoints + 2 i.  Writes X[3], returns the status: an observation in an invalid frame -> NaN point, STATUS_INVALID_FRAME (the one
// deliberate divergence, see include/pvlm.h); any coordinate +-inf -> STATUS_INF (:56-57); otherwise STATUS_OK, a NaN point included.
PVLM_EQ_UD int triangulate_track(int rows, int cols, long long o0, long long o1, const int* frame_ids, const float* keypoints, const float* bearings,
                                 const double* T_cw, const unsigned char* frame_valid, double* X) {
  if (frame_valid)
    for (long long i = o0; i < o1; ++i)
      if (!frame_valid[frame_ids[i]]) { X[0] = X[1] = X[2] = (double)NAN; return STATUS_INVALID_FRAME; }
  const long long len = o1 - o0;
  auto bearing = [&](long long i, float* b) {
    if (bearings) { b[0] = bearings[3 * i]; b[1] = bearings[3 * i + 1]; b[2] = bearings[3 * i + 2]; }
    else pvlm_sfm_filter::image_to_cam_point2i(rows, cols, keypoints[2 * i], keypoints[2 * i + 1], b);
  };
  if (len == 2) {
    float p1[3], p2[3];
    bearing(o0, p1); bearing(o0 + 1, p2);
    triangulate_pair(T_cw + 12 * (long long)frame_ids[o0], T_cw + 12 * (long long)frame_ids[o0 + 1], p1, p2, X);
  } else if (len > 2) {
    double ata[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = o0; i < o1; ++i) {
      float b[3];
      bearing(i, b);
      ata_add(T_cw + 12 * (long long)frame_ids[i], b, ata);
    }
    double p[4];
    eig4_smallest(ata, p);
    X[0] = p[0] / p[3]; X[1] = p[1] / p[3]; X[2] = p[2] / p[3];          // hnormalized()
  } else {
    X[0] = X[1] = X[2] = (double)INFINITY;                                // "Invalid number in triangulate"
  }
  const bool inf = (X[0] == (double)INFINITY || X[0] == -(double)INFINITY) || (X[1] == (double)INFINITY || X[1] == -(double)INFINITY) ||
                   (X[2] == (double)INFINITY || X[2] == -(double)INFINITY);
  return inf ? STATUS_INF : STATUS_OK;
}

// One track of FilterTracksToFar: the distinct frame ids of [o0, o1) ascending (std::set<size_t>), those with a valid pose give the centres
// t_wc (n_frames x 3).  baseline = FurthestPoints: the largest centre distance, strict > from -1 over the pairs, 0 with fewer than two
// centres; a maximum does not depend on the order of the pairs, a NaN distance never wins, and sqrt is monotonic, so the squared
// distances are compared and one root is taken.  average = the mean of |centre - X| in ascending id order (0 / 0 = NaN without centres).
// Returns 1 = keep: the track goes when threshold * baseline < average (false for NaN).
PVLM_EQ_UD unsigned char keep_track_far(long long o0, long long o1, const int* frame_ids, const double* X, const double* t_wc,
                                        const unsigned char* frame_valid, double threshold) {
  double sum = 0.0;
  int count = 0;
  for (long long prev = -1;;) {                       // next distinct id above prev
    long long next = -1;
    for (long long i = o0; i < o1; ++i) { const long long f = frame_ids[i]; if (f > prev && (next < 0 || f < next)) next = f; }
    if (next < 0) break;
    prev = next;
    if (frame_valid && !frame_valid[next]) continue;
    const double* c = t_wc + 3 * next;
    const double dx = c[0] - X[0], dy = c[1] - X[1], dz = c[2] - X[2];
    sum = sum + sqrt((dx * dx + dy * dy) + dz * dz);
    ++count;
  }
  double baseline = 0.0;
  if (count > 1) {
    double best = -1.0;
    for (long long i = o0; i < o1; ++i) {
      const int fi = frame_ids[i];
      if (frame_valid && !frame_valid[fi]) continue;
      for (long long j = i + 1; j < o1; ++j) {
        const int fj = frame_ids[j];
        if (fj == fi || (frame_valid && !frame_valid[fj])) continue;
        const double dx = t_wc[3 * (long long)fi] - t_wc[3 * (long long)fj], dy = t_wc[3 * (long long)fi + 1] - t_wc[3 * (long long)fj + 1],
                     dz = t_wc[3 * (long long)fi + 2] - t_wc[3 * (long long)fj + 2];
        const double sq = (dx * dx + dy * dy) + dz * dz;
        if (sq > best) best = sq;
      }
    }
    baseline = best < 0.0 ? -1.0 : sqrt(best);
  }
  const double average = sum / (double)count;
  return threshold * baseline < average ? 0 : 1;
}

}  // namespace pvlm_triangulate
