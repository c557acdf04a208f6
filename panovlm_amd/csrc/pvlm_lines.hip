// K4 — vote matrix of AssociateLine2Line (lidar_mapping/LidarFeatureAssociate.cpp:457-473), its row maxima, and K4b, the residual rows of the line-to-line term;
// K7 — equirectangular projection (sensors/Equirectangular.h) and the LiDAR-seeded depth image; K8 — the point x image-line voting loop of
// CameraLidarLineAssociate::AssociateByAngle (joint_optimization/CameraLidarLineAssociate.cpp:394-426) and the sparse read-back of its votes.  Kernels first, in
// that order; then the host side: K7's calls, the vote sequence K4 and K8 share (queue_votes and its tails), K4's calls, K4b's, K8's.  Compiled with
// -ffp-contract=off: every threshold test must take the same branch as a non-FMA x86-64 build of the reference.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pvlm_depth_launch.h"
#include "pvlm_internal.h"
#include "pvlm_workers.h"
#include "pvlm_exact_math.h"
#include "pvlm_equirect_core.h"

// ---- K4 -----------------------------------------------------------------------------------------
// PointToLineDistance3D (base/Geometry.hpp:198-211), fp64, line = (point, direction).
__device__ __forceinline__ double point_to_line(double px, double py, double pz, const double* l) {
  const double x0 = l[0], y0 = l[1], z0 = l[2], nx = l[3], ny = l[4], nz = l[5];
  const double k = (nx * (px - x0) + ny * (py - y0) + nz * (pz - z0)) / (nx * nx + ny * ny + nz * nz);
  const double qx = k * nx + x0, qy = k * ny + y0, qz = k * nz + z0;
  return sqrt((qx - px) * (qx - px) + (qy - py) * (qy - py) + (qz - pz) * (qz - pz));
}

// One launch for every (ref, nei) pair of an outer iteration (the reference calls AssociateLine2Line twice per pair per outer iteration,
// LidarLineMatch.cpp:68 and Optimization.cpp:379); pvlm_line2line_votes is a batch of one.
// Work item = (pair, nei corner point, ref segment); the pair is found by bisection on the prefix of work sizes.
struct pvlm_line_pair_desc {
  const float* xyz; const int* p2s_off; const int* p2s_ids;
  int n_pts, n_ref;
  long long line_off;   // first world line of the pair's ref scan in `lines` (units of 6 doubles)
  long long vote_off;   // first vote of the pair (n_nei_seg x n_ref_seg block)
  long long work_off;   // prefix sum of n_pts * n_ref
};

__device__ __forceinline__ int find_pair(const long long* __restrict__ work_off, int n_pairs, long long g) {
  int lo = 0, hi = n_pairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (work_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_line_votes_batch(int n_pairs, const pvlm_line_pair_desc* __restrict__ desc,
                                                          const long long* __restrict__ work_off, long long total,
                                                          const double* __restrict__ lines, double thr, int* __restrict__ votes) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const int p = find_pair(work_off, n_pairs, g);
  const pvlm_line_pair_desc d = desc[p];
  const long long l = g - d.work_off;
  const int i = (int)(l / d.n_ref), s = (int)(l - (long long)i * d.n_ref);
  const double dist = point_to_line((double)d.xyz[3 * i], (double)d.xyz[3 * i + 1], (double)d.xyz[3 * i + 2], lines + 6 * (d.line_off + s));
  if (dist > thr) return;
  for (int k = d.p2s_off[i]; k < d.p2s_off[i + 1]; ++k) atomicAdd(&votes[d.vote_off + (long long)d.p2s_ids[k] * d.n_ref + s], 1);
}

// The same votes with a thread per (pair, neighbour corner point) that walks the pair's reference segments (round 6; pvlm_line2line_best_batch).  The thread-per-test
// form above pays per TEST for what belongs to the point or to the pair: a 15-step bisection through the pair offsets (dependent loads), a 64-bit division for
// (point, segment), the 64-byte descriptor, the point's coordinates and segment list — and a square root the decision does not need: sqrt is monotone and correctly
// rounded, so dist > thr  <=>  q > T with T = the largest double whose root is still <= thr, found once on the host (q: the squared distance, as upstream sums it).
// The division inside PointToLineDistance3D stays (its quotient enters q).  334 M tests of a Floor-sized call: 4.5 -> 1.x ms.  Same vote blocks, bit for bit.
__global__ __launch_bounds__(256) void k_line_votes_points(int n_pairs, const pvlm_line_pair_desc* __restrict__ desc, const long long* __restrict__ pt_off, long long total,
                                                           const double* __restrict__ lines, double T, int* __restrict__ votes) {
  __shared__ int s_p0;
  const long long g0 = (long long)blockIdx.x * 256;
  if (threadIdx.x == 0) s_p0 = find_pair(pt_off, n_pairs, g0 < total ? g0 : total - 1);
  __syncthreads();
  const long long g = g0 + threadIdx.x;
  if (g >= total) return;
  int p = s_p0;
  while (p + 1 < n_pairs && pt_off[p + 1] <= g) ++p;
  const pvlm_line_pair_desc* d = desc + p;
  const int i = (int)(g - pt_off[p]);
  const int* p2s_off = d->p2s_off;
  const int k0 = p2s_off[i], k1 = p2s_off[i + 1];
  if (k0 == k1) return;                                            // a point of no segment votes for nothing
  const float* xyz = d->xyz;
  const double px = (double)xyz[3 * i], py = (double)xyz[3 * i + 1], pz = (double)xyz[3 * i + 2];
  const int n_ref = d->n_ref;
  const double* l = lines + 6 * d->line_off;
  int* v = votes + d->vote_off;
  const int* p2s_ids = d->p2s_ids;
  for (int s = 0; s < n_ref; ++s, l += 6) {
    const double x0 = l[0], y0 = l[1], z0 = l[2], nx = l[3], ny = l[4], nz = l[5];
    const double k = (nx * (px - x0) + ny * (py - y0) + nz * (pz - z0)) / (nx * nx + ny * ny + nz * nz);
    const double qx = k * nx + x0, qy = k * ny + y0, qz = k * nz + z0;
    const double q = (qx - px) * (qx - px) + (qy - py) * (qy - py) + (qz - pz) * (qz - pz);
    if (q > T) continue;
    for (int kk = k0; kk < k1; ++kk) atomicAdd(&v[(long long)p2s_ids[kk] * n_ref + s], 1);
  }
}
// the largest double whose (correctly rounded) square root does not exceed thr
static double sqrt_threshold(double thr) {
  if (!(thr >= 0.0)) return -1.0;                                  // dist > thr for every dist >= 0 (and q > -1 for every q >= 0); NaN thr: dist > NaN is false, handled by the caller
  double x = thr * thr;
  while (std::sqrt(x) > thr) x = std::nextafter(x, 0.0);
  while (std::sqrt(std::nextafter(x, INFINITY)) <= thr && std::isfinite(x)) x = std::nextafter(x, INFINITY);
  return x;
}

// First statement of FindAssociations (lidar_mapping/LidarFeatureAssociate.cpp:126-133) on the device: per neighbour segment (a row of the pair's
// vote block) the reference segment with the most votes — the first of equals, as `if (v > max)` keeps it — and that count.  One thread per row;
// what goes back to the host is 8 bytes per neighbour segment instead of the block (70 MB of blocks for the 11 k pairs of a Floor sequence).
struct pvlm_row_desc { long long vote_off; int n_ref; };
__global__ __launch_bounds__(256) void k_line_row_best(int n_pairs, const pvlm_row_desc* __restrict__ desc, const long long* __restrict__ row_off, long long rows,
                                                       const int* __restrict__ votes, int* __restrict__ best_col, int* __restrict__ best_count) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= rows) return;
  const int p = find_pair(row_off, n_pairs, g);
  const pvlm_row_desc d = desc[p];
  const int* v = votes + d.vote_off + (g - row_off[p]) * d.n_ref;
  int col = 0, cnt = d.n_ref > 0 ? v[0] : 0;
  for (int c = 1; c < d.n_ref; ++c) { const int x = v[c]; if (x > cnt) { cnt = x; col = c; } }
  best_col[g] = col; best_count[g] = cnt;
}

// ---- K4b: residual rows of the line-to-line term ---------------------------------------------------------------
// One workgroup per match (a neighbour segment associated with a reference segment): thread i turns point i of the
// neighbour segment into the SoA row [World2Local_nei(p) | A | unit(A - B)] of the Point2Line functors
// (A, B = ref_local_point +- 0.1 dir, util/Optimization.cpp:410-434; the functor's constructor normalises A - B,
// base/CostFunction.h:778-783 — done once per match on the host, in the arithmetic pvlm_resset_upload uses).
struct pvlm_match_desc {
  const float* pts;      // the neighbour segment's points (world frame)
  int n_pts, pair;       // pair: index into the pair table (poses of the neighbour scan)
  long long dst;         // first row of the match inside the column block
  double line[6];        // A (3) | unit direction (3)
};
struct pvlm_match_pose { double R[9], t[3]; };   // R_wl, t_wl of the neighbour scan of a pair

__global__ __launch_bounds__(64) void k_line_rows(const pvlm_match_desc* __restrict__ matches, const pvlm_match_pose* __restrict__ poses,
                                                  double* __restrict__ cols, long long stride) {
  const pvlm_match_desc m = matches[blockIdx.x];
  const pvlm_match_pose& P = poses[m.pair];
  for (int i = threadIdx.x; i < m.n_pts; i += 64) {
    const double x = (double)m.pts[3 * i], y = (double)m.pts[3 * i + 1], z = (double)m.pts[3 * i + 2];
    const long long d = m.dst + i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {     // World2Local: R_wl^T p - R_wl^T t   (sensors/Velodyne.cpp:1850-1853)
      const double a = (P.R[k] * x + P.R[3 + k] * y) + P.R[6 + k] * z;
      const double b = (P.R[k] * P.t[0] + P.R[3 + k] * P.t[1]) + P.R[6 + k] * P.t[2];
      cols[(size_t)k * stride + d] = a - b;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) cols[(size_t)(3 + k) * stride + d] = m.line[k];
  }
}

// ---- K7 -----------------------------------------------------------------------------------------
// FastAtan2 (base/Math.h:15-29).  For T = float the polynomial is evaluated in double (double
// literals) and rounded to float on assignment, as are M_PI_2 - r and M_PI - r.
using pvlm_equirect::fast_atan2;   // csrc/pvlm_equirect_core.h (shared with K30)

template <typename T>
__global__ void k_cam_to_image(int rows, int cols, long long n, const T* __restrict__ cam, T* __restrict__ px) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T x = cam[3 * i], y = cam[3 * i + 1], z = cam[3 * i + 2];
  // CamToSphere: (FastAtan2(x, z), -FastAtan2(y, (T)sqrt(x*x + z*z)))   Equirectangular.h:50-51
  // SphereToImage: cols * (0.5 + lon / (2 pi)), rows * (0.5 - lat / pi)   :84-85
  if constexpr (sizeof(T) == 4) {     // float: same floats from cheaper sequences (pvlm_exact_math.h)
    const float lon = fast_atan2<float>(x, z);
    const float lat = -fast_atan2<float>(y, pvlm_exact::sqrt_via_double(x * x + z * z));
    px[2 * i] = (float)(cols * (0.5 + pvlm_exact::div_two_pi(lon)));
    px[2 * i + 1] = (float)(rows * (0.5 - pvlm_exact::div_pi(lat)));
  } else {
    pvlm_equirect::cam_to_image_f64(rows, cols, x, y, z, &px[2 * i], &px[2 * i + 1]);
  }
}

// sin and cos of a FLOAT argument, each the double-precision value rounded to float — what round 1 obtained from two calls
// of the device library's double sin / cos (the reference calls std::sin / std::cos on floats).  The library routines carry
// a full-range argument reduction and cost ~150 instructions each, which made ImageToCam<float> VALU-bound at 0.25 of the
// HBM roof.  A float argument bounded by a few turns needs neither: one Cody-Waite step against pi/2 (the 33-bit head
// leaves q * head exact for |q| < 2^20) and the fdlibm kernel polynomials (|error| < 2^-58 on [-pi/4, pi/4]) give a double
// within 2 ulp of the exact value, i.e. the same float after rounding except when the exact value lies within ~2e-16
// (relative) of a float rounding boundary.  tests/test_equirect_gpu.py compares the two paths on every pixel of a
// 5760 x 2880 panorama and on sub-pixel positions; PVLM_EXACT_TRIG=1 selects the library path.
__device__ __attribute__((noinline)) float2 sincos_f32_arg_large(float xf) {   // |x| >= 1e5: never a pixel
  const double x = (double)xf;
  return make_float2((float)sin(x), (float)cos(x));
}
__device__ __forceinline__ void sincos_f32_arg(float xf, float* s_out, float* c_out) {
  const double x = (double)xf;
  if (!(fabs(x) < 1.0e5)) { const float2 sc = sincos_f32_arg_large(xf); *s_out = sc.x; *c_out = sc.y; return; }   // out of line: the library path is 450 instructions
  const double q = rint(x * 0.63661977236758134308);
  double y = fma(-q, 1.57079632673412561417e+00, x);
  y = fma(-q, 6.07710050650619224932e-11, y);
  const double z = y * y;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma(z, ps, 2.75573137070700676789e-06);
  ps = fma(z, ps, -1.98412698298579493134e-04);
  ps = fma(z, ps, 8.33333333332248946124e-03);
  ps = fma(z, ps, -1.66666666666666324348e-01);
  const float sn = (float)fma(y * z, ps, y);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma(z, pc, -2.75573143513906633035e-07);
  pc = fma(z, pc, 2.48015872894767294178e-05);
  pc = fma(z, pc, -1.38888888888741095749e-03);
  pc = fma(z, pc, 4.16666666666666019037e-02);
  const float cs = (float)fma(z * z, pc, fma(z, -0.5, 1.0));
  // quadrant: selection and sign commute with the rounding to float (round-to-nearest is odd), so they are done on floats
  const int n = (int)q & 3;
  const float sv = (n & 1) ? cs : sn, cv = (n & 1) ? sn : cs;
  *s_out = (n & 2) ? -sv : sv;
  *c_out = ((n + 1) & 2) ? -cv : cv;
}

// N arguments in lock step: every polynomial coefficient is used N times in a row, so the compiler materialises each
// 64-bit constant once per N evaluations (one evaluation at a time it re-created them: 183 v_mov per 4 pixels).  Same
// arithmetic, per argument, as sincos_f32_arg.
template <int N>
__device__ __forceinline__ void sincos_f32_args(const float (&xf)[N], float (&s_out)[N], float (&c_out)[N]) {
  double y[N], z[N], ps[N], pc[N];
  int n[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double x = (double)xf[i];
    const double q = rint(x * 0.63661977236758134308);
    y[i] = fma(-q, 1.57079632673412561417e+00, x);
    y[i] = fma(-q, 6.07710050650619224932e-11, y[i]);
    z[i] = y[i] * y[i];
    n[i] = (int)q & 3;
  }
#define PVLM_STEP(arr, C)                      \
  _Pragma("unroll") for (int i = 0; i < N; ++i) arr[i] = fma(z[i], arr[i], C)
#pragma unroll
  for (int i = 0; i < N; ++i) ps[i] = fma(z[i], 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  PVLM_STEP(ps, 2.75573137070700676789e-06);
  PVLM_STEP(ps, -1.98412698298579493134e-04);
  PVLM_STEP(ps, 8.33333333332248946124e-03);
  PVLM_STEP(ps, -1.66666666666666324348e-01);
#pragma unroll
  for (int i = 0; i < N; ++i) pc[i] = fma(z[i], -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  PVLM_STEP(pc, -2.75573143513906633035e-07);
  PVLM_STEP(pc, 2.48015872894767294178e-05);
  PVLM_STEP(pc, -1.38888888888741095749e-03);
  PVLM_STEP(pc, 4.16666666666666019037e-02);
#undef PVLM_STEP
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float sn = (float)fma(y[i] * z[i], ps[i], y[i]);
    const float cs = (float)fma(z[i] * z[i], pc[i], fma(z[i], -0.5, 1.0));
    const float sv = (n[i] & 1) ? cs : sn, cv = (n[i] & 1) ? sn : cs;
    s_out[i] = (n[i] & 2) ? -sv : sv;
    c_out[i] = ((n[i] + 1) & 2) ? -cv : cv;
    if (!(fabsf(xf[i]) < 1.0e5f)) { const float2 sc = sincos_f32_arg_large(xf[i]); s_out[i] = sc.x; c_out[i] = sc.y; }   // never a pixel
  }
}

// streaming accesses of the whole-panorama maps.  PVLM_NT_MAPS = 1 makes them non-temporal: measured and rejected — CamToImage drops
// from 0.66 to 0.555 of the HBM peak, ImageToCam does not move (profiles/r2_ab_eval_loads.txt).
#ifndef PVLM_NT_MAPS
#define PVLM_NT_MAPS 0
#endif
typedef float pvlm_flt4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 map_load4(const float4* p) {
#if PVLM_NT_MAPS
  const pvlm_flt4 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) pvlm_flt4*)(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}
__device__ __forceinline__ void map_store4(float4* p, float4 v) {
#if PVLM_NT_MAPS
  pvlm_flt4 w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
  __builtin_nontemporal_store(w, (__attribute__((address_space(1))) pvlm_flt4*)(p));
#else
  *p = v;
#endif
}

// four points per lane, 16-byte vector accesses only (3 loads, 2 stores): the device-resident whole-panorama form
__global__ __launch_bounds__(256) void k_cam_to_image_f32x4(int rows, int cols, long long n4, const float4* __restrict__ cam, float4* __restrict__ px) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 a = map_load4(cam + 3 * i), b = map_load4(cam + 3 * i + 1), c = map_load4(cam + 3 * i + 2);
  const float p[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
  float o[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
    const float lon = fast_atan2<float>(x, z);
    const float lat = -fast_atan2<float>(y, pvlm_exact::sqrt_via_double(x * x + z * z));
    o[2 * k] = (float)(cols * (0.5 + pvlm_exact::div_two_pi(lon)));
    o[2 * k + 1] = (float)(rows * (0.5 - pvlm_exact::div_pi(lat)));
  }
  map_store4(px + 2 * i, make_float4(o[0], o[1], o[2], o[3]));
  map_store4(px + 2 * i + 1, make_float4(o[4], o[5], o[6], o[7]));
}

template <typename T, bool LIBRARY_TRIG>
__global__ void k_image_to_cam(int rows, int cols, long long n, const T* __restrict__ px, T r, T* __restrict__ cam) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // ImageToSphere :102-103 ; SphereToCam :125-128 (float trig = the double value rounded to float)
  const T sx = (T)((2 * px[2 * i] / cols - 1) * 3.14159265358979323846);
  const T sy = (T)((0.5 - px[2 * i + 1] / rows) * 3.14159265358979323846);
  T cy, sny, snx, csx;
  if (sizeof(T) == 4 && !LIBRARY_TRIG) {
    float a, b, c, d;
    sincos_f32_arg((float)sy, &a, &b);
    sincos_f32_arg((float)sx, &c, &d);
    sny = (T)a; cy = (T)b; snx = (T)c; csx = (T)d;
  } else {
    cy = (T)cos((double)sy); sny = (T)sin((double)sy); snx = (T)sin((double)sx); csx = (T)cos((double)sx);
  }
  cam[3 * i] = r * cy * snx;
  cam[3 * i + 1] = -r * sny;
  cam[3 * i + 2] = r * cy * csx;
}
static bool exact_trig() { static const bool v = getenv("PVLM_EXACT_TRIG") != nullptr; return v; }

// Whole-panorama form of the float map: four pixels per lane, every global access a 16-byte vector (2 loads, 3 stores)
// instead of 8- and 12-byte pieces — the kernel is a 20 B/pixel stream once the trigonometry is cheap.
__global__ __launch_bounds__(256) void k_image_to_cam_f32x4(int rows, int cols, long long n4, const float4* __restrict__ px, float r, float4* __restrict__ cam) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 a = map_load4(px + 2 * i), b = map_load4(px + 2 * i + 1);
  const float u[4] = {a.x, a.z, b.x, b.z}, v[4] = {a.y, a.w, b.y, b.w};
  float o[12];
  const float fc = (float)cols, fr = (float)rows, inv_c = 1.0f / fc, inv_r = 1.0f / fr;
  float arg[8], sn[8], cs[8];       // sy of the four pixels, then sx of the four pixels
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // 2 u / cols and v / rows: the correctly rounded float quotients by one FMA correction of x * RN(1 / c)
    // (pvlm_exact::div_f32; identical wherever the quotient is a normal number, and the "- 1" / "0.5 -" absorb the rest)
    arg[4 + k] = (float)((pvlm_exact::div_f32(2 * u[k], fc, inv_c) - 1) * 3.14159265358979323846);
    arg[k] = (float)((0.5 - pvlm_exact::div_f32(v[k], fr, inv_r)) * 3.14159265358979323846);
  }
  sincos_f32_args<8>(arg, sn, cs);
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[3 * k] = r * cs[k] * sn[4 + k]; o[3 * k + 1] = -r * sn[k]; o[3 * k + 2] = r * cs[k] * cs[4 + k]; }
  map_store4(cam + 3 * i, make_float4(o[0], o[1], o[2], o[3]));
  map_store4(cam + 3 * i + 1, make_float4(o[4], o[5], o[6], o[7]));
  map_store4(cam + 3 * i + 2, make_float4(o[8], o[9], o[10], o[11]));
}

// ---- LiDAR-seeded sparse depth image: ProjectLidar2PanoramaDepth (util/Visualization.h:407-441) ----------------
// The reference paints the points in cloud order, so a pixel ends up with the depth of the LAST point whose window
// covers it.  Pass 1: every point atomically maximises (point index << 16 | depth16) over its window — the winner is
// exactly that last writer; pass 2 keeps the low 16 bits.
__global__ __launch_bounds__(256) void k_depth_splat(int rows, int cols, long long n, const float* __restrict__ xyz, const double* __restrict__ T_cl,
                                                     int half, unsigned long long* __restrict__ img) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = (float)(T_cl[4 * r] * (double)x + T_cl[4 * r + 1] * (double)y + T_cl[4 * r + 2] * (double)z + T_cl[4 * r + 3]);
  const float lon = fast_atan2<float>(p[0], p[2]);
  const float lat = -fast_atan2<float>(p[1], pvlm_exact::sqrt_via_double(p[0] * p[0] + p[2] * p[2]));
  const float px = (float)(cols * (0.5 + pvlm_exact::div_two_pi(lon)));
  const float py = (float)(rows * (0.5 - pvlm_exact::div_pi(lat)));
  const int rbx = (int)(ceilf(px) + (float)half), rby = (int)(ceilf(py) + (float)half);
  const int ltx = (int)(floorf(px) - (float)half), lty = (int)(floorf(py) - (float)half);
  if (!(rbx >= 0 && rby >= 0 && rbx + 1 <= cols && rby + 1 <= rows)) return;
  if (!(ltx >= 0 && lty >= 0 && ltx + 1 <= cols && lty + 1 <= rows)) return;
  const float depth = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const unsigned short rel = (unsigned short)(unsigned int)((double)depth * 256.0);
  const unsigned long long key = ((unsigned long long)(i + 1) << 16) | rel;
  for (int u = lty; u <= rby; ++u)
    for (int v = ltx; v <= rbx; ++v) atomicMax(&img[(size_t)u * cols + v], key);
}

__global__ void k_depth_finish(long long npix, const unsigned long long* __restrict__ img, unsigned short* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npix) out[i] = (unsigned short)(img[i] & 0xffffull);
}

// ---- K8 -----------------------------------------------------------------------------------------
__device__ __forceinline__ double vangle(const double* a, const double* b) {  // VectorAngle3D, Geometry.hpp:450-466
  double c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double n1 = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const double n2 = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  c = c / (n1 * n2);
  if (c >= 1.0) return 0.0;
  if (c <= -1.0) return 3.14159265358979323846;
  return acos(c);
}

// line table row: [image_plane(4, normalised) | p4(3) | image_line_scope(1)]
// One launch for every (frame, LiDAR) pair of AssociateLineMulti (joint_optimization/CameraLidarOptimizer.cpp:345-377); pvlm_cam_lidar_votes is a batch
// of one.  Work item = (pair, image line, corner point).
struct pvlm_cam_pair_desc {
  const float* xyz; const int* p2s_off; const int* p2s_ids;
  int n_pts, n_lines, n_seg;
  long long tab_off;    // first line-table row of the pair (rows of 8 doubles)
  long long vote_off;   // first vote of the pair (n_lines x n_seg block)
  long long work_off;
  double T[12];         // T_cl rows 0..2
  long long pt_off;     // prefix sum of n_pts (k_cam_lidar_votes_points: a thread per point)
};

__device__ __forceinline__ void cam_vote_one(const float* __restrict__ xyz_local, const int* __restrict__ p2s_off, const int* __restrict__ p2s_ids,
                                             int i, int li, const double* __restrict__ L, const double* T_cl, int n_seg, double angle_thr,
                                             int* __restrict__ votes) {
  if (p2s_off[i] == p2s_off[i + 1]) return;
  const float x = xyz_local[3 * i], y = xyz_local[3 * i + 1], z = xyz_local[3 * i + 2];
  const float range = x * x + y * y + z * z;
  if (range > 15 * 15) return;
  double p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = (double)(float)(T_cl[r * 4] * (double)x + T_cl[r * 4 + 1] * (double)y + T_cl[r * 4 + 2] * (double)z + T_cl[r * 4 + 3]);
  const double dis = fabs(L[0] * p[0] + L[1] * p[1] + L[2] * p[2] + L[3]);
  double pp[3] = {p[0] - dis * L[0], p[1] - dis * L[1], p[2] - dis * L[2]};
  if (fabs(L[0] * pp[0] + L[1] * pp[1] + L[2] * pp[2] + L[3]) > 1e-4) {
    pp[0] = p[0] + dis * L[0]; pp[1] = p[1] + dis * L[1]; pp[2] = p[2] + dis * L[2];
  }
  if (vangle(p, pp) >= angle_thr) return;
  if (vangle(L + 4, pp) >= L[7] + angle_thr) return;
  for (int k = p2s_off[i]; k < p2s_off[i + 1]; ++k) atomicAdd(&votes[(size_t)li * n_seg + p2s_ids[k]], 1);
}

__global__ __launch_bounds__(256) void k_cam_lidar_votes_batch(int n_pairs, const pvlm_cam_pair_desc* __restrict__ desc,
                                                               const long long* __restrict__ work_off, long long total,
                                                               const double* __restrict__ line_tab, double angle_thr, int* __restrict__ votes) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const int p = find_pair(work_off, n_pairs, g);
  const pvlm_cam_pair_desc* d = desc + p;
  const long long l = g - d->work_off;
  const int li = (int)(l / d->n_pts), i = (int)(l - (long long)li * d->n_pts);
  cam_vote_one(d->xyz, d->p2s_off, d->p2s_ids, i, li, line_tab + 8 * (d->tab_off + li), d->T, d->n_seg, angle_thr, votes + d->vote_off);
}

// K8 with a thread per (pair, corner point) that walks the pair's image lines (round 6).  The thread-per-test form above pays per TEST for what belongs to the point:
// the bisection through the pair offsets, a 64-bit division, the pair's 3 x 4 transform and the transformed point itself — and takes two arc cosines, two divisions
// and four square roots to compare two angles with thresholds.  Here the point is transformed once, and an angle is compared with its threshold on squared
// quantities: angle(a, b) >= t  <=>  a.b / (|a| |b|) <= cos t for 0 < t < pi, decided as sign and (a.b)^2 against cos^2 t |a|^2 |b|^2 whenever the two sides
// differ by more than 10^-11 of their sum (the rounding of either side is ~10^-15); inside that band, for thresholds within 0.8 degrees of 0 or pi (where acos
// amplifies the rounding of its argument) and for non-finite input the reference's own chain — VectorAngle3D with its roots, quotient and acos — decides, as in the
// form above.  cos(scope + threshold) of every table row comes from k_cam_line_cos (NaN outside (0, pi): the exact chain).  Same vote blocks.
__device__ __forceinline__ int angle_ge_fast(double d, double A2, double B2, double ct) {      // 1: angle >= t, 0: angle < t, -1: undecided
  if (!(fabs(ct) <= 0.9999)) return -1;
  const double S = A2 * B2;
  if (!(S > 0.0) || !(S < 1.0e300) || !(fabs(d) < 1.0e150)) return -1;
  const double lhs = d * d, rhs = ct * ct * S;
  if (fabs(lhs - rhs) <= 1.0e-11 * (lhs + rhs)) return -1;
  if (ct >= 0.0) return d <= 0.0 ? 1 : (lhs < rhs ? 1 : 0);
  return d >= 0.0 ? 0 : (lhs > rhs ? 1 : 0);
}
__global__ __launch_bounds__(256) void k_cam_line_cos(long long n_rows, const double* __restrict__ line_tab, double angle_thr, double* __restrict__ cs) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const double t = line_tab[8 * r + 7] + angle_thr;
  cs[r] = (t > 0.0 && t < 3.14159265358979323846) ? cos(t) : __longlong_as_double(0x7ff8000000000000ll);
}
__device__ __forceinline__ int find_cam_pair(const pvlm_cam_pair_desc* __restrict__ desc, int n_pairs, long long g) {
  int lo = 0, hi = n_pairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].pt_off <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_cam_lidar_votes_points(int n_pairs, const pvlm_cam_pair_desc* __restrict__ desc, long long total_pts,
                                                                const double* __restrict__ line_tab, const double* __restrict__ line_cos, double angle_thr, double cos_thr,
                                                                int* __restrict__ votes) {
  __shared__ int s_p0;
  const long long g0 = (long long)blockIdx.x * 256;
  if (threadIdx.x == 0) s_p0 = find_cam_pair(desc, n_pairs, g0 < total_pts ? g0 : total_pts - 1);
  __syncthreads();
  const long long g = g0 + threadIdx.x;
  if (g >= total_pts) return;
  int pr = s_p0;
  while (pr + 1 < n_pairs && desc[pr + 1].pt_off <= g) ++pr;
  const pvlm_cam_pair_desc* d = desc + pr;
  const int i = (int)(g - d->pt_off);
  const int* p2s_off = d->p2s_off;
  const int k0 = p2s_off[i], k1 = p2s_off[i + 1];
  if (k0 == k1) return;
  const float* xyz = d->xyz;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  const float range = x * x + y * y + z * z;
  if (range > 15 * 15) return;
  double p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = (double)(float)(d->T[r * 4] * (double)x + d->T[r * 4 + 1] * (double)y + d->T[r * 4 + 2] * (double)z + d->T[r * 4 + 3]);
  const double A2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  const int n_lines = d->n_lines, n_seg = d->n_seg;
  const double* L = line_tab + 8 * d->tab_off;
  const double* cs = line_cos + d->tab_off;
  int* v = votes + d->vote_off;
  const int* p2s_ids = d->p2s_ids;
  for (int li = 0; li < n_lines; ++li, L += 8) {
    const double l0 = L[0], l1 = L[1], l2 = L[2], l3 = L[3];
    const double dis = fabs(l0 * p[0] + l1 * p[1] + l2 * p[2] + l3);
    double pp[3] = {p[0] - dis * l0, p[1] - dis * l1, p[2] - dis * l2};
    if (fabs(l0 * pp[0] + l1 * pp[1] + l2 * pp[2] + l3) > 1e-4) {
      pp[0] = p[0] + dis * l0; pp[1] = p[1] + dis * l1; pp[2] = p[2] + dis * l2;
    }
    const double B2 = pp[0] * pp[0] + pp[1] * pp[1] + pp[2] * pp[2];
    int r1 = angle_ge_fast(p[0] * pp[0] + p[1] * pp[1] + p[2] * pp[2], A2, B2, cos_thr);
    if (r1 < 0) r1 = vangle(p, pp) >= angle_thr ? 1 : 0;
    if (r1) continue;                                                  // :419
    const double q0 = L[4], q1 = L[5], q2 = L[6];
    int r2 = angle_ge_fast(q0 * pp[0] + q1 * pp[1] + q2 * pp[2], q0 * q0 + q1 * q1 + q2 * q2, B2, cs[li]);
    if (r2 < 0) r2 = vangle(L + 4, pp) >= L[7] + angle_thr ? 1 : 0;
    if (r2) continue;                                                  // :422
    for (int k = k0; k < k1; ++k) atomicAdd(&v[(size_t)li * n_seg + p2s_ids[k]], 1);
  }
}

// Sparse read-back of a vote buffer: of the n_lines x n_segments counters of a pair a few per cent are non-zero (43 MB of dense blocks for
// the 1 362 pairs of a Room sequence).  Tile = 4096 consecutive counters, 16 per thread: k_votes_count leaves the non-zeros per tile, the host
// turns them into offsets, k_votes_emit writes (dense index, count) in dense order — the order the host walks the pairs in.
#define PVLM_NZ_TILE 4096
__global__ __launch_bounds__(256) void k_votes_count(long long n, const int* __restrict__ votes, int* __restrict__ tile_count) {
  const long long base = (long long)blockIdx.x * PVLM_NZ_TILE + threadIdx.x * 16;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) c += (base + k < n && votes[base + k] != 0) ? 1 : 0;
  __shared__ int s[256];
  s[threadIdx.x] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) { if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off]; __syncthreads(); }
  if (threadIdx.x == 0) tile_count[blockIdx.x] = s[0];
}
__global__ __launch_bounds__(256) void k_votes_emit(long long n, const int* __restrict__ votes, const long long* __restrict__ tile_off, long long* __restrict__ nz_index,
                                                    int* __restrict__ nz_count) {
  const long long base = (long long)blockIdx.x * PVLM_NZ_TILE + threadIdx.x * 16;
  int v[16], c = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { v[k] = base + k < n ? votes[base + k] : 0; c += v[k] != 0 ? 1 : 0; }
  __shared__ int s[256];
  s[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {            // inclusive scan of the per-thread counts
    const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  long long o = tile_off[blockIdx.x] + s[threadIdx.x] - c;
#pragma unroll
  for (int k = 0; k < 16; ++k) if (v[k] != 0) { nz_index[o] = base + k; nz_count[o] = v[k]; ++o; }
}

// ---- host: what the calls below share -------------------------------------------------------------------------------
namespace {
template <typename T> struct HostEq {
  int rows, cols;
  void ImageToCam(const T* px, T r, T* cam) const {
    T s[2];
    s[0] = (2 * px[0] / cols - 1) * M_PI;
    s[1] = (0.5 - px[1] / rows) * M_PI;
    T cy = (T)std::cos((double)s[1]);
    cam[0] = r * cy * (T)std::sin((double)s[0]);
    cam[1] = -r * (T)std::sin((double)s[1]);
    cam[2] = r * cy * (T)std::cos((double)s[0]);
  }
};
inline double h_vangle(const double* a, const double* b) {
  double c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double n1 = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const double n2 = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  c = c / (n1 * n2);
  if (c >= 1.0) return 0.0;
  if (c <= -1.0) return M_PI;
  return std::acos(c);
}
}  // namespace

// status of a HIP call that hands back a hipError_t of its own (hipGetLastError after a launch, hipMemsetAsync); the copies and the
// synchronisation go through pvlm_i_h2d_q / pvlm_i_d2h_q / pvlm_i_sync, whose status and error text are passed on as they are
static pvlm_status hip_status(pvlm_ctx* ctx, const char* what, hipError_t e) {
  if (e == hipSuccess) return PVLM_OK;
  PVLM_SET_ERR(ctx, "%s: %s", what, hipGetErrorString(e));
  return PVLM_ERR_HIP;
}
// the one synchronisation of a call, on every way out: the staged read-backs reach the caller's buffers, and the call's pvlm_dev_scratch
// (declared before it) may hand its blocks back
static pvlm_status finish(pvlm_ctx* ctx, pvlm_status st) {
  const pvlm_status s2 = pvlm_i_sync(ctx);
  return st ? st : s2;
}

pvlm_status pvlm_depth_launch::splat(pvlm_ctx* ctx, const char* who, int rows, int cols, long long n, const float* d_xyz, const double* d_T, unsigned size,
                                     unsigned long long* d_img) {
  if (n <= 0) return PVLM_OK;
  hipLaunchKernelGGL(k_depth_splat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, n, d_xyz, d_T, (int)(size / 2), d_img);
  return hip_status(ctx, who, hipGetLastError());
}

// ---- host: K7 and the depth image -----------------------------------------------------------------------------------
template <typename T, typename K>
static pvlm_status run_map(pvlm_ctx* ctx, long long n, const T* in, int in_w, T* out, int out_w, K launch) {
  if (n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_dev_scratch tmp(ctx);
  T *d_in = nullptr, *d_out = nullptr;
  pvlm_status st = tmp.alloc(&d_in, (size_t)n * in_w);
  if (!st) st = tmp.alloc(&d_out, (size_t)n * out_w);
  if (!st) st = pvlm_i_h2d_q(ctx, d_in, in, (size_t)n * in_w * sizeof(T));
  if (!st) { launch(d_in, d_out); st = hip_status(ctx, "equirect map", hipGetLastError()); }
  if (!st) st = pvlm_i_d2h_q(ctx, out, d_out, (size_t)n * out_w * sizeof(T));
  return finish(ctx, st);
}

extern "C" {

pvlm_status pvlm_cam_to_image_f32(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* cam, float* px) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!cam || !px))) return PVLM_ERR_ARG;
  return run_map<float>(ctx, n, cam, 3, px, 2, [&](float* di, float* dout) {
    hipLaunchKernelGGL(k_cam_to_image<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, di, dout);
  });
}
pvlm_status pvlm_cam_to_image_f64(pvlm_ctx* ctx, int rows, int cols, int64_t n, const double* cam, double* px) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!cam || !px))) return PVLM_ERR_ARG;
  return run_map<double>(ctx, n, cam, 3, px, 2, [&](double* di, double* dout) {
    hipLaunchKernelGGL(k_cam_to_image<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, di, dout);
  });
}
pvlm_status pvlm_image_to_cam_f32(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* px, float r, float* cam) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!cam || !px))) return PVLM_ERR_ARG;
  return run_map<float>(ctx, n, px, 2, cam, 3, [&](float* di, float* dout) {
    if (exact_trig()) hipLaunchKernelGGL((k_image_to_cam<float, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, di, r, dout);
    else hipLaunchKernelGGL((k_image_to_cam<float, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, di, r, dout);
  });
}
pvlm_status pvlm_image_to_cam_f64(pvlm_ctx* ctx, int rows, int cols, int64_t n, const double* px, double r, double* cam) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!cam || !px))) return PVLM_ERR_ARG;
  return run_map<double>(ctx, n, px, 2, cam, 3, [&](double* di, double* dout) {
    hipLaunchKernelGGL((k_image_to_cam<double, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, di, r, dout);
  });
}

pvlm_status pvlm_project_lidar_depth(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* xyz, const double* T_cl, unsigned size,
                                     uint16_t* depth) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || !T_cl || !depth || (n > 0 && !xyz)) return PVLM_ERR_ARG;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  const size_t npix = (size_t)rows * cols;
  pvlm_dev_scratch tmp(ctx);
  float* d_xyz = nullptr; double* d_T = nullptr; unsigned long long* d_img = nullptr; unsigned short* d_out = nullptr;
  pvlm_status st = tmp.alloc(&d_xyz, (size_t)n * 3);
  if (!st) st = tmp.alloc(&d_T, (size_t)16);
  if (!st) st = tmp.alloc(&d_img, npix);
  if (!st) st = tmp.alloc(&d_out, npix);
  if (!st) st = hip_status(ctx, "project_lidar_depth", hipMemsetAsync(d_img, 0, npix * sizeof(unsigned long long), ctx->stream));
  if (!st && n > 0) st = pvlm_i_h2d_q(ctx, d_xyz, xyz, (size_t)n * 3 * sizeof(float));
  if (!st) st = pvlm_i_h2d_q(ctx, d_T, T_cl, 16 * sizeof(double));
  if (!st) st = pvlm_depth_launch::splat(ctx, "project_lidar_depth", rows, cols, (long long)n, d_xyz, d_T, size, d_img);
  if (!st) {
    hipLaunchKernelGGL(k_depth_finish, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, ctx->stream, (long long)npix, d_img, d_out);
    st = hip_status(ctx, "project_lidar_depth", hipGetLastError());
  }
  if (!st) st = pvlm_i_d2h_q(ctx, depth, d_out, npix * sizeof(unsigned short));
  return finish(ctx, st);
}

// device-resident variants (async on the ctx stream, no copies): the panorama-sized maps of the MVS / depth-prior
// consumers and of bench.py's panorama block
pvlm_status pvlm_cam_to_image_f32_dev(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* d_cam, float* d_px) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!d_cam || !d_px))) return PVLM_ERR_ARG;
  if (n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if ((((uintptr_t)d_px | (uintptr_t)d_cam) & 15) == 0 && n >= 4) {
    const long long n4 = n / 4, tail = n - 4 * n4;
    hipLaunchKernelGGL(k_cam_to_image_f32x4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, n4, reinterpret_cast<const float4*>(d_cam),
                       reinterpret_cast<float4*>(d_px));
    if (tail) hipLaunchKernelGGL(k_cam_to_image<float>, dim3(1), dim3(64), 0, ctx->stream, rows, cols, tail, d_cam + 12 * n4, d_px + 8 * n4);
  } else hipLaunchKernelGGL(k_cam_to_image<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, d_cam, d_px);
  PVLM_HIP(ctx, hipGetLastError());
  return PVLM_OK;
}
pvlm_status pvlm_image_to_cam_f32_dev(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* d_px, float r, float* d_cam) {
  if (!ctx || n < 0 || rows <= 0 || cols <= 0 || (n > 0 && (!d_cam || !d_px))) return PVLM_ERR_ARG;
  if (n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (exact_trig()) hipLaunchKernelGGL((k_image_to_cam<float, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, d_px, r, d_cam);
  else if ((((uintptr_t)d_px | (uintptr_t)d_cam) & 15) == 0 && n >= 4) {
    const long long n4 = n / 4, tail = n - 4 * n4;
    hipLaunchKernelGGL(k_image_to_cam_f32x4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, n4, reinterpret_cast<const float4*>(d_px), r,
                       reinterpret_cast<float4*>(d_cam));
    if (tail) hipLaunchKernelGGL((k_image_to_cam<float, false>), dim3(1), dim3(64), 0, ctx->stream, rows, cols, tail, d_px + 8 * n4, r, d_cam + 12 * n4);
  } else hipLaunchKernelGGL((k_image_to_cam<float, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rows, cols, (long long)n, d_px, r, d_cam);
  PVLM_HIP(ctx, hipGetLastError());
  return PVLM_OK;
}

}  // extern "C"

// ---- host: the vote calls of K4 and K8 ------------------------------------------------------------------------------
// TransformLines(ref.segment_coeffs, ref.GetPose())   LidarFeatureAssociate.cpp:219-236, :455
static void world_lines(const pvlm_scan* ref, double* lw) {
  const double* R = ref->R_wl; const double* t = ref->t_wl;
  for (int s = 0; s < ref->n_segments; ++s) {
    const double* c = &ref->h_seg_coeffs[6 * s];
    for (int i = 0; i < 3; ++i) {
      lw[6 * s + i] = ((R[i * 3] * c[0] + R[i * 3 + 1] * c[1]) + R[i * 3 + 2] * c[2]) + t[i];
      lw[6 * s + 3 + i] = (R[i * 3] * c[3] + R[i * 3 + 1] * c[4]) + R[i * 3 + 2] * c[5];
    }
  }
}

// per-line constants of AssociateByAngle (CameraLidarLineAssociate.cpp:396-406), host fp64:
// [image plane (4, normalised) | midpoint p4 (3) | half arc angle]
static void line_table_row(int rows, int cols, const float* l, double* t) {
  HostEq<double> eq{rows, cols};
  const double a[2] = {l[0], l[1]}, b[2] = {l[2], l[3]};
  double p1[3], p2[3];
  eq.ImageToCam(a, 1.0, p1);
  eq.ImageToCam(b, 1.0, p2);
  const double p3[3] = {0, 0, 0};   // FormPlane(p1, p2, 0): Geometry.hpp:328-336
  double pa = ((p2[1] - p1[1]) * (p3[2] - p1[2]) - (p2[2] - p1[2]) * (p3[1] - p1[1]));
  double pb = ((p2[2] - p1[2]) * (p3[0] - p1[0]) - (p2[0] - p1[0]) * (p3[2] - p1[2]));
  double pc = ((p2[0] - p1[0]) * (p3[1] - p1[1]) - (p2[1] - p1[1]) * (p3[0] - p1[0]));
  double pd = -(pa * p1[0] + pb * p1[1] + pc * p1[2]);
  const double nn = std::sqrt(pa * pa + pb * pb + pc * pc + pd * pd);
  if (nn * nn > 0.0) { pa /= nn; pb /= nn; pc /= nn; pd /= nn; }
  t[0] = pa; t[1] = pb; t[2] = pc; t[3] = pd;
  t[4] = (p1[0] + p2[0]) / 2.0; t[5] = (p1[1] + p2[1]) / 2.0; t[6] = (p1[2] + p2[2]) / 2.0;
  t[7] = h_vangle(p1, t + 4);
}

// The vote sequence of K4 and K8, on device pointers: descriptors, the offsets the chosen kernel finds its pair by and the table (world lines / line-table
// rows) go up, the vote block is zeroed, launch(...) queues the vote kernel when there is a test to make (off.back() > 0).  Nothing is synchronised and
// nothing is read back: *d_votes (n_votes counters, owned by `tmp`) is what the three tails below start from.  What the launcher needs besides the tables
// comes from a scratch of its own that goes back to the pool right behind the launch — the pool is stream-ordered — so that a tail can have the block.
template <typename D, typename Launch>
static pvlm_status queue_votes(pvlm_ctx* ctx, pvlm_dev_scratch& tmp, const char* what, const std::vector<D>& desc, const std::vector<long long>& off,
                               const std::vector<double>& tab, long long n_votes, Launch launch, int** d_votes) {
  D* d_desc = nullptr; long long* d_off = nullptr; double* d_tab = nullptr;
  pvlm_status st = tmp.alloc(&d_desc, desc.size());
  if (!st) st = tmp.alloc(&d_off, off.size());
  if (!st) st = tmp.alloc(&d_tab, tab.size());
  if (!st) st = tmp.alloc(d_votes, (size_t)n_votes);
  if (!st) st = pvlm_i_h2d_q(ctx, d_desc, desc.data(), desc.size() * sizeof(D));
  if (!st) st = pvlm_i_h2d_q(ctx, d_off, off.data(), off.size() * sizeof(long long));
  if (!st && !tab.empty()) st = pvlm_i_h2d_q(ctx, d_tab, tab.data(), tab.size() * sizeof(double));
  if (!st) st = hip_status(ctx, what, hipMemsetAsync(*d_votes, 0, (size_t)n_votes * sizeof(int), ctx->stream));
  if (!st && off.back() > 0) {
    pvlm_dev_scratch launch_tmp(ctx);
    st = launch(ctx, launch_tmp, (int)desc.size(), d_desc, d_off, off.back(), d_tab, *d_votes);
    if (!st) st = hip_status(ctx, what, hipGetLastError());
  }
  return st;
}

// dense tail: the whole vote block comes back (both *_votes_batch forms and the single-pair forms, which are a batch of one)
template <typename D, typename Launch>
static pvlm_status dense_votes(pvlm_ctx* ctx, const char* what, const std::vector<D>& desc, const std::vector<long long>& off, const std::vector<double>& tab,
                               long long n_votes, Launch launch, int32_t* votes) {
  pvlm_dev_scratch tmp(ctx);
  int* d_v = nullptr;
  pvlm_status st = queue_votes(ctx, tmp, what, desc, off, tab, n_votes, launch, &d_v);
  if (!st && n_votes > 0) st = pvlm_i_d2h_q(ctx, votes, d_v, (size_t)n_votes * sizeof(int));
  return finish(ctx, st);
}

// K4's pairs: descriptors, the world lines of the reference scans (a scan's lines once per call, not once per pair; left out of a sizing call, which needs
// none) and the prefixes over the pairs — tests (thread-per-test kernel), corner points (thread-per-point kernel) and rows (k_line_row_best).  A pair without
// reference segments has no rows and no points (FindAssociations: nr > 0).  false: a null scan.
struct LinePlan {
  std::vector<pvlm_line_pair_desc> desc;
  std::vector<long long> work_off, pt_off, row_off;
  std::vector<double> lines;
  long long n_votes = 0;
};
static bool line_batch_plan(int n_pairs, const pvlm_scan* const* ref, const pvlm_scan* const* nei, bool with_lines, LinePlan& pl) {
  pl.desc.assign((size_t)n_pairs, pvlm_line_pair_desc());
  pl.work_off.assign((size_t)n_pairs + 1, 0); pl.pt_off.assign((size_t)n_pairs + 1, 0); pl.row_off.assign((size_t)n_pairs + 1, 0);
  std::unordered_map<const pvlm_scan*, long long> line_off_of;
  long long nv = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (!ref[p] || !nei[p]) return false;
    pvlm_line_pair_desc& d = pl.desc[p];
    d.xyz = nei[p]->corner.d_xyz; d.p2s_off = nei[p]->d_p2s_off; d.p2s_ids = nei[p]->d_p2s_ids;
    d.n_pts = nei[p]->n_segments > 0 ? nei[p]->corner.n : 0; d.n_ref = ref[p]->n_segments;
    d.vote_off = nv; d.work_off = pl.work_off[p];
    if (with_lines) {
      auto it = line_off_of.find(ref[p]);
      if (it == line_off_of.end()) {
        it = line_off_of.emplace(ref[p], (long long)pl.lines.size() / 6).first;
        pl.lines.resize(pl.lines.size() + (size_t)ref[p]->n_segments * 6);
        world_lines(ref[p], pl.lines.data() + (size_t)it->second * 6);
      }
      d.line_off = it->second;
    }
    nv += (long long)nei[p]->n_segments * ref[p]->n_segments;
    pl.work_off[p + 1] = pl.work_off[p] + (long long)d.n_pts * d.n_ref;
    pl.pt_off[p + 1] = pl.pt_off[p] + (d.n_ref > 0 ? d.n_pts : 0);
    pl.row_off[p + 1] = pl.row_off[p] + (d.n_ref > 0 ? nei[p]->n_segments : 0);
  }
  pl.n_votes = nv;
  return true;
}
// K4's vote kernel.  by_points: a thread per corner point (off = the plan's pt_off), else a thread per test (off = work_off).
struct LineLaunch {
  double thr; bool by_points;
  const std::vector<long long>& off(const LinePlan& pl) const { return by_points ? pl.pt_off : pl.work_off; }
  pvlm_status operator()(pvlm_ctx* c, pvlm_dev_scratch&, int np, const pvlm_line_pair_desc* dd, const long long* d_off, long long total, const double* dl, int* dv) const {
    if (by_points) hipLaunchKernelGGL(k_line_votes_points, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, np, dd, d_off, total, dl, sqrt_threshold(thr), dv);
    else hipLaunchKernelGGL(k_line_votes_batch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, np, dd, d_off, total, dl, thr, dv);
    return PVLM_OK;
  }
};

extern "C" {

// a batch of one through the thread-per-test kernel; the early ways out touch no device
pvlm_status pvlm_line2line_votes(pvlm_ctx* ctx, const pvlm_scan* ref, const pvlm_scan* nei, float dist_threshold, int32_t* votes) {
  if (!ctx || !ref || !nei || !votes) return PVLM_ERR_ARG;
  const int nr = ref->n_segments, nn = nei->n_segments;
  if (nr == 0 || nn == 0) return PVLM_OK;
  std::memset(votes, 0, (size_t)nr * nn * sizeof(int32_t));
  if (nei->corner.n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  LinePlan pl;
  line_batch_plan(1, &ref, &nei, true, pl);
  return dense_votes(ctx, "line votes", pl.desc, pl.work_off, pl.lines, pl.n_votes, LineLaunch{(double)dist_threshold, false}, votes);
}

pvlm_status pvlm_line2line_votes_batch(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, float dist_threshold,
                                       int64_t* vote_offsets, int32_t* votes, int64_t capacity) {
  if (!ctx || n_pairs < 0 || !vote_offsets || (n_pairs > 0 && (!ref || !nei))) return PVLM_ERR_ARG;
  LinePlan pl;
  if (!line_batch_plan(n_pairs, ref, nei, votes != nullptr, pl)) return PVLM_ERR_ARG;
  const long long nv = pl.n_votes;
  for (int p = 0; p < n_pairs; ++p) vote_offsets[p] = pl.desc[p].vote_off;
  vote_offsets[n_pairs] = nv;
  if (!votes) return PVLM_OK;                       // sizing call
  if (capacity < nv) { PVLM_SET_ERR(ctx, "pvlm_line2line_votes_batch: %lld votes do not fit the capacity %lld", nv, (long long)capacity); return PVLM_ERR_CAPACITY; }
  if (nv == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  return dense_votes(ctx, "batched votes", pl.desc, pl.work_off, pl.lines, nv, LineLaunch{(double)dist_threshold, false}, votes);
}

// row-best tail: k_line_row_best over the vote block, 8 bytes per neighbour segment come back
pvlm_status pvlm_line2line_best_batch(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, float dist_threshold,
                                      int64_t* row_offsets, int32_t* best_col, int32_t* best_count, int64_t capacity) {
  if (!ctx || n_pairs < 0 || !row_offsets || (n_pairs > 0 && (!ref || !nei)) || ((best_col == nullptr) != (best_count == nullptr))) return PVLM_ERR_ARG;
  if (best_col) pvlm_i_trace("line2line_best_batch: enter");
  LinePlan pl;
  if (!line_batch_plan(n_pairs, ref, nei, best_col != nullptr, pl)) return PVLM_ERR_ARG;
  const long long rows = pl.row_off[n_pairs];
  for (int p = 0; p <= n_pairs; ++p) row_offsets[p] = pl.row_off[p];
  if (!best_col) return PVLM_OK;                    // sizing call
  if (capacity < rows) { PVLM_SET_ERR(ctx, "pvlm_line2line_best_batch: %lld rows do not fit the capacity %lld", rows, (long long)capacity); return PVLM_ERR_CAPACITY; }
  if (rows == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  std::vector<pvlm_row_desc> rdesc((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) { rdesc[p].vote_off = pl.desc[p].vote_off; rdesc[p].n_ref = pl.desc[p].n_ref; }
  pvlm_i_trace("line2line_best_batch: tables built on the host");
  // PVLM_LINE_VOTES=tests: the thread-per-test kernel of rounds 2-5 (A/B; the same vote blocks)
  static const bool per_test = getenv("PVLM_LINE_VOTES") && std::strcmp(getenv("PVLM_LINE_VOTES"), "tests") == 0;
  const double thr = (double)dist_threshold;
  const LineLaunch launch{thr, !per_test && thr == thr};            // a NaN threshold: dist > NaN is false for every test — the old kernel says so by itself
  pvlm_dev_scratch tmp(ctx);
  pvlm_row_desc* d_rdesc = nullptr; long long* d_row = nullptr; int *d_v = nullptr, *d_col = nullptr, *d_cnt = nullptr;
  pvlm_status st = tmp.alloc(&d_rdesc, rdesc.size());
  if (!st) st = tmp.alloc(&d_row, pl.row_off.size());
  if (!st) st = tmp.alloc(&d_col, (size_t)rows);
  if (!st) st = tmp.alloc(&d_cnt, (size_t)rows);
  if (!st) st = pvlm_i_h2d_q(ctx, d_rdesc, rdesc.data(), rdesc.size() * sizeof(pvlm_row_desc));
  if (!st) st = pvlm_i_h2d_q(ctx, d_row, pl.row_off.data(), pl.row_off.size() * sizeof(long long));
  if (!st) st = queue_votes(ctx, tmp, "pvlm_line2line_best_batch", pl.desc, launch.off(pl), pl.lines, pl.n_votes, launch, &d_v);
  if (!st) {
    hipLaunchKernelGGL(k_line_row_best, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, n_pairs, d_rdesc, d_row, rows, d_v, d_col, d_cnt);
    st = hip_status(ctx, "pvlm_line2line_best_batch", hipGetLastError());
  }
  if (getenv("PVLM_TRACE")) { char msg[128]; snprintf(msg, sizeof msg, "line2line_best_batch: %d pairs, %lld votes, %lld tests, %lld rows: queued", n_pairs, pl.n_votes, pl.work_off[n_pairs], rows); pvlm_i_trace(msg); }
  if (!st) st = pvlm_i_d2h_q(ctx, best_col, d_col, (size_t)rows * sizeof(int));
  if (!st) st = pvlm_i_d2h_q(ctx, best_count, d_cnt, (size_t)rows * sizeof(int));
  st = finish(ctx, st);
  pvlm_i_trace("line2line_best_batch: synchronised");
  return st;
}

// ---- host: K4b ----------------------------------------------------------------------------------------------------------
// 0: match m can be used; 1: its pair index is out of range or not sorted, or the pair has a null scan; 2: a segment index is out of range, or the
// neighbour scan was uploaded without its segment points
static int match_fault(int m, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, const int* match_pair, const int* match_nei_seg, const int* match_ref_seg) {
  const int p = match_pair[m];
  if (p < 0 || p >= n_pairs || (m > 0 && p < match_pair[m - 1]) || !ref[p] || !nei[p]) return 1;
  const int a = match_nei_seg[m], b = match_ref_seg[m];
  if (a < 0 || a >= nei[p]->n_segments || b < 0 || b >= ref[p]->n_segments || !nei[p]->d_seg_xyz) return 2;
  return 0;
}

pvlm_status pvlm_line2line_residuals(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, int n_matches, const int* match_pair,
                                     const int* match_nei_seg, const int* match_ref_seg, pvlm_functor kind, unsigned flags, double weight,
                                     pvlm_resset** out) {
  if (!ctx || !out || n_pairs < 0 || n_matches < 0 || (n_pairs > 0 && (!ref || !nei)) || (n_matches > 0 && (!match_pair || !match_nei_seg || !match_ref_seg)))
    return PVLM_ERR_ARG;
  *out = nullptr;
  if (kind != PVLM_POINT2LINE_ANGLE && kind != PVLM_POINT2LINE_METER) { PVLM_SET_ERR(ctx, "kind must be a point-to-line functor"); return PVLM_ERR_ARG; }
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_i_trace("line2line_residuals: enter");
  pvlm_resset* rs = new (std::nothrow) pvlm_resset();
  if (!rs) return PVLM_ERR_NOMEM;
  rs->kind = kind; rs->flags = flags & 0xFFu; rs->weight = weight; rs->ncols = 9;
  std::vector<pvlm_match_desc> md((size_t)n_matches);
  std::vector<pvlm_match_pose> poses;
  rs->h_out_start.assign(1, 0);
  // The per-match part — where the neighbour segment's points lie, how many they are, the reference line as (point, unit direction) — is independent work with a
  // cache miss or two per match (359 000 matches per outer iteration at Floor size: 8 ms on one thread): shared out over the host threads.  The bookkeeping that
  // runs ALONG the list (rows, pair table) stays serial below and only adds up the counts.
  {
    std::atomic<int> bad{-1};
    auto fill = [&](int m) {
      if (match_fault(m, n_pairs, ref, nei, match_pair, match_nei_seg, match_ref_seg)) { int none = -1; bad.compare_exchange_strong(none, m); return; }
      const pvlm_scan* R = ref[match_pair[m]]; const pvlm_scan* N = nei[match_pair[m]];
      const int a = match_nei_seg[m], b = match_ref_seg[m];
      pvlm_match_desc& d = md[(size_t)m];
      d.pts = N->d_seg_xyz + 3 * (size_t)N->h_seg_pt_off[(size_t)a];
      d.n_pts = N->h_seg_pt_off[(size_t)a + 1] - N->h_seg_pt_off[(size_t)a];
      const double* loc = &R->h_seg_coeffs[6 * (size_t)b];
      double A[3], B[3];
      for (int c = 0; c < 3; ++c) { A[c] = 0.1 * loc[3 + c] + loc[c]; B[c] = -0.1 * loc[3 + c] + loc[c]; }   // Line2Line::line_point1 / 2
      double dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];                                           // ctor: (A - B).normalized()
      const double n2 = dx * dx + dy * dy + dz * dz;
      if (n2 > 0.0) { const double nn = std::sqrt(n2); dx /= nn; dy /= nn; dz /= nn; }
      d.line[0] = A[0]; d.line[1] = A[1]; d.line[2] = A[2]; d.line[3] = dx; d.line[4] = dy; d.line[5] = dz;
    };
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>({pvlm_thread_cap(), (size_t)n_matches / 8192 + 1, (size_t)std::max(1u, std::thread::hardware_concurrency())}));
    std::atomic<int> next{0};
    auto work = [&]() { for (int lo = next.fetch_add(4096); lo < n_matches; lo = next.fetch_add(4096)) for (int m = lo; m < std::min(n_matches, lo + 4096); ++m) fill(m); };
    pvlm_run_workers(n_threads, work);                       // fill() allocates nothing and throws nothing
    if (bad.load() >= 0) {
      // the FIRST offending match is reported, as the serial loop did: there is one at bad or before it
      int first = 0, fault;
      while ((fault = match_fault(first, n_pairs, ref, nei, match_pair, match_nei_seg, match_ref_seg)) == 0) ++first;
      if (fault == 1) PVLM_SET_ERR(ctx, "match %d: pair index out of range or not sorted", first);
      else PVLM_SET_ERR(ctx, "match %d: segment out of range, or the neighbour scan was uploaded without seg_points_xyz", first);
      pvlm_i_resset_free(ctx, rs); return PVLM_ERR_ARG;
    }
  }
  long long row = 0;
  int last_pair = -1;
  for (int m = 0; m < n_matches; ++m) {
    const int p = match_pair[m];
    if (p != last_pair) {
      const pvlm_scan* R = ref[p]; const pvlm_scan* N = nei[p];
      if (last_pair >= 0) { rs->h_out_start.push_back(row); row = pvlm_i_seg_rows(row); }
      rs->h_seg_start.push_back(row);
      rs->h_ref.push_back(R->id); rs->h_nei.push_back(N->id);
      pvlm_match_pose P; std::memcpy(P.R, N->R_wl, 72); std::memcpy(P.t, N->t_wl, 24);
      poses.push_back(P);
      last_pair = p;
    }
    pvlm_match_desc& d = md[(size_t)m];
    d.pair = (int)poses.size() - 1;
    d.dst = row;
    row += d.n_pts;
  }
  // compact rows: the padding between segments is not counted
  rs->n_pairs = (int)rs->h_ref.size();
  if (rs->n_pairs > 0) rs->h_out_start.push_back(row);
  {   // h_out_start was filled with device rows so far: turn it into compact offsets
    long long compact = 0;
    std::vector<int64_t> off((size_t)rs->n_pairs + 1, 0);
    for (int p = 0; p < rs->n_pairs; ++p) { compact += rs->h_out_start[(size_t)p + 1] - rs->h_seg_start[(size_t)p]; off[(size_t)p + 1] = compact; }
    rs->h_out_start = off;
    rs->n = compact;
  }
  const long long R_rows = std::max<long long>(pvlm_i_seg_rows(row), 16);
  pvlm_i_trace("line2line_residuals: match table built");
  rs->n_dev = R_rows;
  rs->h_pair_block.assign((size_t)rs->n_pairs, 0);
  rs->h_seg_start.push_back(R_rows);
  double* d_block = nullptr;
  pvlm_status st = pvlm_i_alloc(ctx, &d_block, (size_t)R_rows * 9);
  if (st) { pvlm_i_resset_free(ctx, rs); return st; }
  rs->col_blocks.push_back(d_block); rs->block_rows.push_back(R_rows);
  pvlm_i_trace("line2line_residuals: column block allocated");
  pvlm_dev_scratch tmp(ctx);                         // the match and pose tables: read by k_line_rows only
  pvlm_match_desc* d_md = nullptr; pvlm_match_pose* d_po = nullptr;
  if (n_matches > 0) {
    st = tmp.alloc(&d_md, md.size());
    if (!st) st = tmp.alloc(&d_po, poses.size());
    if (!st) {
      pvlm_i_trace("line2line_residuals: tables allocated");
      st = pvlm_i_h2d_q(ctx, d_md, md.data(), md.size() * sizeof(pvlm_match_desc));
      if (!st) st = pvlm_i_h2d_q(ctx, d_po, poses.data(), poses.size() * sizeof(pvlm_match_pose));
      if (getenv("PVLM_TRACE")) { char msg[96]; snprintf(msg, sizeof msg, "line2line_residuals: %d matches, %lld rows: copies queued", n_matches, R_rows); pvlm_i_trace(msg); }
      if (!st) { hipLaunchKernelGGL(k_line_rows, dim3((unsigned)n_matches), dim3(64), 0, ctx->stream, d_md, d_po, d_block, R_rows); st = hip_status(ctx, "pvlm_line2line_residuals", hipGetLastError()); }
    }
  }
  pvlm_i_trace("line2line_residuals: copies + kernel queued");
  if (!st) st = pvlm_i_resset_finalize(ctx, rs);     // synchronises: the staging vectors above may go
  pvlm_i_trace("line2line_residuals: finalize (sync)");
  if (st) { pvlm_i_sync(ctx); pvlm_i_resset_free(ctx, rs); return st; }
  *out = rs;
  return PVLM_OK;
}

// ---- host: K8 -----------------------------------------------------------------------------------------------------------
// descriptors, work offsets and vote offsets of a batch of (frame, LiDAR) pairs; false: bad arguments
// Line blocks with the same content get ONE set of table rows: every frame meets its three neighbouring scans with the same image lines
// (AssociateLineMulti: 1 362 pairs, 454 distinct blocks).  Rewrites desc[p].tab_off to rows of the reduced table and returns the line ranges to build.
static void cam_dedupe_lines(int n_pairs, const int64_t* line_offsets, const float* lines, std::vector<pvlm_cam_pair_desc>& desc,
                             std::vector<std::pair<long long, long long>>& build /* (first line, count) */) {
  std::unordered_map<unsigned long long, std::vector<int>> seen;     // content hash -> pairs that introduced a block with it
  long long rows = 0;
  build.clear();
  std::vector<long long> first_row((size_t)n_pairs, 0);
  for (int p = 0; p < n_pairs; ++p) {
    const long long a = line_offsets[p], n = line_offsets[p + 1] - a;
    if (n <= 0) { desc[p].tab_off = 0; continue; }
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(lines + 4 * a);
    unsigned long long h = 1469598103934665603ull ^ (unsigned long long)n;
    for (size_t k = 0; k < (size_t)n * 16; k += 8) { unsigned long long w; std::memcpy(&w, bytes + k, 8); h = (h ^ w) * 1099511628211ull; h ^= h >> 29; }
    std::vector<int>& cand = seen[h];
    int same = -1;
    for (int q : cand)
      if (line_offsets[q + 1] - line_offsets[q] == n && std::memcmp(lines + 4 * line_offsets[q], lines + 4 * a, (size_t)n * 16) == 0) { same = q; break; }
    if (same >= 0) { first_row[(size_t)p] = first_row[(size_t)same]; }
    else { cand.push_back(p); first_row[(size_t)p] = rows; build.emplace_back(a, n); rows += n; }
    desc[p].tab_off = first_row[(size_t)p];
  }
}
static bool cam_batch_plan(int n_pairs, const int64_t* line_offsets, const pvlm_scan* const* lidar_local, const double* T_cl, std::vector<pvlm_cam_pair_desc>& desc,
                           std::vector<long long>& work_off, int64_t* vote_offsets, long long* n_votes) {
  desc.assign((size_t)n_pairs, pvlm_cam_pair_desc());
  work_off.assign((size_t)n_pairs + 1, 0);
  long long nv = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (!lidar_local[p] || line_offsets[p + 1] < line_offsets[p]) return false;
    pvlm_cam_pair_desc& d = desc[p];
    const pvlm_scan* l = lidar_local[p];
    d.xyz = l->corner.d_xyz; d.p2s_off = l->d_p2s_off; d.p2s_ids = l->d_p2s_ids;
    d.n_lines = (int)(line_offsets[p + 1] - line_offsets[p]); d.n_seg = l->n_segments;
    d.n_pts = (d.n_seg > 0 && d.n_lines > 0) ? l->corner.n : 0;
    d.tab_off = line_offsets[p]; d.vote_off = nv; d.work_off = work_off[p];
    d.pt_off = p == 0 ? 0 : desc[(size_t)p - 1].pt_off + desc[(size_t)p - 1].n_pts;
    for (int k = 0; k < 12; ++k) d.T[k] = T_cl[(size_t)p * 16 + k];
    vote_offsets[p] = nv;
    nv += (long long)d.n_lines * d.n_seg;
    work_off[p + 1] = work_off[p] + (long long)d.n_pts * d.n_lines;
  }
  vote_offsets[n_pairs] = nv;
  *n_votes = nv;
  return true;
}
// the per-line constants of every image line of the batch: host fp64 (the libm the reference was built on), rows shared out over the host threads
// (272 400 rows for a Room sequence: 13 ms on one thread)
static void cam_line_tables(int rows, int cols, const float* lines, const std::vector<std::pair<long long, long long>>& build, std::vector<double>& tab) {
  std::vector<long long> src;                       // table row -> line
  for (const auto& b : build) for (long long k = 0; k < b.second; ++k) src.push_back(b.first + k);
  const long long n_rows = (long long)src.size();
  tab.resize((size_t)n_rows * 8);
  const size_t n_threads = std::max<size_t>(1, std::min<size_t>({pvlm_thread_cap(), (size_t)(n_rows / 4096 + 1), (size_t)std::max(1u, std::thread::hardware_concurrency())}));
  std::atomic<long long> next{0};
  auto work = [&]() {
    for (long long b = next.fetch_add(1024); b < n_rows; b = next.fetch_add(1024))
      for (long long r = b; r < std::min(n_rows, b + 1024); ++r) line_table_row(rows, cols, lines + 4 * src[(size_t)r], &tab[8 * (size_t)r]);
  };
  pvlm_run_workers(n_threads, work);
}
// K8's vote kernel.  Default: a thread per corner point (k_cam_line_cos into a block of the launch's own scratch, then k_cam_lidar_votes_points).  per_test,
// or PVLM_CAM_VOTES=tests for the batch forms (A/B): the thread-per-test kernel of rounds 2-5, the same vote blocks.  Called with tests to make only, so
// there are corner points and table rows.
struct CamLaunch {
  long long n_rows = 0, total_pts = 0;   // rows of the (de-duplicated) line table; corner points of all pairs
  bool per_test = false;
  CamLaunch(const std::vector<pvlm_cam_pair_desc>& desc, const std::vector<double>& tab, bool per_test_)
      : n_rows((long long)(tab.size() / 8)), total_pts(desc.empty() ? 0 : desc.back().pt_off + desc.back().n_pts), per_test(per_test_) {}
  pvlm_status operator()(pvlm_ctx* c, pvlm_dev_scratch& own, int np, const pvlm_cam_pair_desc* dd, const long long* dw, long long tot, const double* dl, int* dv) const {
    pvlm_prof_scope prof(c, 3);
    const double thr = 3.0 / 180.0 * M_PI;
    const char* mode = getenv("PVLM_CAM_VOTES");
    if (per_test || (mode && std::strcmp(mode, "tests") == 0)) {
      hipLaunchKernelGGL(k_cam_lidar_votes_batch, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, np, dd, dw, tot, dl, thr, dv);
      return PVLM_OK;
    }
    double* d_cos = nullptr;
    const pvlm_status st = own.alloc(&d_cos, (size_t)n_rows);
    if (st) return st;
    hipLaunchKernelGGL(k_cam_line_cos, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, c->stream, n_rows, dl, thr, d_cos);
    hipLaunchKernelGGL(k_cam_lidar_votes_points, dim3((unsigned)((total_pts + 255) / 256)), dim3(256), 0, c->stream, np, dd, total_pts, dl, (const double*)d_cos, thr, std::cos(thr), dv);
    return PVLM_OK;
  }
};

// a batch of one through the thread-per-test kernel (whatever PVLM_CAM_VOTES says); the early ways out touch no device
pvlm_status pvlm_cam_lidar_votes(pvlm_ctx* ctx, int rows, int cols, const float* lines, int n_lines, const pvlm_scan* lidar,
                                 const double* T_cl, int32_t* votes) {
  if (!ctx || !lidar || !T_cl || n_lines < 0 || rows <= 0 || cols <= 0 || (n_lines > 0 && (!lines || !votes))) return PVLM_ERR_ARG;
  const int ns = lidar->n_segments;
  if (n_lines == 0 || ns == 0) return PVLM_OK;
  std::memset(votes, 0, (size_t)n_lines * ns * sizeof(int32_t));
  if (lidar->corner.n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  const int64_t line_offsets[2] = {0, n_lines};
  int64_t vote_offsets[2];
  std::vector<pvlm_cam_pair_desc> desc;
  std::vector<long long> work_off;
  std::vector<double> tab;
  long long nv = 0;
  cam_batch_plan(1, line_offsets, &lidar, T_cl, desc, work_off, vote_offsets, &nv);
  cam_line_tables(rows, cols, lines, {{0, (long long)n_lines}}, tab);
  return dense_votes(ctx, "cam-lidar votes", desc, work_off, tab, nv, CamLaunch(desc, tab, true), votes);
}

pvlm_status pvlm_cam_lidar_votes_batch(pvlm_ctx* ctx, int n_pairs, int rows, int cols, const int64_t* line_offsets, const float* lines,
                                       pvlm_scan* const* lidar_local, const double* T_cl, int64_t* vote_offsets, int32_t* votes, int64_t capacity) {
  if (!ctx || n_pairs < 0 || !vote_offsets || rows <= 0 || cols <= 0 || (n_pairs > 0 && (!line_offsets || !lidar_local || !T_cl))) return PVLM_ERR_ARG;
  std::vector<pvlm_cam_pair_desc> desc;
  std::vector<long long> work_off;
  long long nv = 0;
  const long long n_lines_total = n_pairs > 0 ? line_offsets[n_pairs] : 0;
  if (n_lines_total > 0 && !lines) return PVLM_ERR_ARG;
  if (!cam_batch_plan(n_pairs, line_offsets, lidar_local, T_cl, desc, work_off, vote_offsets, &nv)) return PVLM_ERR_ARG;
  if (!votes) return PVLM_OK;
  if (capacity < nv) { PVLM_SET_ERR(ctx, "pvlm_cam_lidar_votes_batch: %lld votes do not fit the capacity %lld", nv, (long long)capacity); return PVLM_ERR_CAPACITY; }
  if (nv == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  std::vector<double> tab;
  std::vector<std::pair<long long, long long>> build;
  cam_dedupe_lines(n_pairs, line_offsets, lines, desc, build);
  cam_line_tables(rows, cols, lines, build, tab);
  return dense_votes(ctx, "batched votes", desc, work_off, tab, nv, CamLaunch(desc, tab, false), votes);
}

// sparse tail: k_votes_count, the tile offsets on the host, k_votes_emit; (dense index, count) of the non-zero counters come back
pvlm_status pvlm_cam_lidar_votes_batch_sparse(pvlm_ctx* ctx, int n_pairs, int rows, int cols, const int64_t* line_offsets, const float* lines,
                                              pvlm_scan* const* lidar_local, const double* T_cl, int64_t* vote_offsets, int64_t* nz_index, int32_t* nz_count,
                                              int64_t capacity, int64_t* n_nz) {
  if (!ctx || n_pairs < 0 || !vote_offsets || !n_nz || capacity < 0 || (capacity > 0 && (!nz_index || !nz_count)) || rows <= 0 || cols <= 0 ||
      (n_pairs > 0 && (!line_offsets || !lidar_local || !T_cl)))
    return PVLM_ERR_ARG;
  *n_nz = 0;
  std::vector<pvlm_cam_pair_desc> desc;
  std::vector<long long> work_off;
  long long nv = 0;
  const long long n_lines_total = n_pairs > 0 ? line_offsets[n_pairs] : 0;
  if (n_lines_total > 0 && !lines) return PVLM_ERR_ARG;
  if (!cam_batch_plan(n_pairs, line_offsets, lidar_local, T_cl, desc, work_off, vote_offsets, &nv)) return PVLM_ERR_ARG;
  if (nv == 0 || work_off[n_pairs] == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  std::vector<double> tab;
  std::vector<std::pair<long long, long long>> build;
  cam_dedupe_lines(n_pairs, line_offsets, lines, desc, build);
  cam_line_tables(rows, cols, lines, build, tab);
  const long long tiles = (nv + PVLM_NZ_TILE - 1) / PVLM_NZ_TILE;
  std::vector<int> tile_count((size_t)tiles);
  std::vector<long long> tile_off((size_t)tiles);
  long long total = 0;
  pvlm_dev_scratch tmp(ctx);
  int *d_v = nullptr, *d_tc = nullptr, *d_nc = nullptr; long long *d_to = nullptr, *d_ni = nullptr;
  pvlm_status st = tmp.alloc(&d_tc, (size_t)tiles);
  if (!st) st = tmp.alloc(&d_to, (size_t)tiles);
  if (!st) st = queue_votes(ctx, tmp, "batched votes", desc, work_off, tab, nv, CamLaunch(desc, tab, false), &d_v);
  if (!st) {
    hipLaunchKernelGGL(k_votes_count, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, nv, d_v, d_tc);
    st = hip_status(ctx, "batched votes", hipGetLastError());
  }
  if (!st) st = pvlm_i_d2h_q(ctx, tile_count.data(), d_tc, (size_t)tiles * sizeof(int));
  if (!st) st = pvlm_i_sync(ctx);                   // the host turns the tile counts into offsets (and learns how much comes back)
  if (!st) {
    for (long long t = 0; t < tiles; ++t) { tile_off[(size_t)t] = total; total += tile_count[(size_t)t]; }
    *n_nz = total;
    if (total > capacity) { PVLM_SET_ERR(ctx, "pvlm_cam_lidar_votes_batch_sparse: %lld non-zero votes do not fit the capacity %lld", total, (long long)capacity); st = PVLM_ERR_CAPACITY; }
  }
  if (!st && total > 0) {
    st = tmp.alloc(&d_ni, (size_t)total);
    if (!st) st = tmp.alloc(&d_nc, (size_t)total);
    if (!st) st = pvlm_i_h2d_q(ctx, d_to, tile_off.data(), (size_t)tiles * sizeof(long long));
    if (!st) {
      hipLaunchKernelGGL(k_votes_emit, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, nv, d_v, d_to, d_ni, d_nc);
      st = hip_status(ctx, "batched votes", hipGetLastError());
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "index width");
    if (!st) st = pvlm_i_d2h_q(ctx, nz_index, d_ni, (size_t)total * sizeof(int64_t));
    if (!st) st = pvlm_i_d2h_q(ctx, nz_count, d_nc, (size_t)total * sizeof(int32_t));
  }
  return finish(ctx, st);
}

}  // extern "C"

// pvlm_preload: HIP loads the code object of a translation unit at the first launch of one of its kernels (15 ms for the larger ones) — an empty launch from here
// moves that out of the first call that needs this file's kernels
__global__ void k_preload_lines() {}
void pvlm_i_preload_lines(hipStream_t s) { hipLaunchKernelGGL(k_preload_lines, dim3(1), dim3(1), 0, s); }
