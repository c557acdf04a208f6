// K37: DepthCompletion (util/DepthCompletion.cpp:154-316) and the loop body of SfM::ComputeDepthImage (sfm/SfM.cpp:170-226) on the GPU.  The definition is
// pvlm_depthfill_core.h; this file wraps its per-pixel functions in three tiled kernels, one per phase between the two column scans:
//   k_fill_a  S0-S4  (reach 3 + 2 + 2 + 2 = 9)   input (uint16, fp32 or the splat's 64-bit image) -> s4, top 1
//   k_fill_b  S5     (reach 4)                    s4, top 1 -> s5, top 2
//   k_fill_c  S7a-u16 (reach 6 x 2 + 2 + 2 = 16)  s5, top 2 -> the dense fp32 and / or uint16 image
// A workgroup of 256 lanes owns a kTileH x kTileW tile of one image (blockIdx.z) and loads it with the phase's reach as halo into LDS.  No pass is in place over its
// neighbours: every stencil pass reads one of two LDS images and writes the other (a square is a row pass and a column pass), on a region that shrinks by the pass's
// reach (region<HALO, MR, MC>: the tile grown by MR rows and MC columns), so that every tap a pass reads was computed by the pass before it.  The only in-place
// update, the blend of a fill round, reads its own pixel alone.  A pixel outside the image holds, for the next reader, the value that never wins (0 for a maximum of
// values >= +0, +inf for a minimum); the medians clamp and the bilateral reflects their coordinates, which stays inside the loaded region.
// The column scans ride on the phases before them: a tile takes the minimum row of its valid pixels per column in LDS and sends one integer atomicMin per column
// (integer minima: no order dependence).
#include <cmath>
#include <cstdlib>

#include "pvlm_depth_launch.h"
#include "pvlm_depthfill_core.h"
#include "pvlm_depthset.h"
#include "pvlm_internal.h"

namespace {
namespace df = pvlm_depthfill;

constexpr int kTileH = 32;
constexpr int kTileW = 64;
constexpr int kThreads = 256;
constexpr int kTopNone = 0x7f7f7f7f;                    // a column without a valid pixel (hipMemsetAsync of 0x7f); read as row 0
constexpr size_t kBatchBytes = (size_t)1 << 30;         // device scratch of one batch of whole images

template <int HALO> struct Buf { static constexpr int H = kTileH + 2 * HALO, W = kTileW + 2 * HALO, N = H * W; };

// f(LDS index, image row, image column) for every position of the tile grown by MR rows and MC columns, then a barrier
template <int HALO, int MR, int MC, class F> __device__ __forceinline__ void region(int r0, int c0, F f) {
  static_assert(MR >= 0 && MC >= 0 && MR <= HALO && MC <= HALO, "a region lies inside the loaded tile");
  constexpr int W = kTileW + 2 * MC, H = kTileH + 2 * MR;
  for (int idx = threadIdx.x; idx < W * H; idx += kThreads) {
    const int rr = idx / W, cc = idx - rr * W;
    f((HALO - MR + rr) * Buf<HALO>::W + (HALO - MC + cc), r0 - MR + rr, c0 - MC + cc);
  }
  __syncthreads();
}

struct SrcU16 { const unsigned short* p; __device__ float operator()(size_t i) const { return df::from_u16(p[i]); } };
struct SrcF32 { const float* p; __device__ float operator()(size_t i) const { return p[i]; } };
struct SrcSplat { const unsigned long long* p; __device__ float operator()(size_t i) const { return df::from_u16((unsigned)(p[i] & 0xffffull)); } };

// the tile's share of a column scan and of a pixel count: colmin[c] -> top, the lanes' counts -> *total
__device__ __forceinline__ void tile_finish(int cols, int c0, const int* colmin, int* top_f, int* cnt, int my, unsigned long long* total) {
  if (my) atomicAdd(cnt, my);
  __syncthreads();
  if (top_f && threadIdx.x < kTileW && colmin[threadIdx.x] != kTopNone && c0 + (int)threadIdx.x < cols) atomicMin(&top_f[c0 + threadIdx.x], colmin[threadIdx.x]);
  if (total && threadIdx.x == 0 && *cnt) atomicAdd(total, (unsigned long long)*cnt);
}

template <class Src>
__global__ __launch_bounds__(kThreads) void k_fill_a(int rows, int cols, Src src, float M, float* __restrict__ s4, int* __restrict__ top, unsigned long long* valid_in) {
  constexpr int HALO = df::kReachA;
  using B = Buf<HALO>;
  __shared__ float A[B::N], Bf[B::N];
  __shared__ int colmin[kTileW], cnt;
  const int r0 = blockIdx.y * kTileH, c0 = blockIdx.x * kTileW;
  const size_t base = (size_t)blockIdx.z * rows * cols;
  const float inf = __builtin_inff();
  if (threadIdx.x < kTileW) colmin[threadIdx.x] = kTopNone;
  if (threadIdx.x == 0) cnt = 0;
  auto in = [&](int r, int c) { return r >= 0 && r < rows && c >= 0 && c < cols; };
  int my = 0;
  region<HALO, HALO, HALO>(r0, c0, [&](int i, int r, int c) {                                        // S0
    float v = 0.f;
    if (in(r, c)) {
      v = df::s0_of(src(base + (size_t)r * cols + c), M);
      my += (v > df::kValid) && r >= r0 && r < r0 + kTileH && c >= c0 && c < c0 + kTileW;
    }
    A[i] = v;
  });
  region<HALO, 6, 6>(r0, c0, [&](int i, int r, int c) {                                              // S1, S2
    Bf[i] = in(r, c) ? df::s2_pixel([&](int dr, int dc) { return A[i + dr * B::W + dc]; }, M) : 0.f;
  });
  region<HALO, 6, 4>(r0, c0, [&](int i, int r, int c) { A[i] = in(r, c) ? df::run_max<2>([&](int k) { return Bf[i + k]; }) : 0.f; });          // S3: dilate
  region<HALO, 4, 4>(r0, c0, [&](int i, int r, int c) { Bf[i] = in(r, c) ? df::run_max<2>([&](int k) { return A[i + k * B::W]; }) : inf; });
  region<HALO, 4, 2>(r0, c0, [&](int i, int r, int c) { A[i] = in(r, c) ? df::run_min<2>([&](int k) { return Bf[i + k]; }) : inf; });          //     erode
  region<HALO, 2, 2>(r0, c0, [&](int i, int r, int c) { Bf[i] = in(r, c) ? df::run_min<2>([&](int k) { return A[i + k * B::W]; }) : 0.f; });
  region<HALO, 0, 0>(r0, c0, [&](int i, int r, int c) {                                              // S4
    if (!in(r, c)) return;
    const float s3 = Bf[i];
    float out = s3;
    if (s3 > df::kValid)
      out = df::median5([&](int dr, int dc) { return Bf[(df::clampi(r + dr, rows) - (r0 - HALO)) * B::W + (df::clampi(c + dc, cols) - (c0 - HALO))]; });
    s4[base + (size_t)r * cols + c] = out;
    if (out > df::kValid) atomicMin(&colmin[c - c0], r);
  });
  tile_finish(cols, c0, colmin, top + (size_t)blockIdx.z * cols, &cnt, my, valid_in);
}

__device__ __forceinline__ int top_row(int t) { return t == kTopNone ? 0 : t; }

__global__ __launch_bounds__(kThreads) void k_fill_b(int rows, int cols, const float* __restrict__ s4, const int* __restrict__ top, float* __restrict__ s5,
                                                     int* __restrict__ top2) {
  constexpr int HALO = df::kReachB;
  using B = Buf<HALO>;
  __shared__ float A[B::N], Bf[B::N];
  __shared__ int colmin[kTileW], cnt;
  const int r0 = blockIdx.y * kTileH, c0 = blockIdx.x * kTileW;
  const size_t base = (size_t)blockIdx.z * rows * cols;
  if (threadIdx.x < kTileW) colmin[threadIdx.x] = kTopNone;
  if (threadIdx.x == 0) cnt = 0;
  auto in = [&](int r, int c) { return r >= 0 && r < rows && c >= 0 && c < cols; };
  region<HALO, HALO, HALO>(r0, c0, [&](int i, int r, int c) { A[i] = in(r, c) ? s4[base + (size_t)r * cols + c] : 0.f; });
  region<HALO, HALO, 0>(r0, c0, [&](int i, int r, int c) { Bf[i] = in(r, c) ? df::run_max<4>([&](int k) { return A[i + k]; }) : 0.f; });
  region<HALO, 0, 0>(r0, c0, [&](int i, int r, int c) {                                              // S5
    if (!in(r, c)) return;
    float v = A[i];
    if (!(v > df::kValid) && r >= top_row(top[(size_t)blockIdx.z * cols + c])) v = df::run_max<4>([&](int k) { return Bf[i + k * B::W]; });
    s5[base + (size_t)r * cols + c] = v;
    if (v > df::kValid) atomicMin(&colmin[c - c0], r);
  });
  tile_finish(cols, c0, colmin, top2 + (size_t)blockIdx.z * cols, &cnt, 0, nullptr);
}

// one fill round of S7a and the rounds after it: ROUND leaves the tile grown by kReachC - 2 (ROUND + 1) valid
template <int ROUND, class In>
__device__ __forceinline__ void fill_rounds(int r0, int c0, float* A, float* Bf, const int* tops, const In& in) {
  constexpr int HALO = df::kReachC, REM = HALO - 2 * (ROUND + 1);
  using B = Buf<HALO>;
  region<HALO, REM + 2, REM>(r0, c0, [&](int i, int r, int c) { Bf[i] = in(r, c) ? df::run_max<2>([&](int k) { return A[i + k]; }) : 0.f; });
  region<HALO, REM, REM>(r0, c0, [&](int i, int r, int c) {
    if (in(r, c) && A[i] < df::kValid && r >= tops[c - (c0 - HALO)]) A[i] = df::run_max<2>([&](int k) { return Bf[i + k * B::W]; });   // its own pixel of A only
  });
  if constexpr (ROUND + 1 < df::kFillRounds) fill_rounds<ROUND + 1>(r0, c0, A, Bf, tops, in);
}

__global__ __launch_bounds__(kThreads) void k_fill_c(int rows, int cols, const float* __restrict__ s5, const int* __restrict__ top2, float M,
                                                     float* __restrict__ dense, unsigned short* __restrict__ u16, unsigned long long* valid_out) {
  constexpr int HALO = df::kReachC;
  using B = Buf<HALO>;
  static_assert(HALO == 2 * df::kFillRounds + 4, "six fills, a median and the bilateral");
  __shared__ float A[B::N], Bf[B::N];
  __shared__ int tops[B::W], cnt;
  const int r0 = blockIdx.y * kTileH, c0 = blockIdx.x * kTileW;
  const size_t base = (size_t)blockIdx.z * rows * cols;
  if (threadIdx.x == 0) cnt = 0;
  for (int k = threadIdx.x; k < B::W; k += kThreads) {
    const int c = c0 - HALO + k;
    tops[k] = (c >= 0 && c < cols) ? top_row(top2[(size_t)blockIdx.z * cols + c]) : 0;
  }
  auto in = [&](int r, int c) { return r >= 0 && r < rows && c >= 0 && c < cols; };
  region<HALO, HALO, HALO>(r0, c0, [&](int i, int r, int c) { A[i] = in(r, c) ? s5[base + (size_t)r * cols + c] : 0.f; });
  fill_rounds<0>(r0, c0, A, Bf, tops, in);                                                           // S7a
  region<HALO, 2, 2>(r0, c0, [&](int i, int r, int c) {                                              // S7b
    if (!in(r, c)) return;
    float s7 = A[i];
    if (s7 > df::kValid && r >= tops[c - (c0 - HALO)])
      s7 = df::median5([&](int dr, int dc) { return A[(df::clampi(r + dr, rows) - (r0 - HALO)) * B::W + (df::clampi(c + dc, cols) - (c0 - HALO))]; });
    Bf[i] = s7;
  });
  int my = 0;
  region<HALO, 0, 0>(r0, c0, [&](int i, int r, int c) {                                              // S7c, S8, u16
    if (!in(r, c)) return;
    float s7 = Bf[i];
    if (A[i] > df::kValid && r >= tops[c - (c0 - HALO)])
      s7 = df::bilateral([&](int dy, int dx) { return Bf[(df::reflect101(r + dy, rows) - (r0 - HALO)) * B::W + (df::reflect101(c + dx, cols) - (c0 - HALO))]; });
    const float out = df::invert(s7, M);
    my += out > df::kValid;
    if (dense) dense[base + (size_t)r * cols + c] = out;
    if (u16) u16[base + (size_t)r * cols + c] = df::to_u16(out);
  });
  tile_finish(cols, c0, nullptr, nullptr, &cnt, my, valid_out);
}

// the images of one batch
int batch_images(int n_images, size_t bytes_per_image) {
  long long limit = (long long)std::max<size_t>(1, kBatchBytes / std::max<size_t>(1, bytes_per_image));
  limit = std::min<long long>(limit, 65535);                                                          // gridDim.z
  return (int)std::min<long long>(pvlm_i_env_limit("PVLM_DEPTHFILL_BATCH_IMAGES", limit), n_images);
}

struct Work {                                            // the device images of one batch of nb images: scratch of the frame, the two counters zeroed
  float* x; float* y; int* top; unsigned short* u16; unsigned long long* counts;
  Work(pvlm_call& c, size_t npix, int cols, int nb, bool want_u16)
      : x(c.alloc<float>(npix * nb)), y(c.alloc<float>(npix * nb)), top(c.alloc<int>(2 * (size_t)nb * cols)), u16(want_u16 ? c.alloc<unsigned short>(npix * nb) : nullptr),
        counts(c.alloc<unsigned long long>(2)) {}
};

// phases A, B, C of nb images on the stream: src -> (w.x | w.u16), the fp32 result in w.x when want_f32
template <class Src>
void run_phases(pvlm_call& c, int rows, int cols, int nb, Src src, float M, const Work& w, bool want_f32, bool want_u16) {
  const dim3 grid((unsigned)((cols + kTileW - 1) / kTileW), (unsigned)((rows + kTileH - 1) / kTileH), (unsigned)nb);
  c.memset(w.top, 0x7f, 2 * (size_t)nb * cols * sizeof(int));
  int* top2 = w.top + (size_t)nb * cols;
  c.launch(k_fill_a<Src>, grid, dim3(kThreads), 0, rows, cols, src, M, w.x, w.top, w.counts);
  c.check_launches();
  c.launch(k_fill_b, grid, dim3(kThreads), 0, rows, cols, w.x, w.top, w.y, top2);
  c.check_launches();
  c.launch(k_fill_c, grid, dim3(kThreads), 0, rows, cols, w.y, top2, M, want_f32 ? w.x : nullptr, want_u16 ? w.u16 : nullptr, w.counts + 1);
  c.check_launches();
}

// the device time of a batch's stages for the statistics: three events on the context's stream, read after the batch's synchronisation
struct StageClock {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  bool on = false;
  explicit StageClock(bool want) {
    if (!want) return;
    on = true;
    for (hipEvent_t& x : e) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; on = false; }
  }
  ~StageClock() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  void mark(pvlm_ctx* ctx, int k) { if (on) (void)hipEventRecord(e[k], ctx->stream); }
  double ms(int a, int b) const { float t = 0.f; return on && hipEventElapsedTime(&t, e[a], e[b]) == hipSuccess ? (double)t : 0.0; }
};

}  // namespace

extern "C" pvlm_status pvlm_depth_completion(pvlm_ctx* ctx, int rows, int cols, int n_images, const uint16_t* sparse_u16, const float* sparse_f32, float max_depth,
                                             float* dense_f32, uint16_t* dense_u16, pvlm_depthfill_stats* stats) {
  const char* who = "pvlm_depth_completion";
  if (!ctx) return PVLM_ERR_ARG;
  if (rows <= 0 || cols <= 0 || n_images < 0) { PVLM_SET_ERR(ctx, "%s: rows, cols or n_images", who); return PVLM_ERR_ARG; }
  if ((sparse_u16 != nullptr) == (sparse_f32 != nullptr)) { PVLM_SET_ERR(ctx, "%s: exactly one of the two inputs", who); return PVLM_ERR_ARG; }
  if (!dense_f32 && !dense_u16) { PVLM_SET_ERR(ctx, "%s: no output", who); return PVLM_ERR_ARG; }
  if (!std::isfinite(max_depth) || !(max_depth > 0.f)) { PVLM_SET_ERR(ctx, "%s: max_depth must be finite and > 0", who); return PVLM_ERR_ARG; }
  const size_t npix = (size_t)rows * cols;
  if (sparse_f32)
    for (size_t i = 0; i < npix * (size_t)n_images; ++i)
      if (!df::input_ok(sparse_f32[i])) { PVLM_SET_ERR(ctx, "%s: value %zu of the fp32 input is negative or not finite", who, i); return PVLM_ERR_ARG; }
  if (stats) *stats = pvlm_depthfill_stats{0, 0, 0, 0, 0.0, 0.0};
  if (n_images == 0) return PVLM_OK;
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const size_t in_bytes = sparse_u16 ? 2 : 4;
  const int limit = batch_images(n_images, npix * (in_bytes + 8 + (dense_u16 ? 2 : 0)));
  StageClock clock(stats != nullptr);
  for (int k0 = 0; k0 < n_images && !c.st; k0 += limit) {
    const int nb = std::min(limit, n_images - k0);
    pvlm_call::batch bs(c);                              // this batch's scratch
    const Work w(c, npix, cols, nb, dense_u16 != nullptr);
    unsigned long long counts[2] = {0, 0};
    c.memset(w.counts, 0, 2 * sizeof(unsigned long long));
    unsigned short* d_in16 = sparse_u16 ? c.upload(sparse_u16 + npix * k0, npix * nb) : nullptr;
    float* d_in32 = sparse_f32 ? c.upload(sparse_f32 + npix * k0, npix * nb) : nullptr;
    clock.mark(ctx, 1);
    if (sparse_u16) run_phases(c, rows, cols, nb, SrcU16{d_in16}, max_depth, w, dense_f32 != nullptr, dense_u16 != nullptr);
    else run_phases(c, rows, cols, nb, SrcF32{d_in32}, max_depth, w, dense_f32 != nullptr, dense_u16 != nullptr);
    clock.mark(ctx, 2);
    if (dense_f32) c.d2h(dense_f32 + npix * k0, w.x, npix * nb * 4);
    if (dense_u16) c.d2h(dense_u16 + npix * k0, w.u16, npix * nb * 2);
    c.d2h(counts, w.counts, sizeof(counts));
    if (!c.sync() && stats) { stats->images += nb; stats->batches += 1; stats->valid_in += (long long)counts[0]; stats->valid_out += (long long)counts[1]; stats->fill_ms += clock.ms(1, 2); }
  }
  return c.st;
}

namespace {
// The body of pvlm_compute_depth_images and pvlm_depthset_compute: the checks, the batches and the stream order are one; the destination of k_fill_c's uint16
// images is the parameter.  host_out: each batch's images land in a batch scratch and are downloaded behind its kernels.  dev_out (n_scans images of device memory
// that outlives the call): k_fill_c writes there and nothing but the two counters returns.  Exactly one of the two, unless n_scans is 0.
pvlm_status depth_images(pvlm_ctx* ctx, const char* who, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl, unsigned size,
                         float max_depth, uint16_t* host_out, unsigned short* dev_out, pvlm_depthfill_stats* stats) {
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const size_t npix = (size_t)rows * cols;
  const int limit = batch_images(n_scans, npix * (8 + 8 + 2));
  StageClock clock(stats != nullptr);
  double* d_T = c.upload(T_cl, (size_t)16);
  for (int k0 = 0; k0 < n_scans && !c.st; k0 += limit) {
    const int nb = std::min(limit, n_scans - k0);
    const long long p0 = first_point[k0], np = first_point[k0 + nb] - p0;
    pvlm_call::batch bs(c);                              // this batch's scratch
    Work w(c, npix, cols, nb, host_out != nullptr);
    if (dev_out) w.u16 = dev_out + npix * k0;
    unsigned long long* d_img = c.alloc<unsigned long long>(npix * nb);
    float* d_xyz = c.alloc<float>(3 * (size_t)np);
    unsigned long long counts[2] = {0, 0};
    clock.mark(ctx, 0);
    c.memset(w.counts, 0, 2 * sizeof(unsigned long long));
    c.memset(d_img, 0, npix * nb * sizeof(unsigned long long));
    c.h2d(d_xyz, xyz + 3 * (size_t)p0, 3 * (size_t)np * sizeof(float));
    for (int k = 0; k < nb && !c.st; ++k)                // the splat is pvlm_lines.hip's: it takes the context and reports a status
      c.st = pvlm_depth_launch::splat(ctx, who, rows, cols, first_point[k0 + k + 1] - first_point[k0 + k], d_xyz + 3 * (size_t)(first_point[k0 + k] - p0), d_T, size,
                                      d_img + npix * k);
    clock.mark(ctx, 1);
    run_phases(c, rows, cols, nb, SrcSplat{d_img}, max_depth, w, false, true);
    clock.mark(ctx, 2);
    if (host_out) c.d2h(host_out + npix * k0, w.u16, npix * nb * 2);
    c.d2h(counts, w.counts, sizeof(counts));
    if (!c.sync() && stats) {
      stats->images += nb; stats->batches += 1; stats->valid_in += (long long)counts[0]; stats->valid_out += (long long)counts[1];
      stats->splat_ms += clock.ms(0, 1); stats->fill_ms += clock.ms(1, 2);
    }
  }
  return c.st;
}

// the argument checks of the two entries; *run = 0 when there is nothing to do
pvlm_status depth_images_args(pvlm_ctx* ctx, const char* who, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl, float max_depth,
                              bool have_dst, pvlm_depthfill_stats* stats, int* run) {
  *run = 0;
  if (!ctx) return PVLM_ERR_ARG;
  if (rows <= 0 || cols <= 0 || n_scans < 0 || !T_cl || (n_scans > 0 && (!first_point || !have_dst))) { PVLM_SET_ERR(ctx, "%s: null argument or size", who); return PVLM_ERR_ARG; }
  if (!std::isfinite(max_depth) || !(max_depth > 0.f)) { PVLM_SET_ERR(ctx, "%s: max_depth must be finite and > 0", who); return PVLM_ERR_ARG; }
  if (stats) *stats = pvlm_depthfill_stats{0, 0, 0, 0, 0.0, 0.0};
  if (n_scans == 0) return PVLM_OK;
  if (first_point[0] != 0) { PVLM_SET_ERR(ctx, "%s: first_point must start at 0", who); return PVLM_ERR_ARG; }
  for (int s = 0; s < n_scans; ++s)
    if (first_point[s + 1] < first_point[s]) { PVLM_SET_ERR(ctx, "%s: first_point is not ascending at scan %d", who, s); return PVLM_ERR_ARG; }
  if (first_point[n_scans] > 0 && !xyz) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  *run = 1;
  return PVLM_OK;
}

bool set_usable(pvlm_ctx* ctx, const pvlm_depthset* set, const char* who) {
  if (!set) { PVLM_SET_ERR(ctx, "%s: null set", who); return false; }
  if (set->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the set belongs to another context", who); return false; }
  return true;
}
}  // namespace

extern "C" pvlm_status pvlm_compute_depth_images(pvlm_ctx* ctx, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl,
                                                 unsigned size, float max_depth, uint16_t* depth_u16, pvlm_depthfill_stats* stats) {
  const char* who = "pvlm_compute_depth_images";
  int run = 0;
  const pvlm_status st = depth_images_args(ctx, who, rows, cols, n_scans, first_point, xyz, T_cl, max_depth, depth_u16 != nullptr, stats, &run);
  if (st || !run) return st;
  return depth_images(ctx, who, rows, cols, n_scans, first_point, xyz, T_cl, size, max_depth, depth_u16, nullptr, stats);
}

// ---- pvlm_depthset: the maps stay where k_fill_c writes them ------------------------------------------------------------------------------------
extern "C" pvlm_status pvlm_depthset_create(pvlm_ctx* ctx, int n_frames, pvlm_depthset** out) {
  if (!ctx) return PVLM_ERR_ARG;
  if (n_frames < 0 || !out) { PVLM_SET_ERR(ctx, "pvlm_depthset_create: n_frames or null argument"); return PVLM_ERR_ARG; }
  pvlm_depthset* s = new pvlm_depthset();
  s->owner = ctx; s->n_frames = n_frames;
  s->rows.assign((size_t)n_frames, 0); s->cols.assign((size_t)n_frames, 0); s->d_map.assign((size_t)n_frames, nullptr); s->d_own.assign((size_t)n_frames, nullptr);
  *out = s;
  return PVLM_OK;
}

extern "C" void pvlm_depthset_destroy(pvlm_ctx* ctx, pvlm_depthset* set) {
  if (!ctx || !set || set->owner != ctx) return;
  for (unsigned short* p : set->d_own) pvlm_i_free(ctx, p);
  pvlm_i_free(ctx, set->d_block);
  delete set;
}

extern "C" pvlm_status pvlm_depthset_compute(pvlm_ctx* ctx, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl,
                                             unsigned size, float max_depth, pvlm_depthset** out, pvlm_depthfill_stats* stats) {
  const char* who = "pvlm_depthset_compute";
  int run = 0;
  pvlm_status st = depth_images_args(ctx, who, rows, cols, n_scans, first_point, xyz, T_cl, max_depth, out != nullptr, stats, &run);
  if (st) return st;
  if (!out) { PVLM_SET_ERR(ctx, "%s: null argument or size", who); return PVLM_ERR_ARG; }
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  pvlm_depthset* s = nullptr;
  if ((st = pvlm_depthset_create(ctx, n_scans, &s))) return st;
  if (run) {
    const size_t npix = (size_t)rows * cols;
    st = pvlm_i_alloc(ctx, &s->d_block, npix * (size_t)n_scans);           // the set's own block: it outlives the call, pvlm_depthset_destroy frees it
    if (!st) st = depth_images(ctx, who, rows, cols, n_scans, first_point, xyz, T_cl, size, max_depth, nullptr, s->d_block, stats);
    if (st) { pvlm_depthset_destroy(ctx, s); return st; }
    for (int f = 0; f < n_scans; ++f) { s->rows[(size_t)f] = rows; s->cols[(size_t)f] = cols; s->d_map[(size_t)f] = s->d_block + npix * (size_t)f; }
  }
  *out = s;
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_depthset_upload(pvlm_ctx* ctx, pvlm_depthset* set, int frame, int rows, int cols, const uint16_t* depth_u16) {
  const char* who = "pvlm_depthset_upload";
  if (!ctx) return PVLM_ERR_ARG;
  if (!set_usable(ctx, set, who)) return PVLM_ERR_ARG;
  if (frame < 0 || frame >= set->n_frames || rows <= 0 || cols <= 0 || !depth_u16) { PVLM_SET_ERR(ctx, "%s: frame, size or null argument", who); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const size_t npix = (size_t)rows * cols;
  unsigned short* d = nullptr;
  if ((c.st = pvlm_i_alloc(ctx, &d, npix))) return c.st;                    // the frame's own block: it outlives the call
  c.h2d(d, depth_u16, npix * sizeof(unsigned short));
  if (c.sync()) { pvlm_i_free(ctx, d); return c.st; }
  pvlm_i_free(ctx, set->d_own[(size_t)frame]);                             // a map uploaded before (a map inside d_block stays with the block)
  set->d_own[(size_t)frame] = d; set->d_map[(size_t)frame] = d; set->rows[(size_t)frame] = rows; set->cols[(size_t)frame] = cols;
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_depthset_info(const pvlm_depthset* set, int frame, int* rows, int* cols) {
  if (!set || frame < 0 || frame >= set->n_frames || !rows || !cols) return PVLM_ERR_ARG;
  *rows = set->d_map[(size_t)frame] ? set->rows[(size_t)frame] : 0;
  *cols = set->d_map[(size_t)frame] ? set->cols[(size_t)frame] : 0;
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_depthset_read(pvlm_ctx* ctx, const pvlm_depthset* set, int frame, uint16_t* depth_u16) {
  const char* who = "pvlm_depthset_read";
  if (!ctx) return PVLM_ERR_ARG;
  if (!set_usable(ctx, set, who)) return PVLM_ERR_ARG;
  if (frame < 0 || frame >= set->n_frames || !depth_u16) { PVLM_SET_ERR(ctx, "%s: frame or null argument", who); return PVLM_ERR_ARG; }
  if (!set->d_map[(size_t)frame]) { PVLM_SET_ERR(ctx, "%s: frame %d has no map", who, frame); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  c.d2h(depth_u16, set->d_map[(size_t)frame], (size_t)set->rows[(size_t)frame] * (size_t)set->cols[(size_t)frame] * sizeof(unsigned short));
  return c.sync();
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_depthfill() {}
void pvlm_i_preload_depthfill(hipStream_t s) { hipLaunchKernelGGL(k_preload_depthfill, dim3(1), dim3(1), 0, s); }
