// K41: SIFT keypoints and (Root)SIFT descriptors of a batch of grey images (util/SIFT.cpp:10-128 behind Frame::ExtractKeyPoints / ComputeDescriptor), on the
// definition of pvlm_sift_core.h.
//
// Per image, octave by octave:
//   (a) k_blur<FromU8, TAPS>   the doubled image is formed in the tile loader and blurred in the same kernel: the doubled image never exists in memory
//   (b) k_blur<FromF32, TAPS>  layer i from layer i - 1: a tile of 64 x 32 outputs with its halo in LDS, the row pass into LDS, the column pass out of it; the
//                        difference layer i - 1 is written from the column pass's sum and the tile's own centre value, so no Gaussian layer is read twice
//   (c) k_decimate       every second pixel of layer 3
//   (d) k_detect_count / k_tile_scan / k_detect_scatter: one lane per pixel of the three inner difference layers, tiles of 4096 pixels in (layer, row, column)
//                        order through the ordered compaction of pvlm_compact.h; a lane that finds an extremum refines it itself
//   (e) k_orient         one wave per candidate, a 36-bin histogram per lane in LDS (stride 65, as (f)), summed over the lanes in lane order; k_tile_scan over the peak counts and
//                        k_expand place the keypoints in candidate order, ascending bin
//   the selection        on the host, between (e) and (f): it needs an n-th largest response and a duplicate search over a few tens of thousands of 24-byte
//                        records that come down in one copy; the layers stay on the device meanwhile
//   (f) k_describe       one wave per selected keypoint, 128 bins per lane in LDS (stride 65: conflict-free both ways), RootSIFT in the same kernel
// One image is in flight at a time: its layers (about 4 GB at 5760 x 2880) come from the context's pool and go back to it before the next image.  Open: several
// images at a time, launch sizes from device-side counts instead of two synchronisations per octave, the selection of image i beside the pyramid of image i + 1.
// Every index that reaches memory is folded (reflect101), clamped or tested against the layer's size first.  Vector stores and plain C++ only.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_compact.h"
#include "pvlm_internal.h"
#include "pvlm_sift_core.h"

namespace {

namespace sf = pvlm_sift;
namespace pc = pvlm_compact;

constexpr int kTX = 64, kTY = 32, kIW = kTX + 2 * sf::kMaxRadius, kIH = kTY + 2 * sf::kMaxRadius, kBlurThreads = 256;

struct FromU8 {                                       // the doubled image of an 8-bit one
  const unsigned char* img; int rows, cols;
  __device__ __forceinline__ float operator()(int y, int x) const { return sf::doubled_at(img, rows, cols, y, x); }
};
struct FromF32 {
  const float* img; int cols;
  __device__ __forceinline__ float operator()(int y, int x) const { return img[(size_t)y * cols + x]; }
};

// TAPS is the kernel's size at compile time (the six kernels have 11, 11, 13, 17, 21 and 27 taps): the coefficients are fetched once and both passes unroll; with a
// run-time count every tap waited for its coefficient's scalar load.  The order of the sums is the same.
template <class Src, int TAPS>
__global__ __launch_bounds__(kBlurThreads) void k_blur(Src src, int rows, int cols, sf::Kernel K, float* __restrict__ G, float* __restrict__ D) {
  __shared__ float s_in[kIH * kIW];
  __shared__ float s_tmp[kIH * kTX];
  float cf[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) cf[k] = K.c[k];
  const int r = TAPS / 2, x0 = (int)blockIdx.x * kTX, y0 = (int)blockIdx.y * kTY, tid = (int)threadIdx.x;
  const int iw = kTX + 2 * r, ih = kTY + 2 * r;
  for (int i = tid; i < ih * iw; i += kBlurThreads) {
    const int ly = i / iw, lx = i - ly * iw;
    s_in[ly * kIW + lx] = src(sf::reflect101(y0 - r + ly, rows), sf::reflect101(x0 - r + lx, cols));
  }
  __syncthreads();
  for (int i = tid; i < ih * kTX; i += kBlurThreads) {
    const int ly = i / kTX, tx = i - ly * kTX;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) s = s + cf[k] * s_in[ly * kIW + tx + k];
    s_tmp[ly * kTX + tx] = s;
  }
  __syncthreads();
  for (int i = tid; i < kTY * kTX; i += kBlurThreads) {
    const int ty = i / kTX, tx = i - ty * kTX, y = y0 + ty, x = x0 + tx;
    if (y >= rows || x >= cols) continue;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) s = s + cf[k] * s_tmp[(ty + k) * kTX + tx];
    G[(size_t)y * cols + x] = s;
    if (D) D[(size_t)y * cols + x] = s - s_in[(ty + r) * kIW + tx + r];
  }
}

__global__ __launch_bounds__(256) void k_decimate(const float* __restrict__ up, int ucols, float* __restrict__ dst, int rows, int cols) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  const int y = (int)(i / cols), x = (int)(i - (long long)y * cols);
  dst[i] = up[(size_t)(2 * y) * ucols + 2 * x];
}

// a bin's 64 per-lane values lie 65 floats apart from the next bin's: the lanes' adds (consecutive lanes, one bin each) and the final sums (one bin per lane,
// the same l) both fall on distinct banks
constexpr int kHistStride = sf::kLanes + 1;
struct DogPtrs { const float* d[sf::kDog]; };
struct GaussPtrs { const float* g[sf::kGauss]; };
struct LayerDesc { int tile0, n_tiles; };             // k_tile_scan's item type; no per-item counts are asked for

// the pixel `pix` of detection layer `layer`: an extremum that survives its refinement?
__device__ __forceinline__ bool detect_at(const DogPtrs& P, int rows, int cols, int octave, int layer, int pix, sf::Cand* out) {
  const int y = pix / cols, x = pix - y * cols;
  if (y < sf::kBorder || y >= rows - sf::kBorder || x < sf::kBorder || x >= cols - sf::kBorder) return false;
  if (!sf::is_extremum(P.d, cols, layer, y, x)) return false;
  int moved;
  return sf::refine(P.d, rows, cols, octave, layer, y, x, out, &moved) == sf::kKeep;
}

// tile t of an octave: layer 1 + t / tiles_per_layer, pixels p0 .. p0 + n
__device__ __forceinline__ void tile_of(int t, int tiles_per_layer, int n_pix, int* layer, int* p0, int* n) {
  *layer = 1 + t / tiles_per_layer;
  *p0 = (t % tiles_per_layer) * pc::kTile;
  *n = n_pix - *p0 < pc::kTile ? n_pix - *p0 : pc::kTile;
}

__global__ __launch_bounds__(pc::kThreads) void k_detect_count(DogPtrs P, int rows, int cols, int octave, int tiles_per_layer, int* __restrict__ tile_count) {
  int layer, p0, n;
  tile_of((int)blockIdx.x, tiles_per_layer, rows * cols, &layer, &p0, &n);
  int c = 0;
  for (int r = 0; r < pc::kRounds; ++r) {
    const int j = r * pc::kThreads + (int)threadIdx.x;
    sf::Cand k;
    c += (j < n && detect_at(P, rows, cols, octave, layer, p0 + j, &k)) ? 1 : 0;
  }
  pc::tile_total(c, tile_count);
}

__global__ __launch_bounds__(pc::kThreads) void k_detect_scatter(DogPtrs P, int rows, int cols, int octave, int tiles_per_layer, const long long* __restrict__ tile_base,
                                                                 sf::Cand* __restrict__ out, long long capacity) {
  int layer, p0, n;
  tile_of((int)blockIdx.x, tiles_per_layer, rows * cols, &layer, &p0, &n);
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  __shared__ int pre[pc::kRounds * pc::kWaves];
  static_assert(pc::kRounds == 16, "the ranks of a lane (below 64 each) are packed a byte per round into two words");
  unsigned keep = 0;
  unsigned long long rank_lo = 0, rank_hi = 0;
  for (int r = 0; r < pc::kRounds; ++r) {
    const int j = r * pc::kThreads + (int)threadIdx.x;
    sf::Cand k;
    const bool kept = j < n && detect_at(P, rows, cols, octave, layer, p0 + j, &k);
    const unsigned long long m = __ballot(kept);
    keep |= (kept ? 1u : 0u) << r;
    const unsigned long long rk = (unsigned long long)__popcll(m & below);
    if (r < 8) rank_lo |= rk << (8 * r); else rank_hi |= rk << (8 * (r - 8));
    if (lane == 0) pre[r * pc::kWaves + w] = __popcll(m);
  }
  pc::tile_offsets(pre);
  const long long base = tile_base[blockIdx.x];
  for (int r = 0; r < pc::kRounds; ++r) {
    if (!((keep >> r) & 1u)) continue;
    const int rk = (int)(((r < 8 ? rank_lo >> (8 * r) : rank_hi >> (8 * (r - 8)))) & 255ull);
    const long long at = base + pre[r * pc::kWaves + w] + rk;
    if (at >= capacity) continue;
    sf::Cand k;
    if (detect_at(P, rows, cols, octave, layer, p0 + r * pc::kThreads + (int)threadIdx.x, &k)) out[at] = k;     // the same decision again: the record was not kept in registers
  }
}

__global__ __launch_bounds__(sf::kLanes) void k_orient(const sf::Cand* __restrict__ cands, GaussPtrs P, int rows, int cols, int* __restrict__ cnt, float* __restrict__ angles) {
  __shared__ float part[sf::kOriBins * kHistStride];
  __shared__ float raw[sf::kOriBins];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const sf::Cand k = cands[i];
  const float* G = P.g[sf::clampi(k.layer, 0, sf::kGauss - 1)];
  const sf::OriWindow w = sf::ori_window(k);
  for (int b = 0; b < sf::kOriBins; ++b) part[b * kHistStride + lane] = 0.f;
  for (int j = lane; j < w.count; j += sf::kLanes) {
    int b; float v;
    if (sf::ori_sample(G, rows, cols, w, j, &b, &v)) part[b * kHistStride + lane] = part[b * kHistStride + lane] + v;
  }
  __syncthreads();
  if (lane < sf::kOriBins) {
    float s = 0.f;
    for (int l = 0; l < sf::kLanes; ++l) s = s + part[lane * kHistStride + l];
    raw[lane] = s;
  }
  __syncthreads();
  if (lane == 0) {
    float ang[sf::kMaxPeaks];
    const int n = sf::ori_peaks(raw, ang);
    cnt[i] = n;
    for (int q = 0; q < n; ++q) angles[(size_t)i * sf::kMaxPeaks + q] = ang[q];
  }
}

__global__ __launch_bounds__(256) void k_expand(const sf::Cand* __restrict__ cands, int n, const int* __restrict__ cnt, const float* __restrict__ angles,
                                               const long long* __restrict__ base, sf::Keypoint* __restrict__ out) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const sf::Cand k = cands[i];
  const int m = cnt[i];
  for (int q = 0; q < m && q < sf::kMaxPeaks; ++q) out[base[i] + q] = sf::Keypoint{k.x, k.y, k.size, angles[(size_t)i * sf::kMaxPeaks + q], k.response, k.word};
}

struct LayerRef { const float* g; int rows, cols; };

__global__ __launch_bounds__(sf::kLanes) void k_describe(const sf::Keypoint* __restrict__ kps, const LayerRef* __restrict__ layers, int n_oct, int root, float* __restrict__ out) {
  __shared__ float part[sf::kDescBins * kHistStride];
  __shared__ float hist[sf::kDescBins];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const sf::Keypoint k = kps[i];
  const sf::DescWindow w0 = sf::desc_window(k, 1, 1);
  const LayerRef L = layers[sf::clampi(w0.octave_index, 0, n_oct - 1) * sf::kGauss + sf::clampi(w0.layer, 0, sf::kGauss - 1)];
  const sf::DescWindow w = sf::desc_window(k, L.rows, L.cols);
  for (int b = 0; b < sf::kDescBins; ++b) part[b * kHistStride + lane] = 0.f;
  for (int j = lane; j < w.count; j += sf::kLanes) {
    int b[8]; float v[8];
    const int n = sf::desc_sample(L.g, L.rows, L.cols, w, j, b, v);
    for (int q = 0; q < n; ++q) part[b[q] * kHistStride + lane] = part[b[q] * kHistStride + lane] + v[q];
  }
  __syncthreads();
  for (int b = lane; b < sf::kDescBins; b += sf::kLanes) {
    float s = 0.f;
    for (int l = 0; l < sf::kLanes; ++l) s = s + part[b * kHistStride + l];
    hist[b] = s;
  }
  __syncthreads();
  if (lane == 0) sf::desc_finish(hist, root != 0, out + (size_t)i * sf::kDescBins);
}

struct Octave { float* G[sf::kGauss]; float* D[sf::kDog]; int rows, cols; };

// the blur kernel compiled for the kernel's tap count; false for a count make_kernels does not produce
template <class Src>
bool launch_blur(pvlm_call& c, dim3 grid, Src src, int rows, int cols, const sf::Kernel& K, float* G, float* D) {
  switch (K.taps) {
    case 11: c.launch(k_blur<Src, 11>, grid, dim3(kBlurThreads), 0, src, rows, cols, K, G, D); return true;
    case 13: c.launch(k_blur<Src, 13>, grid, dim3(kBlurThreads), 0, src, rows, cols, K, G, D); return true;
    case 17: c.launch(k_blur<Src, 17>, grid, dim3(kBlurThreads), 0, src, rows, cols, K, G, D); return true;
    case 21: c.launch(k_blur<Src, 21>, grid, dim3(kBlurThreads), 0, src, rows, cols, K, G, D); return true;
    case 27: c.launch(k_blur<Src, 27>, grid, dim3(kBlurThreads), 0, src, rows, cols, K, G, D); return true;
    default: PVLM_SET_ERR(c.ctx, "%s: no blur kernel of %d taps", c.who, K.taps); c.st = PVLM_ERR_STATE; return false;
  }
}

// device time of the parts (a)-(f) by event pairs on the call's stream, only when the caller asked for statistics; read after a synchronisation
struct PartTimer {
  hipStream_t stream; bool on;
  struct Span { int part; hipEvent_t a, b; };
  std::vector<Span> spans;
  PartTimer(hipStream_t s, bool enabled) : stream(s), on(enabled) {}
  ~PartTimer() { for (Span& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); } }
  void begin(int part) {
    if (!on) return;
    Span s{part, nullptr, nullptr};
    if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(s.a, stream);
    spans.push_back(s);
  }
  void end() { if (on && !spans.empty()) (void)hipEventRecord(spans.back().b, stream); }
  void collect(double* ms) {                          // behind a synchronisation of the stream
    for (Span& s : spans) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) ms[s.part] += (double)t;
      (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
    }
    spans.clear();
  }
};

struct Debug {                                        // what pvlm_sift_pyramid_debug asks of one octave
  int octave; float* gauss; float* dog; std::vector<sf::Cand>* cands;
};

// the pyramid of one image and its keypoints before the selection; the Gaussian layers stay allocated in `oct` (the caller's batch scope owns them)
void detect_image(pvlm_call& c, const unsigned char* d_img, int rows, int cols, const sf::Kernel* K, const sf::Sizes& sz, std::vector<Octave>& oct,
                  std::vector<sf::Keypoint>& kps, pvlm_sift_stats* stats, Debug* dbg, PartTimer& pt) {
  oct.assign((size_t)sz.n_oct, Octave{});
  for (int o = 0; o < sz.n_oct && !c.st; ++o) {
    Octave& O = oct[(size_t)o];
    O.rows = sz.rows[o]; O.cols = sz.cols[o];
    const size_t n_pix = (size_t)O.rows * O.cols;
    for (int l = 0; l < sf::kGauss; ++l) O.G[l] = c.alloc<float>(n_pix);
    for (int l = 0; l < sf::kDog; ++l) O.D[l] = c.alloc<float>(n_pix);
    if (c.st) return;
    const dim3 grid((unsigned)((O.cols + kTX - 1) / kTX), (unsigned)((O.rows + kTY - 1) / kTY));
    pt.begin(o == 0 ? 0 : 2);
    if (o == 0) {
      launch_blur(c, grid, FromU8{d_img, rows, cols}, O.rows, O.cols, K[0], O.G[0], (float*)nullptr);
    } else {
      const Octave& U = oct[(size_t)o - 1];
      c.launch(k_decimate, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, (const float*)U.G[sf::kLayers], U.cols, O.G[0], O.rows, O.cols);
    }
    pt.end();
    pt.begin(1);
    for (int l = 1; l < sf::kGauss; ++l)
      launch_blur(c, grid, FromF32{O.G[l - 1], O.cols}, O.rows, O.cols, K[l], O.G[l], O.D[l - 1]);
    pt.end();
    c.check_launches();
    if (dbg && dbg->octave == o) {
      for (int l = 0; l < sf::kGauss && dbg->gauss; ++l) c.d2h(dbg->gauss + (size_t)l * n_pix, O.G[l], n_pix * sizeof(float));
      for (int l = 0; l < sf::kDog && dbg->dog; ++l) c.d2h(dbg->dog + (size_t)l * n_pix, O.D[l], n_pix * sizeof(float));
    }
    if (O.rows <= 2 * sf::kBorder || O.cols <= 2 * sf::kBorder) continue;          // no pixel inside the border
    // (d)
    const int tpl = (int)((n_pix + pc::kTile - 1) / pc::kTile), n_tiles = sf::kLayers * tpl;
    DogPtrs DP; GaussPtrs GP;
    for (int l = 0; l < sf::kDog; ++l) DP.d[l] = O.D[l];
    for (int l = 0; l < sf::kGauss; ++l) GP.g[l] = O.G[l];
    int* d_tcount = c.alloc<int>((size_t)n_tiles);
    long long* d_tbase = c.alloc<long long>((size_t)n_tiles);
    long long* d_total = c.alloc<long long>(2);
    pt.begin(3);
    c.launch(k_detect_count, dim3((unsigned)n_tiles), dim3(pc::kThreads), 0, DP, O.rows, O.cols, o, tpl, d_tcount);
    c.launch(pc::k_tile_scan<LayerDesc>, dim3(1), dim3(pc::kScanThreads), 0, (const int*)d_tcount, n_tiles, d_tbase, (const LayerDesc*)nullptr, 0, d_total, (long long*)nullptr);
    pt.end();
    c.check_launches();
    long long n_cand = 0;
    c.d2h(&n_cand, d_total, sizeof(long long));
    if (c.sync()) return;
    if (n_cand > 0x7fffffffll / sf::kMaxPeaks) { PVLM_SET_ERR(c.ctx, "%s: too many candidates in one octave", c.who); c.st = PVLM_ERR_ARG; return; }
    if (stats) stats->candidates += n_cand;
    if (n_cand == 0) continue;
    sf::Cand* d_cand = c.alloc<sf::Cand>((size_t)n_cand);
    pt.begin(3);
    c.launch(k_detect_scatter, dim3((unsigned)n_tiles), dim3(pc::kThreads), 0, DP, O.rows, O.cols, o, tpl, (const long long*)d_tbase, d_cand, n_cand);
    pt.end();
    // (e)
    int* d_cnt = c.alloc<int>((size_t)n_cand);
    float* d_ang = c.alloc<float>((size_t)n_cand * sf::kMaxPeaks);
    long long* d_kbase = c.alloc<long long>((size_t)n_cand);
    pt.begin(4);
    c.launch(k_orient, dim3((unsigned)n_cand), dim3(sf::kLanes), 0, (const sf::Cand*)d_cand, GP, O.rows, O.cols, d_cnt, d_ang);
    c.launch(pc::k_tile_scan<LayerDesc>, dim3(1), dim3(pc::kScanThreads), 0, (const int*)d_cnt, (int)n_cand, d_kbase, (const LayerDesc*)nullptr, 0, d_total + 1, (long long*)nullptr);
    pt.end();
    c.check_launches();
    long long n_kp = 0;
    c.d2h(&n_kp, d_total + 1, sizeof(long long));
    if (dbg && dbg->octave == o && dbg->cands) { dbg->cands->resize((size_t)n_cand); c.d2h(dbg->cands->data(), d_cand, (size_t)n_cand * sizeof(sf::Cand)); }
    if (c.sync()) return;
    if (n_kp == 0) continue;
    sf::Keypoint* d_kp = c.alloc<sf::Keypoint>((size_t)n_kp);
    pt.begin(4);
    c.launch(k_expand, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, (const sf::Cand*)d_cand, (int)n_cand, (const int*)d_cnt, (const float*)d_ang, (const long long*)d_kbase, d_kp);
    pt.end();
    c.check_launches();
    const size_t at = kps.size();
    kps.resize(at + (size_t)n_kp);
    c.d2h(kps.data() + at, d_kp, (size_t)n_kp * sizeof(sf::Keypoint));
    if (c.sync()) return;
  }
}

pvlm_status check_image_args(pvlm_ctx* ctx, const char* who, int rows, int cols) {
  if (rows < sf::kMinSide || cols < sf::kMinSide) { PVLM_SET_ERR(ctx, "%s: an image side below %d pixels", who, sf::kMinSide); return PVLM_ERR_ARG; }
  if ((long long)rows * cols > (1ll << 27)) { PVLM_SET_ERR(ctx, "%s: more than 2^27 pixels in one image", who); return PVLM_ERR_ARG; }
  return PVLM_OK;
}

}  // namespace

static_assert(sizeof(pvlm_sift_keypoint) == sizeof(pvlm_sift::Keypoint) && sizeof(pvlm_sift_keypoint) == 24, "the keypoint record");
static_assert(sizeof(pvlm_sift_candidate) == sizeof(pvlm_sift::Cand), "the candidate record");

extern "C" pvlm_status pvlm_sift_extract(pvlm_ctx* ctx, int n_images, int rows, int cols, const unsigned char* const* images, const unsigned char* mask, int nfeatures,
                                         unsigned flags, long long* kp_offsets, pvlm_sift_keypoint* keypoints, float* descriptors, long long capacity,
                                         long long* needed, pvlm_sift_stats* stats) {
  const char* who = "pvlm_sift_extract";
  if (!ctx) return PVLM_ERR_ARG;
  if (n_images < 0 || !kp_offsets || !needed || capacity < 0 || (n_images > 0 && !images) || (capacity > 0 && !keypoints)) {
    PVLM_SET_ERR(ctx, "%s: null argument or negative count", who); return PVLM_ERR_ARG;
  }
  if (nfeatures <= 0) { PVLM_SET_ERR(ctx, "%s: nfeatures must be positive", who); return PVLM_ERR_ARG; }
  if (flags & ~PVLM_FLAG_SIFT_ROOT) { PVLM_SET_ERR(ctx, "%s: unknown flag", who); return PVLM_ERR_ARG; }
  if (const pvlm_status s = check_image_args(ctx, who, rows, cols)) return s;
  for (int i = 0; i < n_images; ++i) if (!images[i]) { PVLM_SET_ERR(ctx, "%s: image %d is null", who, i); return PVLM_ERR_ARG; }
  if (stats) *stats = pvlm_sift_stats{0, 0, 0, 0, 0, {0, 0, 0, 0, 0, 0}};
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  sf::Kernel K[sf::kGauss];
  sf::make_kernels(K);
  const sf::Sizes sz = sf::octave_sizes(rows, cols);
  const size_t n_pix = (size_t)rows * cols;
  long long total = 0;
  kp_offsets[0] = 0;
  std::vector<Octave> oct;
  std::vector<sf::Keypoint> kps;
  std::vector<LayerRef> refs((size_t)sz.n_oct * sf::kGauss);
  for (int i = 0; i < n_images; ++i) {
    pvlm_call::batch bs(c);                                  // this image's layers
    const unsigned char* d_img = c.upload(images[i], n_pix);
    kps.clear();
    PartTimer pt(ctx->stream, stats != nullptr);
    detect_image(c, d_img, rows, cols, K, sz, oct, kps, stats, nullptr, pt);
    if (c.st) return c.st;
    if (stats) { stats->images += 1; stats->octaves += sz.n_oct; stats->keypoints_detected += (long long)kps.size(); }
    sf::select(kps, nfeatures, rows, cols, mask);
    const long long m = (long long)kps.size();
    const long long fit = total >= capacity ? 0 : (capacity - total < m ? capacity - total : m);
    if (fit > 0 && descriptors) {                            // descriptors == NULL: the detection alone
      for (int o = 0; o < sz.n_oct; ++o)
        for (int l = 0; l < sf::kGauss; ++l) refs[(size_t)o * sf::kGauss + l] = LayerRef{oct[(size_t)o].G[l], oct[(size_t)o].rows, oct[(size_t)o].cols};
      const LayerRef* d_refs = c.upload(refs.data(), refs.size());
      const sf::Keypoint* d_kp = c.upload(kps.data(), (size_t)fit);
      float* d_desc = c.alloc<float>((size_t)fit * sf::kDescBins);
      pt.begin(5);
      c.launch(k_describe, dim3((unsigned)fit), dim3(sf::kLanes), 0, d_kp, d_refs, sz.n_oct, (flags & PVLM_FLAG_SIFT_ROOT) ? 1 : 0, d_desc);
      pt.end();
      c.check_launches();
      c.d2h(descriptors + (size_t)total * sf::kDescBins, d_desc, (size_t)fit * sf::kDescBins * sizeof(float));
    }
    if (fit > 0) std::memcpy(keypoints + total, kps.data(), (size_t)fit * sizeof(sf::Keypoint));
    if (c.sync()) return c.st;
    if (stats) pt.collect(stats->part_ms);
    total += m;
    kp_offsets[i + 1] = total;
    if (stats) stats->keypoints += m;
  }
  *needed = total;
  if (total > capacity) { PVLM_SET_ERR(ctx, "%s: %lld keypoints, capacity %lld", who, total, capacity); return PVLM_ERR_CAPACITY; }
  return c.st;
}

extern "C" pvlm_status pvlm_sift_pyramid_debug(pvlm_ctx* ctx, int rows, int cols, const unsigned char* image, int octave, int* n_octaves, int* octave_rows,
                                               int* octave_cols, float* gauss, float* dog, pvlm_sift_candidate* candidates, long long candidate_capacity,
                                               long long* candidates_needed, pvlm_sift_keypoint* keypoints, long long keypoint_capacity, long long* keypoints_needed) {
  const char* who = "pvlm_sift_pyramid_debug";
  if (!ctx) return PVLM_ERR_ARG;
  if (!image || !n_octaves || !octave_rows || !octave_cols || !candidates_needed || !keypoints_needed || candidate_capacity < 0 || keypoint_capacity < 0 ||
      (candidate_capacity > 0 && !candidates) || (keypoint_capacity > 0 && !keypoints)) {
    PVLM_SET_ERR(ctx, "%s: null argument or negative capacity", who); return PVLM_ERR_ARG;
  }
  if (const pvlm_status s = check_image_args(ctx, who, rows, cols)) return s;
  const sf::Sizes sz = sf::octave_sizes(rows, cols);
  *n_octaves = sz.n_oct;
  if (octave < 0 || octave >= sz.n_oct) { PVLM_SET_ERR(ctx, "%s: octave %d of %d", who, octave, sz.n_oct); return PVLM_ERR_ARG; }
  *octave_rows = sz.rows[octave]; *octave_cols = sz.cols[octave];
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  sf::Kernel K[sf::kGauss];
  sf::make_kernels(K);
  std::vector<Octave> oct;
  std::vector<sf::Keypoint> kps;
  std::vector<sf::Cand> cands;
  Debug dbg{octave, gauss, dog, &cands};
  PartTimer pt(ctx->stream, false);
  const unsigned char* d_img = c.upload(image, (size_t)rows * cols);
  detect_image(c, d_img, rows, cols, K, sz, oct, kps, nullptr, &dbg, pt);
  if (c.sync()) return c.st;
  *candidates_needed = (long long)cands.size(); *keypoints_needed = (long long)kps.size();
  const size_t nc = (size_t)std::min<long long>(candidate_capacity, (long long)cands.size()), nk = (size_t)std::min<long long>(keypoint_capacity, (long long)kps.size());
  if (nc) std::memcpy(candidates, cands.data(), nc * sizeof(sf::Cand));
  if (nk) std::memcpy(keypoints, kps.data(), nk * sizeof(sf::Keypoint));
  if (*candidates_needed > candidate_capacity || *keypoints_needed > keypoint_capacity) { PVLM_SET_ERR(ctx, "%s: capacity", who); return PVLM_ERR_CAPACITY; }
  return c.st;
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_sift() {}
void pvlm_i_preload_sift(hipStream_t s) { hipLaunchKernelGGL(k_preload_sift, dim3(1), dim3(1), 0, s); }
