// K30: the colour stage of Texture::ColorizeLidarPointCloud (mvs/Texture.cpp:14-80) for many (scan, frame) pairs — range test, transform to the camera,
// CamToImage, the pixel, OpenCV's 8-bit HSV sky test and the record PointXYZRGB{x, y, z of the LiDAR-frame point, bgr} (per-point statement:
// pvlm_texture_core.h).  Kept points in pair order, then point order, as 16-byte records (x, y, z, colour word).
// The order-preserving compaction is pvlm_compact.h's: a tile of 4096 points (tiles never span two pairs) writes the colour word of each point (0 = dropped)
// and its count, one workgroup scans the counts into 64-bit tile bases (pvlm_compact::k_tile_scan<PairDesc>), and each tile writes its kept points at
// base + rank (k_tex_scatter).
// Device clouds and images (pvlm_colorize_scans_dev): k_tex_word_dev does the whole statement, the gather from the device image included.
// Host clouds and images (pvlm_colorize_scans): the images never cross the link.  Per piece of whole pairs: the clouds go up, K30a (k_tex_project) turns every
// point into the byte offset of its pixel or -1 (the double-precision trigonometry), the offsets come down, host workers gather the BGR of those pixels,
// the gathered words go up and K30b (k_tex_word_host, then the scan and the scatter) applies the HSV test and writes the records.  The next piece's upload
// and projection run while the host gathers this one's pixels.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_workers.h"
#include "pvlm_compact.h"
#include "pvlm_texture_core.h"

namespace {

using namespace pvlm_compact;          // kThreads, kRounds, kTile, kWaves, kScanThreads, kPiecePoints
constexpr int kPiecePairs = 16384;
constexpr unsigned kHit = 1u << 24;                  // host path: the gathered word of a point that reached the image (b | g << 8 | r << 16 | kHit)

struct PairDesc {
  double T[12];                  // camera <- LiDAR, rows 0..2
  const float* xyz;
  const unsigned char* bgr;      // device image (device path only)
  long long row_bytes;
  int stride, vec;               // vec: xyz 16-B aligned with a stride of whole float4s (one float4 load per point)
  int rows, cols;
  int tile0, n_tiles;
};
struct TileDesc {                                          // first point inside the pair, points (<= kTile), pair, first point in the launch's arrays
  int p0, n, pair, pad; long long g0;
  static TileDesc make(int p0, int n, int pair, long long g0) { return TileDesc{p0, n, pair, 0, g0}; }
};

__device__ __forceinline__ float3 load_xyz(const PairDesc& d, int i) {
  const size_t o = (size_t)i * (size_t)d.stride;
  if (d.vec) { const float4 p = *(const float4*)(d.xyz + o); return make_float3(p.x, p.y, p.z); }
  return make_float3(d.xyz[o], d.xyz[o + 1], d.xyz[o + 2]);
}

// K30a: the byte offset of every point's pixel in its image, -1 when the point is dropped before the image test
__global__ __launch_bounds__(kThreads) void k_tex_project(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, double sq_min, double sq_max,
                                                          int* __restrict__ offset) {
  const TileDesc td = tiles[blockIdx.x];
  const PairDesc& d = pairs[td.pair];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = d.T[k];
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    if (j >= td.n) break;
    const float3 p = load_xyz(d, td.p0 + j);
    int px, py;
    const bool hit = pvlm_texture::project(T, d.rows, d.cols, p.x, p.y, p.z, sq_min, sq_max, &px, &py);
    offset[td.g0 + j] = hit ? (int)((long long)py * d.row_bytes + 3ll * px) : -1;
  }
}

// K30b, first pass: the HSV test on the gathered pixels -> colour words (0 = dropped) and the tile's count
__global__ __launch_bounds__(kThreads) void k_tex_word_host(const TileDesc* __restrict__ tiles, const unsigned* __restrict__ gathered, unsigned* __restrict__ word,
                                                            int* __restrict__ tile_count) {
  const TileDesc td = tiles[blockIdx.x];
  int c = 0;
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    if (j >= td.n) break;
    const unsigned g = gathered[td.g0 + j];
    const unsigned w = (g & kHit) ? pvlm_texture::colour_word((int)(g & 255u), (int)((g >> 8) & 255u), (int)((g >> 16) & 255u)) : 0u;
    word[td.g0 + j] = w;
    c += w != 0u;
  }
  tile_total(c, tile_count);
}

// the whole statement on device clouds and images -> colour words and the tile's count
__global__ __launch_bounds__(kThreads) void k_tex_word_dev(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, double sq_min, double sq_max,
                                                           unsigned* __restrict__ word, int* __restrict__ tile_count) {
  const TileDesc td = tiles[blockIdx.x];
  const PairDesc& d = pairs[td.pair];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = d.T[k];
  int c = 0;
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    if (j >= td.n) break;
    const float3 p = load_xyz(d, td.p0 + j);
    int px, py;
    unsigned w = 0u;
    if (pvlm_texture::project(T, d.rows, d.cols, p.x, p.y, p.z, sq_min, sq_max, &px, &py)) {
      const unsigned char* q = d.bgr + (size_t)py * (size_t)d.row_bytes + 3 * (size_t)px;
      w = pvlm_texture::colour_word(q[0], q[1], q[2]);
    }
    word[td.g0 + j] = w;
    c += w != 0u;
  }
  tile_total(c, tile_count);
}

// second pass: the kept points of the tile at base + rank, as float4 (x, y, z, bits of the colour word)
__global__ __launch_bounds__(kThreads) void k_tex_scatter(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, const unsigned* __restrict__ word,
                                                          const long long* __restrict__ tile_base, float4* __restrict__ out, long long capacity) {
  const TileDesc td = tiles[blockIdx.x];
  const PairDesc& d = pairs[td.pair];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  __shared__ int pre[kRounds * kWaves];
  unsigned wd[kRounds];
  int rank[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    wd[r] = j < td.n ? word[td.g0 + j] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const unsigned long long m = __ballot(wd[r] != 0u);
    rank[r] = __popcll(m & below);
    if (lane == 0) pre[r * kWaves + w] = __popcll(m);
  }
  tile_offsets(pre);
  const long long base = tile_base[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!wd[r]) continue;
    const long long at = base + pre[r * kWaves + w] + rank[r];
    if (at >= capacity) continue;
    const float3 p = load_xyz(d, td.p0 + r * kThreads + (int)threadIdx.x);
    out[at] = make_float4(p.x, p.y, p.z, __uint_as_float(wd[r]));
  }
}

__global__ void k_tex_debug_hsv(long long n, const unsigned char* __restrict__ bgr, unsigned char* __restrict__ hsv) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int h, s, v;
  pvlm_texture::bgr2hsv_u8(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], &h, &s, &v);
  hsv[3 * i] = (unsigned char)h; hsv[3 * i + 1] = (unsigned char)s; hsv[3 * i + 2] = (unsigned char)v;
}

void fill_desc(PairDesc& pd, const pvlm_colorize_pair& s, const float* xyz, int stride) {
  std::memset(&pd, 0, sizeof(PairDesc));
  if (s.n <= 0) return;                                  // no tiles read it (its pose and image may be absent)
  for (int k = 0; k < 12; ++k) pd.T[k] = s.T_cl[k];
  pd.xyz = xyz; pd.stride = stride;
  pd.vec = (stride % 4 == 0 && ((uintptr_t)xyz & 15) == 0) ? 1 : 0;
  pd.bgr = s.bgr; pd.row_bytes = s.row_bytes; pd.rows = s.rows; pd.cols = s.cols;
}

pvlm_status check_pairs(pvlm_ctx* ctx, const char* what, int n_pairs, const pvlm_colorize_pair* pairs, long long* total) {
  if (n_pairs < 0 || (n_pairs > 0 && !pairs)) { PVLM_SET_ERR(ctx, "%s: bad pair list", what); return PVLM_ERR_ARG; }
  *total = 0;
  for (int s = 0; s < n_pairs; ++s) {
    const pvlm_colorize_pair& d = pairs[s];
    if (d.n < 0 || (d.n > 0 && (!d.xyz || !d.T_cl || d.stride_floats < 3 || !d.bgr || d.rows < 0 || d.cols < 0 ||
                                d.row_bytes < 3ll * d.cols || (long long)d.rows * d.row_bytes > (long long)INT32_MAX))) {
      PVLM_SET_ERR(ctx, "%s: bad descriptor (pair %d: a cloud, T_cl, stride >= 3, a BGR8 image with row_bytes >= 3 cols and < 2 GB)", what, s);
      return PVLM_ERR_ARG;
    }
    *total += d.n;
  }
  return PVLM_OK;
}

// scan + scatter of the words of one launch set
pvlm_status compact(pvlm_ctx* ctx, hipStream_t S, const PairDesc* d_pd, int n_pairs, const TileDesc* d_td, int n_tiles, const unsigned* d_word, int* d_tcount,
                    long long* d_tbase, float4* d_out, long long capacity, long long* d_total, long long* d_per_pair) {
  hipLaunchKernelGGL(k_tile_scan<PairDesc>, dim3(1), dim3(kScanThreads), 0, S, (const int*)d_tcount, n_tiles, d_tbase, d_pd, n_pairs, d_total, d_per_pair);
  PVLM_HIP(ctx, hipGetLastError());
  if (n_tiles > 0) hipLaunchKernelGGL(k_tex_scatter, dim3((unsigned)n_tiles), dim3(kThreads), 0, S, d_pd, d_td, d_word, (const long long*)d_tbase, d_out, capacity);
  PVLM_HIP(ctx, hipGetLastError());
  return PVLM_OK;
}

// PVLM_COLORIZE_PROFILE=1: the host gather's wall and thread milliseconds of every pvlm_colorize_scans call on stderr (tools/colorize_bench.py)
bool profile_on() { static const bool on = [] { const char* v = std::getenv("PVLM_COLORIZE_PROFILE"); return v && v[0] == '1'; }(); return on; }
inline double ms_since(std::chrono::steady_clock::time_point t0) { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

extern "C" pvlm_status pvlm_colorize_scans(pvlm_ctx* ctx, int n_pairs, const pvlm_colorize_pair* pairs, double min_dist, double max_dist, float* out_records,
                                           long long capacity, long long* n_out, long long* per_pair_or_null) {
  if (!ctx) return PVLM_ERR_ARG;
  if (!n_out || capacity < 0 || (capacity > 0 && !out_records)) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans: n_out, capacity >= 0 and an output buffer are required"); return PVLM_ERR_ARG; }
  long long total = 0;
  if (pvlm_status st = check_pairs(ctx, "pvlm_colorize_scans", n_pairs, pairs, &total)) return st;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (ctx->capturing) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans inside a graph capture"); return PVLM_ERR_STATE; }
  *n_out = 0;
  if (per_pair_or_null) std::memset(per_pair_or_null, 0, sizeof(long long) * (size_t)n_pairs);
  if (total == 0) return PVLM_OK;
  const double sq_min = min_dist * min_dist, sq_max = max_dist * max_dist;
  try {
    // pieces of whole pairs: at most P points (a larger pair is a piece of its own) and kPiecePairs pairs
    const std::vector<int> n = point_counts(pairs, n_pairs);
    const Pieces pc = make_pieces(n.data(), n_pairs, kPiecePairs);
    const std::vector<int>& piece0 = pc.piece0;
    const std::vector<long long>& pt0 = pc.pt0;
    const int n_pieces = pc.count();
    const long long P = pc.P;
    const size_t pts_b = align256((size_t)P * 16), w_b = align256((size_t)P * 4), cnt_b = align256((size_t)(pc.scap + 1) * 8),
                 pd_b = align256((size_t)pc.scap * sizeof(PairDesc)), td_b = align256((size_t)pc.tcap * sizeof(TileDesc));
    // pinned window (the context's pool, as K29): per parity in | offsets | gathered | out | counts | descriptors
    const size_t hset_b = 2 * pts_b + 2 * w_b + cnt_b + pd_b + td_b;
    pvlm_pinned_lease lease(ctx, 2 * hset_b);
    char* h = lease.p;
    if (!h) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans: %zu bytes of pinned memory unavailable", 2 * hset_b); return PVLM_ERR_NOMEM; }
    struct Host { float4* in; int* off; unsigned* gath; float4* out; long long* cnt; char* desc; } H[2];
    for (int k = 0; k < 2; ++k) {
      char* b = h + k * hset_b;
      H[k].in = (float4*)b; H[k].out = (float4*)(b + pts_b); H[k].off = (int*)(b + 2 * pts_b); H[k].gath = (unsigned*)(b + 2 * pts_b + w_b);
      H[k].cnt = (long long*)(b + 2 * pts_b + 2 * w_b); H[k].desc = b + 2 * pts_b + 2 * w_b + cnt_b;
    }
    // device: the same per parity (offsets reused for the words), plus the tile counts and bases
    const size_t tc_b = align256((size_t)pc.tcap * 4), tb_b = align256((size_t)pc.tcap * 8);
    const size_t dset_b = 2 * pts_b + 2 * w_b + cnt_b + pd_b + td_b + tc_b + tb_b;
    char* dev = nullptr;
    if (pvlm_status st = pvlm_i_alloc_bytes(ctx, (void**)&dev, 2 * dset_b)) return st;
    struct Dev { float4* in; float4* out; int* off; unsigned* gath; long long* cnt; PairDesc* pd; TileDesc* td; int* tcount; long long* tbase; } D[2];
    for (int k = 0; k < 2; ++k) {
      char* b = dev + k * dset_b;
      D[k].in = (float4*)b; D[k].out = (float4*)(b + pts_b); D[k].off = (int*)(b + 2 * pts_b); D[k].gath = (unsigned*)(b + 2 * pts_b + w_b);
      D[k].cnt = (long long*)(b + 2 * pts_b + 2 * w_b); D[k].pd = (PairDesc*)(b + 2 * pts_b + 2 * w_b + cnt_b);
      D[k].td = (TileDesc*)(b + 2 * pts_b + 2 * w_b + cnt_b + pd_b); D[k].tcount = (int*)(b + 2 * pts_b + 2 * w_b + cnt_b + pd_b + td_b);
      D[k].tbase = (long long*)(b + 2 * pts_b + 2 * w_b + cnt_b + pd_b + td_b + tc_b);
    }
    hipStream_t S = ctx->stream;
    // events: [0..1] offsets of a piece down, [2..3] counts down, [4..5] records down
    hipEvent_t ev[6] = {};
    // on every way out, an exception included: nothing may still read or write the pinned window or the device sets when they go back
    struct Guard {
      pvlm_ctx* c; hipStream_t s; hipEvent_t* ev; char* dev;
      ~Guard() { (void)hipStreamSynchronize(s); for (int k = 0; k < 6; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]); pvlm_i_free(c, dev); }
    } guard{ctx, S, ev, dev};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    const size_t n_threads_max = pvlm_i_threads_max();
    std::vector<TileDesc> tiles;
    int n_tiles[2] = {0, 0};
    // host side of piece q: its clouds packed as float4 into H[q & 1].in, descriptors pointing into the device set
    auto pack = [&](int q) {
      const int par = q & 1, s0 = piece0[q], s1 = piece0[q + 1];
      const long long base = pt0[(size_t)s0];
      PairDesc* pd = (PairDesc*)H[par].desc;
      for (int s = s0; s < s1; ++s) fill_desc(pd[s - s0], pairs[s], (const float*)(D[par].in + (pt0[(size_t)s] - base)), 4);
      make_tiles(n.data() + s0, s1 - s0, pd, tiles);
      n_tiles[par] = (int)tiles.size();
      std::memcpy(H[par].desc + pd_b, tiles.data(), tiles.size() * sizeof(TileDesc));
      std::atomic<int> next{s0};
      pvlm_run_workers(std::max<size_t>(1, std::min<size_t>(n_threads_max, (size_t)(s1 - s0) / 4 + 1)), [&]() {
        for (int s = next++; s < s1; s = next++) {
          const pvlm_colorize_pair& d = pairs[s];
          float4* dst = H[par].in + (pt0[(size_t)s] - base);
          if (d.stride_floats == 4) std::memcpy(dst, d.xyz, (size_t)d.n * 16);
          else for (int i = 0; i < d.n; ++i) { const float* p = d.xyz + (size_t)i * d.stride_floats; dst[i] = make_float4(p[0], p[1], p[2], 0.f); }
        }
      });
    };
    // piece q up, K30a, the offsets down (all on S: behind the previous piece's second half, which last used this parity's device set)
    auto project = [&](int q) -> hipError_t {
      const int par = q & 1, ns = pc.items(q);
      const size_t pts = pc.points(q);
      hipError_t r = hipMemcpyAsync(D[par].in, H[par].in, pts * 16, hipMemcpyHostToDevice, S);
      if (r == hipSuccess) r = hipMemcpyAsync(D[par].pd, H[par].desc, (size_t)ns * sizeof(PairDesc), hipMemcpyHostToDevice, S);
      if (r == hipSuccess && n_tiles[par]) r = hipMemcpyAsync(D[par].td, H[par].desc + pd_b, (size_t)n_tiles[par] * sizeof(TileDesc), hipMemcpyHostToDevice, S);
      if (r == hipSuccess && n_tiles[par]) {
        hipLaunchKernelGGL(k_tex_project, dim3((unsigned)n_tiles[par]), dim3(kThreads), 0, S, (const PairDesc*)D[par].pd, (const TileDesc*)D[par].td, sq_min, sq_max, D[par].off);
        r = hipGetLastError();
      }
      if (r == hipSuccess) r = hipMemcpyAsync(H[par].off, D[par].off, pts * 4, hipMemcpyDeviceToHost, S);
      if (r == hipSuccess) r = hipEventRecord(ev[par], S);
      return r;
    };
    double gather_wall_ms = 0, gather_thread_ms = 0;
    const auto call_t0 = std::chrono::steady_clock::now();
    // the BGR of every indexed pixel, read where the caller's image lies
    auto gather = [&](int q) {
      const int par = q & 1, s0 = piece0[q], s1 = piece0[q + 1];
      const long long base = pt0[(size_t)s0];
      constexpr int kChunk = 1 << 14;
      struct Item { int s, i0; };
      std::vector<Item> items;
      for (int s = s0; s < s1; ++s) for (int i0 = 0; i0 < pairs[s].n; i0 += kChunk) items.push_back(Item{s, i0});
      std::atomic<size_t> next{0};
      const auto w0 = std::chrono::steady_clock::now();
      std::atomic<long long> thread_us{0};
      pvlm_run_workers(std::max<size_t>(1, std::min(n_threads_max, items.size())), [&]() {
        const auto t0 = std::chrono::steady_clock::now();
        struct Busy { std::atomic<long long>& acc; std::chrono::steady_clock::time_point t0; ~Busy() { acc += (long long)(1e3 * ms_since(t0)); } } busy{thread_us, t0};
        for (size_t k = next++; k < items.size(); k = next++) {
          const Item it = items[k];
          const unsigned char* img = pairs[it.s].bgr;
          const size_t o = (size_t)(pt0[(size_t)it.s] - base);
          const int i1 = std::min(pairs[it.s].n, it.i0 + kChunk);
          for (int i = it.i0; i < i1; ++i) {
            const int off = H[par].off[o + i];
            unsigned g = 0u;
            if (off >= 0) { const unsigned char* p = img + off; g = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | kHit; }
            H[par].gath[o + i] = g;
          }
        }
      });
      gather_wall_ms += ms_since(w0); gather_thread_ms += 1e-3 * (double)thread_us.load();
    };
    pvlm_status st = PVLM_OK;
    long long kept = 0;
    bool overflow = false;
    if (e == hipSuccess) { pack(0); e = project(0); }
    for (int q = 0; q < n_pieces && e == hipSuccess && st == PVLM_OK; ++q) {
      const int par = q & 1, s0 = piece0[q], ns = pc.items(q);
      const size_t pts = pc.points(q);
      // the next piece goes up and is projected while this one's pixels are gathered
      if (q + 1 < n_pieces) { pack(q + 1); e = project(q + 1); }
      if (e == hipSuccess) e = hipEventSynchronize(ev[par]);
      if (e != hipSuccess) break;
      gather(q);
      e = hipMemcpyAsync(D[par].gath, H[par].gath, pts * 4, hipMemcpyHostToDevice, S);
      if (e == hipSuccess && n_tiles[par]) {
        unsigned* d_word = (unsigned*)D[par].off;           // the offsets have come down: their buffer holds the words
        hipLaunchKernelGGL(k_tex_word_host, dim3((unsigned)n_tiles[par]), dim3(kThreads), 0, S, (const TileDesc*)D[par].td, (const unsigned*)D[par].gath, d_word, D[par].tcount);
        e = hipGetLastError();
      }
      if (e == hipSuccess) st = compact(ctx, S, D[par].pd, ns, D[par].td, n_tiles[par], (const unsigned*)D[par].off, D[par].tcount, D[par].tbase, D[par].out, P,
                                        D[par].cnt, D[par].cnt + 1);
      if (st) break;
      if (e == hipSuccess) e = hipMemcpyAsync(H[par].cnt, D[par].cnt, (size_t)(ns + 1) * 8, hipMemcpyDeviceToHost, S);
      if (e == hipSuccess) e = hipEventRecord(ev[2 + par], S);
      if (e == hipSuccess) e = hipEventSynchronize(ev[2 + par]);
      if (e != hipSuccess) break;
      const long long m = H[par].cnt[0];
      if (per_pair_or_null) std::memcpy(per_pair_or_null + s0, H[par].cnt + 1, (size_t)ns * 8);
      if (!overflow && kept + m > capacity) overflow = true;
      if (!overflow && m > 0) {
        e = hipMemcpyAsync(H[par].out, D[par].out, (size_t)m * 16, hipMemcpyDeviceToHost, S);
        if (e == hipSuccess) e = hipEventRecord(ev[4 + par], S);
        if (e == hipSuccess) e = hipEventSynchronize(ev[4 + par]);
        if (e == hipSuccess) unpack_records(out_records, H[par].out, kept, m, n_threads_max);
      }
      kept += m;
    }
    if (st) return st;
    if (e != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans: %s", hipGetErrorString(e)); return PVLM_ERR_HIP; }
    *n_out = kept;
    if (profile_on())
      fprintf(stderr, "colorize_profile pieces %d points %lld kept %lld call_ms %.3f gather_wall_ms %.3f gather_thread_ms %.3f\n", n_pieces, total, kept,
              ms_since(call_t0), gather_wall_ms, gather_thread_ms);
    if (kept > capacity) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans: %lld points kept, capacity %lld", kept, capacity); return PVLM_ERR_ARG; }
    return PVLM_OK;
  } catch (const std::bad_alloc&) {
    PVLM_SET_ERR(ctx, "pvlm_colorize_scans: out of host memory");
    return PVLM_ERR_NOMEM;
  }
}

extern "C" pvlm_status pvlm_colorize_scans_dev(pvlm_ctx* ctx, int n_pairs, const pvlm_colorize_pair* device_pairs, double min_dist, double max_dist, float* d_out,
                                               long long capacity, long long* d_n_out, long long* d_per_pair_or_null) {
  if (!ctx) return PVLM_ERR_ARG;
  if (!d_n_out || capacity < 0 || (capacity > 0 && !d_out) || ((uintptr_t)d_out & 15)) {
    PVLM_SET_ERR(ctx, "pvlm_colorize_scans_dev: d_n_out, capacity >= 0 and a 16-byte aligned d_out (float4 stores) are required");
    return PVLM_ERR_ARG;
  }
  long long total = 0;
  if (pvlm_status st = check_pairs(ctx, "pvlm_colorize_scans_dev", n_pairs, device_pairs, &total)) return st;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (ctx->capturing) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans_dev inside a graph capture"); return PVLM_ERR_STATE; }
  try {
    std::vector<PairDesc> pd((size_t)std::max(n_pairs, 1));
    for (int s = 0; s < n_pairs; ++s) fill_desc(pd[(size_t)s], device_pairs[s], device_pairs[s].xyz, device_pairs[s].stride_floats);
    std::vector<TileDesc> tiles;
    make_tiles(point_counts(device_pairs, n_pairs).data(), n_pairs, pd.data(), tiles);
    if (tiles.size() >= (size_t)INT32_MAX) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans_dev: batch too large (split it)"); return PVLM_ERR_ARG; }
    const int n_tiles = (int)tiles.size();
    PairDesc* d_pd = nullptr; TileDesc* d_td = nullptr; unsigned* d_word = nullptr; int* d_tcount = nullptr; long long* d_tbase = nullptr;
    pvlm_status st = pvlm_i_alloc(ctx, &d_pd, (size_t)std::max(n_pairs, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_td, (size_t)std::max(n_tiles, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_word, (size_t)std::max(total, 1ll));
    if (!st) st = pvlm_i_alloc(ctx, &d_tcount, (size_t)std::max(n_tiles, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_tbase, (size_t)std::max(n_tiles, 1));
    if (!st && n_pairs > 0) st = pvlm_i_h2d_q(ctx, d_pd, pd.data(), (size_t)n_pairs * sizeof(PairDesc));
    if (!st && n_tiles > 0) st = pvlm_i_h2d_q(ctx, d_td, tiles.data(), (size_t)n_tiles * sizeof(TileDesc));
    if (!st && n_tiles > 0) {
      hipLaunchKernelGGL(k_tex_word_dev, dim3((unsigned)n_tiles), dim3(kThreads), 0, ctx->stream, (const PairDesc*)d_pd, (const TileDesc*)d_td, min_dist * min_dist,
                         max_dist * max_dist, d_word, d_tcount);
      if (hipGetLastError() != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_colorize_scans_dev: launch failed"); st = PVLM_ERR_HIP; }
    }
    if (!st) st = compact(ctx, ctx->stream, d_pd, n_pairs, d_td, n_tiles, d_word, d_tcount, d_tbase, (float4*)d_out, capacity, d_n_out, d_per_pair_or_null);
    // the pool is ordered by the context's stream: these blocks are reused only by work queued behind the kernels
    pvlm_i_free(ctx, d_pd); pvlm_i_free(ctx, d_td); pvlm_i_free(ctx, d_word); pvlm_i_free(ctx, d_tcount); pvlm_i_free(ctx, d_tbase);
    return st;
  } catch (const std::bad_alloc&) {
    PVLM_SET_ERR(ctx, "pvlm_colorize_scans_dev: out of host memory");
    return PVLM_ERR_NOMEM;
  }
}

extern "C" pvlm_status pvlm_colorize_debug_hsv(pvlm_ctx* ctx, long long n, const unsigned char* bgr, unsigned char* hsv_out) {
  if (!ctx) return PVLM_ERR_ARG;
  if (n < 0 || (n > 0 && (!bgr || !hsv_out))) { PVLM_SET_ERR(ctx, "pvlm_colorize_debug_hsv: n >= 0 and both buffers are required"); return PVLM_ERR_ARG; }
  if (n == 0) return PVLM_OK;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (ctx->capturing) { PVLM_SET_ERR(ctx, "pvlm_colorize_debug_hsv inside a graph capture"); return PVLM_ERR_STATE; }
  unsigned char* d = nullptr;
  if (pvlm_status st = pvlm_i_alloc(ctx, &d, (size_t)n * 6)) return st;
  hipError_t e = hipMemcpyAsync(d, bgr, (size_t)n * 3, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_tex_debug_hsv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, (const unsigned char*)d, d + (size_t)n * 3);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hsv_out, d + (size_t)n * 3, (size_t)n * 3, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  pvlm_i_free(ctx, d);
  if (e != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_colorize_debug_hsv: %s", hipGetErrorString(e)); return PVLM_ERR_HIP; }
  return PVLM_OK;
}

// pvlm_preload: the code object of this translation unit loaded ahead of the first call that needs it
__global__ void k_preload_texture() {}
void pvlm_i_preload_texture(hipStream_t s) { hipLaunchKernelGGL(k_preload_texture, dim3(1), dim3(1), 0, s); }
