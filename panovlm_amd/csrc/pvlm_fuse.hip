// K29: the fused LiDAR map of LidarOdometry::FuseLidar / CameraLidarOptimizer::FuseLidar (lidar_mapping/LidarOdometry.cpp:323-348) — the range filter and the
// world transform of every point of the selected scans, kept points in scan order, then point order.  The order-preserving compaction is pvlm_compact.h's: a
// tile of 4096 points counts what it keeps (k_fuse_count), one workgroup turns the tile counts into 64-bit tile bases, the total and the per-scan counts
// (pvlm_compact::k_tile_scan<ScanDesc>), and each tile recomputes its keep flags and writes float4 (x', y', z', intensity) at base + rank (k_fuse_scatter).
// Tiles never span two scans: a tile reads one scan's pose and layout.
// Host clouds (pvlm_fuse_scans) go through a bounded pinned window in pieces of whole scans — the upload of piece k + 1 on a second stream beside the kernels
// and the download of piece k; device clouds (pvlm_fuse_scans_dev) are read where they lie, in one pass of the three kernels.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_workers.h"
#include "pvlm_compact.h"
#include "pvlm_fuse_core.h"

namespace {

using namespace pvlm_compact;          // kThreads, kRounds, kTile, kWaves, kScanThreads; kPiecePoints: 32 MB per buffer of the pinned window (two in, two out: 128 MB)
constexpr int kPieceScans = 16384;

struct ScanDesc {
  double T[12];                 // world <- sensor, rows 0..2 of the 4x4
  const float* xyz;
  const float* inten;
  int stride, vec;              // vec: xyz 16-B aligned with a stride of whole float4s (one float4 load per point; bit 1: intensity is its w)
  int tile0, n_tiles;
};
struct TileDesc {                                     // first point inside the scan, points (<= kTile), scan
  int p0, n, scan, pad;
  static TileDesc make(int p0, int n, int scan, long long) { return TileDesc{p0, n, scan, 0}; }
};

__device__ __forceinline__ float4 load_point(const ScanDesc& d, int i) {
  const size_t o = (size_t)i * (size_t)d.stride;
  float4 p;
  if (d.vec) {
    p = *(const float4*)(d.xyz + o);
    if (!(d.vec & 2)) p.w = d.inten[o];
  } else {
    p = make_float4(d.xyz[o], d.xyz[o + 1], d.xyz[o + 2], d.inten[o]);
  }
  return p;
}

__global__ __launch_bounds__(kThreads) void k_fuse_count(const ScanDesc* __restrict__ scans, const TileDesc* __restrict__ tiles, double sq_min, double sq_max,
                                                         int* __restrict__ tile_count) {
  const TileDesc td = tiles[blockIdx.x];
  const ScanDesc& d = scans[td.scan];
  float4 p[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    if (j < td.n) p[r] = load_point(d, td.p0 + j);
  }
  int c = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    c += (j < td.n && pvlm_fuse::keep_point(p[r].x, p[r].y, p[r].z, sq_min, sq_max)) ? 1 : 0;
  }
  tile_total(c, tile_count);
}

__global__ __launch_bounds__(kThreads) void k_fuse_scatter(const ScanDesc* __restrict__ scans, const TileDesc* __restrict__ tiles,
                                                           const long long* __restrict__ tile_base, double sq_min, double sq_max, float4* __restrict__ out,
                                                           long long capacity) {
  const TileDesc td = tiles[blockIdx.x];
  const ScanDesc& d = scans[td.scan];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  __shared__ int pre[kRounds * kWaves];
  float4 p[kRounds];
  unsigned keep = 0;
  int rank[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    if (j < td.n) p[r] = load_point(d, td.p0 + j);
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    const bool k = j < td.n && pvlm_fuse::keep_point(p[r].x, p[r].y, p[r].z, sq_min, sq_max);
    const unsigned long long m = __ballot(k);
    keep |= (k ? 1u : 0u) << r;
    rank[r] = __popcll(m & below);
    if (lane == 0) pre[r * kWaves + w] = __popcll(m);
  }
  tile_offsets(pre);
  const long long base = tile_base[blockIdx.x];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = d.T[k];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!((keep >> r) & 1u)) continue;
    const long long at = base + pre[r * kWaves + w] + rank[r];
    if (at >= capacity) continue;
    float q[3];
    pvlm_fuse::transform_point(T, p[r].x, p[r].y, p[r].z, q);
    out[at] = make_float4(q[0], q[1], q[2], p[r].w);
  }
}

void fill_desc(ScanDesc& sd, const pvlm_fuse_scan& s, const float* xyz, const float* inten, int stride) {
  std::memset(&sd, 0, sizeof(ScanDesc));
  if (s.n <= 0) return;                                  // no tiles read it (its pose may be absent)
  for (int k = 0; k < 12; ++k) sd.T[k] = s.T_wl[k];
  sd.xyz = xyz; sd.inten = inten; sd.stride = stride;
  sd.vec = (stride % 4 == 0 && ((uintptr_t)xyz & 15) == 0) ? (inten == xyz + 3 ? 3 : 1) : 0;
  sd.tile0 = 0; sd.n_tiles = 0;
}

pvlm_status check_scans(pvlm_ctx* ctx, const char* what, int n_scans, const pvlm_fuse_scan* scans, long long* total) {
  if (n_scans < 0 || (n_scans > 0 && !scans)) { PVLM_SET_ERR(ctx, "%s: bad scan list", what); return PVLM_ERR_ARG; }
  *total = 0;
  for (int s = 0; s < n_scans; ++s) {
    const pvlm_fuse_scan& d = scans[s];
    if (d.n < 0 || (d.n > 0 && (!d.xyz || !d.intensity || !d.T_wl || d.stride_floats < 3))) { PVLM_SET_ERR(ctx, "%s: bad descriptor (scan %d)", what, s); return PVLM_ERR_ARG; }
    *total += d.n;
  }
  return PVLM_OK;
}

pvlm_status launch(pvlm_ctx* ctx, hipStream_t S, const ScanDesc* d_sd, int n_scans, const TileDesc* d_td, int n_tiles, int* d_tcount, long long* d_tbase,
                   double sq_min, double sq_max, float4* d_out, long long capacity, long long* d_total, long long* d_per_scan) {
  if (n_tiles > 0) hipLaunchKernelGGL(k_fuse_count, dim3((unsigned)n_tiles), dim3(kThreads), 0, S, d_sd, d_td, sq_min, sq_max, d_tcount);
  PVLM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_tile_scan<ScanDesc>, dim3(1), dim3(kScanThreads), 0, S, (const int*)d_tcount, n_tiles, d_tbase, d_sd, n_scans, d_total, d_per_scan);
  PVLM_HIP(ctx, hipGetLastError());
  if (n_tiles > 0) hipLaunchKernelGGL(k_fuse_scatter, dim3((unsigned)n_tiles), dim3(kThreads), 0, S, d_sd, d_td, (const long long*)d_tbase, sq_min, sq_max, d_out, capacity);
  PVLM_HIP(ctx, hipGetLastError());
  return PVLM_OK;
}

}  // namespace

extern "C" pvlm_status pvlm_fuse_scans(pvlm_ctx* ctx, int n_scans, const pvlm_fuse_scan* scans, double min_range, double max_range, float* out_xyzi,
                                       long long capacity, long long* n_out, long long* per_scan_or_null) {
  if (!ctx) return PVLM_ERR_ARG;
  if (!n_out || capacity < 0 || (capacity > 0 && !out_xyzi)) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans: n_out, capacity >= 0 and an output buffer are required"); return PVLM_ERR_ARG; }
  long long total = 0;
  if (pvlm_status st = check_scans(ctx, "pvlm_fuse_scans", n_scans, scans, &total)) return st;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (ctx->capturing) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans inside a graph capture"); return PVLM_ERR_STATE; }
  *n_out = 0;
  if (per_scan_or_null) std::memset(per_scan_or_null, 0, sizeof(long long) * (size_t)n_scans);
  if (total == 0) return PVLM_OK;
  const double sq_min = min_range * min_range, sq_max = max_range * max_range;
  try {
    // pieces of whole scans: at most P points (a larger scan is a piece of its own) and kPieceScans scans
    const std::vector<int> n = point_counts(scans, n_scans);
    const Pieces pc = make_pieces(n.data(), n_scans, kPieceScans);
    const std::vector<int>& piece0 = pc.piece0;
    const std::vector<long long>& pt0 = pc.pt0;
    const int n_pieces = pc.count();
    const long long P = pc.P;
    const size_t pts_b = align256((size_t)P * 16), cnt_b = align256((size_t)(pc.scap + 1) * 8), sd_b = align256((size_t)pc.scap * sizeof(ScanDesc)),
                 td_b = align256((size_t)pc.tcap * sizeof(TileDesc));
    // pinned window: the context's pool (no pinned state of its own): in[2] | out[2] | counts[2] | descriptors[2]
    const size_t bytes = 4 * pts_b + 2 * cnt_b + 2 * (sd_b + td_b);
    pvlm_pinned_lease lease(ctx, bytes);
    char* h = lease.p;
    if (!h) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans: %zu bytes of pinned memory unavailable", bytes); return PVLM_ERR_NOMEM; }
    float4* h_in[2] = {(float4*)h, (float4*)(h + pts_b)};
    float4* h_out[2] = {(float4*)(h + 2 * pts_b), (float4*)(h + 3 * pts_b)};
    long long* h_cnt[2] = {(long long*)(h + 4 * pts_b), (long long*)(h + 4 * pts_b + cnt_b)};
    char* h_desc[2] = {h + 4 * pts_b + 2 * cnt_b, h + 4 * pts_b + 2 * cnt_b + sd_b + td_b};
    // device: the same two sets, plus the tile counts and bases
    const size_t tc_b = align256((size_t)pc.tcap * 4), tb_b = align256((size_t)pc.tcap * 8);
    const size_t set_b = 2 * pts_b + cnt_b + sd_b + td_b + tc_b + tb_b;
    char* dev = nullptr;
    if (pvlm_status st = pvlm_i_alloc_bytes(ctx, (void**)&dev, 2 * set_b)) return st;
    struct Dev { char* in; char* out; long long* cnt; ScanDesc* sd; TileDesc* td; int* tcount; long long* tbase; } D[2];
    for (int k = 0; k < 2; ++k) {
      char* b = dev + k * set_b;
      D[k].in = b; D[k].out = b + pts_b; D[k].cnt = (long long*)(b + 2 * pts_b); D[k].sd = (ScanDesc*)(b + 2 * pts_b + cnt_b);
      D[k].td = (TileDesc*)(b + 2 * pts_b + cnt_b + sd_b); D[k].tcount = (int*)(b + 2 * pts_b + cnt_b + sd_b + td_b);
      D[k].tbase = (long long*)(b + 2 * pts_b + cnt_b + sd_b + td_b + tc_b);
    }
    hipStream_t S = ctx->stream;
    if (!ctx->aux_stream && hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->aux_stream = nullptr; }
    hipStream_t U = ctx->aux_stream ? ctx->aux_stream : S;      // uploads: a stream of their own when one can be had
    // events: [0..1] upload done, [2..3] kernels done (the device input set is free), [4..5] counts down, [6..7] points down, [8] start
    hipEvent_t ev[9] = {};
    // on every way out, an exception included: nothing may still read or write the pinned window or the device sets when they go back (`lease`, declared
    // before this guard, returns the window after it has run)
    struct Guard {
      pvlm_ctx* c; hipStream_t s, u; hipEvent_t* ev; char* dev;
      ~Guard() { (void)hipStreamSynchronize(u); (void)hipStreamSynchronize(s); for (int k = 0; k < 9; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]); pvlm_i_free(c, dev); }
    } guard{ctx, S, U, ev, dev};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 9 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    const size_t n_threads_max = pvlm_i_threads_max();
    std::vector<TileDesc> tiles;
    std::vector<int> n_tiles(2, 0);
    // host side of piece q: its scans packed as float4 into h_in[q & 1], descriptors pointing into the device input set
    auto pack = [&](int q) {
      const int par = q & 1, s0 = piece0[q], s1 = piece0[q + 1];
      const long long base = pt0[(size_t)s0];
      ScanDesc* sd = (ScanDesc*)h_desc[par];
      for (int s = s0; s < s1; ++s) {
        const float* dx = (const float*)D[par].in + (size_t)(pt0[(size_t)s] - base) * 4;
        fill_desc(sd[s - s0], scans[s], dx, dx + 3, 4);
      }
      make_tiles(n.data() + s0, s1 - s0, sd, tiles);
      n_tiles[par] = (int)tiles.size();
      std::memcpy(h_desc[par] + sd_b, tiles.data(), tiles.size() * sizeof(TileDesc));
      const int ns = s1 - s0;
      const size_t nt = std::max<size_t>(1, std::min<size_t>(n_threads_max, (size_t)ns / 4 + 1));
      std::atomic<int> next{s0};
      pvlm_run_workers(nt, [&]() {
        for (int s = next++; s < s1; s = next++) {
          const pvlm_fuse_scan& d = scans[s];
          float4* dst = h_in[par] + (pt0[(size_t)s] - base);
          if (d.stride_floats == 4 && d.intensity == d.xyz + 3) std::memcpy(dst, d.xyz, (size_t)d.n * 16);
          else for (int i = 0; i < d.n; ++i) { const float* p = d.xyz + (size_t)i * d.stride_floats; dst[i] = make_float4(p[0], p[1], p[2], d.intensity[(size_t)i * d.stride_floats]); }
        }
      });
    };
    auto upload = [&](int q) -> hipError_t {
      const int par = q & 1;
      const size_t pts = pc.points(q);
      const int ns = pc.items(q);
      hipError_t r = hipStreamWaitEvent(U, q >= 2 ? ev[2 + par] : ev[8], 0);       // the device input set of piece q - 2 has been read
      if (r == hipSuccess) r = hipMemcpyAsync(D[par].in, h_in[par], pts * 16, hipMemcpyHostToDevice, U);
      if (r == hipSuccess) r = hipMemcpyAsync(D[par].sd, h_desc[par], (size_t)ns * sizeof(ScanDesc), hipMemcpyHostToDevice, U);
      if (r == hipSuccess && n_tiles[par]) r = hipMemcpyAsync(D[par].td, h_desc[par] + sd_b, (size_t)n_tiles[par] * sizeof(TileDesc), hipMemcpyHostToDevice, U);
      if (r == hipSuccess) r = hipEventRecord(ev[par], U);
      return r;
    };
    pvlm_status st = PVLM_OK;
    long long kept = 0, written = 0;
    bool overflow = false;
    long long down_at[2] = {0, 0}, down_m[2] = {0, 0};
    if (e == hipSuccess) e = hipEventRecord(ev[8], S);                  // uploads are ordered behind what the context's stream holds
    if (e == hipSuccess) { pack(0); e = upload(0); }
    for (int q = 0; q < n_pieces && e == hipSuccess && st == PVLM_OK; ++q) {
      const int par = q & 1, s0 = piece0[q], ns = pc.items(q);
      e = hipStreamWaitEvent(S, ev[par], 0);
      if (e == hipSuccess) st = launch(ctx, S, D[par].sd, ns, D[par].td, n_tiles[par], D[par].tcount, D[par].tbase, sq_min, sq_max, (float4*)D[par].out,
                                       P, D[par].cnt, D[par].cnt + 1);
      if (st) break;
      if (e == hipSuccess) e = hipEventRecord(ev[2 + par], S);
      if (e == hipSuccess) e = hipMemcpyAsync(h_cnt[par], D[par].cnt, (size_t)(ns + 1) * 8, hipMemcpyDeviceToHost, S);
      if (e == hipSuccess) e = hipEventRecord(ev[4 + par], S);
      // the next piece goes up beside this one's kernels and download
      if (e == hipSuccess && q + 1 < n_pieces) {
        e = hipEventSynchronize(ev[par ^ 1]);                           // h_in / descriptors of piece q - 1 have left
        if (e == hipSuccess) { pack(q + 1); e = upload(q + 1); }
      }
      if (e == hipSuccess) e = hipEventSynchronize(ev[4 + par]);
      if (e != hipSuccess) break;
      const long long m = h_cnt[par][0];
      if (per_scan_or_null) std::memcpy(per_scan_or_null + s0, h_cnt[par] + 1, (size_t)ns * 8);
      kept += m;
      down_m[par] = 0;
      if (!overflow && written + m > capacity) overflow = true;
      if (!overflow && m > 0) {
        e = hipMemcpyAsync(h_out[par], D[par].out, (size_t)m * 16, hipMemcpyDeviceToHost, S);
        if (e == hipSuccess) e = hipEventRecord(ev[6 + par], S);
        down_at[par] = written; down_m[par] = m; written += m;
      }
      // the previous piece's points reach the caller's buffer while this one comes down
      if (e == hipSuccess && q > 0 && down_m[par ^ 1] > 0) {
        e = hipEventSynchronize(ev[6 + (par ^ 1)]);
        if (e == hipSuccess) unpack_records(out_xyzi, h_out[par ^ 1], down_at[par ^ 1], down_m[par ^ 1], n_threads_max);
        down_m[par ^ 1] = 0;
      }
    }
    if (e == hipSuccess && st == PVLM_OK) {
      const int par = (n_pieces - 1) & 1;
      if (down_m[par] > 0) { e = hipEventSynchronize(ev[6 + par]); if (e == hipSuccess) unpack_records(out_xyzi, h_out[par], down_at[par], down_m[par], n_threads_max); }
    }
    if (st) return st;
    if (e != hipSuccess) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans: %s", hipGetErrorString(e)); return PVLM_ERR_HIP; }
    *n_out = kept;
    if (kept > capacity) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans: %lld points kept, capacity %lld", kept, capacity); return PVLM_ERR_ARG; }
    return PVLM_OK;
  } catch (const std::bad_alloc&) {
    PVLM_SET_ERR(ctx, "pvlm_fuse_scans: out of host memory");
    return PVLM_ERR_NOMEM;
  }
}

extern "C" pvlm_status pvlm_fuse_scans_dev(pvlm_ctx* ctx, int n_scans, const pvlm_fuse_scan* device_clouds, double min_range, double max_range, float* d_out,
                                           long long capacity, long long* d_n_out, long long* d_per_scan_or_null) {
  if (!ctx) return PVLM_ERR_ARG;
  if (!d_n_out || capacity < 0 || (capacity > 0 && !d_out) || ((uintptr_t)d_out & 15)) {
    PVLM_SET_ERR(ctx, "pvlm_fuse_scans_dev: d_n_out, capacity >= 0 and a 16-byte aligned d_out (float4 stores) are required");
    return PVLM_ERR_ARG;
  }
  long long total = 0;
  if (pvlm_status st = check_scans(ctx, "pvlm_fuse_scans_dev", n_scans, device_clouds, &total)) return st;
  if (pvlm_i_bind(ctx)) return PVLM_ERR_HIP;
  if (ctx->capturing) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans_dev inside a graph capture"); return PVLM_ERR_STATE; }
  try {
    std::vector<ScanDesc> sd((size_t)std::max(n_scans, 1));
    for (int s = 0; s < n_scans; ++s) {
      const pvlm_fuse_scan& d = device_clouds[s];
      fill_desc(sd[(size_t)s], d, d.xyz, d.intensity, d.stride_floats);
    }
    std::vector<TileDesc> tiles;
    make_tiles(point_counts(device_clouds, n_scans).data(), n_scans, sd.data(), tiles);
    if (tiles.size() >= (size_t)INT32_MAX) { PVLM_SET_ERR(ctx, "pvlm_fuse_scans_dev: batch too large (split it)"); return PVLM_ERR_ARG; }
    const int n_tiles = (int)tiles.size();
    ScanDesc* d_sd = nullptr; TileDesc* d_td = nullptr; int* d_tcount = nullptr; long long* d_tbase = nullptr;
    pvlm_status st = pvlm_i_alloc(ctx, &d_sd, (size_t)std::max(n_scans, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_td, (size_t)std::max(n_tiles, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_tcount, (size_t)std::max(n_tiles, 1));
    if (!st) st = pvlm_i_alloc(ctx, &d_tbase, (size_t)std::max(n_tiles, 1));
    if (!st && n_scans > 0) st = pvlm_i_h2d_q(ctx, d_sd, sd.data(), (size_t)n_scans * sizeof(ScanDesc));
    if (!st && n_tiles > 0) st = pvlm_i_h2d_q(ctx, d_td, tiles.data(), (size_t)n_tiles * sizeof(TileDesc));
    if (!st) st = launch(ctx, ctx->stream, d_sd, n_scans, d_td, n_tiles, d_tcount, d_tbase, min_range * min_range, max_range * max_range, (float4*)d_out, capacity,
                         d_n_out, d_per_scan_or_null);
    // the pool is ordered by the context's stream: these blocks are reused only by work queued behind the kernels
    pvlm_i_free(ctx, d_sd); pvlm_i_free(ctx, d_td); pvlm_i_free(ctx, d_tcount); pvlm_i_free(ctx, d_tbase);
    return st;
  } catch (const std::bad_alloc&) {
    PVLM_SET_ERR(ctx, "pvlm_fuse_scans_dev: out of host memory");
    return PVLM_ERR_NOMEM;
  }
}

// pvlm_preload: HIP loads the code object of a translation unit at the first launch of one of its kernels (15 ms for the larger ones) — an empty launch from here
// moves that out of the first call that needs this file's kernels
__global__ void k_preload_fuse() {}
void pvlm_i_preload_fuse(hipStream_t s) { hipLaunchKernelGGL(k_preload_fuse, dim3(1), dim3(1), 0, s); }
