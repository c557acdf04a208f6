// The ordered compaction of K29 (pvlm_fuse.hip) and K30 (pvlm_texture.hip): kept records in item order, then point order, in two passes and with no waits between
// workgroups.  The items (scans, pairs) are cut into tiles of 4096 points (one workgroup, 16 rounds of 256; a tile never spans two items).  First pass: every tile
// counts what it keeps (tile_total).  One workgroup turns the tile counts into 64-bit tile bases, the total and the per-item counts (k_tile_scan).  Second pass:
// every tile ranks its kept points (wave ballots, tile_offsets) and writes them at base + rank.  What a stage keeps, how it loads a point and the record it writes are the stage's.
// Device code here is integer only; the host half cuts a batch into pieces of whole items and tiles, and copies records out of the pinned window.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"

namespace pvlm_compact {

constexpr int kThreads = 256;
constexpr int kRounds = 16;
constexpr int kTile = kThreads * kRounds;           // points per workgroup
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;
constexpr long long kPiecePoints = 1ll << 21;       // points per piece of a host entry (32 MB of float4 in, 32 MB of records out)
// tile_offsets turns the (round, wave) counts into offsets with ONE wave: one lane per count
static_assert(kRounds * kWaves == 64, "tile_offsets: one wave scans the (round, wave) counts");

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's sum of c -> tile_count[blockIdx.x]
__device__ __forceinline__ void tile_total(int c, int* tile_count) {
  __shared__ int part[kWaves];
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// The places of a tile's kept points, in point order (round-major, then wave, then lane).  A scatter kernel ballots its flags round by round: a kept point's
// rank among the wave's kept points of the round, and by lane 0 the wave's count into pre[r * kWaves + wave] (kRounds * kWaves ints of LDS).  tile_offsets, called
// once by every thread after the last round, turns the counts into exclusive offsets: the kept point of round r goes to tile base + pre[r * kWaves + wave] + rank.
// (The per-round ballot stays in the kernels: as a function called from their unrolled loops it changed k_fuse_scatter's register allocation.)
__device__ __forceinline__ void tile_offsets(int* pre) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  __syncthreads();
  if (w == 0) {                                    // one wave: one lane per count
    const int v = pre[lane];
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    pre[lane] = incl - v;
  }
  __syncthreads();
}

// one workgroup: exclusive scan of the tile counts in order (64-bit bases), the total, the per-item counts (Desc: tile0 / n_tiles of every item)
template <typename Desc>
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(const int* __restrict__ tile_count, int n_tiles, long long* __restrict__ tile_base,
                                                            const Desc* __restrict__ items, int n_items, long long* __restrict__ total,
                                                            long long* __restrict__ per_item) {
  __shared__ int wtot[kScanThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry = 0;
  int next = tid < n_tiles ? tile_count[tid] : 0;
  for (int b = 0; b < n_tiles; b += kScanThreads) {
    const int i = b + tid, v = next;
    next = i + kScanThreads < n_tiles ? tile_count[i + kScanThreads] : 0;     // the next chunk's load in flight during this one's scan
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) { const int t = wtot[k]; before += k < w ? t : 0; all += t; }
    if (i < n_tiles) tile_base[i] = carry + before + (incl - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
  if (!per_item) return;
  for (int s = tid; s < n_items; s += kScanThreads) {
    const int t0 = items[s].tile0, nt = items[s].n_tiles;
    per_item[s] = nt ? tile_base[t0 + nt - 1] + tile_count[t0 + nt - 1] - tile_base[t0] : 0;
  }
}

// the point counts of a batch's descriptors (pvlm_fuse_scan, pvlm_colorize_pair: validated, n >= 0)
template <typename Item>
std::vector<int> point_counts(const Item* items, int count) {
  std::vector<int> n((size_t)count);
  for (int s = 0; s < count; ++s) n[(size_t)s] = items[s].n;
  return n;
}

// tiles of `count` items of n[k] points: fills `tiles` with Tile::make(first point inside the item, points (<= kTile), item, first point counted from the first
// item's) and sets tile0 / n_tiles of every descriptor
template <typename Tile, typename Desc>
void make_tiles(const int* n, int count, Desc* desc, std::vector<Tile>& tiles) {
  tiles.clear();
  long long g = 0;
  for (int s = 0; s < count; ++s) {
    desc[s].tile0 = (int)tiles.size();
    for (int p0 = 0; p0 < n[s]; p0 += kTile) tiles.push_back(Tile::make(p0, std::min(kTile, n[s] - p0), s, g + p0));
    desc[s].n_tiles = (int)tiles.size() - desc[s].tile0;
    g += std::max(n[s], 0);
  }
}

// a batch cut into pieces of whole items: at most P points (a larger item is a piece of its own) and item_cap items
struct Pieces {
  std::vector<int> piece0;        // first item of every piece, and the batch's item count behind the last
  std::vector<long long> pt0;     // first point of every item, and the batch's point count behind the last
  long long P = 0, tcap = 0;      // points and tiles a piece holds at most
  int scap = 0;                   // items a piece holds at most
  int count() const { return (int)piece0.size() - 1; }
  int items(int q) const { return piece0[q + 1] - piece0[q]; }
  size_t points(int q) const { return (size_t)(pt0[(size_t)piece0[q + 1]] - pt0[(size_t)piece0[q]]); }
};
inline Pieces make_pieces(const int* n, int count, int item_cap) {
  Pieces pc;
  pc.pt0.assign((size_t)count + 1, 0);
  int max_n = 0;
  for (int s = 0; s < count; ++s) { pc.pt0[(size_t)s + 1] = pc.pt0[(size_t)s] + n[s]; max_n = std::max(max_n, n[s]); }
  pc.P = std::min(pc.pt0[(size_t)count], std::max(kPiecePoints, (long long)max_n));
  pc.piece0.push_back(0);
  for (int s = 0; s < count;) {
    long long pts = 0; int k = s;
    while (k < count && k - s < item_cap && (k == s || pts + n[k] <= pc.P)) pts += n[k++];
    pc.piece0.push_back(k); s = k;
  }
  for (int q = 0; q < pc.count(); ++q) pc.scap = std::max(pc.scap, pc.items(q));
  pc.tcap = pc.P / kTile + pc.scap + 1;
  return pc;
}

// caller's buffer <- pinned window: `m` 16-byte records to record `at` of dst
inline void unpack_records(float* dst, const float4* src, long long at, long long m, size_t n_threads_max) {
  const size_t chunk = (size_t)1 << 16;                               // records (1 MB) per worker item
  const size_t items = (size_t)((m + (long long)chunk - 1) / (long long)chunk);
  std::atomic<size_t> next{0};
  pvlm_run_workers(std::max<size_t>(1, std::min(n_threads_max, items)), [&]() {
    for (size_t c = next++; c < items; c = next++) {
      const size_t a = c * chunk, b = std::min((size_t)m, a + chunk);
      std::memcpy(dst + (size_t)(at + (long long)a) * 4, src + a, (b - a) * 16);
    }
  });
}

}  // namespace pvlm_compact
