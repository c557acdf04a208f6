// K33: brute-force 2-NN SIFT matching — MatchSIFT (util/SIFT.cpp:130-162, the cv::cuda knnMatch(..., 2) branch) and the loop body of
// SfM::MatchImagePairs (sfm/SfM.cpp:253-286) for a list of image pairs.  The statement is pvlm_match_core.h; built with -ffp-contract=off.
// Three stages, each batched over pairs with ragged row counts (absent rows are never read: loads are guarded, tiles are zero-filled):
//   k_match_exact   the definition on the vector ALU for a list of (pair, query) items, a wave per item: the query row through scalar loads, two train rows
//                   per lane at a time, per-lane top two, butterfly merge.  All of PVLM_FLAG_MATCH_EXACT, and the fallback of the fast path.
//   k_match_screen  s(i, j) = |a_i|^2 + |b_j|^2 - 2 a_i.b_j on v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain, so s is reproducible).  A block is
//                   128 queries of one pair, a wave 32 of them.  The queries sit on the MFMA's B side, whose column is fixed per lane: a lane's 16
//                   accumulators are 16 train rows of ONE query, so its running 4 smallest (s, j) live in its registers; lane and lane + 32 are merged once
//                   at the end.  The query fragments stay in registers for the whole pass (16 float4 per lane: lane half h holds k = 8 g + 4 h .. + 3, the
//                   k order inside the chain is free); the train rows stream through LDS in tiles of 64 (rows padded to 132 floats), the next tile's global
//                   loads in flight during the products.  Then the 4 candidates are evaluated with the definition (two per lane half), and the exact top
//                   two are accepted only when pvlm_matching::certified holds; the other queries are appended to the fallback list (counted).
//   k_match_pair_stats / k_match_count / k_tile_scan / k_match_scatter   the ratio test, per pair the count and dmax, the 0.8 filter, the second count, and the
//                   ordered compaction of pvlm_compact.h into (query, train, distance) records.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_compact.h"
#include "pvlm_match_core.h"
#include "pvlm_match_launch.h"
#include "pvlm_descset.h"

namespace {

using namespace pvlm_compact;
using pvlm_matching::kDim;
using pvlm_matching::Knn2;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kScreenQ = 128;                 // queries per block of k_match_screen
using pvlm_match_launch::PairDesc;
using pvlm_match_launch::QTile;
using pvlm_match_launch::KnnRec;
constexpr int kScreenT = 64;                  // train rows per LDS tile
constexpr int kLd = kDim + 4;                 // LDS row stride: 16 rows x 4 floats cover the banks once
constexpr long long kBatchQueries = 1ll << 20;
constexpr int kBatchPairs = 8192;

struct TileDesc {                             // first query inside the pair, queries (<= kTile), pair
  int p0, n, pair, pad;
  static TileDesc make(int p0, int n, int pair, long long) { return TileDesc{p0, n, pair, 0}; }
};

__global__ __launch_bounds__(256) void k_desc_norms(const float* __restrict__ desc, long long n_rows, float* __restrict__ norm, int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const float4* a = (const float4*)(desc + i * kDim);
  float c = 0.0f; bool finite = true;
  for (int k = 0; k < kDim / 4; ++k) {
    const float4 v = a[k];
    finite = finite && fabsf(v.x) <= 3.402823466e38f && fabsf(v.y) <= 3.402823466e38f && fabsf(v.z) <= 3.402823466e38f && fabsf(v.w) <= 3.402823466e38f;
    c = pvlm_matching::fma_f(v.x, v.x, c); c = pvlm_matching::fma_f(v.y, v.y, c); c = pvlm_matching::fma_f(v.z, v.z, c); c = pvlm_matching::fma_f(v.w, v.w, c);
  }
  norm[i] = c;
  if (!finite) atomicOr(bad, 1);
}

// the definition's chain over two rows read as float4 (k ascending)
__device__ __forceinline__ float d2_rows(const float4* __restrict__ a, const float4* __restrict__ b) {
  float c = 0.0f;
#pragma unroll 8
  for (int k = 0; k < kDim / 4; ++k) {
    const float4 x = a[k], y = b[k];
    float t = x.x - y.x; c = pvlm_matching::fma_f(t, t, c);
    t = x.y - y.y; c = pvlm_matching::fma_f(t, t, c);
    t = x.z - y.z; c = pvlm_matching::fma_f(t, t, c);
    t = x.w - y.w; c = pvlm_matching::fma_f(t, t, c);
  }
  return c;
}

__global__ __launch_bounds__(256) void k_match_exact(const PairDesc* __restrict__ pairs, int n_pairs, const int2* __restrict__ items, const int* __restrict__ count_ptr,
                                                     int n_items, KnnRec* __restrict__ knn) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const int n = count_ptr ? *count_ptr : n_items;
  for (int item = (int)blockIdx.x * 4 + w; item < n; item += (int)gridDim.x * 4) {
    int p, q;
    if (items) { const int2 it = items[item]; p = it.x; q = it.y; }
    else {                                                   // the last pair with q0 <= item (pairs without queries share the q0 of the next one)
      int lo = 0, hi = n_pairs - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pairs[mid].q0 <= item) lo = mid; else hi = mid - 1; }
      p = lo; q = item - pairs[lo].q0;
    }
    p = __builtin_amdgcn_readfirstlane(p); q = __builtin_amdgcn_readfirstlane(q);
    const PairDesc& P = pairs[p];
    const int n2 = P.n2;
    const float4* a = (const float4*)(P.a + (size_t)q * kDim);         // wave-uniform: scalar loads
    const float* B = P.b;
    Knn2 r = pvlm_matching::knn2_empty();
    for (int j = lane; j < n2; j += 128) {
      const int j1 = j + 64;
      const float4* b0 = (const float4*)(B + (size_t)j * kDim);
      const float4* b1 = (const float4*)(B + (size_t)(j1 < n2 ? j1 : j) * kDim);
      float c0 = 0.0f, c1 = 0.0f;
#pragma unroll 4
      for (int k = 0; k < kDim / 4; ++k) {
        const float4 x = a[k], y0 = b0[k], y1 = b1[k];
        float t0 = x.x - y0.x, t1 = x.x - y1.x; c0 = pvlm_matching::fma_f(t0, t0, c0); c1 = pvlm_matching::fma_f(t1, t1, c1);
        t0 = x.y - y0.y; t1 = x.y - y1.y; c0 = pvlm_matching::fma_f(t0, t0, c0); c1 = pvlm_matching::fma_f(t1, t1, c1);
        t0 = x.z - y0.z; t1 = x.z - y1.z; c0 = pvlm_matching::fma_f(t0, t0, c0); c1 = pvlm_matching::fma_f(t1, t1, c1);
        t0 = x.w - y0.w; t1 = x.w - y1.w; c0 = pvlm_matching::fma_f(t0, t0, c0); c1 = pvlm_matching::fma_f(t1, t1, c1);
      }
      pvlm_matching::knn2_push(r, c0, j);
      if (j1 < n2) pvlm_matching::knn2_push(r, c1, j1);
    }
    for (int o = 32; o > 0; o >>= 1) {                       // butterfly: every lane ends with the two smallest of the wave
      const float e0 = __shfl_xor(r.d2[0], o, 64), e1 = __shfl_xor(r.d2[1], o, 64);
      const int i0 = __shfl_xor(r.idx[0], o, 64), i1 = __shfl_xor(r.idx[1], o, 64);
      if (i0 >= 0) pvlm_matching::knn2_push(r, e0, i0);
      if (i1 >= 0) pvlm_matching::knn2_push(r, e1, i1);
    }
    if (lane == 0) knn[(size_t)P.q0 + q] = KnnRec{r.idx[0], r.idx[1], r.d2[0], r.d2[1]};
  }
}

__global__ __launch_bounds__(256) void k_match_screen(const PairDesc* __restrict__ pairs, const QTile* __restrict__ qtiles, KnnRec* __restrict__ knn,
                                                      int2* __restrict__ fb_list, int* __restrict__ fb_count) {
  __shared__ float sT[kScreenT * kLd];
  __shared__ float sNb[kScreenT];
  const QTile qt = qtiles[blockIdx.x];
  const PairDesc& P = pairs[qt.pair];
  const int n1 = P.n1, n2 = P.n2;
  const float* __restrict__ B = P.b;
  const float* __restrict__ nbv = P.nb;
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int q = qt.q0 + 32 * w + r;
  const bool qv = q < n1;
  const float* arow = P.a + (size_t)(qv ? q : n1 - 1) * kDim;          // a block exists only for n1 > 0
  float4 bq[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) bq[g] = *(const float4*)(arow + 8 * g + 4 * h);
  const float na = P.na[qv ? q : n1 - 1];
  float s0 = pvlm_matching::inf_f(), s1 = s0, s2 = s0, s3 = s0;
  int j0 = -1, j1 = -1, j2 = -1, j3 = -1;
  // (s, j) into the sorted four; within a lane j only grows, so a tie keeps the earlier entry
  auto insert = [&](float s, int j, bool lex) {
    if (!(s < s3 || (lex && s == s3 && j < j3))) return;
    s3 = s; j3 = j;
    if (s3 < s2 || (lex && s3 == s2 && j3 < j2)) { float t = s2; s2 = s3; s3 = t; int u = j2; j2 = j3; j3 = u; }
    if (s2 < s1 || (lex && s2 == s1 && j2 < j1)) { float t = s1; s1 = s2; s2 = t; int u = j1; j1 = j2; j2 = u; }
    if (s1 < s0 || (lex && s1 == s0 && j1 < j0)) { float t = s0; s0 = s1; s1 = t; int u = j0; j0 = j1; j1 = u; }
  };
  float4 pre[8];
  auto fetch = [&](int t0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = i * 256 + tid, row = idx >> 5, c4 = idx & 31, j = t0 + row;
      pre[i] = j < n2 ? *(const float4*)(B + (size_t)j * kDim + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  if (n2 > 0) fetch(0);
  for (int t0 = 0; t0 < n2; t0 += kScreenT) {
    __syncthreads();                                          // the previous tile has been read
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = i * 256 + tid, row = idx >> 5, c4 = idx & 31;
      *(float4*)(sT + row * kLd + 4 * c4) = pre[i];
    }
    if (tid < kScreenT) sNb[tid] = t0 + tid < n2 ? nbv[t0 + tid] : pvlm_matching::inf_f();
    __syncthreads();
    if (t0 + kScreenT < n2) fetch(t0 + kScreenT);
    f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float4 a0 = *(const float4*)(sT + r * kLd + 8 * g + 4 * h);
      const float4 a1 = *(const float4*)(sT + (32 + r) * kLd + 8 * g + 4 * h);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, bq[g].x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, bq[g].x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, bq[g].y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, bq[g].y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, bq[g].z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, bq[g].z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, bq[g].w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, bq[g].w, acc1, 0, 0, 0);
    }
    // D[row = train][col = query]: register e of this lane is train row (e & 3) + 8 (e >> 2) + 4 h of the tile; an absent row has nb = inf and is never inserted
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
      insert(pvlm_matching::screen_value(na, sNb[row], acc0[e]), t0 + row, false);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      insert(pvlm_matching::screen_value(na, sNb[row], acc1[e]), t0 + row, false);
    }
  }
  // the other half's four, merged in (s, j) order: both halves end with the same list
  {
    const float p0 = __shfl_xor(s0, 32, 64), p1 = __shfl_xor(s1, 32, 64), p2 = __shfl_xor(s2, 32, 64), p3 = __shfl_xor(s3, 32, 64);
    const int i0 = __shfl_xor(j0, 32, 64), i1 = __shfl_xor(j1, 32, 64), i2 = __shfl_xor(j2, 32, 64), i3 = __shfl_xor(j3, 32, 64);
    if (i0 >= 0) insert(p0, i0, true);
    if (i1 >= 0) insert(p1, i1, true);
    if (i2 >= 0) insert(p2, i2, true);
    if (i3 >= 0) insert(p3, i3, true);
  }
  // the definition on the candidates: half h takes candidates 2 h and 2 h + 1
  const int ja = h ? j2 : j0, jb = h ? j3 : j1;
  const float ea = ja >= 0 ? d2_rows((const float4*)arow, (const float4*)(B + (size_t)ja * kDim)) : pvlm_matching::inf_f();
  const float eb = jb >= 0 ? d2_rows((const float4*)arow, (const float4*)(B + (size_t)jb * kDim)) : pvlm_matching::inf_f();
  const float oa = __shfl_xor(ea, 32, 64), ob = __shfl_xor(eb, 32, 64);
  if (h || !qv) return;
  Knn2 k2 = pvlm_matching::knn2_empty();
  if (j0 >= 0) pvlm_matching::knn2_push(k2, ea, j0);
  if (j1 >= 0) pvlm_matching::knn2_push(k2, eb, j1);
  if (j2 >= 0) pvlm_matching::knn2_push(k2, oa, j2);
  if (j3 >= 0) pvlm_matching::knn2_push(k2, ob, j3);
  if (pvlm_matching::certified(s3, pvlm_matching::screen_bound(na, P.nbmax), k2.d2[1])) knn[(size_t)P.q0 + q] = KnnRec{k2.idx[0], k2.idx[1], k2.d2[0], k2.d2[1]};
  else fb_list[atomicAdd(fb_count, 1)] = make_int2(qt.pair, q);
}

// the ratio test of one query; *d0 = distance0
__device__ __forceinline__ bool is_match(const KnnRec& k, float ratio, float* d0) {
  Knn2 r; r.idx[0] = k.i0; r.idx[1] = k.i1; r.d2[0] = k.d0; r.d2[1] = k.d1;
  return pvlm_matching::ratio_keep(r, ratio, d0);
}

// a workgroup per pair: count of ratio-test matches, dmax, the count the 0.8 filter leaves, the pair's keep flag (sfm/SfM.cpp:266-275)
__global__ __launch_bounds__(256) void k_match_pair_stats(const PairDesc* __restrict__ pairs, const KnnRec* __restrict__ knn, float ratio, int threshold,
                                                          int* __restrict__ pair_keep, float* __restrict__ pair_dmax) {
  __shared__ int sc[4]; __shared__ float sm[4];
  const PairDesc& P = pairs[blockIdx.x];
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  int c = 0; float m = 0.0f;
  for (int q = tid; q < P.n1; q += 256) { float d; if (is_match(knn[(size_t)P.q0 + q], ratio, &d)) { ++c; m = fmaxf(m, d); } }
  c = wave_sum(c);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) { sc[w] = c; sm[w] = m; }
  __syncthreads();
  const int count1 = (sc[0] + sc[1]) + (sc[2] + sc[3]);
  const float dmax = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  __syncthreads();
  int keep = count1 >= threshold ? 1 : 0;
  if (keep) {
    int c2 = 0;
    for (int q = tid; q < P.n1; q += 256) { float d; if (is_match(knn[(size_t)P.q0 + q], ratio, &d) && pvlm_matching::filter_keep(d, dmax)) ++c2; }
    c2 = wave_sum(c2);
    if (lane == 0) sc[w] = c2;
    __syncthreads();
    keep = (sc[0] + sc[1]) + (sc[2] + sc[3]) >= threshold ? 1 : 0;
  }
  if (tid == 0) { pair_keep[blockIdx.x] = keep; pair_dmax[blockIdx.x] = dmax; }
}

__device__ __forceinline__ bool kept_match(const KnnRec& k, float ratio, int pair_keep, float dmax, float* d0) {
  return pair_keep && is_match(k, ratio, d0) && pvlm_matching::filter_keep(*d0, dmax);
}

__global__ __launch_bounds__(kThreads) void k_match_count(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, const KnnRec* __restrict__ knn,
                                                          float ratio, const int* __restrict__ pair_keep, const float* __restrict__ pair_dmax,
                                                          int* __restrict__ tile_count) {
  const TileDesc td = tiles[blockIdx.x];
  const size_t q0 = (size_t)pairs[td.pair].q0 + td.p0;
  const int pk = pair_keep[td.pair]; const float dmax = pair_dmax[td.pair];
  int c = 0;
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    float d;
    c += (j < td.n && kept_match(knn[q0 + j], ratio, pk, dmax, &d)) ? 1 : 0;
  }
  tile_total(c, tile_count);
}

__global__ __launch_bounds__(kThreads) void k_match_scatter(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, const KnnRec* __restrict__ knn,
                                                            float ratio, const int* __restrict__ pair_keep, const float* __restrict__ pair_dmax,
                                                            const long long* __restrict__ tile_base, pvlm_match* __restrict__ out, long long capacity) {
  const TileDesc td = tiles[blockIdx.x];
  const size_t q0 = (size_t)pairs[td.pair].q0 + td.p0;
  const int pk = pair_keep[td.pair]; const float dmax = pair_dmax[td.pair];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  __shared__ int pre[kRounds * kWaves];
  unsigned keep = 0;
  int rank[kRounds], train[kRounds]; float dist[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    bool k = false; dist[r] = 0.0f; train[r] = -1;
    if (j < td.n) { const KnnRec kr = knn[q0 + j]; train[r] = kr.i0; k = kept_match(kr, ratio, pk, dmax, &dist[r]); }
    const unsigned long long m = __ballot(k);
    keep |= (k ? 1u : 0u) << r;
    rank[r] = __popcll(m & below);
    if (lane == 0) pre[r * kWaves + w] = __popcll(m);
  }
  tile_offsets(pre);
  const long long base = tile_base[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!((keep >> r) & 1u)) continue;
    const long long at = base + pre[r * kWaves + w] + rank[r];
    if (at >= capacity) continue;
    out[at] = pvlm_match{td.p0 + r * kThreads + (int)threadIdx.x, train[r], dist[r]};
  }
}

struct Batches { std::vector<int> first; long long qcap = 0; int pcap = 0; };       // first pair of every batch, and n_pairs behind the last
// PVLM_MATCH_BATCH_QUERIES (read at every call) lowers the query limit of a batch: how the tests run many batches on small inputs
Batches make_batches(const pvlm_descset* set, int n_pairs, const int* src) {
  Batches b;
  const long long limit = pvlm_i_env_limit("PVLM_MATCH_BATCH_QUERIES", kBatchQueries);
  b.first.push_back(0);
  for (int p = 0; p < n_pairs;) {
    long long nq = 0; int k = p;
    while (k < n_pairs && k - p < kBatchPairs && (k == p || nq + set->rows[(size_t)src[k]] <= limit)) nq += set->rows[(size_t)src[k++]];
    b.qcap = std::max(b.qcap, nq); b.pcap = std::max(b.pcap, k - p);
    b.first.push_back(k); p = k;
  }
  return b;
}

// both entry points: knn2 (idx / dist non-null) or pairs (keep / match_offsets non-null)
pvlm_status run(pvlm_ctx* ctx, const char* who, const pvlm_descset* set, int n_pairs, const int* src, const int* tgt, unsigned flags, int* idx, float* dist, float ratio,
                int threshold, unsigned char* keep, long long* match_offsets, pvlm_match* out, long long capacity, long long* needed, pvlm_match_stats* stats) {
  if (stats) *stats = pvlm_match_stats{0, 0, 0};
  if (needed) *needed = 0;
  if (match_offsets) match_offsets[0] = 0;
  if (set->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the descriptor set belongs to another context", who); return PVLM_ERR_ARG; }
  if (n_pairs == 0) return PVLM_OK;
  for (int p = 0; p < n_pairs; ++p)
    if (src[p] < 0 || src[p] >= set->n_frames || tgt[p] < 0 || tgt[p] >= set->n_frames) { PVLM_SET_ERR(ctx, "%s: pair %d names a frame outside the set", who, p); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const bool exact = (flags & PVLM_FLAG_MATCH_EXACT) != 0;
  const Batches bt = make_batches(set, n_pairs, src);
  const size_t Q = (size_t)std::max<long long>(bt.qcap, 1), PB = (size_t)bt.pcap;
  const size_t TB = Q / kTile + PB + 1, QT = pvlm_match_launch::qtile_capacity(Q, PB);
  pvlm_pinned_lease lease(ctx, keep ? Q * sizeof(pvlm_match) : 1);
  if (!lease.p) { PVLM_SET_ERR(ctx, "%s: pinned memory unavailable", who); return PVLM_ERR_NOMEM; }
  PairDesc* d_pairs = c.alloc<PairDesc>(PB);
  KnnRec* d_knn = c.alloc<KnnRec>(Q);
  QTile* d_qt = exact ? nullptr : c.alloc<QTile>(QT);         // the screening path's query tiles, fallback list and its counter
  int2* d_fb = exact ? nullptr : c.alloc<int2>(Q);
  int* d_cnt = exact ? nullptr : c.alloc<int>(2);
  TileDesc* d_tiles = keep ? c.alloc<TileDesc>(TB) : nullptr;
  int* d_tcount = keep ? c.alloc<int>(TB) : nullptr;
  long long* d_tbase = keep ? c.alloc<long long>(TB) : nullptr;
  int* d_keep = keep ? c.alloc<int>(PB) : nullptr;
  float* d_dmax = keep ? c.alloc<float>(PB) : nullptr;
  long long* d_per = keep ? c.alloc<long long>(PB + 1) : nullptr;
  pvlm_match* d_out = keep ? c.alloc<pvlm_match>(Q) : nullptr;
  std::vector<PairDesc> pd; std::vector<TileDesc> tiles; std::vector<int> n1s, h_keep; std::vector<long long> h_per; std::vector<KnnRec> h_knn;
  long long q_done = 0, written = 0, total = 0;
  for (size_t bi = 0; bi + 1 < bt.first.size() && !c.st; ++bi) {
    const int p0 = bt.first[bi], np = bt.first[bi + 1] - p0;
    pd.assign((size_t)np, PairDesc()); n1s.assign((size_t)np, 0);
    long long nq = 0;
    for (int k = 0; k < np; ++k) {
      const int s = src[p0 + k], t = tgt[p0 + k];
      PairDesc& P = pd[(size_t)k];
      P.a = set->d_desc + set->row0[(size_t)s] * kDim; P.b = set->d_desc + set->row0[(size_t)t] * kDim;
      P.na = set->d_norm + set->row0[(size_t)s]; P.nb = set->d_norm + set->row0[(size_t)t];
      P.n1 = set->rows[(size_t)s]; P.n2 = set->rows[(size_t)t]; P.q0 = (int)nq; P.nbmax = set->nmax[(size_t)t];
      n1s[(size_t)k] = P.n1;
      nq += P.n1;
    }
    make_tiles(n1s.data(), np, pd.data(), tiles);
    int fb = 0;
    pvlm_match_launch::knn_batch(c, pd.data(), np, nq, exact, d_pairs, d_qt, d_knn, d_fb, d_cnt, &fb);
    if (!keep) {                                              // knn2: indices and distances of every query
      h_knn.resize((size_t)nq);
      c.d2h(h_knn.data(), d_knn, (size_t)nq * sizeof(KnnRec));
      if (c.sync()) break;
      for (long long i = 0; i < nq; ++i) {
        const KnnRec& k = h_knn[(size_t)i];
        idx[2 * (q_done + i)] = k.i0; idx[2 * (q_done + i) + 1] = k.i1;
        dist[2 * (q_done + i)] = pvlm_matching::sqrt_f(k.d0); dist[2 * (q_done + i) + 1] = pvlm_matching::sqrt_f(k.d1);
      }
    } else {
      const int nt = (int)tiles.size();
      c.h2d(d_tiles, tiles.data(), (size_t)nt * sizeof(TileDesc));
      c.launch(k_match_pair_stats, dim3((unsigned)np), dim3(256), 0, d_pairs, d_knn, ratio, threshold, d_keep, d_dmax);
      if (nt > 0) c.launch(k_match_count, dim3((unsigned)nt), dim3(kThreads), 0, d_pairs, d_tiles, d_knn, ratio, d_keep, d_dmax, d_tcount);
      c.launch(k_tile_scan<PairDesc>, dim3(1), dim3(kScanThreads), 0, d_tcount, nt, d_tbase, d_pairs, np, d_per, d_per + 1);
      if (nt > 0) c.launch(k_match_scatter, dim3((unsigned)nt), dim3(kThreads), 0, d_pairs, d_tiles, d_knn, ratio, d_keep, d_dmax, d_tbase, d_out, (long long)Q);
      c.check_launches();
      h_keep.resize((size_t)np); h_per.resize((size_t)np + 1);
      c.d2h(h_keep.data(), d_keep, (size_t)np * sizeof(int));
      c.d2h(h_per.data(), d_per, ((size_t)np + 1) * sizeof(long long));
      if (c.sync()) break;
      const long long m = h_per[0];
      for (int k = 0; k < np; ++k) { keep[p0 + k] = (unsigned char)h_keep[(size_t)k]; match_offsets[p0 + k + 1] = match_offsets[p0 + k] + h_per[(size_t)k + 1]; }
      const long long fit = std::max<long long>(0, std::min(m, capacity - written));
      if (fit > 0) {                                          // a direct copy into the pinned lease: the records bypass the staging arena
        if (hipMemcpyAsync(lease.p, d_out, (size_t)fit * sizeof(pvlm_match), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
          PVLM_SET_ERR(ctx, "%s: download failed", who); c.st = PVLM_ERR_HIP; break;
        }
        std::memcpy(out + written, lease.p, (size_t)fit * sizeof(pvlm_match));
        written += fit;
      }
      total += m;
    }
    q_done += nq;
    if (stats) { stats->queries += nq; stats->fallback_queries += exact ? nq : fb; stats->batches += 1; }
  }
  if (c.st) return c.st;
  if (needed) *needed = total;
  if (keep && total > capacity) { PVLM_SET_ERR(ctx, "%s: %lld records, capacity %lld", who, total, capacity); return PVLM_ERR_CAPACITY; }
  return PVLM_OK;
}

}  // namespace

size_t pvlm_match_launch::qtile_capacity(size_t queries, size_t pairs) { return queries / kScreenQ + pairs + 1; }

void pvlm_match_launch::knn_batch(pvlm_call& c, const PairDesc* pd, int np, long long nq, bool exact, PairDesc* d_pairs, QTile* d_qt, KnnRec* d_knn, int2* d_fb, int* d_cnt,
                                  int* fallback) {
  *fallback = exact ? (int)nq : 0;
  c.h2d(d_pairs, pd, (size_t)np * sizeof(PairDesc));
  if (nq <= 0) return;
  if (exact) {
    c.launch(k_match_exact, dim3((unsigned)std::min<long long>((nq + 3) / 4, 8192)), dim3(256), 0, d_pairs, np, nullptr, nullptr, (int)nq, d_knn);
  } else {
    std::vector<QTile> qts;                                   // copied into the staging arena when the copy is queued
    for (int k = 0; k < np; ++k) for (int q0 = 0; q0 < pd[k].n1; q0 += kScreenQ) qts.push_back(QTile{k, q0});
    c.h2d(d_qt, qts.data(), qts.size() * sizeof(QTile));
    c.memset(d_cnt, 0, 2 * sizeof(int));
    c.launch(k_match_screen, dim3((unsigned)qts.size()), dim3(256), 0, d_pairs, d_qt, d_knn, d_fb, d_cnt);
    c.launch(k_match_exact, dim3(2048), dim3(256), 0, d_pairs, np, d_fb, d_cnt, 0, d_knn);
    c.d2h(fallback, d_cnt, sizeof(int));
  }
  c.check_launches();
}

void pvlm_match_launch::row_norms(pvlm_call& c, const float* desc, long long n_rows, float* norm, int* bad) {
  if (n_rows <= 0) return;
  c.launch(k_desc_norms, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, desc, n_rows, norm, bad);
  c.check_launches();
}

extern "C" pvlm_status pvlm_descset_create(pvlm_ctx* ctx, int n_frames, const int* rows, int width, const float* const* descs, pvlm_descset** out) {
  if (!ctx || !out || n_frames < 0 || (n_frames > 0 && (!rows || !descs))) return PVLM_ERR_ARG;
  *out = nullptr;
  if (width != kDim) { PVLM_SET_ERR(ctx, "pvlm_descset_create: descriptors of %d floats (128 are required)", width); return PVLM_ERR_ARG; }
  long long total = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (rows[f] < 0 || (rows[f] > 0 && !descs[f])) { PVLM_SET_ERR(ctx, "pvlm_descset_create: bad frame %d", f); return PVLM_ERR_ARG; }
    total += rows[f];
  }
  pvlm_call c(ctx, "pvlm_descset_create");
  if (c.enter()) return c.st;
  pvlm_descset* s = new pvlm_descset();
  s->owner = ctx; s->n_frames = n_frames; s->rows.assign(rows, rows + n_frames); s->row0.assign((size_t)n_frames + 1, 0); s->nmax.assign((size_t)n_frames, 0.0f);
  for (int f = 0; f < n_frames; ++f) s->row0[(size_t)f + 1] = s->row0[(size_t)f] + rows[f];
  int bad = 0;
  std::vector<float> norm((size_t)total);
  c.st = pvlm_i_alloc(ctx, &s->d_desc, (size_t)total * kDim);          // the set's own blocks: they outlive the call, pvlm_descset_destroy frees them
  if (!c.st) c.st = pvlm_i_alloc(ctx, &s->d_norm, (size_t)total);
  int* d_bad = c.alloc<int>(1);
  for (int f = 0; f < n_frames; ++f) c.h2d(s->d_desc + s->row0[(size_t)f] * kDim, descs[f], (size_t)rows[f] * kDim * sizeof(float));
  c.memset(d_bad, 0, sizeof(int));
  pvlm_match_launch::row_norms(c, s->d_desc, total, s->d_norm, d_bad);
  c.d2h(norm.data(), s->d_norm, (size_t)total * sizeof(float));
  c.d2h(&bad, d_bad, sizeof(int));
  if (!c.sync() && bad) { PVLM_SET_ERR(ctx, "pvlm_descset_create: a descriptor value is not finite"); c.st = PVLM_ERR_ARG; }
  if (c.st) { pvlm_descset_destroy(ctx, s); return c.st; }
  for (int f = 0; f < n_frames; ++f)
    for (long long i = s->row0[(size_t)f]; i < s->row0[(size_t)f + 1]; ++i) s->nmax[(size_t)f] = std::max(s->nmax[(size_t)f], norm[(size_t)i]);
  *out = s;
  return PVLM_OK;
}

extern "C" void pvlm_descset_destroy(pvlm_ctx* ctx, pvlm_descset* set) {
  if (!ctx || !set) return;
  pvlm_i_free(set->owner, set->d_desc); pvlm_i_free(set->owner, set->d_norm);      // back to the pool they came from
  delete set;
}

extern "C" pvlm_status pvlm_match_knn2(pvlm_ctx* ctx, const pvlm_descset* set, int n_pairs, const int* src, const int* tgt, unsigned flags, int* idx, float* dist,
                                       pvlm_match_stats* stats) {
  if (!ctx || !set || n_pairs < 0 || (n_pairs > 0 && (!src || !tgt || !idx || !dist))) return PVLM_ERR_ARG;
  return run(ctx, "pvlm_match_knn2", set, n_pairs, src, tgt, flags, idx, dist, 0.0f, 0, nullptr, nullptr, nullptr, 0, nullptr, stats);
}

extern "C" pvlm_status pvlm_match_pairs(pvlm_ctx* ctx, const pvlm_descset* set, int n_pairs, const int* src, const int* tgt, float ratio, int matches_threshold,
                                        unsigned flags, unsigned char* keep, long long* match_offsets, pvlm_match* out, long long capacity, long long* needed,
                                        pvlm_match_stats* stats) {
  if (!ctx || !set || n_pairs < 0 || !match_offsets || !needed || capacity < 0 || (capacity > 0 && !out) || (n_pairs > 0 && (!src || !tgt || !keep))) return PVLM_ERR_ARG;
  if (matches_threshold < 0) { PVLM_SET_ERR(ctx, "pvlm_match_pairs: matches_threshold < 0"); return PVLM_ERR_ARG; }
  return run(ctx, "pvlm_match_pairs", set, n_pairs, src, tgt, flags, nullptr, nullptr, ratio, matches_threshold, keep, match_offsets, out, capacity, needed, stats);
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_match() {}
void pvlm_i_preload_match(hipStream_t s) { hipLaunchKernelGGL(k_preload_match, dim3(1), dim3(1), 0, s); }
