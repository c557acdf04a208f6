// K49: MVS::SelectNeighborSFM (mvs/MVS.cpp:248-332) by the definition of pvlm_neighbor_sfm_core.h: the neighbour views of every reference view from the
// triangulated tracks the views share.
//
// The view -> track index (ns::Index: a counting sort by view, tracks ascending inside a view) is made in the call's set-up on the host and goes up once with the
// tracks, the points and the poses.  Then two kernels:
//   k_ns_accumulate   ONE WAVE per reference row, its score row (floats) and the cells' contribution counts in LDS.  The lane items of a row are the partner
//                     observations of its tracks, in track order; the wave takes 64 items a pass.  Every lane finds its item's track by a bounded binary search in
//                     the running item counts and computes its product (two square roots, a division, acos, powf: the expensive part) on its own.  The additions
//                     are then applied track by track, in track order, with a barrier between tracks: within one track the cells are distinct, so lanes never
//                     collide, and every cell sees upstream's order.  A TRACK THAT REPEATS A VIEW is one item: its lane walks the track's (i, j) loop for this row as
//                     written (ns::track_into_row) at the track's turn.  Rows wider than the tile (kTileCols columns, PVLM_NEIGHBOR_TILE lowers it) are done a
//                     column tile at a time: the row's items are walked once per tile and an item outside the tile costs its search only.  The finished tile goes
//                     to the F x F score and count matrices in device memory, which never leave the device (pvlm_mvs_neighbor_sfm_score_row reads one row back for
//                     the tests by running this kernel for that row alone).
//   k_ns_select       one workgroup per row: repeated arg-max over (score, column) below the previous pick — upstream's std::greater order —, T_nr and ||t_nr|| in
//                     double by every lane alike, the literal test norm > sq_distance_threshold, R_nr / t_nr / score written as float by lane 0; the certainty
//                     test of the core on every adjacent pair the walk reaches and on the first candidate behind it.
// Uncertain rows are recomputed on the host by the literal loop for that row alone (ns::row_host, ns::select_row_host) and overwrite the device's.
// No floating-point atomic, no atomic at all.  Every loop is bounded at launch: the item passes by the row's item count, the apply loop by the row's entries, the
// search by kSearchSteps, the walk by F.  Every index was checked on the host before the first launch (ns::check_args).  Vector stores and plain C++ only.
// Compiled with -ffp-contract=off: every product and sum rounds as upstream's.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_neighbor_sfm_core.h"

namespace {

namespace ns = pvlm_neighbor_sfm;

constexpr int kWave = 64;                  // k_ns_accumulate: one wave per row, so the barrier between two tracks is the wave's own
constexpr int kTileCols = 4096;            // columns of a row held in LDS at once: 16 KB of scores + 16 KB of counts
constexpr int kSelectThreads = 256;
constexpr int kSearchSteps = 32;

struct Tracks {
  int F;
  const int* view_off; const int* entry_track; const int* entry_pos; const long long* item_off; const unsigned char* repeat;
  const long long* track_offsets; const int* view_ids; const double* points; const double* T_wc;
};

// rows row0 .. row0 + gridDim.x - 1; score / count: gridDim.x rows of F
__global__ __launch_bounds__(kWave) void k_ns_accumulate(Tracks g, int row0, int tile, float* __restrict__ score, int* __restrict__ count) {
  __shared__ float cells[kTileCols];
  __shared__ int counts[kTileCols];
  const int lane = (int)threadIdx.x, row = row0 + (int)blockIdx.x, F = g.F;
  const int e0 = g.view_off[row], e1 = g.view_off[row + 1];
  const long long i0 = g.item_off[e0], i1 = g.item_off[e1];
  double Crow[3];
  ns::centre_of(g.T_wc, row, Crow);
  for (int col0 = 0; col0 < F; col0 += tile) {
    const int col1 = col0 + tile < F ? col0 + tile : F;
    for (int c = lane; c < col1 - col0; c += kWave) { cells[c] = 0.f; counts[c] = 0; }
    __syncthreads();
    for (long long base = i0; base < i1; base += kWave) {
      const long long item = base + lane;
      const bool has = item < i1;
      int e = e0;
      if (has) {                                                       // the last entry that starts at or before the item: it is not empty
        int lo = e0, hi = e1;
        for (int s = 0; s < kSearchSteps && hi - lo > 1; ++s) { const int mid = lo + ((hi - lo) >> 1); if (g.item_off[mid] <= item) lo = mid; else hi = mid; }
        e = lo;
      }
      const long long n_has = i1 - base < kWave ? i1 - base : kWave;
      const int e_lo = __shfl(e, 0), e_hi = __shfl(e, (int)n_has - 1);
      const int t = g.entry_track[e], p = g.entry_pos[e];
      const long long o0 = g.track_offsets[t];
      const int len = (int)(g.track_offsets[t + 1] - o0);
      const bool rep = g.repeat[t] != 0;
      const double* X = g.points + 3 * (long long)t;
      bool add = false; int col = 0; double prod = 0;
      if (has && !rep) {
        int q = (int)(item - g.item_off[e]);
        if (q >= p) ++q;
        col = g.view_ids[o0 + q];
        if (col >= col0 && col < col1) {
          double Ccol[3], p12, p21;
          ns::centre_of(g.T_wc, col, Ccol);
          if (q > p) { ns::pair_terms(X, Crow, Ccol, &p12, &p21); prod = p12; }      // (i, j) = (p, q): id1 = row
          else { ns::pair_terms(X, Ccol, Crow, &p12, &p21); prod = p21; }             // (i, j) = (q, p): id2 = row
          add = true;
        }
      }
      for (int k = e_lo; k <= e_hi; ++k) {                             // uniform over the wave
        if (has && e == k) {
          if (rep) ns::track_into_row(g.view_ids + o0, len, X, g.T_wc, row, col0, col1, cells, counts);
          else if (add) { cells[col - col0] = ns::add_to_cell(cells[col - col0], prod); ++counts[col - col0]; }
        }
        __syncthreads();
      }
    }
    __syncthreads();
    for (int c = lane; c < col1 - col0; c += kWave) {
      score[(size_t)blockIdx.x * F + col0 + c] = cells[c];
      count[(size_t)blockIdx.x * F + col0 + c] = counts[c];
    }
    __syncthreads();
  }
}

struct Selected { int* n_neighbors; int* ids; float* R_nr; float* t_nr; float* scores; int* n_candidates; unsigned char* uncertain; };

// the largest key of the workgroup, in every thread
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* red) {
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
  __syncthreads();
  if (((int)threadIdx.x & 63) == 0) red[(int)threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = red[0];
  for (int w = 1; w < kSelectThreads / 64; ++w) m = red[w] > m ? red[w] : m;
  return m;
}

__global__ __launch_bounds__(kSelectThreads) void k_ns_select(int F, const double* __restrict__ T_wc, const float* __restrict__ score, const int* __restrict__ count,
                                                              int neighbor_size, double threshold, Selected out) {
  __shared__ unsigned long long red[kSelectThreads / 64];
  __shared__ int cand[kSelectThreads / 64];
  const int row = (int)blockIdx.x, tid = (int)threadIdx.x;
  const float* s = score + (size_t)row * F;
  const int* n = count + (size_t)row * F;
  int mine = 0;
  for (int c = tid; c < F; c += kSelectThreads) mine += s[c] > 0.f ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if ((tid & 63) == 0) cand[tid >> 6] = mine;
  __syncthreads();
  int n_cand = 0;
  for (int w = 0; w < kSelectThreads / 64; ++w) n_cand += cand[w];
  // a positive float orders as its bits do: the key is (score bits, column + 1), 0 for "none"
  unsigned long long prev = ~0ull;
  float prev_s = 0.f; int prev_n = 0; bool have_prev = false, unc = false;
  int accepted = 0;
  for (int iter = 0; iter < F; ++iter) {
    unsigned long long best = 0;
    for (int c = tid; c < F; c += kSelectThreads) {
      const float v = s[c];
      if (v > 0.f) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(c + 1);
        if (key < prev && key > best) best = key;
      }
    }
    best = block_max(best, red);
    if (best == 0) break;
    const float bs = __uint_as_float((unsigned)(best >> 32));
    const int bc = (int)(best & 0xffffffffull) - 1, bn = n[bc];
    if (have_prev && (double)prev_s - (double)bs < ns::bound(prev_s, prev_n) + ns::bound(bs, bn)) unc = true;
    if (accepted == neighbor_size) break;                               // the first candidate behind the walk: looked at for the certainty test only
    float R[9], t[3];
    const double norm = ns::relative_pose(T_wc + 12 * (size_t)bc, T_wc + 12 * (size_t)row, R, t);
    if (ns::near_threshold(norm, threshold)) unc = true;
    if (norm > threshold) {
      if (tid == 0) {
        const size_t at = (size_t)row * neighbor_size + accepted;
        out.ids[at] = bc; out.scores[at] = bs;
        for (int k = 0; k < 9; ++k) out.R_nr[9 * at + k] = R[k];
        for (int k = 0; k < 3; ++k) out.t_nr[3 * at + k] = t[k];
      }
      ++accepted;
    }
    prev = best; prev_s = bs; prev_n = bn; have_prev = true;
  }
  if (tid == 0) { out.n_neighbors[row] = accepted; out.n_candidates[row] = n_cand; out.uncertain[row] = unc ? 1 : 0; }
}

double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// the tracks, the index, the points and the poses on the device
struct DeviceTracks {
  Tracks g{}; int tile = kTileCols;
  void upload(pvlm_call& c, const ns::Index& ix, int F, const double* T_wc, int T, const int64_t* track_offsets, const int* view_ids, const double* points) {
    static_assert(sizeof(long long) == sizeof(int64_t), "track_offsets goes up as it is");
    g.F = F;
    g.view_off = c.upload(ix.view_off.data(), ix.view_off.size()); g.entry_track = c.upload(ix.entry_track.data(), ix.entry_track.size());
    g.entry_pos = c.upload(ix.entry_pos.data(), ix.entry_pos.size()); g.item_off = c.upload(ix.item_off.data(), ix.item_off.size());
    g.repeat = c.upload(ix.repeat.data(), ix.repeat.size());
    g.track_offsets = c.upload((const long long*)track_offsets, (size_t)T + 1);
    g.view_ids = c.upload(view_ids, (size_t)track_offsets[T]);
    g.points = c.upload(points, 3 * (size_t)T);
    g.T_wc = c.upload(T_wc, 12 * (size_t)F);
    tile = (int)pvlm_i_env_limit("PVLM_NEIGHBOR_TILE", kTileCols);
  }
};

const char* check_all(int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets, const int* view_ids, const double* points,
                      int neighbor_size, double threshold) {
  const char* bad = ns::check_args(F, T_wc, pose_valid, T, track_offsets, view_ids, points, neighbor_size, threshold);
  if (!bad && track_offsets[T] > (int64_t)INT32_MAX) bad = "more than 2^31 - 1 observations";
  if (!bad && neighbor_size > 0 && (long long)F * neighbor_size > (long long)INT32_MAX / 9) bad = "F * neighbor_size too large";
  return bad;
}

}  // namespace

extern "C" pvlm_status pvlm_mvs_select_neighbors_sfm(pvlm_ctx* ctx, int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets,
                                                     const int* view_ids, const double* points, int neighbor_size, double sq_distance_threshold, int* n_neighbors,
                                                     int* ids, float* R_nr, float* t_nr, float* scores, pvlm_neighbor_sfm_stats* stats) {
  static_assert(sizeof(ns::Stats) == sizeof(pvlm_neighbor_sfm_stats), "pvlm_neighbor_sfm_stats is the core's Stats");
  const char* who = "pvlm_mvs_select_neighbors_sfm";
  if (!ctx) return PVLM_ERR_ARG;
  if (!stats || (F > 0 && (!n_neighbors || (neighbor_size > 0 && (!ids || !R_nr || !t_nr || !scores))))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = check_all(F, T_wc, pose_valid, T, track_offsets, view_ids, points, neighbor_size, sq_distance_threshold)) {
    PVLM_SET_ERR(ctx, "%s: %s", who, bad);
    return PVLM_ERR_ARG;
  }
  ns::Stats st{0, 0, 0, 0};
  if (F == 0) { std::memcpy(stats, &st, sizeof st); return PVLM_OK; }
  const auto call_t0 = std::chrono::steady_clock::now();
  const bool profile = std::getenv("PVLM_NEIGHBOR_PROFILE") != nullptr;
  ns::Index ix;
  ix.build(F, T, track_offsets, view_ids);
  const double index_ms = ms_since(call_t0);
  st.n_contributions = ix.n_contributions; st.n_repeat_tracks = ix.n_repeat_tracks;
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](double* ms) { if (profile) { c.sync(); *ms = ms_since(t0); t0 = std::chrono::steady_clock::now(); } };
  double upload_ms = 0, acc_ms = 0, select_ms = 0, copy_ms = 0, host_ms = 0;
  DeviceTracks d;
  d.upload(c, ix, F, T_wc, T, track_offsets, view_ids, points);
  const size_t slots = (size_t)F * (size_t)neighbor_size;
  float* d_score = c.alloc<float>((size_t)F * F);
  int* d_count = c.alloc<int>((size_t)F * F);
  Selected out{c.alloc<int>((size_t)F), c.alloc<int>(slots), c.alloc<float>(9 * slots), c.alloc<float>(3 * slots), c.alloc<float>(slots), c.alloc<int>((size_t)F),
               c.alloc<unsigned char>((size_t)F)};
  c.memset(out.ids, 0xff, slots * sizeof(int)); c.memset(out.R_nr, 0, 9 * slots * sizeof(float)); c.memset(out.t_nr, 0, 3 * slots * sizeof(float));
  c.memset(out.scores, 0, slots * sizeof(float));
  lap(&upload_ms);
  c.launch(k_ns_accumulate, dim3((unsigned)F), dim3(kWave), 0, d.g, 0, d.tile, d_score, d_count);
  c.check_launches();
  lap(&acc_ms);
  c.launch(k_ns_select, dim3((unsigned)F), dim3(kSelectThreads), 0, F, d.g.T_wc, (const float*)d_score, (const int*)d_count, neighbor_size, sq_distance_threshold, out);
  c.check_launches();
  lap(&select_ms);
  std::vector<int> h_n((size_t)F), h_ids(slots), h_cand((size_t)F);
  std::vector<float> h_R(9 * slots), h_t(3 * slots), h_s(slots);
  std::vector<unsigned char> h_unc((size_t)F);
  c.d2h(h_n.data(), out.n_neighbors, h_n.size() * sizeof(int)); c.d2h(h_ids.data(), out.ids, slots * sizeof(int));
  c.d2h(h_R.data(), out.R_nr, 9 * slots * sizeof(float)); c.d2h(h_t.data(), out.t_nr, 3 * slots * sizeof(float)); c.d2h(h_s.data(), out.scores, slots * sizeof(float));
  c.d2h(h_cand.data(), out.n_candidates, h_cand.size() * sizeof(int)); c.d2h(h_unc.data(), out.uncertain, h_unc.size());
  if (c.sync()) return c.st;
  if (profile) { copy_ms = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
  // the uncertain rows, by the literal loop for that row alone
  std::vector<float> row_score;
  for (int row = 0; row < F; ++row) {
    if (!h_unc[(size_t)row]) continue;
    ++st.n_uncertain;
    row_score.resize((size_t)F);
    ns::row_host(ix, F, T_wc, track_offsets, view_ids, points, row, row_score.data(), nullptr);
    const ns::RowResult r = ns::select_row_host(F, T_wc, row, row_score.data(), neighbor_size, sq_distance_threshold);
    h_n[(size_t)row] = r.n; h_cand[(size_t)row] = (int)r.n_candidates;
    for (int k = 0; k < neighbor_size; ++k) {
      const size_t at = (size_t)row * neighbor_size + k;
      const bool in = k < r.n;
      h_ids[at] = in ? r.ids[(size_t)k] : -1; h_s[at] = in ? r.scores[(size_t)k] : 0.f;
      for (int m = 0; m < 9; ++m) h_R[9 * at + m] = in ? r.R_nr[9 * (size_t)k + m] : 0.f;
      for (int m = 0; m < 3; ++m) h_t[3 * at + m] = in ? r.t_nr[3 * (size_t)k + m] : 0.f;
    }
  }
  if (profile) host_ms = ms_since(t0);
  for (int row = 0; row < F; ++row) st.n_candidates += h_cand[(size_t)row];
  std::memcpy(n_neighbors, h_n.data(), h_n.size() * sizeof(int));
  if (slots) {
    std::memcpy(ids, h_ids.data(), slots * sizeof(int)); std::memcpy(scores, h_s.data(), slots * sizeof(float));
    std::memcpy(R_nr, h_R.data(), 9 * slots * sizeof(float)); std::memcpy(t_nr, h_t.data(), 3 * slots * sizeof(float));
  }
  std::memcpy(stats, &st, sizeof st);
  if (profile)
    std::fprintf(stderr, "pvlm_neighbor_profile {\"views\": %d, \"tracks\": %d, \"observations\": %lld, \"contributions\": %lld, \"repeat_tracks\": %lld, \"tile\": %d, "
                 "\"uncertain\": %lld, \"total_ms\": %.3f, \"index_ms\": %.3f, \"upload_ms\": %.3f, \"accumulate_ms\": %.3f, \"select_ms\": %.3f, \"copy_out_ms\": %.3f, "
                 "\"host_rows_ms\": %.3f}\n",
                 F, T, (long long)track_offsets[T], st.n_contributions, st.n_repeat_tracks, d.tile, st.n_uncertain, ms_since(call_t0), index_ms, upload_ms, acc_ms,
                 select_ms, copy_ms, host_ms);
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_mvs_neighbor_sfm_score_row(pvlm_ctx* ctx, int F, const double* T_wc, const unsigned char* pose_valid, int T, const int64_t* track_offsets,
                                                       const int* view_ids, const double* points, int row, float* scores, int* counts) {
  const char* who = "pvlm_mvs_neighbor_sfm_score_row";
  if (!ctx) return PVLM_ERR_ARG;
  if (!scores) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (const char* bad = check_all(F, T_wc, pose_valid, T, track_offsets, view_ids, points, 0, 0.0)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  if (row < 0 || row >= F) { PVLM_SET_ERR(ctx, "%s: the row is out of range", who); return PVLM_ERR_ARG; }
  ns::Index ix;
  ix.build(F, T, track_offsets, view_ids);
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  DeviceTracks d;
  d.upload(c, ix, F, T_wc, T, track_offsets, view_ids, points);
  float* d_score = c.alloc<float>((size_t)F);
  int* d_count = c.alloc<int>((size_t)F);
  c.launch(k_ns_accumulate, dim3(1), dim3(kWave), 0, d.g, row, d.tile, d_score, d_count);
  c.check_launches();
  std::vector<float> h_s((size_t)F);
  std::vector<int> h_n((size_t)F);
  c.d2h(h_s.data(), d_score, h_s.size() * sizeof(float)); c.d2h(h_n.data(), d_count, h_n.size() * sizeof(int));
  if (c.sync()) return c.st;
  std::memcpy(scores, h_s.data(), h_s.size() * sizeof(float));
  if (counts) std::memcpy(counts, h_n.data(), h_n.size() * sizeof(int));
  return PVLM_OK;
}

extern "C" int pvlm_neighbor_sfm_tile_cols(void) { return kTileCols; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_neighbor_sfm() {}
void pvlm_i_preload_neighbor_sfm(hipStream_t s) { hipLaunchKernelGGL(k_preload_neighbor_sfm, dim3(1), dim3(1), 0, s); }
