// K48: the triplets of the pair graph (PoseGraph::FindTriplet, sfm/PoseGraph.cpp:195-226) and the triplet test of SfM::FilterByTriplet (sfm/SfM.cpp:705-778), by
// the definition of pvlm_triplet_core.h.
//
// Rank and rows are made in the call's set-up on the host (tr::Rows::build: one std::sort of P 64-bit keys, which also finds a repeated pair before anything is
// written); the sorted list, its row offsets and the rank -> caller's index table go up once.  The unit of parallelism is the PAIR in rank order: kGroup lanes share
// the candidates of pair (i, j) — the part of row i behind j, ascending — a lane per candidate per round, and look each one up in row j by binary search.
//   k_triplet_count   a ballot and a population count per round: the pair's triplet count;
//   k_tile_scan       pvlm_compact.h's ordered scan over the per-pair counts (one workgroup): 64-bit bases and the total;
//   k_triplet_emit    the same walk; a triangle's position is its pair's base plus the hits of the rounds before plus its rank in the round's ballot (ascending k):
//                     `triplets` and `triplet_pairs` as int32 triples, nothing at or past `cap`;
//   k_triplet_filter  the same walk with no scan and no list: at each triangle the three rotations, c, the verdict against `cut`; a kept triplet stores 1 into the
//                     keep bytes of its three pairs (identical racing stores), one within the band takes a slot of the bounded uncertain list through a vector atomic
//                     on the list's counter; the totals (triplets, kept) go up by one vector atomic per pair.  The entry runs the pass again with the capacity the
//                     counter reported when the list overflowed, and decides the list on the host with the literal std::acos chain.
// No kernel waits for another workgroup.  Every loop is bounded at launch: the grid strides over P, a group makes at most max_rounds rounds (the longest row over
// kGroup, from the host), a search at most kSearchSteps halvings.  The trip counts of the pair loop and of the round loop are uniform over a wave, so every lane
// takes part in every ballot.  Every index was checked on the host before the first launch.  Vector stores and plain C++ only.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_compact.h"
#include "pvlm_triplet_core.h"

namespace {

namespace tr = pvlm_triplet;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;                       // the kernels stride past kMaxBlocks workgroups (PVLM_TRIPLET_MAX_BLOCKS lowers it)
constexpr int kPairsPerBlock = kThreads / tr::kGroup;
constexpr long long kUncertainCap = 4096;              // triplets the uncertain list holds at first (PVLM_TRIPLET_UNCERTAIN_CAP lowers it)
static_assert(64 % tr::kGroup == 0 && tr::kGroup <= 32, "a group's ballot is a field of the wave's");

struct Graph { int P; const int* row_off; const int* first_r; const int* nbr; const int* idx; };
struct NoItems { int tile0, n_tiles; };                // k_tile_scan's per-item part is not used

// The walk of the pairs this workgroup takes.  at_hit(r, q, s, i, j, k, place): a lane's triangle (i, j, k) found at pair rank r with (j, k) at rank q and (i, k)
// at rank s, `place` its rank among the pair's triangles; it returns a flag the group counts too.  at_pair(r, count, flagged): lane 0 of a live pair's group.
template <class AtHit, class AtPair> __device__ __forceinline__ void walk_pairs(const Graph& g, int max_rounds, AtHit at_hit, AtPair at_pair) {
  const int lane = (int)threadIdx.x & 63, gl = lane % tr::kGroup, shift = lane - gl;
  const unsigned long long field = (1ull << tr::kGroup) - 1ull, below = (1ull << gl) - 1ull;
  for (long long r0 = (long long)blockIdx.x * kPairsPerBlock; r0 < g.P; r0 += (long long)gridDim.x * kPairsPerBlock) {
    const long long r = r0 + (int)threadIdx.x / tr::kGroup;
    const bool live = r < g.P;
    int i = 0, j = 0, c0 = 0, c1 = 0, jlo = 0, jhi = 0;
    if (live) { i = g.first_r[r]; j = g.nbr[r]; c0 = (int)r + 1; c1 = g.row_off[i + 1]; jlo = g.row_off[j]; jhi = g.row_off[j + 1]; }
    int count = 0, flagged = 0;
    for (int round = 0; round < max_rounds; ++round) {
      const int s0 = c0 + round * tr::kGroup, s = s0 + gl;
      if (!__any(s0 < c1)) break;                                  // uniform over the wave
      const bool has = s < c1;
      const int k = has ? g.nbr[s] : 0;
      const int q = has ? tr::find_in_row(g.nbr, jlo, jhi, k) : -1;
      const unsigned long long hits = (__ballot(q >= 0) >> shift) & field;
      int flag = 0;
      if (q >= 0) flag = at_hit((int)r, q, s, i, j, k, count + __popcll(hits & below));
      const unsigned long long flags = (__ballot(flag != 0) >> shift) & field;
      count += __popcll(hits); flagged += __popcll(flags);
    }
    if (live && gl == 0) at_pair((int)r, count, flagged);
  }
}

__global__ __launch_bounds__(kThreads) void k_triplet_count(Graph g, int max_rounds, int* __restrict__ count) {
  walk_pairs(g, max_rounds, [](int, int, int, int, int, int, int) { return 0; }, [&](int r, int n, int) { count[r] = n; });
}

__global__ __launch_bounds__(kThreads) void k_triplet_emit(Graph g, int max_rounds, const long long* __restrict__ base, long long cap, int* __restrict__ triplets,
                                                           int* __restrict__ triplet_pairs) {
  walk_pairs(g, max_rounds,
             [&](int r, int q, int s, int i, int j, int k, int place) {
               const long long at = base[r] + place;
               if (at < cap) {
                 if (triplets) { triplets[3 * at] = i; triplets[3 * at + 1] = j; triplets[3 * at + 2] = k; }
                 if (triplet_pairs) { triplet_pairs[3 * at] = g.idx[r]; triplet_pairs[3 * at + 1] = g.idx[q]; triplet_pairs[3 * at + 2] = g.idx[s]; }
               }
               return 0;
             },
             [](int, int, int) {});
}

// counters: [0] triplets, [1] kept without the host, [2] uncertain (the slot counter of the list; it counts past ucap)
__global__ __launch_bounds__(kThreads) void k_triplet_filter(Graph g, int max_rounds, const double* __restrict__ R_21, double cut, unsigned char* __restrict__ keep,
                                                             unsigned long long* __restrict__ counters, int* __restrict__ uncertain, long long ucap) {
  walk_pairs(g, max_rounds,
             [&](int r, int q, int s, int, int, int, int) {
               const int a = g.idx[r], b = g.idx[q], c = g.idx[s];
               const int verdict = tr::classify(tr::loop_cos(R_21 + 9 * (long long)a, R_21 + 9 * (long long)b, R_21 + 9 * (long long)c), cut);
               if (verdict == tr::kKeep) { keep[a] = 1; keep[b] = 1; keep[c] = 1; }
               else if (verdict == tr::kUncertain) {
                 const unsigned long long slot = atomicAdd(&counters[2], 1ull);
                 if (slot < (unsigned long long)ucap) { uncertain[3 * slot] = a; uncertain[3 * slot + 1] = b; uncertain[3 * slot + 2] = c; }
               }
               return verdict == tr::kKeep ? 1 : 0;
             },
             [&](int, int n, int kept) {
               if (n) atomicAdd(&counters[0], (unsigned long long)n);
               if (kept) atomicAdd(&counters[1], (unsigned long long)kept);
             });
}

// the stage clocks of a call under PVLM_TRIPLET_PROFILE: with it set, every stage ends in a wait for the stream
struct Clocks {
  pvlm_call& c; bool on;
  std::chrono::steady_clock::time_point t0;
  explicit Clocks(pvlm_call& call) : c(call), on(std::getenv("PVLM_TRIPLET_PROFILE") != nullptr) {}
  void start() { t0 = std::chrono::steady_clock::now(); }
  // the milliseconds since start(), after a wait when profiling; 0 otherwise
  double stop() {
    if (!on) return 0.0;
    c.sync();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};
double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// the sorted list on the device
struct DeviceRows {
  Graph g{}; int max_rounds = 0; unsigned grid = 1;
  void upload(pvlm_call& c, const tr::Rows& rows) {
    g.P = rows.P;
    g.row_off = c.upload(rows.row_off.data(), rows.row_off.size()); g.first_r = c.upload(rows.first_r.data(), rows.first_r.size());
    g.nbr = c.upload(rows.nbr.data(), rows.nbr.size()); g.idx = c.upload(rows.idx.data(), rows.idx.size());
    max_rounds = rows.max_rounds();
    const long long limit = pvlm_i_env_limit("PVLM_TRIPLET_MAX_BLOCKS", kMaxBlocks), want = ((long long)rows.P + kPairsPerBlock - 1) / kPairsPerBlock;
    grid = (unsigned)(want < 1 ? 1 : (want > limit ? limit : want));
  }
};

}  // namespace

extern "C" pvlm_status pvlm_triplets_find(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, int* triplets, int* triplet_pairs,
                                          long long capacity, long long* needed, long long* pair_counts) {
  const char* who = "pvlm_triplets_find";
  if (!ctx) return PVLM_ERR_ARG;
  if (!needed || capacity < 0) { PVLM_SET_ERR(ctx, "%s: %s", who, needed ? "a negative capacity" : "null argument"); return PVLM_ERR_ARG; }
  if (const char* bad = tr::check_args(n_cameras, n_pairs, first, second)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const auto call_t0 = std::chrono::steady_clock::now();
  tr::Rows rows;
  if (!rows.build(n_cameras, n_pairs, first, second)) { PVLM_SET_ERR(ctx, "%s: a pair named twice", who); return PVLM_ERR_ARG; }
  const double rows_ms = ms_since(call_t0);
  const int P = n_pairs;
  if (P == 0) { *needed = 0; return PVLM_OK; }
  const bool wanted = triplets || triplet_pairs;
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  Clocks clk(c);
  double upload_ms = 0, count_ms = 0, scan_ms = 0, emit_ms = 0, copy_ms = 0;
  clk.start();
  DeviceRows d;
  d.upload(c, rows);
  int* d_count = c.alloc<int>((size_t)P);
  long long* d_base = c.alloc<long long>((size_t)P);
  long long* d_total = c.alloc<long long>(1);
  upload_ms = clk.stop();
  clk.start();
  c.launch(k_triplet_count, dim3(d.grid), dim3(kThreads), 0, d.g, d.max_rounds, d_count);
  c.check_launches();
  count_ms = clk.stop();
  clk.start();
  c.launch(pvlm_compact::k_tile_scan<NoItems>, dim3(1), dim3(pvlm_compact::kScanThreads), 0, (const int*)d_count, P, d_base, (const NoItems*)nullptr, 0, d_total,
           (long long*)nullptr);
  c.check_launches();
  long long total = 0;
  std::vector<int> counts(pair_counts ? (size_t)P : 0);
  c.d2h(&total, d_total, sizeof total);
  if (pair_counts) c.d2h(counts.data(), d_count, counts.size() * sizeof(int));
  if (c.sync()) return c.st;
  scan_ms = clk.on ? ms_since(clk.t0) : 0.0;
  const long long n_write = wanted ? (total < capacity ? total : capacity) : 0;
  if (n_write > 0) {
    clk.start();
    int* d_trip = triplets ? c.alloc<int>(3 * (size_t)n_write) : nullptr;
    int* d_tp = triplet_pairs ? c.alloc<int>(3 * (size_t)n_write) : nullptr;
    c.launch(k_triplet_emit, dim3(d.grid), dim3(kThreads), 0, d.g, d.max_rounds, (const long long*)d_base, n_write, d_trip, d_tp);
    c.check_launches();
    emit_ms = clk.stop();
    clk.start();
    if (triplets) c.d2h(triplets, d_trip, 3 * (size_t)n_write * sizeof(int));
    if (triplet_pairs) c.d2h(triplet_pairs, d_tp, 3 * (size_t)n_write * sizeof(int));
    if (c.sync()) return c.st;
    copy_ms = clk.on ? ms_since(clk.t0) : 0.0;
  }
  *needed = total;
  if (pair_counts) for (int r = 0; r < P; ++r) pair_counts[rows.idx[(size_t)r]] = counts[(size_t)r];
  if (clk.on)
    std::fprintf(stderr, "pvlm_triplet_profile {\"entry\": \"find\", \"cameras\": %d, \"pairs\": %d, \"triplets\": %lld, \"written\": %lld, \"sort\": \"host std::sort\", "
                 "\"total_ms\": %.3f, \"rows_ms\": %.3f, \"upload_ms\": %.3f, \"count_ms\": %.3f, \"scan_ms\": %.3f, \"emit_ms\": %.3f, \"copy_out_ms\": %.3f}\n",
                 n_cameras, P, total, n_write, ms_since(call_t0), rows_ms, upload_ms, count_ms, scan_ms, emit_ms, copy_ms);
  if (wanted && total > capacity) { PVLM_SET_ERR(ctx, "%s: %lld triplets, capacity %lld", who, total, capacity); return PVLM_ERR_CAPACITY; }
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_triplets_filter(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, double angle_threshold_deg,
                                            unsigned char* keep, pvlm_triplet_stats* stats) {
  static_assert(sizeof(tr::Stats) == sizeof(pvlm_triplet_stats), "pvlm_triplet_stats is the core's Stats");
  const char* who = "pvlm_triplets_filter";
  if (!ctx) return PVLM_ERR_ARG;
  if (!stats || (n_pairs > 0 && (!R_21 || !keep))) { PVLM_SET_ERR(ctx, "%s: null argument", who); return PVLM_ERR_ARG; }
  if (!std::isfinite(angle_threshold_deg)) { PVLM_SET_ERR(ctx, "%s: the threshold is not finite", who); return PVLM_ERR_ARG; }
  if (const char* bad = tr::check_args(n_cameras, n_pairs, first, second)) { PVLM_SET_ERR(ctx, "%s: %s", who, bad); return PVLM_ERR_ARG; }
  const auto call_t0 = std::chrono::steady_clock::now();
  tr::Rows rows;
  if (!rows.build(n_cameras, n_pairs, first, second)) { PVLM_SET_ERR(ctx, "%s: a pair named twice", who); return PVLM_ERR_ARG; }
  const double rows_ms = ms_since(call_t0);
  const int P = n_pairs;
  tr::Stats st{0, 0, 0, 0};
  if (P == 0) { std::memcpy(stats, &st, sizeof st); return PVLM_OK; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  Clocks clk(c);
  clk.start();
  DeviceRows d;
  d.upload(c, rows);
  const double* d_R = c.upload(R_21, 9 * (size_t)P);
  unsigned char* d_keep = c.alloc<unsigned char>((size_t)P);
  unsigned long long* d_counters = c.alloc<unsigned long long>(3);
  const double upload_ms = clk.stop();
  const double cut = tr::cut_for(angle_threshold_deg);
  long long ucap = pvlm_i_env_limit("PVLM_TRIPLET_UNCERTAIN_CAP", kUncertainCap);
  unsigned long long counters[3] = {0, 0, 0};
  int* d_unc = nullptr;
  int passes = 0;
  clk.start();
  // at most two passes: the counter of the first gives the capacity of the second, and the pass is a function of its input
  for (; passes < 2;) {
    d_unc = c.alloc<int>(3 * (size_t)ucap);
    c.memset(d_keep, 0, (size_t)P);
    c.memset(d_counters, 0, sizeof counters);
    c.launch(k_triplet_filter, dim3(d.grid), dim3(kThreads), 0, d.g, d.max_rounds, d_R, cut, d_keep, d_counters, d_unc, ucap);
    c.check_launches();
    c.d2h(counters, d_counters, sizeof counters);
    if (c.sync()) return c.st;
    ++passes;
    if ((long long)counters[2] <= ucap) break;
    ucap = (long long)counters[2];
  }
  if ((long long)counters[2] > ucap) { PVLM_SET_ERR(ctx, "%s: the uncertain list overflowed twice", who); return PVLM_ERR_HIP; }
  const double filter_ms = clk.on ? ms_since(clk.t0) : 0.0;
  clk.start();
  std::vector<unsigned char> kept((size_t)P);
  std::vector<int> unc(3 * (size_t)counters[2]);
  c.d2h(kept.data(), d_keep, kept.size());
  c.d2h(unc.data(), d_unc, unc.size() * sizeof(int));
  if (c.sync()) return c.st;
  const double copy_ms = clk.on ? ms_since(clk.t0) : 0.0;
  st.n_triplets = (long long)counters[0]; st.n_kept_triplets = (long long)counters[1]; st.n_uncertain = (long long)counters[2];
  for (size_t u = 0; u < unc.size(); u += 3) tr::decide_uncertain(&unc[u], R_21, angle_threshold_deg, kept.data(), &st.n_kept_triplets);
  for (int p = 0; p < P; ++p) st.n_kept_pairs += kept[(size_t)p];
  std::memcpy(keep, kept.data(), kept.size());
  std::memcpy(stats, &st, sizeof st);
  if (clk.on)
    std::fprintf(stderr, "pvlm_triplet_profile {\"entry\": \"filter\", \"cameras\": %d, \"pairs\": %d, \"triplets\": %lld, \"uncertain\": %lld, \"passes\": %d, "
                 "\"sort\": \"host std::sort\", \"total_ms\": %.3f, \"rows_ms\": %.3f, \"upload_ms\": %.3f, \"filter_ms\": %.3f, \"copy_out_ms\": %.3f}\n",
                 n_cameras, P, st.n_triplets, st.n_uncertain, passes, ms_since(call_t0), rows_ms, upload_ms, filter_ms, copy_ms);
  return PVLM_OK;
}

extern "C" int pvlm_triplet_group_size(void) { return tr::kGroup; }

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_triplet() {}
void pvlm_i_preload_triplet(hipStream_t s) { hipLaunchKernelGGL(k_preload_triplet, dim3(1), dim3(1), 0, s); }
