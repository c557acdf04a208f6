// K34: the loop body of SfM::FilterImagePairs (sfm/SfM.cpp:298-480) up to RefineRelativePose, on the definition of pvlm_essential_core.h.
//
// The unit of parallelism is the CHAIN (pair, run): n_pairs x n_runs independent sequential loops of hypotheses.  k_ess_chain runs one chain per
// workgroup of one wave.  Per hypothesis: every lane draws the same 8 positions (Philox), lanes 0..44 each add the 8 products of one entry of AtA, the
// 9 x 9 cyclic Jacobi runs with the matrix in LDS (all lanes derive the rotation, lanes 0..8 each turn one row: the rows of a rotation are independent,
// so this is the serial order bit for bit), lane 0 projects to rank 2, the lanes take the residuals, a bitonic sort orders (residual, match index) (a strict
// total order: any correct sort is std::sort), and the NFA scan is a wave reduction that keeps the lowest k among equal values.
// N_LDS (pvlm_essential::kNLds = 1024): up to this many matches the pair's bearings (gathered once through the match records), the (key, index) array
// and the sampling set sit in LDS (36 B per match + 12 B per slot of the sort: 43 KB at N_LDS, sized per launch by the largest such pair of the batch).
// A pair above it takes the same code with the three arrays in global scratch and the bearings gathered through the match records (the fall-back, same
// launch).  The tail of a chain (filter entry only): DecomposeEssential by lane 0, CheckRT x 4 over the chain's inliers by all lanes, the selection inside
// the run.  k_ess_select picks the run of every pair; the inlier indices and triangulated points of the winning run come out in match order through the
// ordered compaction of pvlm_compact.h (count, scan, scatter).  Vector stores and plain C++ only.
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "pvlm_compact.h"
#include "pvlm_essential_core.h"

namespace {

using namespace pvlm_compact;
namespace es = pvlm_essential;

constexpr int kChainThreads = 64;
constexpr int kHeadDoubles = 81 + 81 + 45 + 9 + 9 + 36 + 12 + 1;      // A, V, ata, E, bestE, R x 4, t x 4 (+ 1: even)
constexpr int kBatchChains = 1 << 15;
constexpr long long kBatchMatches = 1ll << 22;

struct PairDesc {
  const float* b1; const float* b2;       // the bearings of the two frames
  long long m0;                           // first match record of the pair in the batch
  long long mask0, list0, fkey0, fset0;   // run 0's inlier mask (words), inlier list (raw entry), fall-back sort slots and sampling set; a run's stride follows from n
  int n, src, tgt, tab0;
  int tile0, n_tiles;
};
struct TileDesc {
  int p0, n, pair; long long g0;
  static TileDesc make(int p0, int n, int pair, long long g0) { return TileDesc{p0, n, pair, g0}; }
};
struct ChainRes { int valid, count; double R[9], t[3]; };

__host__ __device__ inline int pow2ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

template <bool kLds>
__device__ __forceinline__ void bearings_of(const PairDesc& P, const pvlm_match* __restrict__ m, const float* sb1, const float* sb2, int i, float* p1, float* p2) {
  if (kLds) {
    p1[0] = sb1[3 * i]; p1[1] = sb1[3 * i + 1]; p1[2] = sb1[3 * i + 2]; p2[0] = sb2[3 * i]; p2[1] = sb2[3 * i + 1]; p2[2] = sb2[3 * i + 2];
  } else {
    const pvlm_match r = m[i];
    const float* a = P.b1 + 3 * (size_t)r.query; const float* b = P.b2 + 3 * (size_t)r.train;
    p1[0] = a[0]; p1[1] = a[1]; p1[2] = a[2]; p2[0] = b[0]; p2[1] = b[1]; p2[2] = b[2];
  }
}

// one chain.  head: A | V | ata | E | bestE | R4 | t4 in LDS; key / idx: n2 = pow2ceil(n) slots; set: n; sb1 / sb2: the staged bearings (kLds)
template <bool kLds>
__device__ void chain_body(const PairDesc& P, const pvlm_match* __restrict__ m, const double* __restrict__ tab, int run, int n_runs, int max_iterations, unsigned flags,
                           unsigned long long seed, double cos_reject, int tri_threshold, double* head, double* key, int* idx, int* set, float* sb1, float* sb2,
                           unsigned* __restrict__ mask, double* __restrict__ E_out, double* __restrict__ nfa_out, int* __restrict__ cnt_out, int* __restrict__ list,
                           int* __restrict__ iters_out, ChainRes* __restrict__ res) {
  const int lane = (int)threadIdx.x, n = P.n, n2 = pow2ceil(n);
  double* A = head; double* V = head + 81; double* ata = head + 162; double* E = head + 207; double* bestE = head + 216; double* R4 = head + 225; double* t4 = head + 261;
  if (kLds)
    for (int i = lane; i < n; i += kChainThreads) {
      const pvlm_match r = m[i];
      const float* a = P.b1 + 3 * (size_t)r.query; const float* b = P.b2 + 3 * (size_t)r.train;
      sb1[3 * i] = a[0]; sb1[3 * i + 1] = a[1]; sb1[3 * i + 2] = a[2]; sb2[3 * i] = b[0]; sb2[3 * i + 1] = b[1]; sb2[3 * i + 2] = b[2];
    }
  for (int i = lane; i < n; i += kChainThreads) set[i] = i;
  if (lane < 45) ata[lane] = 0.0;
  if (lane < 9) bestE[lane] = 0.0;
  const es::ChainKey ck = es::chain_key(seed, P.src, P.tgt, run);
  es::ChainState st = es::chain_begin(max_iterations);
  int msize = n;
  __syncthreads();
  while (es::chain_running(st)) {
    int pos[8];
    es::sample8(ck, st.iter, msize, pos);
    if (lane < 45) {
      int r, c; es::ata_rc(lane, &r, &c);
      double acc = (flags & es::kFreshSample) ? 0.0 : ata[lane];
      for (int s = 0; s < 8; ++s) {
        float p1[3], p2[3];
        bearings_of<kLds>(P, m, sb1, sb2, set[pos[s]], p1, p2);
        acc = acc + es::ata_term(p1, p2, r, c);
      }
      ata[lane] = acc;
    }
    __syncthreads();
    for (int e = lane; e < 81; e += kChainThreads) { A[e] = ata[es::ata_index(e / 9, e % 9)]; V[e] = (e / 9 == e % 9) ? 1.0 : 0.0; }
    __syncthreads();
    for (int sweep = 0; sweep < es::kSweeps; ++sweep) {
      int nz = 0;
      for (int e = lane; e < 81; e += kChainThreads) nz |= (e / 9 < e % 9 && A[e] != 0.0) ? 1 : 0;
      if (!__syncthreads_or(nz)) break;
      for (int p = 0; p < 9; ++p)
        for (int q = p + 1; q < 9; ++q) {
          const double app = A[p * 9 + p], aqq = A[q * 9 + q], apq = A[p * 9 + q];
          const es::Rot R = es::jacobi_coeffs(app, aqq, apq);
          __syncthreads();                                   // every lane has read the three entries before lane 9 rewrites them
          if (R.what == 0) continue;                         // the same in every lane
          if (R.what == 2 && lane < 9) es::jacobi_row(A, V, 9, p, q, lane, R);
          if (lane == 9) es::jacobi_diag(A, 9, p, q, app, aqq, apq, R);
          __syncthreads();
        }
    }
    if (lane == 0) es::essential_from_eig9(A, V, E, nullptr);
    __syncthreads();
    double Er[9];
    for (int i = 0; i < 9; ++i) Er[i] = E[i];
    for (int i = lane; i < n2; i += kChainThreads) {
      if (i < n) {
        float p1[3], p2[3];
        bearings_of<kLds>(P, m, sb1, sb2, i, p1, p2);
        key[i] = es::sort_key(es::residual(Er, p1, p2)); idx[i] = i;
      } else { key[i] = es::inf_d(); idx[i] = 0x7fffffff; }
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < (n2 >> 1); t += kChainThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const double ki = key[i], kl = key[l]; const int ii = idx[i], il = idx[l];
          const bool up = (i & k) == 0;
          if (es::key_less(kl, il, ki, ii) == up) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
        }
        __syncthreads();
      }
    double bn = es::inf_d(); int bk = 0x7fffffff;
    for (int k = es::kMinSample + 1 + lane; k <= n; k += kChainThreads) {
      const double kk = key[k - 1];
      if (kk < es::inf_d()) { const double x = es::nfa_value(tab, n, k, kk); if (x < bn) { bn = x; bk = k; } }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double on = __shfl_xor(bn, o, 64); const int ok = __shfl_xor(bk, o, 64);
      if (on < bn || (on == bn && ok < bk)) { bn = on; bk = ok; }
    }
    if (bk == 0x7fffffff) { bk = 0; bn = es::inf_d(); }
    bool better, swap;
    es::chain_step(st, bn, bk, &better, &swap);
    if (better && lane < 9) bestE[lane] = E[lane];
    if (swap) { for (int i = lane; i < bk; i += kChainThreads) set[i] = idx[i]; msize = bk; }
    __syncthreads();
  }
  const bool model = es::chain_has_model(st);
  if (lane == 0) *iters_out = st.iter;
  if (E_out) {                                               // the raw entry
    if (lane < 9) E_out[lane] = model ? bestE[lane] : 0.0;
    if (lane == 0) { *nfa_out = st.minNFA; *cnt_out = model ? msize : 0; }
    if (model) for (int i = lane; i < msize; i += kChainThreads) list[i] = set[i];
    return;
  }
  const int words = (n + 31) >> 5;
  for (int w = lane; w < words; w += kChainThreads) mask[w] = 0u;
  __syncthreads();
  if (!model) { if (lane == 0) { res->valid = 0; res->count = 0; } return; }
  for (int i = lane; i < msize; i += kChainThreads) { const int s = set[i]; atomicOr(&mask[s >> 5], 1u << (s & 31)); }
  if (lane == 0) es::decompose(bestE, R4, t4);
  __syncthreads();
  int num[4] = {0, 0, 0, 0};
  for (int i = lane; i < n; i += kChainThreads) {
    if (!((mask[i >> 5] >> (i & 31)) & 1u)) continue;
    float p1[3], p2[3]; double X[3];
    bearings_of<kLds>(P, m, sb1, sb2, i, p1, p2);
    for (int j = 0; j < 4; ++j) num[j] += es::check_point(R4 + 9 * j, t4 + 3 * j, p1, p2, cos_reject, X) ? 1 : 0;
  }
  for (int j = 0; j < 4; ++j) num[j] = wave_sum(num[j]);
  const int cand = es::select_candidate(num, tri_threshold);
  if (lane == 0) { res->valid = cand >= 0 ? 1 : 0; res->count = cand >= 0 ? num[cand] : 0; }
  if (cand >= 0) {
    if (lane < 9) res->R[lane] = R4[9 * cand + lane];
    if (lane < 3) res->t[lane] = t4[3 * cand + lane];
  }
}

// one workgroup (one wave) per chain: blockIdx.x = pair * n_runs + run.  lds_n: the largest match count (<= N_LDS) of the batch, the dynamic LDS is sized for it
__global__ __launch_bounds__(kChainThreads) void k_ess_chain(const PairDesc* __restrict__ pairs, const pvlm_match* __restrict__ matches, const double* __restrict__ tabs,
                                                             int n_runs, int max_iterations, unsigned flags, unsigned long long seed, double cos_reject, int tri_threshold,
                                                             int lds_n, double* __restrict__ fkey, int* __restrict__ fidx, int* __restrict__ fset, unsigned* __restrict__ masks,
                                                             double* __restrict__ E_out, double* __restrict__ nfa_out, int* __restrict__ cnt_out, int* __restrict__ lists,
                                                             int* __restrict__ iters, ChainRes* __restrict__ res) {
  extern __shared__ double smem[];
  const int chain = (int)blockIdx.x, pair = chain / n_runs, run = chain % n_runs;
  const PairDesc P = pairs[pair];
  const int n = P.n;
  if (n <= es::kMinSample) {                                 // dropped: no chain
    if (threadIdx.x == 0) {
      iters[chain] = -1;
      if (E_out) { for (int i = 0; i < 9; ++i) E_out[9 * (size_t)chain + i] = 0.0; nfa_out[chain] = es::inf_d(); cnt_out[chain] = 0; }
      else { res[chain].valid = 0; res[chain].count = 0; }
    }
    return;
  }
  const pvlm_match* m = matches + P.m0;
  const double* tab = tabs + P.tab0;
  const int lp = pow2ceil(lds_n);
  double* head = smem;
  unsigned* mask = masks ? masks + P.mask0 + (long long)run * ((n + 31) >> 5) : nullptr;
  double* Eo = E_out ? E_out + 9 * (size_t)chain : nullptr;
  int* list = lists ? lists + P.list0 + (long long)run * n : nullptr;
  if (n <= lds_n) {
    double* key = smem + kHeadDoubles;
    int* idx = (int*)(key + lp); int* set = idx + lp;
    float* sb1 = (float*)(set + lds_n); float* sb2 = sb1 + 3 * lds_n;
    chain_body<true>(P, m, tab, run, n_runs, max_iterations, flags, seed, cos_reject, tri_threshold, head, key, idx, set, sb1, sb2, mask, Eo, nfa_out + chain, cnt_out + chain,
                     list, iters + chain, res + chain);
  } else {
    const int n2 = pow2ceil(n);
    chain_body<false>(P, m, tab, run, n_runs, max_iterations, flags, seed, cos_reject, tri_threshold, head, fkey + P.fkey0 + (long long)run * n2,
                      fidx + P.fkey0 + (long long)run * n2, fset + P.fset0 + (long long)run * n, nullptr, nullptr, mask, Eo, nfa_out + chain, cnt_out + chain, list, iters + chain,
                      res + chain);
  }
}

// the run of every pair (:413-416): the most CheckRT inliers, the lowest run index among equal counts
__global__ void k_ess_select(const ChainRes* __restrict__ res, int n_pairs, int n_runs, int* __restrict__ winner, int* __restrict__ keep, double* __restrict__ R, double* __restrict__ t) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pairs) return;
  int best = -1, count = -1;
  for (int r = 0; r < n_runs; ++r) { const ChainRes& c = res[(size_t)p * n_runs + r]; if (c.valid && c.count > count) { best = r; count = c.count; } }
  winner[p] = best; keep[p] = best >= 0 ? 1 : 0;
  for (int i = 0; i < 9; ++i) R[9 * (size_t)p + i] = best >= 0 ? res[(size_t)p * n_runs + best].R[i] : 0.0;
  for (int i = 0; i < 3; ++i) t[3 * (size_t)p + i] = best >= 0 ? res[(size_t)p * n_runs + best].t[i] : 0.0;
}

// match j of a pair with a winning run: in the chain's inlier set and counted by CheckRT
__device__ __forceinline__ bool kept_point(const PairDesc& P, const pvlm_match* __restrict__ matches, const unsigned* __restrict__ masks, int win, const double* R, const double* t,
                                           double cos_reject, int j, double* X) {
  const unsigned* mask = masks + P.mask0 + (long long)win * ((P.n + 31) >> 5);
  if (!((mask[j >> 5] >> (j & 31)) & 1u)) return false;
  const pvlm_match r = matches[P.m0 + j];
  return es::check_point(R, t, P.b1 + 3 * (size_t)r.query, P.b2 + 3 * (size_t)r.train, cos_reject, X);
}

__global__ __launch_bounds__(kThreads) void k_ess_count(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, const pvlm_match* __restrict__ matches,
                                                        const unsigned* __restrict__ masks, const int* __restrict__ winner, const double* __restrict__ Rs,
                                                        const double* __restrict__ ts, double cos_reject, int* __restrict__ tile_count) {
  const TileDesc td = tiles[blockIdx.x];
  const PairDesc P = pairs[td.pair];
  const int win = winner[td.pair];
  double R[9], t[3], X[3];
  for (int i = 0; i < 9; ++i) R[i] = Rs[9 * (size_t)td.pair + i];
  for (int i = 0; i < 3; ++i) t[i] = ts[3 * (size_t)td.pair + i];
  int c = 0;
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    c += (win >= 0 && j < td.n && kept_point(P, matches, masks, win, R, t, cos_reject, td.p0 + j, X)) ? 1 : 0;
  }
  tile_total(c, tile_count);
}

__global__ __launch_bounds__(kThreads) void k_ess_scatter(const PairDesc* __restrict__ pairs, const TileDesc* __restrict__ tiles, const pvlm_match* __restrict__ matches,
                                                          const unsigned* __restrict__ masks, const int* __restrict__ winner, const double* __restrict__ Rs,
                                                          const double* __restrict__ ts, double cos_reject, const long long* __restrict__ tile_base, int* __restrict__ out_idx,
                                                          double* __restrict__ out_tri, long long capacity) {
  const TileDesc td = tiles[blockIdx.x];
  const PairDesc P = pairs[td.pair];
  const int win = winner[td.pair];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  __shared__ int pre[kRounds * kWaves];
  double R[9], t[3], X[3];
  for (int i = 0; i < 9; ++i) R[i] = Rs[9 * (size_t)td.pair + i];
  for (int i = 0; i < 3; ++i) t[i] = ts[3 * (size_t)td.pair + i];
  unsigned keep = 0;
  int rank[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int j = r * kThreads + (int)threadIdx.x;
    const bool k = win >= 0 && j < td.n && kept_point(P, matches, masks, win, R, t, cos_reject, td.p0 + j, X);
    const unsigned long long mb = __ballot(k);
    keep |= (k ? 1u : 0u) << r;
    rank[r] = __popcll(mb & below);
    if (lane == 0) pre[r * kWaves + w] = __popcll(mb);
  }
  tile_offsets(pre);
  const long long base = tile_base[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!((keep >> r) & 1u)) continue;
    const long long at = base + pre[r * kWaves + w] + rank[r];
    if (at >= capacity) continue;
    const int j = td.p0 + r * kThreads + (int)threadIdx.x;
    (void)kept_point(P, matches, masks, win, R, t, cos_reject, j, X);          // the point again (not kept in registers over the rounds)
    out_idx[at] = j; out_tri[3 * at] = X[0]; out_tri[3 * at + 1] = X[1]; out_tri[3 * at + 2] = X[2];
  }
}

struct Batches { std::vector<int> first; };                 // first pair of every batch, and n_pairs behind the last
// PVLM_ESSENTIAL_BATCH_PAIRS (read at every call) lowers the pair limit of a batch: how the tests run many batches on small inputs
Batches make_batches(int n_pairs, const long long* off, int n_runs) {
  Batches b;
  const int pair_limit = (int)pvlm_i_env_limit("PVLM_ESSENTIAL_BATCH_PAIRS", std::max(1, kBatchChains / n_runs));
  b.first.push_back(0);
  for (int p = 0; p < n_pairs;) {
    long long nm = 0; int k = p;
    while (k < n_pairs && k - p < pair_limit && (k == p || (nm + (off[k + 1] - off[k])) * n_runs <= kBatchMatches)) { nm += off[k + 1] - off[k]; ++k; }
    b.first.push_back(k); p = k;
  }
  return b;
}

// both entry points: raw (pvlm_essential_acransac: E, nfa, the runs' inlier lists) or not (pvlm_filter_image_pairs: keep, R_21, t_21, the winners' inliers and points)
pvlm_status run(pvlm_ctx* ctx, const char* who, bool raw, int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt, const long long* off,
                const pvlm_match* matches, const pvlm_essential_params* prm, unsigned flags, double* E, double* nfa, unsigned char* keep, double* R_21, double* t_21,
                long long* out_offsets, int* out_idx, double* out_tri, long long capacity, long long* needed, pvlm_essential_stats* stats) {
  if (stats) *stats = pvlm_essential_stats{0, 0, 0, 0};
  *needed = 0; out_offsets[0] = 0;
  const int n_runs = prm->n_runs, maxit = prm->max_iterations;
  if (n_runs < 1 || maxit < 1 || maxit > (1 << 24)) { PVLM_SET_ERR(ctx, "%s: n_runs and max_iterations must be >= 1 (max_iterations <= 2^24)", who); return PVLM_ERR_ARG; }
  for (int f = 0; f < n_frames; ++f) if (rows[f] < 0 || (rows[f] > 0 && !bearings[f])) { PVLM_SET_ERR(ctx, "%s: bad frame %d", who, f); return PVLM_ERR_ARG; }
  if (n_pairs > 0 && off[0] != 0) { PVLM_SET_ERR(ctx, "%s: match_offsets[0] != 0", who); return PVLM_ERR_ARG; }
  for (int p = 0; p < n_pairs; ++p) {
    if (src[p] < 0 || src[p] >= n_frames || tgt[p] < 0 || tgt[p] >= n_frames) { PVLM_SET_ERR(ctx, "%s: pair %d names a frame that is not there", who, p); return PVLM_ERR_ARG; }
    if (off[p + 1] < off[p] || off[p + 1] - off[p] > es::kMaxMatches) { PVLM_SET_ERR(ctx, "%s: match_offsets of pair %d (at most 2^29 matches per pair)", who, p); return PVLM_ERR_ARG; }
    for (long long i = off[p]; i < off[p + 1]; ++i)
      if (matches[i].query < 0 || matches[i].query >= rows[src[p]] || matches[i].train < 0 || matches[i].train >= rows[tgt[p]]) {
        PVLM_SET_ERR(ctx, "%s: match %lld of pair %d names a keypoint that is not there", who, i - off[p], p); return PVLM_ERR_ARG;
      }
  }
  if (n_pairs == 0) return PVLM_OK;
  static bool monotone = false;
  static const double cos_reject = es::angle_threshold(&monotone);
  if (!monotone) { PVLM_SET_ERR(ctx, "%s: this libm's acos is not monotone around 3 degrees", who); return PVLM_ERR_STATE; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const Batches bt = make_batches(n_pairs, off, n_runs);
  // the bearings of every frame, once
  std::vector<long long> row0((size_t)n_frames + 1, 0);
  for (int f = 0; f < n_frames; ++f) row0[(size_t)f + 1] = row0[(size_t)f] + rows[f];
  float* d_bear = c.alloc<float>(3 * (size_t)row0[(size_t)n_frames]);
  for (int f = 0; f < n_frames; ++f) c.h2d(d_bear + 3 * row0[(size_t)f], bearings[f], 3 * (size_t)rows[f] * sizeof(float));
  if (c.st) return c.st;
  std::map<int, std::vector<double>> tables;               // one table per distinct match count
  std::vector<PairDesc> pd; std::vector<TileDesc> tiles; std::vector<int> ns, h_iters, h_keep, h_cnt, h_lists; std::vector<long long> h_per; std::vector<double> h_tab, h_E, h_nfa;
  long long written = 0, total = 0;
  for (size_t bi = 0; bi + 1 < bt.first.size() && !c.st; ++bi) {
    const int p0 = bt.first[bi], np = bt.first[bi + 1] - p0;
    const long long M = off[p0 + np] - off[p0];
    const size_t NC = (size_t)np * (size_t)n_runs;
    pd.assign((size_t)np, PairDesc()); ns.assign((size_t)np, 0); h_tab.clear();
    std::map<int, int> tab_at;
    long long words = 0, lists = 0, fkey = 0, fset = 0; int lds_n = 0;
    for (int k = 0; k < np; ++k) {
      PairDesc& P = pd[(size_t)k];
      const int p = p0 + k, n = (int)(off[p + 1] - off[p]);
      P.b1 = d_bear + 3 * row0[(size_t)src[p]]; P.b2 = d_bear + 3 * row0[(size_t)tgt[p]]; P.m0 = off[p] - off[p0]; P.n = n; P.src = src[p]; P.tgt = tgt[p];
      P.mask0 = words; P.list0 = lists; P.fkey0 = fkey; P.fset0 = fset; P.tab0 = 0;
      ns[(size_t)k] = n;
      if (n <= es::kMinSample) continue;
      words += (long long)((n + 31) >> 5) * n_runs; lists += (long long)n * n_runs;
      if (n <= es::kNLds) lds_n = std::max(lds_n, n);
      else { fkey += (long long)pow2ceil(n) * n_runs; fset += (long long)n * n_runs; }
      auto it = tab_at.find(n);
      if (it == tab_at.end()) {
        std::vector<double>& tb = tables[n];
        if (tb.empty()) { tb.resize(2 + 2 * ((size_t)n + 1)); es::nfa_tables(n, tb.data()); }
        it = tab_at.emplace(n, (int)h_tab.size()).first;
        h_tab.insert(h_tab.end(), tb.begin(), tb.end());
      }
      P.tab0 = it->second;
      if (stats) { stats->chains += n_runs; (n <= es::kNLds ? stats->lds_chains : stats->fallback_chains) += n_runs; }
    }
    make_tiles(ns.data(), np, pd.data(), tiles);
    const int nt = (int)tiles.size();
    pvlm_call::batch bs(c);                                  // this batch's scratch
    PairDesc* d_pairs = c.upload(pd.data(), (size_t)np);
    pvlm_match* d_m = c.upload(matches + off[p0], (size_t)M);
    double* d_tab = c.upload(h_tab.data(), h_tab.size());
    int* d_iters = c.alloc<int>(NC);
    double* d_fkey = c.alloc<double>((size_t)fkey);
    int* d_fidx = c.alloc<int>((size_t)fkey);
    int* d_fset = c.alloc<int>((size_t)fset);
    double* d_E = raw ? c.alloc<double>(9 * NC) : nullptr;                       // the raw entry's outputs
    double* d_nfa = raw ? c.alloc<double>(NC) : nullptr;
    int* d_cnt = raw ? c.alloc<int>(NC) : nullptr;
    int* d_lists = raw ? c.alloc<int>((size_t)lists) : nullptr;
    ChainRes* d_res = raw ? nullptr : c.alloc<ChainRes>(NC);                     // the filter entry's: the chains' results, the selection, the ordered compaction
    unsigned* d_mask = raw ? nullptr : c.alloc<unsigned>((size_t)words);
    TileDesc* d_tiles = raw ? nullptr : c.upload(tiles.data(), (size_t)nt);
    int* d_tcount = raw ? nullptr : c.alloc<int>((size_t)nt);
    long long* d_tbase = raw ? nullptr : c.alloc<long long>((size_t)nt);
    long long* d_per = raw ? nullptr : c.alloc<long long>((size_t)np + 1);
    int* d_win = raw ? nullptr : c.alloc<int>((size_t)np);
    int* d_keep = raw ? nullptr : c.alloc<int>((size_t)np);
    double* d_R = raw ? nullptr : c.alloc<double>(9 * (size_t)np);
    double* d_t = raw ? nullptr : c.alloc<double>(3 * (size_t)np);
    int* d_oidx = raw ? nullptr : c.alloc<int>((size_t)M);
    double* d_otri = raw ? nullptr : c.alloc<double>(3 * (size_t)M);
    const int lp = pow2ceil(lds_n);
    const size_t lds_bytes = sizeof(double) * (size_t)(kHeadDoubles + lp) + sizeof(int) * (size_t)(lp + lds_n) + sizeof(float) * 6 * (size_t)lds_n;
    c.launch(k_ess_chain, dim3((unsigned)NC), dim3(kChainThreads), lds_bytes, d_pairs, d_m, d_tab, n_runs, maxit, flags, prm->seed, cos_reject, prm->triangulation_num_threshold,
             lds_n, d_fkey, d_fidx, d_fset, d_mask, d_E, d_nfa, d_cnt, d_lists, d_iters, d_res);
    if (!raw) {
      c.launch(k_ess_select, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, d_res, np, n_runs, d_win, d_keep, d_R, d_t);
      if (nt > 0) c.launch(k_ess_count, dim3((unsigned)nt), dim3(kThreads), 0, d_pairs, d_tiles, d_m, d_mask, d_win, d_R, d_t, cos_reject, d_tcount);
      c.launch(k_tile_scan<PairDesc>, dim3(1), dim3(kScanThreads), 0, d_tcount, nt, d_tbase, d_pairs, np, d_per, d_per + 1);
      if (nt > 0) c.launch(k_ess_scatter, dim3((unsigned)nt), dim3(kThreads), 0, d_pairs, d_tiles, d_m, d_mask, d_win, d_R, d_t, cos_reject, d_tbase, d_oidx, d_otri, M);
    }
    c.check_launches();
    h_iters.resize(NC);
    c.d2h(h_iters.data(), d_iters, NC * sizeof(int));
    long long m_out = 0;
    if (raw) {
      h_cnt.resize(NC); h_lists.resize((size_t)std::max<long long>(lists, 1));
      c.d2h(E + 9 * (size_t)p0 * n_runs, d_E, 9 * NC * sizeof(double));
      c.d2h(nfa + (size_t)p0 * n_runs, d_nfa, NC * sizeof(double));
      c.d2h(h_cnt.data(), d_cnt, NC * sizeof(int));
      c.d2h(h_lists.data(), d_lists, (size_t)lists * sizeof(int));
      if (c.sync()) break;
      for (size_t ch = 0; ch < NC; ++ch) {
        const size_t gc = (size_t)p0 * n_runs + ch;
        const PairDesc& P = pd[ch / (size_t)n_runs];
        const int* src_list = h_lists.data() + P.list0 + (long long)(ch % (size_t)n_runs) * P.n;
        for (int i = 0; i < h_cnt[ch]; ++i) { const long long at = out_offsets[gc] + i; if (at < capacity) out_idx[at] = src_list[i]; }
        out_offsets[gc + 1] = out_offsets[gc] + h_cnt[ch];
        m_out += h_cnt[ch];
      }
    } else {
      h_keep.resize((size_t)np); h_per.resize((size_t)np + 1);
      c.d2h(h_keep.data(), d_keep, (size_t)np * sizeof(int));
      c.d2h(h_per.data(), d_per, ((size_t)np + 1) * sizeof(long long));
      c.d2h(R_21 + 9 * (size_t)p0, d_R, 9 * (size_t)np * sizeof(double));
      c.d2h(t_21 + 3 * (size_t)p0, d_t, 3 * (size_t)np * sizeof(double));
      if (c.sync()) break;
      m_out = h_per[0];
      for (int k = 0; k < np; ++k) { keep[p0 + k] = (unsigned char)h_keep[(size_t)k]; out_offsets[p0 + k + 1] = out_offsets[p0 + k] + h_per[(size_t)k + 1]; }
      const long long fit = std::max<long long>(0, std::min(m_out, capacity - written));
      if (fit > 0) {
        c.d2h(out_idx + written, d_oidx, (size_t)fit * sizeof(int));
        c.d2h(out_tri + 3 * written, d_otri, 3 * (size_t)fit * sizeof(double));
        if (c.sync()) break;
        written += fit;
      }
    }
    total += m_out;
    if (stats) for (size_t ch = 0; ch < NC; ++ch) if (h_iters[ch] > 0) stats->hypotheses += h_iters[ch];
  }
  if (c.st) return c.st;
  *needed = total;
  if (total > capacity) { PVLM_SET_ERR(ctx, "%s: %lld records, capacity %lld", who, total, capacity); return PVLM_ERR_CAPACITY; }
  return PVLM_OK;
}

bool bad_common(pvlm_ctx* ctx, int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt, const long long* off,
                const pvlm_match* matches, const pvlm_essential_params* prm, const long long* out_offsets, const void* out, long long capacity, const long long* needed) {
  return !ctx || n_frames < 0 || (n_frames > 0 && (!bearings || !rows)) || n_pairs < 0 || !prm || !out_offsets || !needed || capacity < 0 || (capacity > 0 && !out) ||
         (n_pairs > 0 && (!src || !tgt || !off || (off[n_pairs] > 0 && !matches)));
}

}  // namespace

extern "C" pvlm_status pvlm_essential_acransac(pvlm_ctx* ctx, int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt,
                                               const long long* match_offsets, const pvlm_match* matches, const pvlm_essential_params* params, unsigned flags, double* E,
                                               double* nfa, long long* inlier_offsets, int* inliers, long long capacity, long long* needed, pvlm_essential_stats* stats) {
  if (bad_common(ctx, n_frames, bearings, rows, n_pairs, src, tgt, match_offsets, matches, params, inlier_offsets, inliers, capacity, needed) || (n_pairs > 0 && (!E || !nfa)))
    return PVLM_ERR_ARG;
  return run(ctx, "pvlm_essential_acransac", true, n_frames, bearings, rows, n_pairs, src, tgt, match_offsets, matches, params, flags, E, nfa, nullptr, nullptr, nullptr,
             inlier_offsets, inliers, nullptr, capacity, needed, stats);
}

extern "C" pvlm_status pvlm_filter_image_pairs(pvlm_ctx* ctx, int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt,
                                               const long long* match_offsets, const pvlm_match* matches, const pvlm_essential_params* params, unsigned flags,
                                               unsigned char* keep, double* R_21, double* t_21, long long* inlier_offsets, int* inlier_idx, double* triangulated, long long capacity,
                                               long long* needed, pvlm_essential_stats* stats) {
  if (bad_common(ctx, n_frames, bearings, rows, n_pairs, src, tgt, match_offsets, matches, params, inlier_offsets, inlier_idx, capacity, needed) ||
      (capacity > 0 && !triangulated) || (n_pairs > 0 && (!keep || !R_21 || !t_21)))
    return PVLM_ERR_ARG;
  return run(ctx, "pvlm_filter_image_pairs", false, n_frames, bearings, rows, n_pairs, src, tgt, match_offsets, matches, params, flags, nullptr, nullptr, keep, R_21, t_21, inlier_offsets,
             inlier_idx, triangulated, capacity, needed, stats);
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_essential() {}
void pvlm_i_preload_essential(hipStream_t s) { hipLaunchKernelGGL(k_preload_essential, dim3(1), dim3(1), 0, s); }
