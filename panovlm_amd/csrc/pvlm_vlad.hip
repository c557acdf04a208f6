// K35: VLAD image retrieval — the k-means codebook, the embedding and the neighbour lists of sfm/VLAD.cpp, which SfM::InitImagePairs (sfm/SfM.cpp:74-97) turns into
// image pairs.  The statement is pvlm_vlad_core.h; built with -ffp-contract=off.  Every stage works through the rows in bounded batches of whole frames (absent rows are
// never read: every load is guarded by a count).
//   assignment      K33's two stages (pvlm_match_launch.h) with the packed alive centres as the train side of every frame: k_match_screen on the fp32 matrix core with
//                   the certificate, k_match_exact for the uncertified queries (all of them with PVLM_FLAG_MATCH_EXACT).  The nearest centre is the first of the two
//                   neighbours; the packed order is the index order, so ties survive.  k_vlad_take_assign maps it back and raises `changed`.
//   grouping        a stable counting sort of the rows by centre inside a segment (k-means: all training rows; embedding: one frame): per tile of 1024 rows a
//                   histogram in LDS (integer atomics), per segment an exclusive scan over its tiles and its centres, then every row's rank among the equal keys
//                   before it in its tile.  The members of a centre come out in ascending row order.
//   centre update   k_vlad_run_sums: a workgroup per (centre, run of kSumChunk members), 128 lanes one component each, the member rows gathered as whole 512-byte
//                   rows, an ascending fp64 chain; k_vlad_means: the ascending pass over the run sums and the division.  No floating-point atomics anywhere.
//   embedding       k_vlad_res_norm (type 2: the fp64 norm of every row's residual; the normalised residual itself is recomputed where it is added, 8 bytes of
//                   scratch per row instead of 512), k_vlad_blocks: a workgroup per (frame, centre), a lane per component along the members in ascending order,
//                   the per-block step and the block's square sum; k_vlad_finish: N and the final scaling.
//   neighbours      k_vlad_sim: 32 x 32 tiles of the upper triangle, both operand tiles through LDS, k ascending, fp64 on the vector ALU, sim(i, j) written to both
//                   triangles; k_vlad_select: a workgroup per row ranks every frame by counting the frames before it in (-sim, index) order.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvlm_internal.h"
#include "pvlm_descset.h"
#include "pvlm_match_launch.h"
#include "pvlm_vlad_core.h"

struct pvlm_vladset {
  pvlm_ctx* owner = nullptr;
  int n_frames = 0, book_size = 0;
  float* d_vlad = nullptr;         // n_frames x 128 book_size
};

namespace {

using pvlm_match_launch::KnnRec;
using pvlm_match_launch::PairDesc;
using pvlm_match_launch::QTile;
using pvlm_vlad::kDim;
using pvlm_vlad::kSumChunk;

constexpr int kGroupTile = 1024;              // rows per workgroup of the grouping
constexpr long long kBatchRows = 1ll << 18;
constexpr int kBatchFrames = 8192;
constexpr int kSimTile = 32, kSimK = 64;

struct GTile { int i0, n, seg, pad; };        // rows [i0, i0 + n) of the key array, all of segment seg
struct GSeg { int tile0, n_tiles, i0, pad; }; // the segment's tiles and its first row

// src[i] = the descriptor-set row of training row i (the concatenation of the train frames in list order)
__global__ __launch_bounds__(256) void k_vlad_train_rows(const long long* __restrict__ tstart, const long long* __restrict__ trow0, int n_train, int n, long long* __restrict__ src) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  int lo = 0, hi = n_train - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tstart[mid] <= i) lo = mid; else hi = mid - 1; }
  src[i] = trow0[lo] + (i - tstart[lo]);
}

__global__ __launch_bounds__(128) void k_vlad_gather(const float* __restrict__ desc, const long long* __restrict__ src, const long long* __restrict__ init, float* __restrict__ codebook) {
  const int c = (int)blockIdx.x, k = (int)threadIdx.x;
  codebook[(size_t)c * kDim + k] = desc[(size_t)src[init[c]] * kDim + k];
}

__global__ __launch_bounds__(256) void k_vlad_take_assign(const KnnRec* __restrict__ knn, const int* __restrict__ map, int nq, int* __restrict__ assign, int* __restrict__ changed) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= nq) return;
  const int c = map[knn[i].i0];
  if (assign[i] != c) { assign[i] = c; if (changed) atomicOr(changed, 1); }
}

__global__ __launch_bounds__(256) void k_group_hist(const int* __restrict__ key, const GTile* __restrict__ tiles, int book, int* __restrict__ hist) {
  __shared__ int h[pvlm_vlad::kMaxBook];
  const GTile t = tiles[blockIdx.x];
  for (int c = (int)threadIdx.x; c < book; c += 256) h[c] = 0;
  __syncthreads();
  for (int j = (int)threadIdx.x; j < t.n; j += 256) atomicAdd(&h[key[t.i0 + j]], 1);
  __syncthreads();
  for (int c = (int)threadIdx.x; c < book; c += 256) hist[(size_t)blockIdx.x * book + c] = h[c];
}

// a workgroup per segment: hist[tile][c] becomes the number of rows of centre c in the segment's earlier tiles; start[seg][c] the first place of centre c inside the
// segment's sorted rows (book + 1 entries)
__global__ __launch_bounds__(256) void k_group_scan(int* __restrict__ hist, const GSeg* __restrict__ segs, int book, int* __restrict__ start) {
  const GSeg s = segs[blockIdx.x];
  int* st = start + (size_t)blockIdx.x * (book + 1);
  for (int c = (int)threadIdx.x; c < book; c += 256) {
    int total = 0;
    for (int t = 0; t < s.n_tiles; ++t) { int* p = hist + (size_t)(s.tile0 + t) * book + c; const int v = *p; *p = total; total += v; }
    st[c + 1] = total;
  }
  __syncthreads();
  if (threadIdx.x == 0) { int run = 0; st[0] = 0; for (int c = 0; c < book; ++c) { run += st[c + 1]; st[c + 1] = run; } }
}

__global__ __launch_bounds__(256) void k_group_scatter(const int* __restrict__ key, const GTile* __restrict__ tiles, const int* __restrict__ hist, const GSeg* __restrict__ segs,
                                                       const int* __restrict__ start, int book, int* __restrict__ order) {
  __shared__ int sk[kGroupTile];
  const GTile t = tiles[blockIdx.x];
  for (int j = (int)threadIdx.x; j < t.n; j += 256) sk[j] = key[t.i0 + j];
  __syncthreads();
  const int* st = start + (size_t)t.seg * (book + 1);
  const int seg0 = segs[t.seg].i0;
  for (int j = (int)threadIdx.x; j < t.n; j += 256) {
    const int c = sk[j];
    int rank = 0;
    for (int l = 0; l < j; ++l) rank += sk[l] == c ? 1 : 0;
    order[seg0 + st[c] + hist[(size_t)blockIdx.x * book + c] + rank] = t.i0 + j;
  }
}

// run0[c] = the first run of centre c among all runs (book + 1 entries); one thread
__global__ void k_vlad_run_prefix(const int* __restrict__ start, int book, int* __restrict__ run0) {
  if (blockIdx.x || threadIdx.x) return;
  int r = 0; run0[0] = 0;
  for (int c = 0; c < book; ++c) { r += (start[c + 1] - start[c] + kSumChunk - 1) / kSumChunk; run0[c + 1] = r; }
}

__global__ __launch_bounds__(128) void k_vlad_run_sums(const float* __restrict__ desc, const long long* __restrict__ src, const int* __restrict__ order,
                                                       const int* __restrict__ start, int book, const int* __restrict__ run0, double* __restrict__ run_sum) {
  const int r = (int)blockIdx.x, k = (int)threadIdx.x;
  if (r >= run0[book]) return;
  int lo = 0, hi = book - 1;                                   // the last centre with run0[c] <= r (centres without runs share the run0 of the next one)
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (run0[mid] <= r) lo = mid; else hi = mid - 1; }
  const int m0 = start[lo] + (r - run0[lo]) * kSumChunk, m1 = min(m0 + kSumChunk, start[lo + 1]);
  double s = 0.0;
  for (int m = m0; m < m1; ++m) s = s + (double)desc[(size_t)src[order[m]] * kDim + k];
  run_sum[(size_t)r * kDim + k] = s;
}

__global__ __launch_bounds__(128) void k_vlad_means(const double* __restrict__ run_sum, const int* __restrict__ run0, const int* __restrict__ start, float* __restrict__ codebook,
                                                    unsigned char* __restrict__ alive) {
  const int c = (int)blockIdx.x, k = (int)threadIdx.x;
  if (!alive[c]) return;                                       // uniform over the workgroup
  const int count = start[c + 1] - start[c];
  __syncthreads();
  if (count == 0) { if (k == 0) alive[c] = 0; codebook[(size_t)c * kDim + k] = 0.0f; return; }
  double total = 0.0;
  for (int r = run0[c]; r < run0[c + 1]; ++r) total = total + run_sum[(size_t)r * kDim + k];
  codebook[(size_t)c * kDim + k] = (float)(total / (double)count);
}

// type 2: nrm[i] = sqrt of the fp64 chain of the squared residual of row i against its centre
__global__ __launch_bounds__(256) void k_vlad_res_norm(const float* __restrict__ rows, const int* __restrict__ assign, const float* __restrict__ codebook, int n, double* __restrict__ nrm) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const float4* a = (const float4*)(rows + (size_t)i * kDim);
  const float4* b = (const float4*)(codebook + (size_t)assign[i] * kDim);
  double s = 0.0;
  for (int k = 0; k < kDim / 4; ++k) {
    const float4 x = a[k], y = b[k];
    double d = (double)(x.x - y.x); s = s + d * d;
    d = (double)(x.y - y.y); s = s + d * d;
    d = (double)(x.z - y.z); s = s + d * d;
    d = (double)(x.w - y.w); s = s + d * d;
  }
  nrm[i] = pvlm_vlad::sqrt_d(s);
}

// the ascending fp64 chain of the squares of sv[0..127] (every lane evaluates it: LDS broadcasts)
__device__ __forceinline__ double lds_sq_chain(const float* sv) {
  double s = 0.0;
  for (int k = 0; k < kDim; ++k) { const double d = (double)sv[k]; s = s + d * d; }
  return s;
}

// grid (book, frames of the batch): block c of frame f of the batch, and its square sum
__global__ __launch_bounds__(128) void k_vlad_blocks(const float* __restrict__ rows, const int* __restrict__ order, const int* __restrict__ start, const GSeg* __restrict__ segs,
                                                     const float* __restrict__ codebook, const double* __restrict__ nrm, int type, int book, float* __restrict__ vlad,
                                                     double* __restrict__ bsum) {
  __shared__ float sv[kDim];
  const int c = (int)blockIdx.x, f = (int)blockIdx.y, k = (int)threadIdx.x;
  const int* st = start + (size_t)f * (book + 1);
  const int seg0 = segs[f].i0, m0 = seg0 + st[c], m1 = seg0 + st[c + 1];
  const float cen = codebook[(size_t)c * kDim + k];
  float v = 0.0f;
  for (int m = m0; m < m1; ++m) {
    const int i = order[m];
    double n = 1.0;
    if (type == 2) { n = nrm[i]; if (n == 0.0) continue; }
    v += pvlm_vlad::residual_k(rows[(size_t)i * kDim + k], cen, type, n);
  }
  double bn = 0.0;
  if (type == 1) { sv[k] = v; __syncthreads(); bn = pvlm_vlad::sqrt_d(lds_sq_chain(sv)); __syncthreads(); }
  v = pvlm_vlad::block_step(v, type, bn);
  sv[k] = v;
  __syncthreads();
  const double s = lds_sq_chain(sv);
  vlad[((size_t)f * book + c) * kDim + k] = v;
  if (k == 0) bsum[(size_t)f * book + c] = s;
}

__global__ __launch_bounds__(256) void k_vlad_finish(float* __restrict__ vlad, const double* __restrict__ bsum, int book) {
  __shared__ double sN;
  const int f = (int)blockIdx.x;
  if (threadIdx.x == 0) { double t = 0.0; for (int c = 0; c < book; ++c) t = t + bsum[(size_t)f * book + c]; sN = pvlm_vlad::sqrt_d(t); }
  __syncthreads();
  const double N = sN;
  if (N == 0.0) return;
  float* v = vlad + (size_t)f * book * kDim;
  for (int k = (int)threadIdx.x; k < book * kDim; k += 256) v[k] = (float)((double)v[k] / N);
}

// grid (T, T), T = ceil(n / 32); the blocks below the diagonal leave at once.  D is a multiple of kSimK.
__global__ __launch_bounds__(256) void k_vlad_sim(const float* __restrict__ V, int n, int D, double* __restrict__ sim) {
  __shared__ float sA[kSimTile][kSimK + 1], sB[kSimTile][kSimK + 1];
  const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
  if (bj < bi) return;
  const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
  for (int k0 = 0; k0 < D; k0 += kSimK) {
    __syncthreads();
    for (int e = tid; e < kSimTile * kSimK; e += 256) {
      const int r = e / kSimK, k = e % kSimK, i = bi * kSimTile + r, j = bj * kSimTile + r;
      sA[r][k] = i < n ? V[(size_t)i * D + k0 + k] : 0.0f;
      sB[r][k] = j < n ? V[(size_t)j * D + k0 + k] : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < kSimK; ++k) {
      const double a0 = (double)sA[2 * ty][k], a1 = (double)sA[2 * ty + 1][k], b0 = (double)sB[2 * tx][k], b1 = (double)sB[2 * tx + 1][k];
      s00 = s00 + a0 * b0; s01 = s01 + a0 * b1; s10 = s10 + a1 * b0; s11 = s11 + a1 * b1;
    }
  }
  const int i0 = bi * kSimTile + 2 * ty, j0 = bj * kSimTile + 2 * tx;
  const double s[4] = {s00, s01, s10, s11};
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + (e >> 1), j = j0 + (e & 1);
    if (i >= n || j >= n) continue;
    sim[(size_t)i * n + j] = s[e];
    if (bi != bj) sim[(size_t)j * n + i] = s[e];               // a diagonal tile evaluates both (i, j) and (j, i): the same chain of the same exact products
  }
}

// a workgroup per row: frame j goes to place rank(j) = the number of frames before it in (-sim, index) order, when that is below m
__global__ __launch_bounds__(256) void k_vlad_select(const double* __restrict__ sim, int n, int m, int* __restrict__ out) {
  const double* s = sim + (size_t)blockIdx.x * n;
  for (int j = (int)threadIdx.x; j < n; j += 256) {
    const double sj = s[j];
    int rank = 0;
    for (int l = 0; l < n; ++l) rank += pvlm_vlad::sim_before(s[l], l, sj, j) ? 1 : 0;
    if (rank < m) out[(size_t)blockIdx.x * m + rank] = j;
  }
}

// `count` frames (list[k], or k itself without a list) cut into batches of whole frames: the first entry of every batch, and count behind the last
std::vector<int> make_batches(const pvlm_descset* set, int count, const int* list, long long* qcap, int* fcap) {
  const long long limit = pvlm_i_env_limit("PVLM_VLAD_BATCH_ROWS", kBatchRows);
  std::vector<int> first(1, 0);
  *qcap = 0; *fcap = 0;
  for (int p = 0; p < count;) {
    long long nq = 0; int k = p;
    while (k < count && k - p < kBatchFrames) {
      const long long r = set->rows[(size_t)(list ? list[k] : k)];
      if (k > p && nq + r > limit) break;
      nq += r; ++k;
    }
    *qcap = std::max(*qcap, nq); *fcap = std::max(*fcap, k - p);
    first.push_back(k); p = k;
  }
  return first;
}

// the alive centres packed in ascending order, on the host and on the device
struct PackedCentres {
  std::vector<float> rows, norm; std::vector<int> map; float nmax = 0.0f;
  void pack(const float* codebook, const unsigned char* alive, int book) {
    rows.clear(); norm.clear(); map.clear(); nmax = 0.0f;
    for (int c = 0; c < book; ++c) {
      if (alive && !alive[c]) continue;
      map.push_back(c); rows.insert(rows.end(), codebook + (size_t)c * kDim, codebook + (size_t)(c + 1) * kDim);
      norm.push_back(pvlm_matching::norm2(codebook + (size_t)c * kDim)); nmax = std::max(nmax, norm.back());
    }
  }
  int count() const { return (int)map.size(); }
};

// the scratch of the assignment and the grouping of one call
struct Scratch {
  PairDesc* d_pairs = nullptr; QTile* d_qt = nullptr; KnnRec* d_knn = nullptr; int2* d_fb = nullptr; int* d_cnt = nullptr;
  float* d_packed = nullptr; float* d_pnorm = nullptr; int* d_map = nullptr;
  GTile* d_tiles = nullptr; GSeg* d_segs = nullptr; int* d_hist = nullptr; int* d_start = nullptr; int* d_order = nullptr;
  void alloc(pvlm_call& c, size_t Q, size_t F, size_t rows_grouped, size_t segs, int book, bool exact) {
    d_pairs = c.alloc<PairDesc>(F);
    d_knn = c.alloc<KnnRec>(Q);
    if (!exact) { d_qt = c.alloc<QTile>(pvlm_match_launch::qtile_capacity(Q, F)); d_fb = c.alloc<int2>(Q); d_cnt = c.alloc<int>(2); }
    d_packed = c.alloc<float>((size_t)book * kDim);
    d_pnorm = c.alloc<float>((size_t)book);
    d_map = c.alloc<int>((size_t)book);
    const size_t NT = rows_grouped / kGroupTile + segs + 1;
    d_tiles = c.alloc<GTile>(NT);
    d_segs = c.alloc<GSeg>(segs);
    d_hist = c.alloc<int>(NT * (size_t)book);
    d_start = c.alloc<int>(segs * ((size_t)book + 1));
    d_order = c.alloc<int>(rows_grouped);
  }
};

void upload_packed(pvlm_call& c, const PackedCentres& P, Scratch& S) {
  c.h2d(S.d_packed, P.rows.data(), P.rows.size() * sizeof(float));
  c.h2d(S.d_pnorm, P.norm.data(), P.norm.size() * sizeof(float));
  c.h2d(S.d_map, P.map.data(), P.map.size() * sizeof(int));
}

// queues the assignment of frames list[k0 .. k1) (or k0 .. k1 themselves) against the packed centres: assign[q] for the batch's rows in order
void assign_batch(pvlm_call& c, const pvlm_descset* set, const int* list, int k0, int k1, const PackedCentres& P, Scratch& S, bool exact, int* d_assign, int* d_changed,
                  long long* nq_out, int* fallback) {
  std::vector<PairDesc> pd((size_t)(k1 - k0));
  long long nq = 0;
  for (int k = k0; k < k1; ++k) {
    const int f = list ? list[k] : k;
    PairDesc& D = pd[(size_t)(k - k0)];
    D.a = set->d_desc + set->row0[(size_t)f] * kDim; D.na = set->d_norm + set->row0[(size_t)f];
    D.b = S.d_packed; D.nb = S.d_pnorm;
    D.n1 = set->rows[(size_t)f]; D.n2 = P.count(); D.q0 = (int)nq; D.nbmax = P.nmax; D.tile0 = 0; D.n_tiles = 0;
    nq += D.n1;
  }
  *nq_out = nq;
  pvlm_match_launch::knn_batch(c, pd.data(), k1 - k0, nq, exact, S.d_pairs, S.d_qt, S.d_knn, S.d_fb, S.d_cnt, fallback);
  if (nq == 0) return;
  c.launch(k_vlad_take_assign, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, S.d_knn, S.d_map, (int)nq, d_assign, d_changed);
  c.check_launches();
}

// tiles and segments of `segs` runs of rows (n[s] rows each, one after the other from row 0)
void make_group(const std::vector<int>& n, std::vector<GTile>& tiles, std::vector<GSeg>& segs) {
  tiles.clear(); segs.clear();
  int i0 = 0;
  for (size_t s = 0; s < n.size(); ++s) {
    GSeg g{(int)tiles.size(), 0, i0, 0};
    for (int p = 0; p < n[s]; p += kGroupTile) tiles.push_back(GTile{i0 + p, std::min(kGroupTile, n[s] - p), (int)s, 0});
    g.n_tiles = (int)tiles.size() - g.tile0;
    segs.push_back(g); i0 += n[s];
  }
}

// queues the stable grouping of key[] (tiles / segments already on the device) into S.d_order and S.d_start
void group_rows(pvlm_call& c, const int* d_key, int n_tiles, int n_segs, int book, Scratch& S) {
  if (n_tiles > 0) c.launch(k_group_hist, dim3((unsigned)n_tiles), dim3(256), 0, d_key, S.d_tiles, book, S.d_hist);
  c.launch(k_group_scan, dim3((unsigned)n_segs), dim3(256), 0, S.d_hist, S.d_segs, book, S.d_start);
  if (n_tiles > 0) c.launch(k_group_scatter, dim3((unsigned)n_tiles), dim3(256), 0, d_key, S.d_tiles, S.d_hist, S.d_segs, S.d_start, book, S.d_order);
  c.check_launches();
}

}  // namespace

extern "C" pvlm_status pvlm_vlad_kmeans(pvlm_ctx* ctx, const pvlm_descset* set, int n_train, const int* train_frames, int book_size, int max_iterations,
                                        const long long* init_rows, unsigned flags, float* codebook, unsigned char* alive, int* assign_or_null, pvlm_vlad_stats* stats) {
  const char* who = "pvlm_vlad_kmeans";
  if (!ctx || !set || n_train < 0 || (n_train > 0 && !train_frames) || !init_rows || !codebook || !alive) return PVLM_ERR_ARG;
  if (stats) *stats = pvlm_vlad_stats{0, 0, 0, 0, 0};
  if (set->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the descriptor set belongs to another context", who); return PVLM_ERR_ARG; }
  if (book_size < 1 || book_size > pvlm_vlad::kMaxBook) { PVLM_SET_ERR(ctx, "%s: book_size %d outside [1, %d]", who, book_size, pvlm_vlad::kMaxBook); return PVLM_ERR_ARG; }
  if (max_iterations < 0) { PVLM_SET_ERR(ctx, "%s: max_iterations < 0", who); return PVLM_ERR_ARG; }
  std::vector<long long> tstart((size_t)n_train + 1, 0), trow0((size_t)std::max(n_train, 1), 0);
  for (int t = 0; t < n_train; ++t) {
    if (train_frames[t] < 0 || train_frames[t] >= set->n_frames) { PVLM_SET_ERR(ctx, "%s: train frame %d is outside the set", who, t); return PVLM_ERR_ARG; }
    tstart[(size_t)t + 1] = tstart[(size_t)t] + set->rows[(size_t)train_frames[t]]; trow0[(size_t)t] = set->row0[(size_t)train_frames[t]];
  }
  const long long N = tstart[(size_t)n_train];
  if ((long long)book_size > N) { PVLM_SET_ERR(ctx, "%s: %d centres for %lld training rows", who, book_size, N); return PVLM_ERR_ARG; }
  if (N >= (1ll << 31) - kGroupTile) { PVLM_SET_ERR(ctx, "%s: %lld training rows (below 2^31 are supported)", who, N); return PVLM_ERR_ARG; }
  for (int c = 0; c < book_size; ++c)
    if (init_rows[c] < 0 || init_rows[c] >= N) { PVLM_SET_ERR(ctx, "%s: init_rows[%d] is outside the training rows", who, c); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const bool exact = (flags & PVLM_FLAG_MATCH_EXACT) != 0;
  long long qcap = 0; int fcap = 0;
  const std::vector<int> first = make_batches(set, n_train, train_frames, &qcap, &fcap);
  const int n_batches = (int)first.size() - 1;
  const size_t max_runs = (size_t)(N / kSumChunk) + (size_t)book_size;
  std::vector<GTile> tiles; std::vector<GSeg> segs;
  make_group(std::vector<int>(1, (int)N), tiles, segs);
  Scratch S;
  S.alloc(c, (size_t)std::max<long long>(qcap, 1), (size_t)std::max(fcap, 1), (size_t)N, 1, book_size, exact);
  long long* d_tstart = c.alloc<long long>((size_t)n_train + 1);
  long long* d_trow0 = c.alloc<long long>((size_t)n_train);
  long long* d_src = c.alloc<long long>((size_t)N);
  long long* d_init = c.alloc<long long>((size_t)book_size);
  float* d_code = c.alloc<float>((size_t)book_size * kDim);
  unsigned char* d_alive = c.alloc<unsigned char>((size_t)book_size);
  int* d_assign = c.alloc<int>((size_t)N);
  int* d_changed = c.alloc<int>(1);
  int* d_run0 = c.alloc<int>((size_t)book_size + 1);
  double* d_runsum = c.alloc<double>(max_runs * kDim);
  if (c.st) return c.st;
  c.h2d(d_tstart, tstart.data(), ((size_t)n_train + 1) * sizeof(long long));
  c.h2d(d_trow0, trow0.data(), (size_t)n_train * sizeof(long long));
  c.h2d(d_init, init_rows, (size_t)book_size * sizeof(long long));
  c.h2d(S.d_tiles, tiles.data(), tiles.size() * sizeof(GTile));
  c.h2d(S.d_segs, segs.data(), sizeof(GSeg));
  c.memset(d_assign, 0, (size_t)N * sizeof(int));
  c.memset(d_alive, 1, (size_t)book_size);
  c.launch(k_vlad_train_rows, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, d_tstart, d_trow0, n_train, (int)N, d_src);
  c.launch(k_vlad_gather, dim3((unsigned)book_size), dim3(128), 0, set->d_desc, d_src, d_init, d_code);
  c.check_launches();
  c.d2h(codebook, d_code, (size_t)book_size * kDim * sizeof(float));
  if (c.sync()) return c.st;
  std::memset(alive, 1, (size_t)book_size);
  PackedCentres P;
  std::vector<int> fbs((size_t)std::max(n_batches, 1), 0);
  int changed = 1, iter = 0;
  long long queries = 0, fallback = 0;
  for (; iter < max_iterations && changed; ++iter) {
    P.pack(codebook, alive, book_size);
    upload_packed(c, P, S);
    c.memset(d_changed, 0, sizeof(int));
    for (int b = 0; b < n_batches && !c.st; ++b) {
      long long nq = 0;
      assign_batch(c, set, train_frames, first[(size_t)b], first[(size_t)b + 1], P, S, exact, d_assign + tstart[(size_t)first[(size_t)b]], d_changed, &nq, &fbs[(size_t)b]);
      queries += nq;
    }
    group_rows(c, d_assign, (int)tiles.size(), 1, book_size, S);
    c.launch(k_vlad_run_prefix, dim3(1), dim3(1), 0, S.d_start, book_size, d_run0);
    c.launch(k_vlad_run_sums, dim3((unsigned)max_runs), dim3(128), 0, set->d_desc, d_src, S.d_order, S.d_start, book_size, d_run0, d_runsum);
    c.launch(k_vlad_means, dim3((unsigned)book_size), dim3(128), 0, d_runsum, d_run0, S.d_start, d_code, d_alive);
    c.check_launches();
    c.d2h(codebook, d_code, (size_t)book_size * kDim * sizeof(float));
    c.d2h(alive, d_alive, (size_t)book_size);
    c.d2h(&changed, d_changed, sizeof(int));
    if (c.sync()) return c.st;
    for (int b = 0; b < n_batches; ++b) fallback += fbs[(size_t)b];
  }
  if (assign_or_null) { c.d2h(assign_or_null, d_assign, (size_t)N * sizeof(int)); if (c.sync()) return c.st; }
  if (stats) {
    stats->queries = queries; stats->fallback_queries = fallback; stats->iterations = iter; stats->batches = n_batches;
    for (int c = 0; c < book_size; ++c) stats->dead_centres += alive[c] ? 0 : 1;
  }
  return PVLM_OK;
}

extern "C" void pvlm_vladset_destroy(pvlm_ctx* ctx, pvlm_vladset* vs) {
  if (!ctx || !vs) return;
  pvlm_i_free(vs->owner, vs->d_vlad);
  delete vs;
}

extern "C" pvlm_status pvlm_vlad_embed(pvlm_ctx* ctx, const pvlm_descset* set, int book_size, const float* codebook, const unsigned char* alive_or_null, int normalization,
                                       unsigned flags, pvlm_vladset** out, pvlm_vlad_stats* stats) {
  const char* who = "pvlm_vlad_embed";
  if (!ctx || !set || !codebook || !out) return PVLM_ERR_ARG;
  *out = nullptr;
  if (stats) *stats = pvlm_vlad_stats{0, 0, 0, 0, 0};
  if (set->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the descriptor set belongs to another context", who); return PVLM_ERR_ARG; }
  if (book_size < 1 || book_size > pvlm_vlad::kMaxBook) { PVLM_SET_ERR(ctx, "%s: book_size %d outside [1, %d]", who, book_size, pvlm_vlad::kMaxBook); return PVLM_ERR_ARG; }
  if (normalization < 0 || normalization > 2) { PVLM_SET_ERR(ctx, "%s: normalization %d", who, normalization); return PVLM_ERR_ARG; }
  for (int c = 0; c < book_size; ++c)
    if (!alive_or_null || alive_or_null[c])
      for (int k = 0; k < kDim; ++k)
        if (!std::isfinite(codebook[(size_t)c * kDim + k])) { PVLM_SET_ERR(ctx, "%s: centre %d has a value that is not finite", who, c); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const bool exact = (flags & PVLM_FLAG_MATCH_EXACT) != 0;
  const int F = set->n_frames;
  const size_t D = (size_t)book_size * kDim;
  PackedCentres P;
  P.pack(codebook, alive_or_null, book_size);
  long long qcap = 0; int fcap = 0;
  const std::vector<int> first = make_batches(set, F, nullptr, &qcap, &fcap);
  const int n_batches = (int)first.size() - 1;
  pvlm_vladset* vs = new pvlm_vladset();
  vs->owner = ctx; vs->n_frames = F; vs->book_size = book_size;
  c.st = pvlm_i_alloc(ctx, &vs->d_vlad, (size_t)F * D);       // the set's own block: it outlives the call, pvlm_vladset_destroy frees it
  long long queries = 0, fallback = 0;
  const size_t Q = (size_t)std::max<long long>(qcap, 1), FB = (size_t)std::max(fcap, 1);
  Scratch S;
  S.alloc(c, Q, FB, Q, FB, book_size, exact);
  float* d_code = c.upload(codebook, D);
  int* d_assign = c.alloc<int>(Q);
  double* d_nrm = c.alloc<double>(Q);
  double* d_bsum = c.alloc<double>(FB * (size_t)book_size);
  if (P.count() > 0) upload_packed(c, P, S);
  else c.memset(vs->d_vlad, 0, (size_t)F * D * sizeof(float));
  std::vector<int> fbs((size_t)std::max(n_batches, 1), 0), n; std::vector<GTile> tiles; std::vector<GSeg> segs;
  for (int b = 0; b < n_batches && !c.st && P.count() > 0; ++b) {
    const int f0 = first[(size_t)b], f1 = first[(size_t)b + 1], nf = f1 - f0;
    long long nq = 0;
    // the descriptor set keeps the frames one after the other, so the batch's rows are one range
    const float* rows = set->d_desc + set->row0[(size_t)f0] * kDim;
    c.memset(d_assign, 0xff, Q * sizeof(int));
    assign_batch(c, set, nullptr, f0, f1, P, S, exact, d_assign, nullptr, &nq, &fbs[(size_t)b]);
    queries += nq;
    n.assign(set->rows.begin() + f0, set->rows.begin() + f1);
    make_group(n, tiles, segs);
    c.h2d(S.d_tiles, tiles.data(), tiles.size() * sizeof(GTile));
    c.h2d(S.d_segs, segs.data(), segs.size() * sizeof(GSeg));
    group_rows(c, d_assign, (int)tiles.size(), nf, book_size, S);
    if (normalization == 2 && nq > 0) c.launch(k_vlad_res_norm, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, rows, d_assign, d_code, (int)nq, d_nrm);
    c.launch(k_vlad_blocks, dim3((unsigned)book_size, (unsigned)nf), dim3(128), 0, rows, S.d_order, S.d_start, S.d_segs, d_code, d_nrm, normalization, book_size,
             vs->d_vlad + (size_t)f0 * D, d_bsum);
    c.launch(k_vlad_finish, dim3((unsigned)nf), dim3(256), 0, vs->d_vlad + (size_t)f0 * D, d_bsum, book_size);
    c.check_launches();
  }
  if (c.sync()) { pvlm_vladset_destroy(ctx, vs); return c.st; }
  for (int b = 0; b < n_batches; ++b) fallback += fbs[(size_t)b];
  if (stats) { stats->queries = queries; stats->fallback_queries = fallback; stats->batches = n_batches; stats->dead_centres = book_size - P.count(); }
  *out = vs;
  return PVLM_OK;
}

extern "C" pvlm_status pvlm_vladset_read(pvlm_ctx* ctx, const pvlm_vladset* vs, float* out) {
  if (!ctx || !vs || !out) return PVLM_ERR_ARG;
  if (vs->owner != ctx) { PVLM_SET_ERR(ctx, "pvlm_vladset_read: the set belongs to another context"); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, "pvlm_vladset_read");
  if (c.enter()) return c.st;
  if (vs->n_frames == 0) return PVLM_OK;
  c.d2h(out, vs->d_vlad, (size_t)vs->n_frames * vs->book_size * kDim * sizeof(float));
  return c.sync();
}

extern "C" pvlm_status pvlm_vlad_neighbors(pvlm_ctx* ctx, const pvlm_vladset* vs, int neighbor_size, int* neighbors, double* sim_or_null) {
  const char* who = "pvlm_vlad_neighbors";
  if (!ctx || !vs || !neighbors) return PVLM_ERR_ARG;
  if (vs->owner != ctx) { PVLM_SET_ERR(ctx, "%s: the set belongs to another context", who); return PVLM_ERR_ARG; }
  if (neighbor_size < 1) { PVLM_SET_ERR(ctx, "%s: neighbor_size < 1", who); return PVLM_ERR_ARG; }
  pvlm_call c(ctx, who);
  if (c.enter()) return c.st;
  const int n = vs->n_frames, m = std::min(neighbor_size, n), D = vs->book_size * kDim;
  if (n == 0) return PVLM_OK;
  double* d_sim = c.alloc<double>((size_t)n * n);
  int* d_nb = c.alloc<int>((size_t)n * m);
  const unsigned T = (unsigned)((n + kSimTile - 1) / kSimTile);
  c.launch(k_vlad_sim, dim3(T, T), dim3(256), 0, vs->d_vlad, n, D, d_sim);
  c.launch(k_vlad_select, dim3((unsigned)n), dim3(256), 0, d_sim, n, m, d_nb);
  c.check_launches();
  c.d2h(neighbors, d_nb, (size_t)n * m * sizeof(int));
  if (sim_or_null) c.d2h(sim_or_null, d_sim, (size_t)n * n * sizeof(double));
  return c.sync();
}

// pvlm_preload: loads this file's code object at context set-up instead of at the first call (see pvlm_ba.hip)
__global__ void k_preload_vlad() {}
void pvlm_i_preload_vlad(hipStream_t s) { hipLaunchKernelGGL(k_preload_vlad, dim3(1), dim3(1), 0, s); }
