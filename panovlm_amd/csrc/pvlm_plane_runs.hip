// The plane-run table of a point-to-plane residual set (pvlm_resset::plane_runs): the two passes that build it when the set is finalised
// (k_plane_run_count, k_plane_run_write, with pvlm_compact::k_tile_scan between them) and the decision which sets get it.  The fused kernels that read
// the table are in pvlm_eval.hip.
#include <string>
#include <vector>

#include "pvlm_compact.h"
#include "pvlm_dispatch_core.h"
#include "pvlm_internal.h"

// The plane of a point-to-plane row is fitted to the query's 10 nearest targets; neighbouring queries of a ring very often have the same ten, and then
// the four plane doubles are bit-identical.  Per work-list entry (pair, chunk) a row starts a new run when it is the chunk's first row or when any of its
// four plane words differs from the previous row's (compared as 64-bit integers: -0.0 is not +0.0, a NaN equals only its own bit pattern).  Two passes on
// the context stream: runs per chunk (k_plane_run_count), an exclusive scan over the chunks (pvlm_compact::k_tile_scan), then the run number of every
// row and the table (k_plane_run_write).
namespace {
struct PlaneScanItem { int tile0, n_tiles; };       // the descriptor type k_tile_scan wants; no per-item totals are asked for

struct PlaneChunk { const unsigned long long* pl; int64_t nd, lo, hi; int p; };
__device__ __forceinline__ PlaneChunk plane_chunk(const double* const* pair_cols, const int64_t* pair_stride, const int64_t* out_start,
                                                  const int* blk_pair, const int* blk_chunk, int chunk_rows) {
  PlaneChunk c;
  c.p = blk_pair[blockIdx.x];
  c.nd = pair_stride[c.p];
  c.pl = reinterpret_cast<const unsigned long long*>(pair_cols[c.p] + 3 * c.nd);    // columns 3..6: a, b, c, d
  const int64_t len = out_start[c.p + 1] - out_start[c.p];
  c.lo = (int64_t)blk_chunk[blockIdx.x] * chunk_rows;
  c.hi = min(len, c.lo + (int64_t)chunk_rows);
  return c;
}
// row j of the chunk (lo <= j < hi): its plane words, and whether it starts a run
__device__ __forceinline__ bool plane_run_starts(const PlaneChunk& c, int64_t j, unsigned long long (&w)[4]) {
  bool differs = j == c.lo;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = c.pl[k * c.nd + j];
    if (j > c.lo) differs |= w[k] != c.pl[k * c.nd + j - 1];
  }
  return differs;
}

__global__ __launch_bounds__(pvlm_compact::kThreads) void k_plane_run_count(const double* const* __restrict__ pair_cols, const int64_t* __restrict__ pair_stride,
                                                                            const int64_t* __restrict__ out_start, const int* __restrict__ blk_pair,
                                                                            const int* __restrict__ blk_chunk, int chunk_rows, int* __restrict__ run_count) {
  const PlaneChunk c = plane_chunk(pair_cols, pair_stride, out_start, blk_pair, blk_chunk, chunk_rows);
  int n = 0;
  unsigned long long w[4];
  for (int64_t j = c.lo + threadIdx.x; j < c.hi; j += pvlm_compact::kThreads) n += plane_run_starts(c, j, w) ? 1 : 0;
  pvlm_compact::tile_total(n, run_count);
}

__global__ __launch_bounds__(pvlm_compact::kThreads) void k_plane_run_write(const double* const* __restrict__ pair_cols, const int64_t* __restrict__ pair_stride,
                                                                            const int64_t* __restrict__ out_start, const int* __restrict__ blk_pair,
                                                                            const int* __restrict__ blk_chunk, int chunk_rows,
                                                                            const int64_t* __restrict__ chunk_plane0, const int64_t* __restrict__ pair_idx0,
                                                                            uint16_t* __restrict__ plane_idx, double* __restrict__ plane_tab,
                                                                            const uint16_t* const* __restrict__ pair_q16) {
  const PlaneChunk c = plane_chunk(pair_cols, pair_stride, out_start, blk_pair, blk_chunk, chunk_rows);
  // pair_q16 (the point table, pvlm_resset::point_table): the pair's query numbers go in beside the run numbers, one 32-bit word per row
  // {run, query} (low, high half: k_eval_fused loads a row's word whole); without it one 16-bit word per row
  const uint16_t* q16 = pair_q16 ? pair_q16[c.p] : nullptr;
  uint16_t* idx = plane_idx + (q16 ? 2 : 1) * pair_idx0[c.p];                                    // indexed by the row inside the pair
  ulonglong2* tab = reinterpret_cast<ulonglong2*>(plane_tab) + 2 * chunk_plane0[blockIdx.x];    // two 16-byte halves per entry
  __shared__ int wave_runs[pvlm_compact::kWaves];
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  int carry = 0;                                             // runs begun in the rows before this round's
  for (int64_t base = c.lo; base < c.hi; base += pvlm_compact::kThreads) {
    const int64_t j = base + threadIdx.x;
    unsigned long long w[4];
    const bool starts = j < c.hi && plane_run_starts(c, j, w);
    const unsigned long long m = __ballot(starts);
    const int upto = __popcll(m & (~0ull >> (63 - lane)));    // runs begun in this wave's rows up to and including mine
    if (lane == 0) wave_runs[wv] = __popcll(m);
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int k = 0; k < pvlm_compact::kWaves; ++k) { const int t = wave_runs[k]; before += k < wv ? t : 0; all += t; }
    if (j < c.hi) {
      const int run = before + upto - 1;                       // >= 0: the chunk's first row starts a run; < chunk_rows <= 65536 (pvlm_i_plane_runs_build)
      if (q16) reinterpret_cast<uint32_t*>(idx)[j] = (uint32_t)run | ((uint32_t)q16[j] << 16);      // idx is 4-byte aligned: 2 * pair_idx0 words into an allocation
      else idx[j] = (uint16_t)run;
      if (starts) { tab[2 * run] = make_ulonglong2(w[0], w[1]); tab[2 * run + 1] = make_ulonglong2(w[2], w[3]); }
    }
    carry += all;
    __syncthreads();
  }
}
}  // namespace

// By bytes the table wins once the mean run length L exceeds 16/15 (24 + 2 + 32 / L < 56).  Measured on the BLOCK form, k_eval_fused (tools/plane_runs_sweep.py:
// 50 M uploaded rows in 32 pairs, Angle + Huber, fused kernel by HIP events; profiles/plane_runs_ab.txt): the table loses at L = 1 and wins at 1.25, 1.5 and 2.
// The lowest run length at which it was seen to win is the threshold; between 16/15 and 1.25 nothing was measured.  The headline batch has L = 1.74.
// Sets that take the WAVE form (pvlm_resset::wave_units: many short segments) keep the seven columns unless PVLM_PLANE_RUNS=1 asks for the table: see
// profiles/plane_runs_ab.txt for what is known about k_eval_fused_wave on the table.
static const double kPlaneRunsMinMean = 1.25;

// Counts the runs, decides (PVLM_PLANE_RUNS=0/1 forces the choice, like PVLM_WAVE_UNITS: A/B runs and the tests) and builds d_plane_idx / d_plane_tab /
// d_chunk_plane0 / d_pair_idx0.  Called by pvlm_i_resset_finalize behind its queued copies of the work list.  A set that cannot have its table (no memory)
// keeps the 7-column path: only a failure of the stream itself is an error.
static pvlm_status plane_runs_build(pvlm_ctx* ctx, pvlm_resset* rs, int64_t padded_rows) {
  rs->plane_runs = false;
  rs->point_table = false;
  rs->half_rotate = false;
  if (rs->ncols != 7 || rs->n_blocks == 0 || rs->chunk_rows > 65536) return PVLM_OK;     // a run number is 16 bits (PVLM_WAVE_CHUNK can ask for longer chunks)
  int force = -1;
  if (const char* env = getenv("PVLM_PLANE_RUNS")) force = atoi(env) != 0;
  if (force == 0 || (force < 0 && rs->wave_units)) return PVLM_OK;
  const int P = rs->n_pairs, nb = rs->n_blocks;
  std::string kept_err = ctx->err;
  auto give_up = [&]() {                      // the set keeps the 7-column path
    pvlm_i_free(ctx, rs->d_plane_idx); pvlm_i_free(ctx, rs->d_plane_tab); pvlm_i_free(ctx, rs->d_chunk_plane0); pvlm_i_free(ctx, rs->d_pair_idx0);
    pvlm_i_free(ctx, rs->d_pair_ptab); rs->d_pair_ptab = nullptr;
    rs->d_plane_idx = nullptr; rs->d_plane_tab = nullptr; rs->d_chunk_plane0 = nullptr; rs->d_pair_idx0 = nullptr;
    ctx->err = kept_err;
    return PVLM_OK;
  };
  pvlm_dev_scratch scratch(ctx);
  int* d_count = nullptr; long long* d_total = nullptr;
  if (scratch.alloc(&d_count, (size_t)nb) || scratch.alloc(&d_total, 1) || pvlm_i_alloc(ctx, &rs->d_chunk_plane0, (size_t)nb)) return give_up();
  static_assert(sizeof(long long) == sizeof(int64_t), "k_tile_scan writes the chunk bases as long long");
  hipLaunchKernelGGL(k_plane_run_count, dim3(nb), dim3(pvlm_compact::kThreads), 0, ctx->stream, rs->d_pair_cols, rs->d_pair_stride, rs->d_out_start,
                     rs->d_blk_pair, rs->d_blk_chunk, rs->chunk_rows, d_count);
  hipLaunchKernelGGL((pvlm_compact::k_tile_scan<PlaneScanItem>), dim3(1), dim3(pvlm_compact::kScanThreads), 0, ctx->stream, d_count, nb,
                     reinterpret_cast<long long*>(rs->d_chunk_plane0), (const PlaneScanItem*)nullptr, 0, d_total, (long long*)nullptr);
  PVLM_HIP(ctx, hipGetLastError());
  long long total = 0;
  pvlm_status st = pvlm_i_d2h(ctx, &total, d_total, sizeof(total));       // waits: the table's size decides the path and its allocation
  if (st) return st;
  rs->n_plane_runs = total;
  auto mark = [&](const char* what) {           // PVLM_TRACE: the time since the previous mark is the count pass / the table build
    char label[200];
    snprintf(label, sizeof(label), "plane runs %s: %lld rows, %lld runs, pool %.3f GB in use of %.3f GB, %llu hipMalloc", what, (long long)rs->n, total,
             ctx->pool.in_use / 1e9, ctx->pool.reserved / 1e9, (unsigned long long)ctx->pool.device_allocs);
    pvlm_i_trace(label);
  };
  mark("counted");
  if (total <= 0 || (force < 0 && (double)rs->n < kPlaneRunsMinMean * (double)total)) return give_up();
  std::vector<int64_t> pair_idx0((size_t)P);
  int64_t o = 0;
  for (int p = 0; p < P; ++p) { pair_idx0[(size_t)p] = o; o += pvlm_i_seg_rows(rs->h_out_start[(size_t)p + 1] - rs->h_out_start[(size_t)p]); }
  // The point table: a set of the association (tables and query numbers are there), block form.  PVLM_POINT_TABLE=1 cannot force it onto a set that lacks
  // them (uploaded, compacted, a neighbour of more than 65 536 queries) or onto the wave form; =0 kept the association from making them.
  bool pt = rs->d_point_tab != nullptr && !rs->wave_units && rs->d_q16.size() == rs->col_blocks.size();
  const uint16_t** d_pair_q16 = nullptr;
  if (pt && (scratch.alloc(&d_pair_q16, (size_t)P) || pvlm_i_alloc(ctx, &rs->d_pair_ptab, (size_t)P))) { pt = false; ctx->err = kept_err; }
  if (pvlm_i_alloc(ctx, &rs->d_pair_idx0, (size_t)P) || pvlm_i_alloc(ctx, &rs->d_plane_idx, (size_t)padded_rows * (pt ? 2 : 1)) ||
      pvlm_i_alloc(ctx, &rs->d_plane_tab, (size_t)total * 4))
    return give_up();
  std::vector<const uint16_t*> pair_q16;
  std::vector<const double*> pair_ptab;
  if (pt) {
    pair_q16.resize((size_t)P); pair_ptab.resize((size_t)P);
    for (int p = 0; p < P; ++p) {
      pair_q16[(size_t)p] = rs->d_q16[(size_t)rs->h_pair_block[(size_t)p]] + rs->h_seg_start[(size_t)p];
      pair_ptab[(size_t)p] = rs->d_point_tab + (size_t)rs->h_pair_tab[(size_t)p] * 3 * PVLM_POINT_TAB_STRIDE;
    }
    if ((st = pvlm_i_h2d_q(ctx, d_pair_q16, pair_q16.data(), (size_t)P * sizeof(uint16_t*)))) return st;
    if ((st = pvlm_i_h2d_q(ctx, rs->d_pair_ptab, pair_ptab.data(), (size_t)P * sizeof(double*)))) return st;
  }
  if ((st = pvlm_i_h2d_q(ctx, rs->d_pair_idx0, pair_idx0.data(), (size_t)P * sizeof(int64_t)))) return st;
  // a lane of k_eval_fused_wave loads the run numbers of its TWO rows at once: the pad row behind an odd last row must name an entry that exists (0).
  // k_eval_fused loads one word per row and none for a pad row: the {run, query} words of a set on the point table, which only it reads, need no such fill.
  if (!pt) PVLM_HIP(ctx, hipMemsetAsync(rs->d_plane_idx, 0, (size_t)padded_rows * sizeof(uint16_t), ctx->stream));
  hipLaunchKernelGGL(k_plane_run_write, dim3(nb), dim3(pvlm_compact::kThreads), 0, ctx->stream, rs->d_pair_cols, rs->d_pair_stride, rs->d_out_start,
                     rs->d_blk_pair, rs->d_blk_chunk, rs->chunk_rows, rs->d_chunk_plane0, rs->d_pair_idx0, rs->d_plane_idx, rs->d_plane_tab,
                     (const uint16_t* const*)d_pair_q16);
  PVLM_HIP(ctx, hipGetLastError());
  if ((st = pvlm_i_sync(ctx))) return st;           // pair_idx0 goes out of scope
  rs->plane_runs = true;
  rs->point_table = pt;
  rs->half_rotate = PVLM_HALF_ROTATE != 0;
  if (const char* env = getenv("PVLM_HALF_ROTATE")) rs->half_rotate = atoi(env) != 0;      // like PVLM_PLANE_RUNS: A/B runs and the tests
  mark("table built");
  return PVLM_OK;
}

// The order in which the grid of k_eval_fused visits the work list of a set on the point table (pvlm_dispatch_core.h); PVLM_DISPATCH_ORDER=0: the identity
// (no table).  Speed only: without memory for it the set runs in work-list order.
static pvlm_status dispatch_order_build(pvlm_ctx* ctx, pvlm_resset* rs) {
  rs->n_positions = rs->n_blocks;
  if (const char* env = getenv("PVLM_DISPATCH_ORDER")) if (atoi(env) == 0) return PVLM_OK;
  std::vector<int64_t> key((size_t)rs->n_blocks);
  for (int p = 0; p < rs->n_pairs; ++p)
    for (int b = rs->h_pair_blk_start[(size_t)p]; b < rs->h_pair_blk_start[(size_t)p + 1]; ++b)
      key[(size_t)b] = pvlm_dispatch::group_key(rs->h_pair_tab[(size_t)p], b - rs->h_pair_blk_start[(size_t)p]);
  std::vector<int> pos;
  pvlm_dispatch::build_order(rs->n_blocks, key.data(), pos);
  const std::string kept_err = ctx->err;
  if (pvlm_i_alloc(ctx, &rs->d_order, pos.size())) { rs->d_order = nullptr; ctx->err = kept_err; return PVLM_OK; }
  pvlm_status st = pvlm_i_h2d_q(ctx, rs->d_order, pos.data(), pos.size() * sizeof(int));
  if (!st) st = pvlm_i_sync(ctx);                    // pos goes out of scope
  if (!st) rs->n_positions = (int)pos.size();
  return st;
}

pvlm_status pvlm_i_plane_runs_build(pvlm_ctx* ctx, pvlm_resset* rs, int64_t padded_rows) {
  pvlm_status st = plane_runs_build(ctx, rs, padded_rows);
  // what only the making of the set needed: the per-block query numbers (now beside the run numbers) and, for a set that does not take the form, the tables
  for (uint16_t* b : rs->d_q16) pvlm_i_free(ctx, b);
  rs->d_q16.clear();
  if (!rs->point_table) { pvlm_i_free(ctx, rs->d_point_tab); rs->d_point_tab = nullptr; rs->n_point_tabs = 0; }
  if (!st && rs->point_table) st = dispatch_order_build(ctx, rs);
  return st;
}
