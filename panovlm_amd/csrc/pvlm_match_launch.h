// The launch core of K33's two search stages (pvlm_match.hip), shared with K35 (pvlm_vlad.hip): the 2-NN of every query of a batch of (query rows, train rows)
// pairs by the definition of pvlm_match_core.h.  A pair names its rows by device address, so the train rows may lie outside a descriptor set (K35: the packed
// alive centres of a codebook).
#pragma once
#include "pvlm_internal.h"

namespace pvlm_match_launch {

struct PairDesc {
  const float* a; const float* b; const float* na; const float* nb;     // query rows, train rows, their norm2 (pvlm_matching::norm2)
  int n1, n2, q0; float nbmax;                                          // rows, the first query's place in the batch, an upper bound of nb[]
  int tile0, n_tiles;
};
struct QTile { int pair, q0; };               // a block of queries of one pair (the screening kernel's block size), first query q0
struct KnnRec { int i0, i1; float d0, d1; };  // squared distances

// the QTile entries d_qt must hold for a batch of at most `queries` queries in at most `pairs` pairs
size_t qtile_capacity(size_t queries, size_t pairs);
// Queues the search of one batch through the caller's frame: pd (np pairs, q0 ascending, nq queries in all) is copied to d_pairs; exact: the definition for every
// (query, train row); otherwise every pair is cut into blocks of queries (d_qt: qtile_capacity entries), every query is screened on the matrix core and the
// uncertified ones are evaluated exactly (d_fb: nq entries, d_cnt: 2 ints).  knn[P.q0 + q] is the result of query q of pair P.  *fallback is a staged copy: it holds
// the number of exactly evaluated queries after the frame's next sync() (exact mode: set to nq at once).  Checks the launches; an error stays in the frame.
void knn_batch(pvlm_call& c, const PairDesc* pd, int np, long long nq, bool exact, PairDesc* d_pairs, QTile* d_qt, KnnRec* d_knn, int2* d_fb, int* d_cnt, int* fallback);
// norm[i] = pvlm_matching::norm2 of row i of desc (n_rows x 128), *bad |= 1 when a value is not finite; queued, the launch checked
void row_norms(pvlm_call& c, const float* desc, long long n_rows, float* norm, int* bad);

}  // namespace pvlm_match_launch
