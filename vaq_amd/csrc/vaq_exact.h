// vaq_exact.h -- the reference's own choice among rows of equal distance (vaq_exact.hip, option "exact_ties"), on
// bucketed indexes and, with the walk vaq_ti.h builds, on TI indexes.
#ifndef VAQ_EXACT_H_
#define VAQ_EXACT_H_

#include "vaq_common.h"

namespace vaq {

// inv[original row] = row of the bucketed order; row_bucket (optional): [original row] = its bucket
hipError_t launch_inverse_perm(const uint32_t *perm, int64_t n, uint32_t *inv, const int *bucket_start, int n_buckets,
                               unsigned short *row_bucket, hipStream_t st);
// int32 words of one list entry's state in a chain over shards (ExactParams::chain)
__host__ __device__ inline int exact_state_words(int k, int seq) { return seq ? 2 * (k + 1) + 2 : 2 * k; }
// The flag step, also on the MERGED k + 1 list of a multi-device index (vaqhip_multi_search.cpp).  in_labels / in_dist:
// the scan's result for k + 1 per query (labels carry id_base); labels / dist: the caller's k per query.  Queries
// whose k + 1 smallest distances are distinct are copied; the others are listed for the replay.  list: [nq] ints,
// count: one word, zeroed first.
hipError_t launch_exact_flag(int nq, int k, const int32_t *in_labels, const float *in_dist, int32_t *labels, float *dist,
                             int *list, unsigned *count, hipStream_t st);
// The replay of the listed queries through the reference's heap in original row order: the index, and what one
// launch is to do with it
struct ExactParams {
  const uint32_t *codes;
  int layout, M, W;
  const SubDesc *sub;
  const uint32_t *inv;  // original row -> row of the bucketed order (nullptr = identity)
  const unsigned short *row_bucket;  // original row -> its bucket (nullptr: no bucket pruning)
  int n_buckets, bucket_shift, bucket_t;
  int64_t n_rows;
  const float *lut;     // [nq][lut_floats], indexed by the listed query
  int lut_floats;
  int lut_in_lds;       // (set by the launch)
  int seq;              // the index sums sequentially -- the heap is BitVecEngine::queryLUT's (std::push_heap / pop_heap /
                        // sort_heap over k + 1 pairs) instead of VAQ::searchHeap's
  int k;
  int64_t id_base;
  int32_t *labels;           // [nq][k] (not in a chain)
  float *dist;
  const int *list;           // [nq] queries to replay
  const unsigned *count;
  // one link of a chain over shards (0: the single-index replay).  Entry e of the list keeps its heap at
  // state[e * 2 * k]: k values, then k ids (global row numbers: id_base + row, -1 = neutral).  Sequential sum: at
  // state[e * exact_state_words(k, 1)]: k + 1 values, k + 1 ids, the heap's length, bsfK.
  int chain;
  int64_t row0;              // sequential sum: position in the whole database of this index's row 0 (queryLUT's
                             // `dataIndex >= k` counts from there)
  int e0;                    // the launch covers list entries e0 .. e0 + n_entries - 1 (those beyond *count exit at once)
  const int32_t *state_in;   // nullptr: the neutral state (first shard)
  int32_t *state_out;
};
// single index (chain == 0): the listed queries' slots of labels / dist are written.  A link: the raw heap goes
// from state_in to state_out ...
hipError_t launch_exact_replay(const ExactParams &p, int n_entries, hipStream_t st);
// ... and the chain's end: heap_reorder (seq: std::sort_heap) on the last state into the listed queries' slots of
// labels / dist [.][k]
hipError_t launch_exact_finish(const int32_t *state, const int *list, const unsigned *count, int n_entries, int seq, int k,
                               int32_t *labels, float *dist, hipStream_t st);

// On a TI index: VAQ::searchTriangleInequality (VAQ.cpp:1540-1692) replayed statement for statement, one workgroup
// per query, over the walk of ti_build_walk and the plan of launch_ti_plan(exact = 1) (vaq_ti.h).  ea: the method
// includes EA.  Labels are id_base + original row, unfilled slots -1 / FLT_MAX.
struct TiExactParams {
  ExactParams x;  // codes, layout, M, W, sub, lut, lut_floats, lut_in_lds, k, id_base, labels, dist
  const uint32_t *perm;  // index row -> original row
  const uint32_t *walk;  // position in the reference's member order -> index row
  const int *start;      // [T + 1] first index row of each cluster
  const float *xcc;      // mCodeToCCDist by index row
  int T;
  const int *order;      // [nq][T]
  const float *qcc;      // [nq][T], in `order`'s order
  const int *nvisit;     // [nq]
  int ea;
};
hipError_t launch_ti_exact_replay(const TiExactParams &p, int nq, hipStream_t st);

} // namespace vaq
#endif
