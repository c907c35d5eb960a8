// vaq_bitvec_naive.h -- the exact cluster form of the Hamming engine (BitVecEngine::queryNaiveWithClusterInfo with
// QueryMethod::Sort, BitVecEngine.cpp:875-918): the visiting plan of the cluster form (vaq_bitvec_clusters.h), then
// euclideanDistNoSQRT of the query to EVERY member of the visited clusters over the refiner's raw rows, and
// KNNFromDistsIndicesSupplied over those float distances.  No bit row is read.  DESIGN.md section 4h, "Exact cluster
// form", has the rules, the layout and the LDS budget.
#ifndef VAQ_BITVEC_NAIVE_H_
#define VAQ_BITVEC_NAIVE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_bitvec_clusters.h"

namespace vaq {

// (the chunk of a tile, BITVEC_EXACT_DC dimensions, is vaq_bitvec_tile.h's)
constexpr int BITVEC_EXACT_POOL = 2048;  // (key, row) slots of the selection pool: VAQHIP_MAX_K + a tile, a power of two

// Per query the candidates are the members of the first plan.visit clusters of its visit list, cluster after cluster,
// each in ascending row order (image row g = start[c] ..; raw row member[g]).  Candidate p has the distance
// euclideanDistNoSQRT(query, rows[member[g]]): one accumulator from 0.0f, distance += (a - b) * (a - b) in dimension
// order, the subtraction, the product and the addition apart (a byte row is widened where it is loaded).  The
// kk = min(k, candidates) smallest by (dist, seq) are written, seq being the slot std::sort (rerank_sort, over the
// (dist, idx) pairs in candidate order) leaves p at for p < kk and p itself behind: labels = member[g] + id_base, the
// squared distances; slots kk .. k - 1 are -1 / FLT_MAX.  The distances are computed once and never stored.
// visit is [nq][T], plan [nq] (launch_bitvec_cluster_plan's; plan.cand is not read, the walk counts for itself).
// 1 <= D <= BITVEC_CLUSTERS_MAX_DIM, 1 <= T <= BITVEC_CLUSTERS_MAX, 1 <= k <= BITVEC_RERANK_MAX, rows.elem 4 or 1.
hipError_t launch_bitvec_cluster_exact_select(const float *queries, int nq, int D, RowsRef rows, int64_t N,
                                              const int32_t *start, const int32_t *member, int T, const int32_t *visit,
                                              const BitvecClusterPlan *plan, int k, int64_t id_base, int32_t *labels,
                                              float *out_dist, hipStream_t st);

}  // namespace vaq
#endif  // VAQ_BITVEC_NAIVE_H_
