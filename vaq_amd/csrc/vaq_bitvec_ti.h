// vaq_bitvec_ti.h -- exact k nearest neighbours over raw rows with triangle-inequality pruning
// (BitVecEngine::computeTriangleInequalityClusters, BitVecEngine.hpp:1036-1088, and ::queryNaiveTriangleInequality,
// BitVecEngine.cpp:722-873, QueryMethod::Heap).  The answer is the exhaustive one; the centres only decide which rows
// are never loaded.  DESIGN.md section 4h, "Triangle-inequality form", has the rules, the slack and the LDS budget.
#ifndef VAQ_BITVEC_TI_H_
#define VAQ_BITVEC_TI_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_bitvec_clusters.h"

namespace vaq {

constexpr int BITVEC_TI_POOL = 2048;  // key slots of the selection pool: VAQHIP_MAX_K + a tile of 256, a power of two
// admissions since the last compaction that make the next tile compact first (the threshold tightens); the pool's
// overflow compacts whatever this says.  profiles/bitvec_naive_ti_1m.json has what was tried.
constexpr int BITVEC_TI_REFRESH = 1;

// The relative slack of a centre bound: the distances qcc, xcc and d(q, x) are each sqrtf of a float sum of D squares
// made in dimension order, off their real values by at most (D / 2 + 2) * 2^-24 of themselves; the real points obey the
// triangle inequality (DESIGN.md 4h derives the constant).
__host__ __device__ inline float bitvec_ti_slack(int D) { return (float)(D + 8) * 1.1920928955078125e-7f; }

// The rows of one cluster that a query at centre distance qcc can still need under the threshold distance thr:
// lo <= xcc <= hi.  It is |qcc - xcc| - g (qcc + xcc) <= thr solved for xcc, so that a cut over the descending xcc of a
// cluster is a comparison against two constants; a row outside is pruned (strictly: a row at a bound stays).
struct TiAnnulus {
  float lo, hi;
};
__host__ __device__ inline TiAnnulus bitvec_ti_annulus(float qcc, float thr, float g) {
  return TiAnnulus{(qcc * (1.0f - g) - thr) / (1.0f + g), (thr + qcc * (1.0f + g)) / (1.0f - g)};
}

// keys[i] = (cluster << 32) | ~bits(sqrtf(dist2[i])), vals[i] = i, for i < n: ascending keys are the clusters in order,
// inside one the farthest row first (xcc >= 0: its bits order as the values do).  *first_bad (the caller sets it to
// INT32_MAX) becomes the first row whose assign is negative, a row the cluster index found no centre for.
hipError_t launch_bitvec_ti_keys(const int32_t *assign, const float *dist2, int64_t n, uint64_t *keys, uint32_t *vals,
                                 int32_t *first_bad, hipStream_t st);
// A stable radix sort of the n (key, val) pairs by the key's low 32 + ceil(log2 T) bits (rocPRIM): equal keys keep
// ascending rows.  temp == nullptr: temp_bytes gets the size the call needs and nothing runs.
hipError_t bitvec_ti_sort(void *temp, size_t &temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                          int32_t *member_out, int64_t n, int T, hipStream_t st);
// From the sorted keys: xcc[g] of every grouped position and start[c] = the first position of cluster c, start[T] = n
// (an empty cluster starts where the next one does).
hipError_t launch_bitvec_ti_bounds(const uint64_t *keys_sorted, int64_t n, int T, int32_t *start, float *xcc, hipStream_t st);

// Per query the T centres by ascending qcc = sqrtf(euclideanDistNoSQRT(query, centre)) (one accumulator from 0.0f in
// dimension order, the subtraction, the product and the addition apart): order_out [nq][T] the centres, qcc_out
// [nq][T] their distances in that order.  Equal distances: ascending centre.  centres_t is [D][T].
hipError_t launch_bitvec_ti_plan(const float *ori_queries, int nq, int D, const float *centres_t, int T, int32_t *order_out,
                                 float *qcc_out, hipStream_t st);

// The k smallest of ALL n rows by (sqrtf(euclideanDistNoSQRT(query, row)), row), the rows read in place through
// member[]: labels = row + id_base, the distances; slots min(k, n) .. k - 1 are -1 / FLT_MAX.  One workgroup walks a
// query's clusters in plan order; inside a cluster only the positions whose xcc lies in the annulus of the present
// threshold are dealt to a lane.  evaluated (int64 [nq], may be null) counts the rows dealt.  refresh >= 1: see
// BITVEC_TI_REFRESH.  1 <= D <= BITVEC_CLUSTERS_MAX_DIM, 1 <= T <= BITVEC_CLUSTERS_MAX, 1 <= k <= BITVEC_RERANK_MAX.
hipError_t launch_bitvec_ti_select(const float *queries, int nq, int D, RowsRef rows, int64_t n, const int32_t *start,
                                   const int32_t *member, const float *xcc, int T, const int32_t *order, const float *qcc,
                                   int k, int refresh, int64_t id_base, int32_t *labels, float *out_dist, int64_t *evaluated,
                                   hipStream_t st);

}  // namespace vaq
#endif  // VAQ_BITVEC_TI_H_
