// vaq_cluster_index.h -- the cluster of every raw row (computeClusterIndex, utils/Experiment.hpp:372-392): what
// vaqhip_bitvec_set_clusters takes as clust_idx, made on the device.  DESIGN.md section 4h, "Cluster index", has the
// rules, the layout and the compiler's figures.
#ifndef VAQ_CLUSTER_INDEX_H_
#define VAQ_CLUSTER_INDEX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_bitvec_clusters.h"

namespace vaq {

constexpr int CLUSTER_INDEX_DC = 32;  // dimensions of a chunk: 256 rows and a block of centres are staged in LDS DC at a time
constexpr int CLUSTER_INDEX_TC = 64;  // centres of a block: a lane keeps their running sums in registers

// Row i of rows (n rows of D elements, float or byte, on the device) gets the first centre c of centroids (float
// [T][D] row-major, on the device) whose distance is the smallest:
//   nearestIdx = -1, nearestDist = FLT_MAX; for c = 0 .. T - 1: dist = 0.0f; for d = 0 .. D - 1:
//   dist += (row[d] - centre[d]) * (row[d] - centre[d]); if (dist < nearestDist) take c
// one float accumulator in dimension order, the subtraction, the product and the addition apart (the unit is built
// without contraction and without packed fp32); a byte is widened where it is loaded.  A NaN, +inf or >= FLT_MAX
// distance never wins; a row with no other distance gets -1.  idx_out is int32 [n]; dist_out (float [n], the chosen
// centre's distance, FLT_MAX beside -1) may be null.  1 <= D <= BITVEC_CLUSTERS_MAX_DIM, 1 <= T <=
// BITVEC_CLUSTERS_MAX, 0 <= n < 2^31, rows.elem 4 or 1.  Nothing is allocated and nothing waited for.
hipError_t launch_cluster_index(RowsRef rows, int64_t n, int D, const float *centroids, int T, int32_t *idx_out,
                                float *dist_out, hipStream_t st);

// The assign step of KMeans::fit (KMeans.hpp:67-77, vaq_kmeans_fit.h): the same kernel with dist = sqrtf(that sum)
// before the `<`, so the first of two centres whose roots are one float wins although its sum is the larger.  dist_out
// gets the root.
hipError_t launch_cluster_index_root(RowsRef rows, int64_t n, int D, const float *centroids, int T, int32_t *idx_out,
                                     float *dist_out, hipStream_t st);

}  // namespace vaq
#endif  // VAQ_CLUSTER_INDEX_H_
