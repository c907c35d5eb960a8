// vaq_bitvec_clusters.h -- the cluster form of the Hamming queries (BitVecEngine::queryWithClusterInfo with
// QueryMethod::Sort, BitVecEngine.cpp:259-304): per query the centres are ranked by euclideanDistNoSQRT, the members
// of the nearest clusters are the candidates, and KNNFromDistsIndicesSupplied picks the k best of them.  Every query
// has a candidate list of its own length, so no distance matrix is written: the selection is fused into the scan.
// DESIGN.md section 4h, "Cluster form", has the rules and the layout.
#ifndef VAQ_BITVEC_CLUSTERS_H_
#define VAQ_BITVEC_CLUSTERS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_bitvec.h"

namespace vaq {

constexpr int BITVEC_CLUSTERS_MAX = 4096;  // centres: their (dist, c) pairs fill 32 KB of the plan's LDS
constexpr int BITVEC_CLUSTERS_MAX_DIM = 8176;  // floats of a centre: the refiner's row limit (the query row is staged)

// what the plan leaves per query beside its visit list
struct BitvecClusterPlan {
  int visit;     // clusters walked: visit[0 .. visit) of the query's list
  int cand;      // C_q, the members of those clusters
  int fallback;  // 1: equal or NaN centre distances, the order is the one-thread std::sort's
  int pad;
};

// One (dist, c) pair of the centre ranking and the comparator queryWithClusterInfo_sort hands std::sort
struct ClusterPair {
  float dist;
  int idx;
};
struct ClusterLt {
  __host__ __device__ inline bool operator()(const ClusterPair &a, const ClusterPair &b) const { return a.dist < b.dist; }
};

// image[g] = rows[member[g]] for g < n, zero for n <= g < n_pad: the bit rows cluster after cluster
hipError_t launch_bitvec_cluster_gather(const uint64_t *rows, const int32_t *member, int64_t n, int64_t n_pad, int W,
                                        uint64_t *image, hipStream_t st);

// The visiting plan of nq queries.  centres_t is [D][T] (dimension-major), start[T + 1] the clusters' first image
// rows.  Per query: dist[c] = euclideanDistNoSQRT(query, centre c) (one accumulator from 0.0f in dimension order, the
// subtraction, the product and the addition apart); the centres in std::sort's order under dist alone; visit = the
// centres walked until their members number k at least, and atleast at least; cand = those members.
// visit_out is [nq][T] (the first plan.visit entries of a row count), plan_out [nq].  1 <= T <= BITVEC_CLUSTERS_MAX,
// 1 <= D <= BITVEC_CLUSTERS_MAX_DIM, 1 <= atleast <= T.
hipError_t launch_bitvec_cluster_plan(const float *ori_queries, int nq, int D, const float *centres_t, int T,
                                      const int32_t *start, int k, int atleast, int32_t *visit_out,
                                      BitvecClusterPlan *plan_out, hipStream_t st);

// KNNFromDistsIndicesSupplied over each query's candidates, the Hamming distances computed on the way and never
// stored: candidate p (in visiting order, a cluster's members in ascending row order) has the distance of image row g
// to the query's W words; the kk = min(k, cand) smallest by (dist, seq) are written, seq being the slot std::sort
// (FAST's, over (dist << 16) | p) leaves p at for p < kk and p itself behind.  labels = member[g] + id_base, the
// distance as a float; slots kk .. k - 1 are -1 / FLT_MAX.  image holds the rows cluster after cluster.
hipError_t launch_bitvec_cluster_select(const uint64_t *image, int W, const int32_t *start, const int32_t *member,
                                        int T, const uint64_t *queries, int nq, const int32_t *visit,
                                        const BitvecClusterPlan *plan, int k, int64_t id_base, int32_t *labels,
                                        float *out_dist, hipStream_t st);

}  // namespace vaq
#endif  // VAQ_BITVEC_CLUSTERS_H_
