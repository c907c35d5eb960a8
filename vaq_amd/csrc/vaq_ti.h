// vaq_ti.h -- triangle-inequality cluster pruning (vaq_ti.hip): regrouping the rows by cluster and the per-query
// visiting plan.  The scan of a TI index is vaq_scan.h's (ScanParams::ti), its "exact_ties" replay vaq_exact.h's.
#ifndef VAQ_TI_H_
#define VAQ_TI_H_

#include "vaq_common.h"

namespace vaq {

// packed index rows -> uint16 N x M in original row order (inverse of launch_pack_codes)
hipError_t launch_unpack_codes(const uint32_t *packed, int64_t n, int M, int layout, int W,
                               const SubDesc *sub, const uint32_t *perm, uint16_t *out, hipStream_t st);
// VAQ::clusterTI's regrouping: d_perm[n], d_start[T+1] (-1 for clusters that do not occur;
// the caller back-fills), d_xcc_sorted[n].  Synchronises the stream.
hipError_t ti_group_rows(const uint16_t *d_codes, int64_t n, int M, int L, int seg, const SubDesc *sub,
                         const float *cent, const float *d_clusters, int T, uint32_t *d_perm,
                         int *d_start, float *d_xcc_sorted, hipStream_t st);
// per query: cluster visiting order, the matching distances, clusters visited
// (clusters_t: the centres dimension-major, T floats per dimension)
// exact = 1 (option "exact_ties" on a TI index): the cluster order is the reference's std::sort's, equal and NaN
// distances included
hipError_t launch_ti_plan(const float *qproj, int nq, int D, int d, const float *clusters_t, int T,
                          const int *start, int max_visit, int k, int *order, float *qcc, int *nvisit,
                          hipStream_t st, int exact = 0);
// d_walk[n]: position in the reference's member order (clusters in index order, VAQ::clusterTI's std::sort
// inside each) -> index row.  d_start: the back-filled cluster starts [T + 1].  Synchronises the stream.
hipError_t ti_build_walk(const uint32_t *d_perm, const int *d_start, const float *d_xcc_sorted, int64_t n, int T,
                         uint32_t *d_walk, hipStream_t st);

} // namespace vaq
#endif
