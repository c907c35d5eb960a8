// vaq_front.h -- the query front end (vaq_front.hip): projection, the per-query lookup tables, and the orders a
// scan is dispatched in (slices, queries of a pass, expensive queries first).
#ifndef VAQ_FRONT_H_
#define VAQ_FRONT_H_

#include "vaq_common.h"

namespace vaq {

// checked != 0: non-finite coordinates of the product become 0 (BitVecEngine.hpp:53-71); E == nullptr = identity
hipError_t launch_project(const float *X, int64_t n, int D, const float *E, float *out,
                          hipStream_t st, int checked = 0);
// launch_project over rows of either type: byte rows are widened where they are loaded, every output is the float
// form's fmaf chain on the float form's operands (any byte address: the tile kernel's packed loads are taken only
// where X is 4-byte aligned)
hipError_t launch_project(RowsRef X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked = 0);
// cent_t: the codebooks dimension-major (entry j * ncent + c of subspace s at cent_off)
// min_ncent: the smallest codebook (subspaces of < 8 centroids take the reference's scalar branch)
// ck: also make the cost keys of launch_cost_order, where table 0 is computed; launch_cost_scatter then ranks.
//     Only for nq >= 16 and a first codebook of >= 8 centroids (n0; shift = bucket_shift) within
//     launch_cost_order's limits: anything else is refused
struct CostKeys {
  unsigned long long *keys;  // [nq]
  int n0, shift;
};
hipError_t launch_lut_build(const float *qproj, int nq, int D, int M, int L,
                            const SubDesc *sub, const float *cent_t, int lut_floats, int max_ncent,
                            float *lut, hipStream_t st, int min_ncent = 1, const CostKeys *ck = nullptr);
hipError_t launch_lut_expand(const float *lut_packed, int nq, int M, const SubDesc *sub,
                             int lut_floats, int ksub, float *lut_ref, hipStream_t st);
// Best-first slice order per query batch (n_slices <= 4096, n_buckets <= 4096)
hipError_t launch_slice_order(const float *lut, int lut_floats, int nq, int qb, const int *bstart,
                              int n_buckets, int bucket_shift, int64_t slice_rows, int n_slices,
                              int64_t n_rows, int *order, hipStream_t st);
// best-first form, one workgroup per query: order[b] = the query block b serves, expensive queries
// first (keys: nq 64-bit scratch words; n0 = entries of table 0, shift = bucket_shift).  launch_cost_order makes
// the keys from tables that are there; launch_cost_scatter is its second half alone, after a launch_lut_build
// that made the keys (CostKeys) on the same stream
hipError_t launch_cost_order(const float *lut, int lut_floats, int nq, int n0, int shift, unsigned long long *keys,
                             int *order, hipStream_t st);
hipError_t launch_cost_scatter(const unsigned long long *keys, int nq, int *order, hipStream_t st);
// order[i] = the query the i-th pass slot takes: by (nearest first code, nearest second code); nq <= 16384
hipError_t launch_query_order(const float *lut, int lut_floats, int nq, int n0, int off1, int n1, int *order,
                              hipStream_t st);

} // namespace vaq
#endif
