// vaq_kmeans_fit.h -- KMeans::fit (KMeans.hpp:42-107) with the caller's seeds, over raw rows that stay where they are:
// the centres that every cluster form of the Hamming engine starts from.  DESIGN.md section 4h, "Fitting the centres",
// has the rules, the launch shapes and the compiler's figures.
#ifndef VAQ_KMEANS_FIT_H_
#define VAQ_KMEANS_FIT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_bitvec_clusters.h"
#include "vaqhip_dev.h"

namespace vaq {

constexpr int KMEANS_FIT_DIMS = 64;   // dimensions a workgroup of the update kernel owns: one lane each, one wave
constexpr int KMEANS_FIT_TILE = 256;  // member row numbers the workgroup stages in LDS at a time
constexpr int KMEANS_FIT_LOADS = 8;   // rows whose loads are in flight before the first of them is added

// What the device tells the host once an iteration: the last iteration in which a centre was replaced, the first row
// that no centre won (INT32_MAX: none) and the first seed outside [0, n) (INT32_MAX: none).
struct KmeansFitFlags {
  int32_t changed_iter, no_centre_row, bad_seed;
};

// The buffers of one fit, grow-only; after kmeans_fit() means holds centres [T][D] and belongs int32 [n].
struct KmeansFitWork {
  vaqhost::DevBuf means, next, stamp, belongs, rows_in, keys_out, member, start, flags, temp;
  size_t temp_bytes = 0;
};

struct KmeansFitResult {
  int iterations = 0;
  KmeansFitFlags flags = {0, INT32_MAX, INT32_MAX};   // of the last iteration executed
  float assign_ms = 0, group_ms = 0, update_ms = 0;  // summed over the iterations (events on st)
};

// The fit over rows (n of D elements, float or byte, on the device), d_seed_rows int32 [T] on the device:
//   means[c] = row seed_rows[c]; then up to max_iter times
//   assign   belongs[i] = the first centre whose sqrtf(sum) is below every earlier one's, from (FLT_MAX, -1)
//            (launch_cluster_index_root); -1 leaves flags.no_centre_row and ends the fit
//   group    a stable radix sort of the rows by centre (rocPRIM): start[T + 1], member[n] ascending inside a centre
//   update   new[c][d] = (the members' values added in member order into one accumulator from +0.0f) / (float)count;
//            a centre whose new vector is not == its old one is replaced whole
// until no centre was replaced.  A seed outside [0, n) leaves flags.bad_seed after the first iteration, whose results
// mean nothing.  The stream is synchronised once per iteration, for the flags; nothing else crosses to the host.
// 1 <= n < 2^31, 1 <= D <= BITVEC_CLUSTERS_MAX_DIM, 1 <= T <= BITVEC_CLUSTERS_MAX, max_iter >= 1.
hipError_t kmeans_fit(RowsRef rows, int64_t n, int D, int T, const int32_t *d_seed_rows, int max_iter, KmeansFitWork &w,
                      KmeansFitResult *res, hipStream_t st);

}  // namespace vaq
#endif  // VAQ_KMEANS_FIT_H_
