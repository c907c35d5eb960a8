// vaq_learn.h -- the kernels of learnQuantization's device forms (vaq_learn.hip; host side in vaqhip_learn.cpp, the
// arithmetic both share in learn_plan.h).  Every launch enqueues only.
#ifndef VAQ_LEARN_H_
#define VAQ_LEARN_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_common.h"

namespace vaq {

// out[i][0 .. D) = (float)X[rows[i]][0 .. D) for i < m: the sampled rows, float or byte, as dense float rows
hipError_t launch_learn_gather(RowsRef X, const int *rows, int m, int D, float *out, hipStream_t st);

// groups[(i0 + i)][0 .. Mc)[ksub] = tables[i][s0 .. s0 + Mc)[ksub] for i < m: the group's columns of a chunk's tables
// (launch_lut_expand's [m][M][ksub]) into the group's [sample][Mc][ksub]
hipError_t launch_learn_slice(const float *tables, int m, int M, int ksub, int s0, int Mc, int64_t i0, float *group,
                              hipStream_t st);

// column sl of the group's tables as sortable keys (vaq_lutfit.h: float_to_key) in table order: keys[i * ksub + c];
// *d_bad is ORed with 1 when a value is not finite
hipError_t launch_learn_keys(const float *group, int64_t sample, int Mc, int ksub, int sl, uint32_t *keys, int *d_bad,
                             hipStream_t st);

// out[j] = key_to_float(sorted[idx[j]]) for j < n_idx: the order statistics the percentiles read
hipError_t launch_learn_fetch(const uint32_t *sorted, const int64_t *idx, int n_idx, float *out, hipStream_t st);

// loss[a * Mc + sl] for the 7 alphas and the group's Mc columns: per (alpha, column) the terms of learn_plan.h's
// loss_term added one after another in table order, in double.  floors, scales: [7][Mc]
hipError_t launch_learn_loss(const float *group, int64_t sample, int Mc, int ksub, const float *floors,
                             const float *scales, double *loss, hipStream_t st);

}  // namespace vaq
#endif
