// vaq_train.h -- the kernels of the training front half (vaq_train.hip; host side in vaqhip_train.cpp, the arithmetic
// both share in vaq_train_rot.h and train_plan.h).  Every launch enqueues only.
#ifndef VAQ_TRAIN_H_
#define VAQ_TRAIN_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_common.h"
#include "vaq_train_rot.h"

namespace vaq {

// tiles of train::MOMENT_TILE sample positions whose partials one pass may hold in `bytes` of scratch (at least 1)
int moment_chunk_tiles(int D, int64_t tiles, size_t bytes);

// The second moment of the s sampled rows of X (float or byte, n x D): sample position i is row d_rows[i], or row i
// when d_rows is null.  d_out[D x D] doubles, exactly symmetric; d_out_f (may be null) its rounding to float.  d_part:
// moment_chunk_tiles(..) * D * D doubles of scratch.  Order of the additions: train_plan.h / include/vaqhip.h.
hipError_t launch_train_moment(RowsRef X, const int *d_rows, int64_t s, int D, double *d_part, int chunk_tiles,
                               double *d_out, float *d_out_f, hipStream_t st);

// *d_bad |= 1 when one of the n doubles is not finite
hipError_t launch_train_finite(const double *d_A, int64_t n, int *d_bad, hipStream_t st);
// V = identity (D x D doubles)
hipError_t launch_train_identity(double *d_V, int D, hipStream_t st);
// Step r of a sweep (vaq_train_rot.h): every pair's rotation into d_rot[slot] and its column update of A and V, the
// rotations applied added to *d_count; then every pair's row update of A.  Two ordinary launches.
hipError_t launch_train_jacobi_step(double *d_A, double *d_V, int D, int r, train::Rot *d_rot, int *d_count,
                                    hipStream_t st);

}  // namespace vaq
#endif
