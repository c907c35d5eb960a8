// vaq_lutfit_dev.h -- BitVecEngine::binaryEncodingLUT from the bit allocation on (vaq_lutfit.hip, arithmetic in
// vaq_lutfit.h): the column fit, the encoder, and the two halves lut_fit_columns is made of, for the fit that runs them
// on different devices (vaqhip_multi_lutfit.cpp): "produce keys" and "fit one column from keys".
#ifndef VAQ_LUTFIT_DEV_H_
#define VAQ_LUTFIT_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_common.h"
#include "vaqhip_dev.h"

namespace vaq {

// lut_fit_columns: centroidsQuantile per column of the n x D rows in PCA space -- d_cent_out [D][256] (centroidsMat:
// 256 x D column-major), d_q_out [D][257], *d_bad set when a value is not finite; synchronises `st`;
// phase_ms (optional) [4]: device time of extract, sort, quantiles, means over all columns.
hipError_t lut_fit_columns(const float *d_Xp, int64_t n, int D, const int *bits, float *d_cent_out, float *d_q_out,
                           int *d_bad, float *phase_ms, hipStream_t st);
// lut_fit_columns over rows of either type: a byte is widened where the extract loads it
hipError_t lut_fit_columns(RowsRef d_Xp, int64_t n, int D, const int *bits, float *d_cent_out, float *d_q_out,
                           int *d_bad, float *phase_ms, hipStream_t st);
// encodeToLUTCode: Xp n x D in PCA space (D == M, one centre column per dimension), codes n x D uint16 row-major;
// d_pm: per dimension s the N + 1 prefix maxima of Q[s] at sub[s].cent_off + s (lutfit::first_boundary)
hipError_t launch_lut_encode(const float *Xp, int64_t n, int D, const SubDesc *h_sub, const SubDesc *d_sub,
                             const float *d_pm, const float *d_cent, uint16_t *codes, int n_cu, hipStream_t st);

// What one column's fit works in on its device: the column's keys as they arrived, sorted, rocprim's scratch and the
// bucket ends.  Freed with the caller's current device, as every DevBuf.
struct LutFitColumnWork {
  vaqhost::DevBuf keys, sorted, temp, ends;
  size_t temp_bytes = 0;
  hipError_t ensure(int64_t n, hipStream_t st);  // for columns of n keys
  void release() { vaqhost::release_all({&keys, &sorted, &temp, &ends}); }
};

// centroidsQuantile of ONE column from w.keys[0 .. n) (any order): radix sort, quantiles, ordered bucket sums.
// d_q [257], d_cent [256] (entries from 1 << bits on are left alone: the caller zeroes them).  e (optional) [4]:
// recorded on `st` before the sort and after the sort, the quantiles and the means.  Enqueues only.
hipError_t lut_fit_column_from_keys(LutFitColumnWork &w, int64_t n, int bits, float *d_q, float *d_cent, hipEvent_t *e,
                                    hipStream_t st);

// Columns [d0, d0 + W), W <= 16, of the n x D rows X as sortable keys: keys[w * n + r] = float_to_key(y), y = the
// row's own value (E null) or ONE fmaf chain over the inner index ascending from acc = 0.0f (launch_project's value,
// bit for bit); *d_bad is ORed with 1 when a y is not finite.  X: float or byte rows at any byte address, a byte
// widened where it is loaded.  Enqueues only.
hipError_t launch_lutfit_project_columns(RowsRef X, int64_t n, int D, const float *E, int d0, int W, uint32_t *keys,
                                         int *d_bad, hipStream_t st);

}  // namespace vaq
#endif
