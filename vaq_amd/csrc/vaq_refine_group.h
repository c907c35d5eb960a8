// vaq_refine_group.h -- Eigen's (q - y).squaredNorm() spread over 16 adjacent lanes of a wave: the distance of
// vaq_refine.hip's kernels and of the exhaustive form's general path and replay (vaq_exhaust.hip).  Device only.
// The row's element type T is float or uint8_t: a byte is widened where it is loaded ((float)uint8 is exact) and
// every subtraction, product and sum after it is the float form's; a byte row moves a quarter of the bytes.
#ifndef VAQ_REFINE_GROUP_H_
#define VAQ_REFINE_GROUP_H_

#include "vaq_restated.h"

namespace vaq {

constexpr int RF_GROUP = 16;    // lanes per candidate row

// the value lane `src` of this lane's group holds
__device__ __forceinline__ float rf_from(float v, int gbase, int src) { return __shfl(v, gbase + src, 64); }

// Squared distance of the group's row y to the staged query qs, complete in lane 0 of the group.  Every lane of the
// wave runs every shuffle; `valid` (the same in all 16 lanes of a group) only masks the loads of a skipped candidate.
template <typename T>
__device__ __forceinline__ float rf_group_sq_norm(const float *qs, const T *__restrict__ y, int D, bool valid, int j,
                                                  int gbase) {
#define T_(idx, ok) ((valid && (ok)) ? km_sq(qs[idx], (float)y[idx]) : 0.0f)
  if (D < 8) {  // res = coeff(0); res += coeff(i)
    const float t = T_(j, j < D);
    float res = rf_from(t, gbase, 0);
    for (int e = 1; e < D; e++) res += rf_from(t, gbase, e);
    return res;
  }
  const int end1 = (D / 8) * 8, end2 = (D / 16) * 16;
  float acc;
  if (end2 >= 16) {  // a0 = packet 0, a1 = packet 1, then the loop over pairs of packets
    acc = T_(j, true);
#pragma unroll 4
    for (int i = 16; i < end2; i += 16) acc += T_(i + j, true);
  } else {  // 8 <= D < 16: only a0 exists
    acc = T_(j, j < 8);
  }
  if (end1 > 8) {
    acc += rf_from(acc, gbase, (j + 8) & 15);                // lanes 0..7: a0 += a1
    if (end1 > end2) acc += T_(end2 + j, j < 8);             // the odd eighth packet
  }
  // predux<Packet8f> in lanes 0..7: the halves added, then (b0 + b2) + (b1 + b3)
  acc += rf_from(acc, gbase, j ^ 4);
  acc += rf_from(acc, gbase, j ^ 2);
  acc += rf_from(acc, gbase, j ^ 1);
  const float t = T_(end1 + j, end1 + j < D);  // the scalar tail, at most 7 elements
  float res = acc;
  for (int e = 0; e < D - end1; e++) res += rf_from(t, gbase, e);
  return res;
#undef T_
}

}  // namespace vaq
#endif  // VAQ_REFINE_GROUP_H_
