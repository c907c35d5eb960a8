// vaq_exhaust.h -- the per-pair distance of the exhaustive form (vaq_exhaust.hip): Eigen's (q - y).squaredNorm() by
// ONE thread that holds the row y in registers, for rows of up to XS_MAX_DIM columns.  The additions are
// vaq::sq_norm_eigen's (vaq_restated.h), operand for operand: Eigen's sixteen accumulator lanes (a0[0..8), a1[0..8))
// are sixteen variables a[0..16), a[e & 15] += (q[e] - y[e])^2 over the paired-packet loop; then a0 += a1, the odd
// eighth packet, predux = ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)), the scalar tail; below 8 columns the plain sequential
// sum.  Host and device run these statements: tests/cpp/exhaust_pair_test.cpp compares them with sq_norm_eigen bit for
// bit on the host.  NP = D / 16 is a template argument so that every index into y is a constant after unrolling (the
// row then lives in registers); what depends on D mod 16 is a uniform branch, and REST = false (D == 16 * NP) drops
// those columns' registers: the kernels' widest instantiation is <XS_MAX_NP, false>.
#ifndef VAQ_EXHAUST_H_
#define VAQ_EXHAUST_H_

#include "vaq_restated.h"

namespace vaq {

constexpr int XS_MAX_NP = 8;                       // pairs of packets a thread keeps
constexpr int XS_MAX_DIM = XS_MAX_NP * 16;         // widest row of the register form (128 row registers, 16 sums)
// slots of the thread's row (slots at or past D are never read)
template <int NP, bool REST> struct XsRow { static constexpr int SLOTS = NP * 16 + (REST ? 15 : 0); };

// needs D / 16 == NP and D >= 1; REST == false: D == 16 * NP
template <int NP, bool REST>
__host__ __device__ __forceinline__ float xs_pair_sq_norm(const float *__restrict__ q, const float *y, const int D) {
  if (NP == 0 && D < 8) {  // res = coeff(0); res += coeff(i)
    float res = km_sq(q[0], y[0]);
#pragma unroll
    for (int e = 1; e < 7; e++)
      if (e < D) res += km_sq(q[e], y[e]);
    return res;
  }
  constexpr int end2 = NP * 16;
  const bool odd = REST && (D & 8) != 0;  // end1 > end2: an eighth packet the paired loop leaves over
  float a[16];
  if (NP >= 1) {
#pragma unroll
    for (int l = 0; l < 16; l++) a[l] = km_sq(q[l], y[l]);
#pragma unroll
    for (int i = 16; i < end2; i += 16) {
#pragma unroll
      for (int l = 0; l < 16; l++) a[l] += km_sq(q[i + l], y[i + l]);
    }
#pragma unroll
    for (int l = 0; l < 8; l++) a[l] += a[8 + l];
    if constexpr (REST) {
      if (odd) {
#pragma unroll
        for (int l = 0; l < 8; l++) a[l] += km_sq(q[end2 + l], y[end2 + l]);
      }
    }
  } else {  // 8 <= D < 16: only a0 exists
#pragma unroll
    for (int l = 0; l < 8; l++) a[l] = km_sq(q[l], y[l]);
  }
  float res = ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
  if constexpr (REST) {
    if (odd) {
#pragma unroll
      for (int j = 0; j < 7; j++)
        if (end2 + 8 + j < D) res += km_sq(q[end2 + 8 + j], y[end2 + 8 + j]);
    } else {
#pragma unroll
      for (int j = 0; j < 7; j++)
        if (end2 + j < D) res += km_sq(q[end2 + j], y[end2 + j]);
    }
  }
  return res;
}

}  // namespace vaq
#endif  // VAQ_EXHAUST_H_
