// vaq_exhaust.h -- the per-pair distance of the exhaustive form (vaq_exhaust.hip): Eigen's (q - y).squaredNorm() by
// ONE thread that holds the row y in registers, for rows of up to XS_MAX_DIM columns.  The additions are
// vaq::sq_norm_eigen's (vaq_restated.h), operand for operand: Eigen's sixteen accumulator lanes (a0[0..8), a1[0..8))
// are sixteen variables a[0..16), a[e & 15] += (q[e] - y[e])^2 over the paired-packet loop; then a0 += a1, the odd
// eighth packet, predux = ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)), the scalar tail; below 8 columns the plain sequential
// sum.  Host and device run these statements: tests/cpp/exhaust_pair_test.cpp compares them with sq_norm_eigen bit for
// bit on the host.  NP = D / 16 is a template argument so that every index into y is a constant after unrolling (the
// row then lives in registers); what depends on D mod 16 is a uniform branch, and REST = false (D == 16 * NP) drops
// those columns' registers: the kernels' widest instantiation is <XS_MAX_NP, false>.
// Byte rows (uint8, a bvecs dataset as stored): the row type Y of xs_pair_sq_norm widens each element where it is read
// ((float)uint8 is exact: the same operands); the kernel widens its row ONCE per tile with xs_widen_row and then runs
// the float instantiation, so its query loop is the float form's.  tests/cpp/refine_u8_pair_test.cpp checks both.
#ifndef VAQ_EXHAUST_H_
#define VAQ_EXHAUST_H_

#include <cstdint>

#include "vaq_restated.h"

namespace vaq {

constexpr int XS_MAX_NP = 8;                       // pairs of packets a thread keeps
constexpr int XS_MAX_DIM = XS_MAX_NP * 16;         // widest row of the register form (128 row registers, 16 sums)
// slots of the thread's row (slots at or past D are never read)
template <int NP, bool REST> struct XsRow { static constexpr int SLOTS = NP * 16 + (REST ? 15 : 0); };

// needs D / 16 == NP and D >= 1; REST == false: D == 16 * NP
template <int NP, bool REST, typename Y = float>
__host__ __device__ __forceinline__ float xs_pair_sq_norm(const float *__restrict__ q, const Y *y, const int D) {
  if (NP == 0 && D < 8) {  // res = coeff(0); res += coeff(i)
    float res = km_sq(q[0], (float)y[0]);
#pragma unroll
    for (int e = 1; e < 7; e++)
      if (e < D) res += km_sq(q[e], (float)y[e]);
    return res;
  }
  constexpr int end2 = NP * 16;
  const bool odd = REST && (D & 8) != 0;  // end1 > end2: an eighth packet the paired loop leaves over
  float a[16];
  if (NP >= 1) {
#pragma unroll
    for (int l = 0; l < 16; l++) a[l] = km_sq(q[l], (float)y[l]);
#pragma unroll
    for (int i = 16; i < end2; i += 16) {
#pragma unroll
      for (int l = 0; l < 16; l++) a[l] += km_sq(q[i + l], (float)y[i + l]);
    }
#pragma unroll
    for (int l = 0; l < 8; l++) a[l] += a[8 + l];
    if constexpr (REST) {
      if (odd) {
#pragma unroll
        for (int l = 0; l < 8; l++) a[l] += km_sq(q[end2 + l], (float)y[end2 + l]);
      }
    }
  } else {  // 8 <= D < 16: only a0 exists
#pragma unroll
    for (int l = 0; l < 8; l++) a[l] = km_sq(q[l], (float)y[l]);
  }
  float res = ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
  if constexpr (REST) {
    if (odd) {
#pragma unroll
      for (int j = 0; j < 7; j++)
        if (end2 + 8 + j < D) res += km_sq(q[end2 + 8 + j], (float)y[end2 + 8 + j]);
    } else {
#pragma unroll
      for (int j = 0; j < 7; j++)
        if (end2 + j < D) res += km_sq(q[end2 + j], (float)y[end2 + j]);
    }
  }
  return res;
}

// A 16-byte load of a byte row whose base allows it.
struct alignas(16) XsBytes16 {
  uint32_t w[4];
};
__host__ __device__ __forceinline__ float xs_byte(uint32_t word, int b) { return (float)((word >> (8 * b)) & 0xffu); }

// The thread's byte row yp (D columns, D / 16 == NP) widened into its XsRow<NP, REST>::SLOTS float slots; slots at or
// past D are 0 and never read.  The row's base is yp = rows + row * D BYTES: with REST == false (D == 16 * NP) it is a
// multiple of 16 and the row comes in 16-byte loads; with D % 4 == 0 in words; any other D (7, 129, ...) leaves row
// bases at odd addresses and keeps byte loads.  `rows` itself is 16-byte aligned (a device allocation).
template <int NP, bool REST>
__host__ __device__ __forceinline__ void xs_widen_row(float *y, const uint8_t *yp, const int D) {
  constexpr int SLOTS = XsRow<NP, REST>::SLOTS;
  if constexpr (!REST) {
    const XsBytes16 *vp = reinterpret_cast<const XsBytes16 *>(yp);
#pragma unroll
    for (int v = 0; v < NP; v++) {
      const XsBytes16 x = vp[v];
#pragma unroll
      for (int e = 0; e < 16; e++) y[v * 16 + e] = xs_byte(x.w[e / 4], e % 4);
    }
  } else if ((D & 3) == 0) {
    const uint32_t *wp = reinterpret_cast<const uint32_t *>(yp);
#pragma unroll
    for (int w = 0; w * 4 < SLOTS; w++) {  // (D is a multiple of 4: a word lies inside the row or past it)
      const uint32_t x = (w * 4 < NP * 16 || w * 4 < D) ? wp[w] : 0u;
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (w * 4 + b < SLOTS) y[w * 4 + b] = xs_byte(x, b);
    }
  } else {
#pragma unroll
    for (int e = 0; e < SLOTS; e++) y[e] = (e < NP * 16 || e < D) ? (float)yp[e] : 0.0f;
  }
}

}  // namespace vaq
#endif  // VAQ_EXHAUST_H_
