// vaq_lutfit.h -- the two lambdas of BitVecEngine::binaryEncodingLUT restated statement by statement, so that
// host and device run the same expressions: centroidsQuantile (BitVecEngine.hpp:811-840) and encodeToLUTCode
// (:889-932).  The kernels of vaq_lutfit.hip call these functions; tests/cpp/lutfit_test.cpp and
// tools/bench_lut_fit.py run the single-thread forms at the end of this file on the CPU.
// Everything is compiled with -ffp-contract=off: no expression below may fuse.
//
// Parity-unpinned: BitVecEngine.hpp includes glpk.h, so the reference's own function cannot be compiled into
// a checker here.  What is pinned is host == device == tests/lutfit_ref.py.
#ifndef VAQ_LUTFIT_H_
#define VAQ_LUTFIT_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vaq {
namespace lutfit {

constexpr int MAX_CENT = 256;            // rows of centroidsMat (:852)
constexpr int MAX_Q = MAX_CENT + 1;      // Q[j] has N + 1 entries, N <= 256

// The monotone float <-> uint map the column is radix-sorted under: a < b as floats implies key(a) < key(b);
// -0 sorts before +0, which std::sort leaves in an order of its own (they compare equal, so only the sign
// of a zero quantile can differ -- no comparison and no distance sees it).
__host__ __device__ inline uint32_t float_to_key(float x) {
  union { float f; uint32_t u; } c;
  c.f = x;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
__host__ __device__ inline float key_to_float(uint32_t k) {
  union { float f; uint32_t u; } c;
  c.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return c.f;
}
__host__ __device__ inline bool is_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// :815-818.  p = (float)(i+1)/N is a float division; the 0.5 literals are double, so both products and
// their sum are double and only `float poi =` rounds.
__host__ __device__ inline float quantile_pos(int i, int N, int64_t n) {
  const float p = (float)(i + 1) / N;
  const float poi = (1 - p) * (-0.5) + p * ((float)(uint64_t)n - 0.5);
  return poi;
}

// :819-821 over the sorted keys Z[0 .. n).  (left <= n - 1 always: poi < n - 0.5; clamped all the same so
// that no read leaves the column.)
__host__ __device__ inline float quantile_value(const uint32_t *Z, int64_t n, float poi) {
  int64_t left = (int64_t)floorf(poi);
  if (left < 0) left = 0;
  if (left > n - 1) left = n - 1;
  int64_t right = (int64_t)ceilf(poi);
  if (right > n - 1) right = n - 1;
  if (right < 0) right = 0;
  const float f = poi - (float)(uint64_t)left;
  return (1 - f) * key_to_float(Z[left]) + f * key_to_float(Z[right]);
}

// Q[q] of a column, q = 0 .. N
__host__ __device__ inline float quantile_at(const uint32_t *Z, int64_t n, int N, int q) {
  if (q == 0) return key_to_float(Z[0]);
  if (q == N) return key_to_float(Z[n - 1]);
  return quantile_value(Z, n, quantile_pos(q - 1, N, n));
}

// The walk of :825-832 stops bucket i at the first index >= lastidx with Z > Q[i+1]; the column being
// sorted, that is max(lastidx, first index with Z > Q[i+1]).  This is the second term (float compare: -0
// and +0 are equal here as they are there).
__host__ __device__ inline int64_t first_above(const uint32_t *Z, int64_t n, float q) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (key_to_float(Z[mid]) <= q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__host__ __device__ inline int64_t bucket_end(int64_t lastidx, int64_t above) { return above > lastidx ? above : lastidx; }

// :834-838; `sum` is the bucket's values added one after another onto the +0 of setZero()
__host__ __device__ inline float bucket_centroid(float sum, int count, float q_lo, float q_hi) {
  return count > 0 ? sum / count : (q_lo + q_hi) / 2.0f;
}

// ---- encodeToLUTCode ----
// The scan of :896-897 takes the FIRST q with x <= Q[q], and Q need not be monotone once rounded (a constant
// column gives (1 - f) * c + f * c, an ulp around c).  With PM[q] = max(Q[0 .. q]) the first q with
// x <= PM[q] is the same q (PM[q] is some Q[j], j <= q, and x <= Q[j] would have stopped the scan at j), and
// PM is monotone: a lower bound finds it.  Branch-free; returns N + 1 when there is none (x above the range,
// NaN).  PM has N + 1 entries.
__host__ __device__ inline int first_boundary(float x, const float *PM, int N) {
  int base = 0, len = N + 1;
  while (len > 1) {
    const int half = len >> 1;
    base += (x <= PM[base + half - 1]) ? 0 : half;
    len -= half;
  }
  return base + ((x <= PM[base]) ? 0 : 1);
}

// :899-928 for the q found (q == N + 1: none); c = the column's N centres
__host__ __device__ inline uint16_t choose_code(float x, int q, int N, const float *c) {
  int code;
  if (q > N) {
    code = N - 1;  // :926-927
  } else if (q == 0) {
    code = 0;
  } else if (q == 1) {
    const float m = fabsf(x - c[0]), r = fabsf(x - c[1]);
    code = (m <= r) ? 0 : 1;
  } else if (q == N) {
    const float m = fabsf(x - c[q - 1]), l = fabsf(x - c[q - 2]);
    code = (m <= l) ? (q - 1) : (q - 2);
  } else {
    const float m = fabsf(x - c[q - 1]), l = fabsf(x - c[q - 2]), r = fabsf(x - c[q]);
    if (m <= l && m <= r) code = q - 1;
    else if (l <= m && l <= r) code = q - 2;
    else code = q;
  }
  return (uint16_t)(uint8_t)code;  // :924
}

__host__ __device__ inline uint16_t encode_value(float x, int N, const float *PM, const float *c) {
  return choose_code(x, first_boundary(x, PM, N), N, c);
}

// ---- single-thread forms (host only): what the kernels compute, in the reference's shape ----
// Z: the column's keys sorted ascending; Q[N + 1]; cent[256] (rows >= N stay 0, :853)
inline void fit_column_host(const uint32_t *Z, int64_t n, int bits, float *Q, float *cent) {
  const int N = 1 << bits;
  for (int q = 0; q <= N; q++) Q[q] = quantile_at(Z, n, N, q);
  for (int i = 0; i < MAX_CENT; i++) cent[i] = 0.0f;
  int64_t lastidx = 0;
  for (int i = 0; i < N; i++) {
    const int64_t end = bucket_end(lastidx, first_above(Z, n, Q[i + 1]));
    float sum = 0.0f;
    for (int64_t j = lastidx; j < end; j++) sum += key_to_float(Z[j]);
    cent[i] = bucket_centroid(sum, (int)(end - lastidx), Q[i], Q[i + 1]);
    lastidx = end;
  }
}
inline void prefix_max_host(const float *Q, int N, float *PM) {
  float m = Q[0];
  for (int q = 0; q <= N; q++) {
    if (Q[q] > m) m = Q[q];
    PM[q] = m;
  }
}

}  // namespace lutfit
}  // namespace vaq
#endif
