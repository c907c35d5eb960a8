// vaq_bitvec_encode.h -- the two encoders of BitVecEngine restated from the point where the projected value is known:
// binaryEncodingSimple (BitVecEngine.hpp:239-255, one sign bit per dimension) and binaryEncoding (:509-590, a quantile
// code of bits[j] bits per dimension), so that host and device run the same statements.  The kernels of
// vaq_bitvec_encode.hip call the functions of the first half; tests/cpp/bitvec_encode_test.cpp runs the single-thread
// forms at the end on the CPU.  Compiled with -ffp-contract=off, as vaq_lutfit.h, whose quantile expression this reuses.
//
// Parity-unpinned, as the LUT fit is: BitVecEngine.hpp includes glpk.h.  What is pinned is
// device == host == tests/bitvec_encode_ref.py.
//
// The projected value x[i][c] is vaqhip_project's, unchecked: one fmaf chain over the inner index ascending from
// acc = 0.0f, a byte widened where it is loaded; with no eigenvectors the row's own value.
#ifndef VAQ_BITVEC_ENCODE_H_
#define VAQ_BITVEC_ENCODE_H_

#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_common.h"
#include "vaq_lutfit.h"

namespace vaq {
namespace bvenc {

constexpr int MAX_DIM = 2048;   // columns of a raw row: one row per wave must fit the workgroup's 32 KB tile
constexpr int MAX_BITS = 8;     // bits of one dimension: Q has 256 rows (:543)
constexpr int THR_STRIDE = 256; // floats of one dimension in a thresholds table [D][256]

// ---- sign form ----
// :243-253 shift the bits in from the right and flush a word every 64 columns: dimension d is bit 63 - d % 64 of word
// d / 64, the bit is `x > 0` (NaN, -0 and +0: 0; a positive denormal and +inf: 1), the tail bits of the last word are 0.
// D % 64 == 63 is outside it: after the loop j = D + 1, so :253 shifts by 64 - 0 = 64 and writes word (D + 1) / 64,
// one past the row's last word.  sign_form_defined() is what the callers refuse by.
__host__ __device__ inline bool sign_form_defined(int D) { return D % 64 != 63; }
__host__ __device__ inline bool sign_bit(float x) { return x > 0; }

// ---- quantile form ----
// T[q], q = 0 .. 2^b - 2, of a dimension with b bits over its column's sorted keys Z: the reference's quantile(Z, N)
// with N = 2^b - 1 has p = (float)(i + 1) / (N + 1) and the poi / left / right interpolation of :516-519 -- Q[1 .. 2^b - 1]
// of the LUT fit with 2^b centres (lutfit::quantile_pos, quantile_value).  T[2^b - 1] = FLT_MAX (:560).
__host__ __device__ inline float threshold_at(const uint32_t *Z, int64_t n, int b, int q) {
  const int N = 1 << b;
  return q == N - 1 ? FLT_MAX : lutfit::quantile_value(Z, n, lutfit::quantile_pos(q, N, n));
}

// :570-571 take the FIRST q < 2^b with x <= T[q]; PM holds the running maximum of T (2^b entries), over which the
// first match is the same q and a lower bound finds it (lutfit::first_boundary).  NaN and +inf match no q: the
// reference then ORs nothing, which is what code 0 ORs.
__host__ __device__ inline uint32_t quantile_code(float x, const float *PM, int b) {
  const int N = 1 << b;
  const int q = lutfit::first_boundary(x, PM, N - 1);
  return q >= N ? 0u : (uint32_t)q;
}

// :574-581: the b bits of `code`, most significant first, at bit `pos` of the row's stream (bit 0 = the top bit of word
// 0).  A code that crosses a word gives two parts; hi_word is the index of the first.  lo is 0 when nothing crosses.
struct CodeParts {
  uint64_t hi, lo;
  int hi_word;
};
__host__ __device__ inline CodeParts place_code(uint32_t code, int pos, int b) {
  CodeParts p;
  p.hi_word = pos / 64;
  const int room = 64 - pos % 64;  // bits left in the first word, 1 .. 64
  if (b <= room) {
    p.hi = (uint64_t)code << (room - b);
    p.lo = 0;
  } else {
    const int right = b - room;  // 1 .. 7
    p.hi = (uint64_t)code >> right;
    p.lo = ((uint64_t)code & (((uint64_t)1 << right) - 1)) << (64 - right);
  }
  return p;
}

// ---- single-thread forms (host only): what the kernels compute, in the reference's shape ----
// xp: n x D projected rows; out: n x W words, W = (D + 63) / 64
inline void sign_encode_host(const float *xp, int64_t n, int D, uint64_t *out) {
  const int W = (D + 63) / 64;
  for (int64_t i = 0; i < n; i++) {
    for (int w = 0; w < W; w++) out[i * W + w] = 0;
    for (int d = 0; d < D; d++)
      if (sign_bit(xp[i * D + d])) out[i * W + d / 64] |= (uint64_t)1 << (63 - d % 64);
  }
}
// T[0 .. 2^b) of one column from its keys sorted ascending
inline void thresholds_host(const uint32_t *Z, int64_t n, int b, float *T) {
  for (int q = 0; q < (1 << b); q++) T[q] = threshold_at(Z, n, b, q);
}
// thr: [D][THR_STRIDE]; out: n x W words, W = (sum(bits) + 63) / 64
inline void quantile_encode_host(const float *xp, int64_t n, int D, const int *bits, const float *thr, uint64_t *out) {
  int total = 0;
  for (int d = 0; d < D; d++) total += bits[d];
  const int W = (total + 63) / 64;
  for (int64_t i = 0; i < n * W; i++) out[i] = 0;
  float PM[THR_STRIDE];
  int pos = 0;
  for (int d = 0; d < D; pos += bits[d], d++) {
    if (bits[d] == 0) continue;
    lutfit::prefix_max_host(thr + (size_t)d * THR_STRIDE, (1 << bits[d]) - 1, PM);
    for (int64_t i = 0; i < n; i++) {
      const CodeParts p = place_code(quantile_code(xp[i * D + d], PM, bits[d]), pos, bits[d]);
      out[i * W + p.hi_word] |= p.hi;
      if (p.lo) out[i * W + p.hi_word + 1] |= p.lo;
    }
  }
}

}  // namespace bvenc

// ---- the device side (vaq_bitvec_encode.hip) ----
// One allocated dimension of the quantile form: its column, its bits, the bit position of its code in the row's
// stream and where its 2^bits running-maximum thresholds start in the ragged table.
struct BitvecLive {
  int col, bits, pos, off;
};
struct BitvecEncodePlan {
  int D;                   // columns of a raw row
  int W;                   // words of a bit row
  const float *eig;        // D x D row-major, or null: the row's own values
  int n_live;              // columns computed: D (sign form) or the allocated dimensions
  const BitvecLive *live;  // null: the sign form
  const float *pm;         // the ragged running maxima, pm_floats of them
  int pm_floats;
};
// rows of one workgroup's tile for rows of D columns (tests size their inputs by it)
int bitvec_encode_tile_rows(int D);
// X (float or byte rows, any byte address) -> out [n][W] words.  Enqueues only; every word of the n rows is written.
hipError_t launch_bitvec_encode(RowsRef X, int64_t n, const BitvecEncodePlan &p, uint64_t *out, hipStream_t st);
// The thresholds of the allocated dimensions of the n x D rows X (projected by E when it is not null) into
// d_thr [D][256]: row d gets its 2^bits[d] entries, nothing else is written; *d_bad is set when a value of an
// allocated column is not finite, and then no threshold is written.  Synchronises st.
hipError_t bitvec_fit_thresholds(RowsRef X, int64_t n, int D, const int *bits, const float *E, float *d_thr, int *h_bad,
                                 hipStream_t st);

}  // namespace vaq
#endif  // VAQ_BITVEC_ENCODE_H_
