// vaq_codes.hip -- building an index: rows to codes, codes to the packed and bucketed device layout.
// (Numerics: vaq_common.h.)
//
// Kernels
//   pack_codes_kernel                             CodebookType (uint16 N x M) -> packed device rows
//   merge_rows_kernel                             appended rows into the bucketed order
//   first_code_keys_kernel, bucket_bounds_kernel  the stable sort by first code (rocprim's radix sort between them)
//   encode_kernel                                 VAQ::encodeImpl              VAQ.cpp:728-748
#include "vaq_codes.h"
#include "vaqhip_dev.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <float.h>

namespace vaq {
// ---------------------------------------------------------------------------
// CodebookType (uint16 N x M row-major, utils/Types.hpp:31) -> device layout.
//  LAYOUT_BYTES (every subspace 8 bits): row-major N x M bytes; byte s = code s.
//  LAYOUT_BITS : field s occupies bits [bit_off, bit_off+bits) of a W-dword
//      little-endian row, LSB-first; rows are stored in planar tiles of 64:
//      word w of row r at (r/64)*64*W + w*64 + (r%64), so a wavefront's load
//      of word w is one coalesced 256-byte access.
// One thread per output dword in [t_begin, t_end); `in` holds rows
// [row_begin, row_end) of the caller's matrix; rows outside it pack to zero
// (the padding past N).
// ---------------------------------------------------------------------------
__global__ void pack_codes_kernel(const uint16_t *__restrict__ in, int64_t row_begin,
                                  int64_t row_end, int M, int layout, int W,
                                  const SubDesc *__restrict__ sub, const uint32_t *__restrict__ perm,
                                  uint32_t *__restrict__ out, int64_t t_begin, int64_t t_end) {
  const int64_t t = t_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= t_end) return;
  uint32_t v = 0;
  if (layout == LAYOUT_BYTES) {
    const int wpr = M / 4;
    const int64_t r = t / wpr;
    const int w = (int)(t - r * wpr);
    if (r >= row_begin && r < row_end) {
      const uint16_t *c = in + ((perm ? (int64_t)perm[r] : r) - row_begin) * M + w * 4;
      v = (uint32_t)(c[0] & 0xff) | ((uint32_t)(c[1] & 0xff) << 8) |
          ((uint32_t)(c[2] & 0xff) << 16) | ((uint32_t)(c[3] & 0xff) << 24);
    }
  } else {
    const int64_t tile = t / ((int64_t)TILE_ROWS * W);
    const int rem = (int)(t - tile * TILE_ROWS * W);
    const int w = rem / TILE_ROWS;
    const int64_t r = tile * TILE_ROWS + (rem % TILE_ROWS);
    if (r >= row_begin && r < row_end) {
      const int64_t src = (perm ? (int64_t)perm[r] : r) - row_begin;
      for (int s = 0; s < M; s++) {
        const SubDesc sd = sub[s];
        const uint32_t code = (uint32_t)in[src * M + s] & (uint32_t)(sd.ncent - 1);
        if (sd.word == w) v |= code << sd.shift;
        else if (sd.word + 1 == w && sd.shift + sd.bits > 32) v |= code >> (32 - sd.shift);
      }
    }
  }
  out[t] = v;
}

int64_t packed_words(int64_t rows, int M, int layout, int W) {
  if (layout == LAYOUT_BYTES) return rows * (M / 4);
  return ((rows + TILE_ROWS - 1) / TILE_ROWS) * TILE_ROWS * W;
}

hipError_t launch_pack_codes(const uint16_t *codes_u16, int64_t row_begin, int64_t row_end,
                             int64_t out_row_end, int M, int layout, int W, const SubDesc *sub,
                             const uint32_t *perm, uint32_t *out, hipStream_t st) {
  const int64_t t_begin = packed_words(row_begin, M, layout, W);
  const int64_t t_end = packed_words(out_row_end, M, layout, W);
  if (t_end <= t_begin) return hipSuccess;
  const int64_t blocks = (t_end - t_begin + 255) / 256;
  hipLaunchKernelGGL(pack_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, codes_u16,
                     row_begin, row_end, M, layout, W, sub, perm, out, t_begin, t_end);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------
// Appending rows to a bucketed index without rebuilding it: the new rows are sorted and packed
// on their own (sort_by_first_code + pack_codes, n_new rows), then merged bucket by bucket --
// bucket b of the result = bucket b of the old order followed by bucket b of the new rows (new
// labels are larger, so this IS the stable order a sort of all rows would give).  One thread per
// output row copies the row's packed words and its label; no unpacking, no global re-sort.
//   tot_start[b] = old_start[b] + new_start[b]   (K0 + 1 entries each)
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t packed_word_index(int64_t row, int w, int layout, int WPR) {
  if (layout == LAYOUT_BYTES) return row * WPR + w;
  return (row / TILE_ROWS) * (int64_t)(TILE_ROWS * WPR) + (int64_t)w * TILE_ROWS + (row % TILE_ROWS);
}

__global__ void merge_rows_kernel(const uint32_t *__restrict__ old_codes, const uint32_t *__restrict__ old_perm,
                                  const int *__restrict__ old_start, const uint32_t *__restrict__ new_codes,
                                  const uint32_t *__restrict__ new_perm, const int *__restrict__ new_start, int K0,
                                  int64_t n_old, int64_t n_total, int layout, int WPR, uint32_t *__restrict__ out_codes,
                                  uint32_t *__restrict__ out_perm) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_total) return;
  // bucket of output row r: largest b with old_start[b] + new_start[b] <= r
  int lo = 0, hi = K0;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)old_start[mid] + new_start[mid] <= r) lo = mid;
    else hi = mid;
  }
  const int b = lo;
  const int64_t off = r - ((int64_t)old_start[b] + new_start[b]);
  const int64_t old_cnt = (int64_t)old_start[b + 1] - old_start[b];
  const bool from_old = off < old_cnt;
  const int64_t src = from_old ? old_start[b] + off : new_start[b] + (off - old_cnt);
  const uint32_t *codes = from_old ? old_codes : new_codes;
  for (int w = 0; w < WPR; w++)
    out_codes[packed_word_index(r, w, layout, WPR)] = codes[packed_word_index(src, w, layout, WPR)];
  out_perm[r] = from_old ? old_perm[src] : (uint32_t)(n_old + new_perm[src]);
}

hipError_t launch_merge_rows(const uint32_t *old_codes, const uint32_t *old_perm, const int *old_start,
                             const uint32_t *new_codes, const uint32_t *new_perm, const int *new_start, int K0,
                             int64_t n_old, int64_t n_total, int M, int layout, int W, uint32_t *out_codes,
                             uint32_t *out_perm, hipStream_t st) {
  if (n_total <= 0) return hipSuccess;
  const int WPR = layout == LAYOUT_BYTES ? M / 4 : W;
  hipLaunchKernelGGL(merge_rows_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, st, old_codes, old_perm,
                     old_start, new_codes, new_perm, new_start, K0, n_old, n_total, layout, WPR, out_codes, out_perm);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Bucketed row order.  The index stores rows stably sorted by (the top bits
// of) the code of subspace 0 -- after PCA the highest-variance subspace.  A
// bucket's rows share the first LUT term (shift == 0) or at least a lower bound
// of it (shift > 0: the minimum over the bucket's 1 << shift codes), so the scan
// skips a whole bucket, without touching its codes, when that bound alone already
// exceeds the threshold of every query in the batch (the bucket-level form of
// VAQ::searchEarlyAbandon's test, VAQ.cpp:1708); with shift == 0 it also reads
// the term once per bucket (wave-uniform) instead of gathering it per row.
// The host picks shift so that buckets average >= ~2048 rows.
//   perm[r]          original row of sorted row r (labels are original rows)
//   bucket_start[b]  first sorted row whose code 0 is >= b  (b = 0 .. K0)
// ---------------------------------------------------------------------------
__global__ void first_code_keys_kernel(const uint16_t *__restrict__ codes, int64_t n, int M,
                                       unsigned mask, int shift, unsigned mask1, int shift1, int t,
                                       uint16_t *__restrict__ keys, uint32_t *__restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned key = (codes[i * M] & mask) >> shift;
  if (t > 0) key = (key << t) | ((codes[i * M + 1] & mask1) >> shift1);  // + top t bits of code 1 (t includes the fine bits)
  keys[i] = (uint16_t)key;
  idx[i] = (uint32_t)i;
}

// start[b] = first i with keys[i] >> fine == b, for the keys that occur (others stay -1);
// sub (optional): the same at the level of the whole key
__global__ void bucket_bounds_kernel(const uint16_t *__restrict__ keys, int64_t n, int fine, int *__restrict__ start,
                                     int *__restrict__ sub) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i], kp = i > 0 ? keys[i - 1] : 0u;
  if (i == 0 || (k >> fine) != (kp >> fine)) start[k >> fine] = (int)i;
  if (sub && (i == 0 || k != kp)) sub[k] = (int)i;
}

// fine > 0 (needs shift == 0): the rows of a bucket are ordered by the NEXT `fine` bits of the second
// code as well -- the sort key is bucket key << fine | those bits -- and d_sub_start[(K0 << fine) + 1]
// receives the first row of every (bucket, fine value) run, like d_bucket_start.  Rows of a run share
// their first two lookup-table terms whenever t + fine == bits1 (vaq_scan_bm.hip skips whole runs).
hipError_t sort_by_first_code(const uint16_t *d_codes, int64_t n, int M, int bits0, int shift, int bits1,
                              int t, uint32_t *d_perm, int *d_bucket_start, hipStream_t st, int fine,
                              int *d_sub_start) {
  const int kbits_b = bits0 - shift + t;  // bucket key: the first code's top bits0 - shift bits [+ t of code 1]
  const int kbits = kbits_b + fine;
  const int K0 = 1 << kbits_b;
  if (fine < 0 || kbits > 16 || (fine > 0 && (shift != 0 || t + fine > bits1 || !d_sub_start))) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_bucket_start, 0xff, (size_t)(K0 + 1) * sizeof(int), st);
  if (e == hipSuccess && fine > 0) e = hipMemsetAsync(d_sub_start, 0xff, ((size_t)(K0 << fine) + 1) * sizeof(int), st);
  if (e != hipSuccess || n == 0) return e;
  vaqhost::DevBuf b_keys_in, b_keys_out, b_idx_in, b_temp;  // (freed on return, after the stream is synchronised)
  size_t temp_bytes = 0;
  if ((e = b_keys_in.ensure((size_t)n * 2)) != hipSuccess || (e = b_keys_out.ensure((size_t)n * 2)) != hipSuccess ||
      (e = b_idx_in.ensure((size_t)n * 4)) != hipSuccess)
    return e;
  uint16_t *keys_in = b_keys_in.as<uint16_t>(), *keys_out = b_keys_out.as<uint16_t>();
  uint32_t *idx_in = b_idx_in.as<uint32_t>();
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(first_code_keys_kernel, dim3(blocks), dim3(256), 0, st, d_codes, n, M,
                     (unsigned)((1 << bits0) - 1), shift, (unsigned)((1 << bits1) - 1), bits1 - (t + fine), t + fine, keys_in,
                     idx_in);
  // stable LSD radix sort on the b0 key bits: equal codes keep ascending original rows
  e = rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, idx_in, d_perm, (size_t)n, 0u,
                                (unsigned)kbits, st);
  if (e == hipSuccess) e = b_temp.ensure(temp_bytes ? temp_bytes : 16);
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(b_temp.p, temp_bytes, keys_in, keys_out, idx_in, d_perm, (size_t)n, 0u,
                                  (unsigned)kbits, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bucket_bounds_kernel, dim3(blocks), dim3(256), 0, st, keys_out, n, fine, d_bucket_start,
                       fine > 0 ? d_sub_start : (int *)nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// ---------------------------------------------------------------------------
// VAQ::encodeImpl, VAQ.cpp:728-748: per subspace, per row, argmin over codes of
// (x_block - c_row).squaredNorm(), strict `<` so the first minimum wins.  The
// reference leaves the summation order to Eigen's vectorised reduction; here
// (and in the oracle) it is the sequential  dist = 0; dist += t*t  over the
// subspace's dimensions, multiply and add unfused.
// grid = (row tile of 256, subspace); one row per thread, its L values in
// registers (LT = compile-time L) or read back from an LDS tile (LT = 0);
// centroids stream through LDS in chunks of 256 (broadcast reads).
// ---------------------------------------------------------------------------
constexpr int ENC_THREADS = 256;
constexpr int ENC_CHUNK = 256;

template <int LT>
__global__ __launch_bounds__(ENC_THREADS) void encode_kernel(
    const float *__restrict__ Xp, int64_t n, int D, int L, const SubDesc *__restrict__ sub,
    const float *__restrict__ cent, int M, uint16_t *__restrict__ codes) {
  extern __shared__ __attribute__((aligned(16))) float esm[];
  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const SubDesc sd = sub[s];
  const int64_t row = (int64_t)blockIdx.x * ENC_THREADS + tid;
  const bool valid = row < n;
  float *cs = esm;                                  // [ENC_CHUNK][L]
  float *xs = esm + (size_t)ENC_CHUNK * L;          // [L][ENC_THREADS] (LT == 0 only)
  float xr[LT > 0 ? LT : 1];
  const float *xp = Xp + (valid ? row : 0) * D + (int64_t)s * L;
  if (LT > 0) {
#pragma unroll
    for (int j = 0; j < LT; j++) xr[j] = xp[j];
  } else {
    for (int j = 0; j < L; j++) xs[j * ENC_THREADS + tid] = xp[j];
  }
  float bsf = FLT_MAX;
  int best = 0;
  const float *cg = cent + sd.cent_off;
  for (int c0 = 0; c0 < sd.ncent; c0 += ENC_CHUNK) {
    const int cn = sd.ncent - c0 < ENC_CHUNK ? sd.ncent - c0 : ENC_CHUNK;
    __syncthreads();
    for (int e = tid; e < cn * L; e += ENC_THREADS) cs[e] = cg[(size_t)c0 * L + e];
    __syncthreads();
    for (int c = 0; c < cn; c++) {
      const float *cr = cs + c * (LT > 0 ? LT : L);
      float dist = 0.0f;
      if (LT > 0) {
#pragma unroll
        for (int j = 0; j < LT; j++) {
          const float t = xr[j] - cr[j];
          dist += t * t;
        }
      } else {
        for (int j = 0; j < L; j++) {
          const float t = xs[j * ENC_THREADS + tid] - cr[j];
          dist += t * t;
        }
      }
      if (dist < bsf) {
        bsf = dist;
        best = c0 + c;
      }
    }
  }
  if (valid) codes[row * M + s] = (uint16_t)best;
}

hipError_t launch_encode(const float *Xp, int64_t n, int D, int M, int L, const SubDesc *sub,
                         const float *cent, uint16_t *codes, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + ENC_THREADS - 1) / ENC_THREADS), M);
  const size_t lds_reg = (size_t)ENC_CHUNK * L * sizeof(float);
  switch (L) {
  case 4:  hipLaunchKernelGGL(encode_kernel<4>, grid, dim3(ENC_THREADS), lds_reg, st, Xp, n, D, L, sub, cent, M, codes); break;
  case 8:  hipLaunchKernelGGL(encode_kernel<8>, grid, dim3(ENC_THREADS), lds_reg, st, Xp, n, D, L, sub, cent, M, codes); break;
  case 16: hipLaunchKernelGGL(encode_kernel<16>, grid, dim3(ENC_THREADS), lds_reg, st, Xp, n, D, L, sub, cent, M, codes); break;
  case 32: hipLaunchKernelGGL(encode_kernel<32>, grid, dim3(ENC_THREADS), lds_reg, st, Xp, n, D, L, sub, cent, M, codes); break;
  default: {
    const size_t lds = lds_reg + (size_t)L * ENC_THREADS * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(encode_kernel<0>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(encode_kernel<0>, grid, dim3(ENC_THREADS), lds, st, Xp, n, D, L, sub, cent, M, codes);
  }
  }
  return hipGetLastError();
}

} // namespace vaq
