// vaq_bitvec_encode.hip -- gfx950 kernels that MAKE the Hamming engine's bit rows from raw rows: the sign form and the
// quantile form of BitVecEngine's encoders (statements in vaq_bitvec_encode.h) with the projection fused, and the fit
// of the quantile form's thresholds.  The n x D projected matrix is never written.
//
// Encode (bitvec_encode_kernel): a workgroup of four waves stages a tile of R = 4 RPW rows in LDS as floats (a byte is
// widened on the way in).  Wave w owns rows [w RPW, (w + 1) RPW) of the tile and walks the blocks of 64 output columns;
// lane = column, RPW accumulators in registers, the row values come as LDS broadcasts (one address per wave), four
// inner indices per read.  Every value is ONE fmaf chain over the inner index ascending from 0.0f: vaqhip_project's
// value bit for bit.  RPW = 16 for D <= 128 and halves as D doubles, so that the tile stays within 32 KB.
//   sign form      the wave's word of a row is the bit-reversed 64-bit ballot of `acc > 0`, stored by one lane into
//                  the tile's words in LDS
//   quantile form  only the allocated dimensions are columns; the lane searches its dimension's running-maximum
//                  thresholds (ragged in LDS, or in global memory when they do not fit beside the tile) and ORs the
//                  placed code into the row's words in LDS (64-bit LDS OR)
// The tile's words go out as one coalesced run.  Workgroups stride over the tiles, so the thresholds are staged once.
//
// Fit (bitvec_fit_thresholds): per run of allocated columns the LUT fit's fused extract (launch_lutfit_project_columns:
// up to 16 columns of sortable keys, the projection fused), one radix sort per column, and one small kernel that
// writes T.  The ordered bucket sums of the LUT fit are not run.
#include "vaq_bitvec_encode.h"

#include "vaq_lutfit_dev.h"
#include "vaqhip_dev.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <vector>

namespace vaq {
namespace {

using namespace bvenc;

constexpr int BE_THREADS = 256, BE_WAVES = BE_THREADS / 64;
constexpr int BE_TILE_FLOATS = 8192;         // 32 KB of rows per workgroup
constexpr int BE_LDS_BYTES = 60 * 1024;      // tile + words + thresholds of one workgroup
constexpr int BE_MAX_GRID = 1024;

inline int padded_dim(int D) { return (D + 3) & ~3; }
inline int rows_per_wave(int D) {
  int r = 16;
  while (r > 1 && BE_WAVES * r * padded_dim(D) > BE_TILE_FLOATS) r >>= 1;
  return r;
}

__device__ __forceinline__ float4 load4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load4(const uint8_t *p) {
  const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
  return make_float4((float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24));
}

// vec: D % 4 == 0 and X aligned for load4 (16 bytes for floats, 4 for bytes); pm_in_lds: the thresholds fit
template <typename T, int RPW, bool QUANT>
__global__ __launch_bounds__(BE_THREADS) void bitvec_encode_kernel(const T *__restrict__ X, int64_t n, BitvecEncodePlan p,
                                                                   int vec, int pm_in_lds, uint64_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = BE_WAVES * RPW;
  const int D = p.D, Dp = (D + 3) & ~3, W = p.W;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float *tile = smem;
  unsigned long long *words = reinterpret_cast<unsigned long long *>(smem + R * Dp);
  const float *pm = p.pm;
  if (QUANT && pm_in_lds) {
    float *spm = reinterpret_cast<float *>(words + R * W);
    for (int i = tid; i < p.pm_floats; i += BE_THREADS) spm[i] = p.pm[i];
    pm = spm;  // (read behind the first tile's barrier)
  }
  const int n_cb = (p.n_live + 63) / 64;
  const int64_t n_tiles = (n + R - 1) / R;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)(n - row0 < R ? n - row0 : R);
    __syncthreads();  // (the tile before and its words have been read)
    if (vec) {
      const int D4 = D >> 2;
      for (int i = tid; i < R * D4; i += BE_THREADS) {
        const int r = i / D4, c = (i - r * D4) * 4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < rows) v = load4(X + (row0 + r) * D + c);
        *reinterpret_cast<float4 *>(&tile[r * Dp + c]) = v;
      }
    } else {
      for (int i = tid; i < R * D; i += BE_THREADS) {
        const int r = i / D, c = i - r * D;
        tile[r * Dp + c] = r < rows ? (float)X[(row0 + r) * D + c] : 0.0f;
      }
    }
    for (int i = tid; i < R * W; i += BE_THREADS) words[i] = 0;
    __syncthreads();
    const float *my = tile + wave * RPW * Dp;
    unsigned long long *my_words = words + wave * RPW * W;
    for (int cb = 0; cb < n_cb; cb++) {
      const int li = cb * 64 + lane;
      const bool live = li < p.n_live;  // (a block of fewer than 64 columns: the others compute column 0 and drop it)
      BitvecLive L = {live ? li : 0, 0, 0, 0};
      if (QUANT) L = p.live[live ? li : 0];
      float acc[RPW];
      if (p.eig) {
#pragma unroll
        for (int r = 0; r < RPW; r++) acc[r] = 0.0f;
        const float *e = p.eig + L.col;
        int j = 0;
        for (; j + 4 <= D; j += 4) {
          const float e0 = e[(size_t)(j + 0) * D], e1 = e[(size_t)(j + 1) * D];
          const float e2 = e[(size_t)(j + 2) * D], e3 = e[(size_t)(j + 3) * D];
#pragma unroll
          for (int r = 0; r < RPW; r++) {
            const float4 xv = *reinterpret_cast<const float4 *>(&my[r * Dp + j]);
            acc[r] = __builtin_fmaf(xv.x, e0, acc[r]);
            acc[r] = __builtin_fmaf(xv.y, e1, acc[r]);
            acc[r] = __builtin_fmaf(xv.z, e2, acc[r]);
            acc[r] = __builtin_fmaf(xv.w, e3, acc[r]);
          }
        }
        for (; j < D; j++) {
          const float e0 = e[(size_t)j * D];
#pragma unroll
          for (int r = 0; r < RPW; r++) acc[r] = __builtin_fmaf(my[r * Dp + j], e0, acc[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < RPW; r++) acc[r] = my[r * Dp + L.col];
      }
      if (!QUANT) {
#pragma unroll
        for (int r = 0; r < RPW; r++) {
          const unsigned long long m = __ballot(live && sign_bit(acc[r]));  // lane i = dimension 64 cb + i = bit 63 - i
          if (lane == r) my_words[r * W + cb] = __brevll(m);
        }
      } else if (live) {
#pragma unroll
        for (int r = 0; r < RPW; r++) {
          const uint32_t code = quantile_code(acc[r], pm + L.off, L.bits);
          if (code == 0) continue;
          const CodeParts c = place_code(code, L.pos, L.bits);
          if (c.hi) atomicOr(&my_words[r * W + c.hi_word], (unsigned long long)c.hi);
          if (c.lo) atomicOr(&my_words[r * W + c.hi_word + 1], (unsigned long long)c.lo);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < rows * W; i += BE_THREADS) out[row0 * W + i] = words[i];
  }
}

template <typename T, int RPW>
hipError_t launch_encode_as(const T *X, int64_t n, const BitvecEncodePlan &p, uint64_t *out, hipStream_t st) {
  const int R = BE_WAVES * RPW, Dp = padded_dim(p.D);
  const size_t base = (size_t)R * Dp * sizeof(float) + (size_t)R * p.W * sizeof(uint64_t);
  const bool quant = p.live != nullptr;
  const int pm_in_lds = quant && base + (size_t)p.pm_floats * sizeof(float) <= (size_t)BE_LDS_BYTES;
  const size_t lds = base + (pm_in_lds ? (size_t)p.pm_floats * sizeof(float) : 0);
  const int vec = p.D % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & (sizeof(T) == 4 ? 15u : 3u)) == 0;
  const dim3 grid((unsigned)std::min<int64_t>((n + R - 1) / R, BE_MAX_GRID));
  if (quant)
    hipLaunchKernelGGL((bitvec_encode_kernel<T, RPW, true>), grid, dim3(BE_THREADS), lds, st, X, n, p, vec, pm_in_lds, out);
  else
    hipLaunchKernelGGL((bitvec_encode_kernel<T, RPW, false>), grid, dim3(BE_THREADS), lds, st, X, n, p, vec, pm_in_lds, out);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_encode_rows(const T *X, int64_t n, const BitvecEncodePlan &p, uint64_t *out, hipStream_t st) {
  switch (rows_per_wave(p.D)) {
    case 16: return launch_encode_as<T, 16>(X, n, p, out, st);
    case 8: return launch_encode_as<T, 8>(X, n, p, out, st);
    case 4: return launch_encode_as<T, 4>(X, n, p, out, st);
    case 2: return launch_encode_as<T, 2>(X, n, p, out, st);
    default: return launch_encode_as<T, 1>(X, n, p, out, st);
  }
}

// Z: one column's keys sorted ascending; T: the dimension's row of the scratch table
__global__ __launch_bounds__(256) void bitvec_thresholds_kernel(const uint32_t *__restrict__ Z, int64_t n, int b,
                                                                float *__restrict__ T) {
  const int q = threadIdx.x;
  if (q < (1 << b)) T[q] = threshold_at(Z, n, b, q);
}

// the allocated dimensions' entries from the scratch table into the caller's; grid = D
__global__ __launch_bounds__(256) void bitvec_thresholds_copy_kernel(const float *__restrict__ src, const int *__restrict__ bits,
                                                                     float *__restrict__ dst) {
  const int d = blockIdx.x, b = bits[d];
  if (b > 0 && (int)threadIdx.x < (1 << b)) dst[(size_t)d * THR_STRIDE + threadIdx.x] = src[(size_t)d * THR_STRIDE + threadIdx.x];
}

#define BE_TRY(expr)                   \
  do {                                 \
    hipError_t e_ = (expr);            \
    if (e_ != hipSuccess) return e_;   \
  } while (0)

}  // namespace

int bitvec_encode_tile_rows(int D) { return BE_WAVES * rows_per_wave(D); }

hipError_t launch_bitvec_encode(RowsRef X, int64_t n, const BitvecEncodePlan &p, uint64_t *out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (p.D < 1 || p.D > MAX_DIM || p.W < 1 || p.n_live < 1) return hipErrorInvalidValue;
  if (X.elem == 1) return launch_encode_rows(static_cast<const uint8_t *>(X.p), n, p, out, st);
  if (X.elem != 4) return hipErrorInvalidValue;
  return launch_encode_rows(static_cast<const float *>(X.p), n, p, out, st);
}

hipError_t bitvec_fit_thresholds(RowsRef X, int64_t n, int D, const int *bits, const float *E, float *d_thr, int *h_bad,
                                 hipStream_t st) {
  // columns per extract (launch_lutfit_project_columns takes 16 at most), fewer where 16 columns of keys pass 1 GB
  const int GROUP = (int)std::max<int64_t>(1, std::min<int64_t>(16, ((int64_t)1 << 28) / n));
  vaqhost::DevBuf keys, sorted, temp, scratch, d_bits, d_bad;
  const size_t col_bytes = (size_t)n * sizeof(uint32_t);
  BE_TRY(keys.ensure(col_bytes * GROUP));
  BE_TRY(sorted.ensure(col_bytes));
  BE_TRY(scratch.ensure((size_t)D * THR_STRIDE * sizeof(float)));
  BE_TRY(d_bits.ensure((size_t)D * sizeof(int)));
  BE_TRY(d_bad.ensure(sizeof(int)));
  size_t temp_bytes = 0;
  BE_TRY(rocprim::radix_sort_keys(nullptr, temp_bytes, keys.as<uint32_t>(), sorted.as<uint32_t>(), (size_t)n, 0u, 32u, st));
  BE_TRY(temp.ensure(temp_bytes ? temp_bytes : 16));
  BE_TRY(hipMemsetAsync(d_bad.p, 0, sizeof(int), st));
  BE_TRY(hipMemcpyAsync(d_bits.p, bits, (size_t)D * sizeof(int), hipMemcpyHostToDevice, st));
  for (int d0 = 0; d0 < D;) {
    if (bits[d0] == 0) {  // (an unallocated column is never looked at: it may hold anything)
      d0++;
      continue;
    }
    int w = 1;
    while (w < GROUP && d0 + w < D && bits[d0 + w] > 0) w++;
    BE_TRY(launch_lutfit_project_columns(X, n, D, E, d0, w, keys.as<uint32_t>(), d_bad.as<int>(), st));
    for (int c = 0; c < w; c++) {
      BE_TRY(rocprim::radix_sort_keys(temp.p, temp_bytes, keys.as<uint32_t>() + (size_t)c * n, sorted.as<uint32_t>(), (size_t)n,
                                      0u, 32u, st));
      hipLaunchKernelGGL(bitvec_thresholds_kernel, dim3(1), dim3(256), 0, st, sorted.as<uint32_t>(), n, bits[d0 + c],
                         scratch.as<float>() + (size_t)(d0 + c) * THR_STRIDE);
      BE_TRY(hipGetLastError());
    }
    d0 += w;
  }
  BE_TRY(hipMemcpyAsync(h_bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  BE_TRY(hipStreamSynchronize(st));
  if (*h_bad) return hipSuccess;
  hipLaunchKernelGGL(bitvec_thresholds_copy_kernel, dim3((unsigned)D), dim3(256), 0, st, scratch.as<float>(), d_bits.as<int>(),
                     d_thr);
  BE_TRY(hipGetLastError());
  return hipStreamSynchronize(st);  // (the scratch is freed on return)
}

}  // namespace vaq
