// vaq_kmeans.hip -- the k-means inside VAQ::clusterTI(true) on gfx950: KMeans::staticFitCodebook ->
// staticFitSampling (KMeans.hpp:487-652, called at VAQ.cpp:896-900), centre for centre and bit for bit.
//
// Compiled with -ffp-contract=off like every file of the library.  Every operation that decides a bit is a
// plain fp32 operation in the reference's order:
//   assign      sqrt((x - mean).squaredNorm()) per (row, centre), centres ascending, strict `<` on the square
//               roots (the first minimum wins, a NaN never does).  squaredNorm is Eigen's linear vectorised
//               reduction (Eigen/src/Core/Redux.h, 8-float packets, two accumulators, unaligned start 0):
//               sq_norm_eigen below
//   accumulate  the reference runs two OpenMP threads with a static schedule: rows [0, ceil(n/2)) and the rest.
//               Per thread, centre and column a float sum from +0 in ascending row order -- here a stable sort
//               of the rows by (half, centre) and one thread per (half, centre, column) walking its run
//   update      new = ((0 + p0) + p1) / float(c0 + c1); a centre whose new row is not elementwise == to the old
//               one is replaced (an empty cluster is 0 / 0 = NaN, unequal for ever: the loop then runs to
//               max_iter, as the reference's does)
// No float atomics, no MFMA, no reassociation.
#include "vaq_kernels.h"
#include "vaqhip_dev.h"

#include <algorithm>
#include <chrono>
#include <rocprim/device/device_radix_sort.hpp>

#include <float.h>
#include <math.h>

namespace vaq {

// floats of centres a workgroup of the assign kernel stages in LDS at a time
constexpr int KM_STAGE_FLOATS = 4096;
// bytes of LDS its tile of decoded rows may take; wider rows are read from global memory
constexpr int KM_TILE_BYTES = 40 * 1024;

// sample codes [rows][seg] out of the N x M matrix in original row order; ids == nullptr: the first `rows` rows
__global__ void km_gather_codes_kernel(const uint16_t *__restrict__ codes, int M, const int *__restrict__ ids,
                                       int64_t rows, int seg, uint16_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * seg) return;
  const int64_t r = i / seg;
  const int s = (int)(i % seg);
  out[i] = codes[(ids ? (int64_t)ids[r] : r) * M + s];
}

// X[r] = the centroids of row r's codes side by side (KMeans.hpp:631-646)
__global__ void km_decode_kernel(const uint16_t *__restrict__ scodes, int64_t rows, int seg, int L,
                                 const SubDesc *__restrict__ sub, const float *__restrict__ cent,
                                 float *__restrict__ X) {
  const int d = seg * L;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * d) return;
  const int64_t r = i / d;
  const int c = (int)(i % d), s = c / L, j = c % L;
  const SubDesc sd = sub[s];
  X[i] = cent[sd.cent_off + (size_t)(scodes[r * seg + s] & (sd.ncent - 1)) * L + j];
}

// means[i] = X[seed_rows[i]] (KMeans.hpp:516-520)
__global__ void km_seed_kernel(const float *__restrict__ X, int d, const int *__restrict__ seed_rows, int T,
                               float *__restrict__ means) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * d) return;
  means[i] = X[(size_t)seed_rows[i / d] * d + i % d];
}

__device__ __forceinline__ float km_sq(float x, float m) {
  const float t = x - m;
  return t * t;
}

// (x - m).squaredNorm() as Eigen reduces it; x[j] is read at xs[j * xstride] (UNIT: at xs[j])
template <bool UNIT>
__device__ __forceinline__ float sq_norm_eigen(const float *xs, int xstride, const float *__restrict__ m, int d) {
#define T_(j) km_sq(xs[UNIT ? (size_t)(j) : (size_t)(j) * xstride], m[j])
  if (d < 8) {  // too small to vectorise: res = coeff(0); res += coeff(i)
    float res = T_(0);
    for (int j = 1; j < d; j++) res += T_(j);
    return res;
  }
  const int end1 = (d / 8) * 8, end2 = (d / 16) * 16;
  float a0[8], a1[8];
#pragma unroll
  for (int l = 0; l < 8; l++) a0[l] = T_(l);
  if (end1 > 8) {
#pragma unroll
    for (int l = 0; l < 8; l++) a1[l] = T_(8 + l);
    for (int i = 16; i < end2; i += 16) {
#pragma unroll
      for (int l = 0; l < 8; l++) a0[l] += T_(i + l);
#pragma unroll
      for (int l = 0; l < 8; l++) a1[l] += T_(i + 8 + l);
    }
#pragma unroll
    for (int l = 0; l < 8; l++) a0[l] += a1[l];
    if (end1 > end2) {
#pragma unroll
      for (int l = 0; l < 8; l++) a0[l] += T_(end2 + l);
    }
  }
  // predux<Packet8f>: the halves added, then (b0 + b2) + (b1 + b3)
  float res = ((a0[0] + a0[4]) + (a0[2] + a0[6])) + ((a0[1] + a0[5]) + (a0[3] + a0[7]));
  for (int j = end1; j < d; j++) res += T_(j);
  return res;
#undef T_
}

// One row per thread.  X_LDS: the workgroup's decoded rows sit in LDS as [dim][row] (each thread reads its own
// column, conflict-free); else every thread reads its row from global memory.  The centres pass through LDS
// `stage` at a time and are read with wave-uniform addresses (broadcast).
// keys[r] = half * T + centre, vals[r] = r: the input of the stable sort that orders the accumulation.
template <bool X_LDS>
__global__ void km_assign_kernel(const float *__restrict__ X, int n, int d, const float *__restrict__ means, int T,
                                 int stage, int half_rows, unsigned *__restrict__ keys, unsigned *__restrict__ vals,
                                 int *__restrict__ flags) {
  extern __shared__ float km_lds[];
  float *cs = km_lds;                         // [stage][d]
  float *xt = km_lds + (size_t)stage * d;     // [d][R]
  const int R = blockDim.x, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int64_t r = r0 + tid;
  const int64_t rr = r < n ? r : n - 1;  // (rows past the end work on the last row and store nothing)
  if (X_LDS) {
    const int64_t lim = (int64_t)n * d;
    for (int i = tid; i < R * d; i += R) {
      const int64_t g = r0 * d + i;
      xt[(size_t)(i % d) * R + i / d] = g < lim ? X[g] : 0.0f;
    }
  }
  float best = FLT_MAX;
  int idx = -1;
  for (int c0 = 0; c0 < T; c0 += stage) {
    const int cn = min(stage, T - c0);
    __syncthreads();  // the last stage is read, the tile is written
    for (int i = tid; i < cn * d; i += R) cs[i] = means[(size_t)c0 * d + i];
    __syncthreads();
    for (int c = 0; c < cn; c++) {
      const float d2 = X_LDS ? sq_norm_eigen<false>(xt + tid, R, cs + (size_t)c * d, d)
                             : sq_norm_eigen<true>(X + (size_t)rr * d, 1, cs + (size_t)c * d, d);
      const float dist = sqrtf(d2);
      if (dist < best) {
        best = dist;
        idx = c0 + c;
      }
    }
  }
  if (r < n) {
    if (idx < 0) flags[1] = 1;  // the reference indexes row -1 here
    keys[r] = (unsigned)((r >= half_rows ? T : 0) + max(idx, 0));
    vals[r] = (unsigned)r;
  }
}

// run [start, end) of every key in the sorted keys (both preset to 0: keys that do not occur are empty)
__global__ void km_bounds_kernel(const unsigned *__restrict__ keys, int n, int *__restrict__ start,
                                 int *__restrict__ end) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i];
  if (i == 0 || keys[i - 1] != k) start[k] = i;
  if (i == n - 1 || keys[i + 1] != k) end[k] = i + 1;
}

// part[(half * T + c) * d + col] = the rows of that run added from +0 in ascending row order; neighbouring
// threads take neighbouring columns of the same run
__global__ void km_accumulate_kernel(const float *__restrict__ X, int d, const unsigned *__restrict__ rows_sorted,
                                     const int *__restrict__ start, const int *__restrict__ end, int n_runs,
                                     float *__restrict__ part) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n_runs * d) return;
  const int g = (int)(gid / d), col = (int)(gid % d);
  float sum = 0.0f;
  for (int i = start[g], e = end[g]; i < e; i++) sum += X[(size_t)rows_sorted[i] * d + col];
  part[gid] = sum;
}

// one wavefront per centre (KMeans.hpp:586-604)
__global__ __launch_bounds__(64) void km_update_kernel(const float *__restrict__ part, const int *__restrict__ start,
                                                      const int *__restrict__ end, int T, int d,
                                                      float *__restrict__ means, int *__restrict__ flags) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int count = (end[c] - start[c]) + (end[T + c] - start[T + c]);
  const float *p0 = part + (size_t)c * d, *p1 = part + (size_t)(T + c) * d;
  float *m = means + (size_t)c * d;
  bool differs = false;
  for (int j = lane; j < d; j += 64) {
    const float v = ((0.0f + p0[j]) + p1[j]) / (float)count;
    if (!(v == m[j])) differs = true;
  }
  if (!__any(differs)) return;
  for (int j = lane; j < d; j += 64) m[j] = ((0.0f + p0[j]) + p1[j]) / (float)count;
  if (lane == 0) flags[0] = 1;
}

hipError_t launch_kmeans_gather(const uint16_t *d_codes, int M, const int *d_ids, int rows, int seg,
                                uint16_t *d_scodes, hipStream_t st) {
  const int64_t n = (int64_t)rows * seg;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(km_gather_codes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_codes, M, d_ids,
                     (int64_t)rows, seg, d_scodes);
  return hipGetLastError();
}

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
} // namespace

hipError_t kmeans_fit(const uint16_t *d_scodes, int rows, int seg, int L, const SubDesc *sub, const float *cent,
                      const int *seed_rows, int T, int max_iter, float *d_means, int *iters_out, int *no_centre_out,
                      KmeansPhases *phases, hipStream_t st) {
  const int d = seg * L, n = rows, n_runs = 2 * T;
  hipError_t e;
  // (freed on return, after the stream is synchronised)
  vaqhost::DevBuf b_x, b_seed, b_keys_in, b_keys_out, b_vals_in, b_vals_out, b_bounds, b_part, b_flags, b_temp;
  if ((e = b_x.ensure((size_t)n * d * sizeof(float))) != hipSuccess ||
      (e = b_seed.ensure((size_t)T * sizeof(int))) != hipSuccess ||
      (e = b_keys_in.ensure((size_t)n * 4)) != hipSuccess || (e = b_keys_out.ensure((size_t)n * 4)) != hipSuccess ||
      (e = b_vals_in.ensure((size_t)n * 4)) != hipSuccess || (e = b_vals_out.ensure((size_t)n * 4)) != hipSuccess ||
      (e = b_bounds.ensure((size_t)2 * n_runs * sizeof(int))) != hipSuccess ||
      (e = b_part.ensure((size_t)n_runs * d * sizeof(float))) != hipSuccess ||
      (e = b_flags.ensure(2 * sizeof(int))) != hipSuccess)
    return e;
  float *X = b_x.as<float>();
  unsigned *keys_in = b_keys_in.as<unsigned>(), *keys_out = b_keys_out.as<unsigned>();
  unsigned *vals_in = b_vals_in.as<unsigned>(), *vals_out = b_vals_out.as<unsigned>();
  int *start = b_bounds.as<int>(), *end = start + n_runs, *flags = b_flags.as<int>();
  unsigned key_bits = 1;
  while ((1u << key_bits) < (unsigned)n_runs) key_bits++;
  size_t temp_bytes = 0;
  if ((e = rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u,
                                     key_bits, st)) != hipSuccess ||
      (e = b_temp.ensure(temp_bytes ? temp_bytes : 16)) != hipSuccess)
    return e;

  const int64_t nd = (int64_t)n * d;
  hipLaunchKernelGGL(km_decode_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, d_scodes, (int64_t)n,
                     seg, L, sub, cent, X);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(b_seed.p, seed_rows, (size_t)T * sizeof(int), hipMemcpyHostToDevice, st)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)((T * d + 255) / 256)), dim3(256), 0, st, X, d,
                     b_seed.as<int>(), T, d_means);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  // launch shape of the assign kernel: the widest workgroup whose tile of decoded rows fits
  int R = 256;
  while (R > 64 && (size_t)R * d * sizeof(float) > KM_TILE_BYTES) R >>= 1;
  const bool x_lds = (size_t)R * d * sizeof(float) <= KM_TILE_BYTES;
  const int stage = std::max(1, std::min(T, KM_STAGE_FLOATS / d));
  const size_t lds = ((size_t)stage * d + (x_lds ? (size_t)R * d : 0)) * sizeof(float);
  const unsigned assign_grid = (unsigned)((n + R - 1) / R);
  const int half_rows = (n + 1) / 2;  // schedule(static) over two threads

  if (phases) *phases = KmeansPhases{};
  auto phase_end = [&](double *acc, std::chrono::steady_clock::time_point &t0) -> hipError_t {
    if (!phases) return hipSuccess;
    hipError_t pe = hipStreamSynchronize(st);
    *acc += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    return pe;
  };
  int iters = 0, host_flags[2] = {1, 0};
  if (phases && (e = hipStreamSynchronize(st)) != hipSuccess) return e;
  auto t0 = std::chrono::steady_clock::now();
  while (host_flags[0] && iters < max_iter) {
    if ((e = hipMemsetAsync(flags, 0, 2 * sizeof(int), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(start, 0, (size_t)2 * n_runs * sizeof(int), st)) != hipSuccess) return e;
    if (x_lds)
      hipLaunchKernelGGL(km_assign_kernel<true>, dim3(assign_grid), dim3(R), lds, st, X, n, d, d_means, T, stage,
                         half_rows, keys_in, vals_in, flags);
    else
      hipLaunchKernelGGL(km_assign_kernel<false>, dim3(assign_grid), dim3(R), lds, st, X, n, d, d_means, T, stage,
                         half_rows, keys_in, vals_in, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = phase_end(phases ? &phases->assign_ms : nullptr, t0)) != hipSuccess) return e;
    // stable: rows of equal (half, centre) stay in ascending order
    if ((e = rocprim::radix_sort_pairs(b_temp.p, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u,
                                       key_bits, st)) != hipSuccess)
      return e;
    hipLaunchKernelGGL(km_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys_out, n, start, end);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(km_accumulate_kernel, dim3((unsigned)(((int64_t)n_runs * d + 255) / 256)), dim3(256), 0, st, X,
                       d, vals_out, start, end, n_runs, b_part.as<float>());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = phase_end(phases ? &phases->accumulate_ms : nullptr, t0)) != hipSuccess) return e;
    hipLaunchKernelGGL(km_update_kernel, dim3(T), dim3(64), 0, st, b_part.as<float>(), start, end, T, d, d_means,
                       flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(host_flags, flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if ((e = phase_end(phases ? &phases->update_ms : nullptr, t0)) != hipSuccess) return e;
    iters++;
    if (host_flags[1]) break;
  }
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  *iters_out = iters;
  *no_centre_out = host_flags[1];
  return hipSuccess;
}

} // namespace vaq
