// vaq_train.hip -- gfx950 kernels of the training front half (VAQ.cpp:11-61; host side in vaqhip_train.cpp):
//   moment_tile_kernel    one tile of 1024 sample positions x one 32 x 32 block of the upper triangle: every thread
//                         adds the products x_ri * x_rj of its four entries row after row, ascending, from +0, in
//                         double (the product of two floats is exact; plain v_mul_f64 / v_add_f64, no MFMA: its order
//                         over k is not ours to restate).  The sampled rows are gathered where they are loaded, a byte
//                         widened there.  Positions past the sample and columns past D are loaded as +0: adding the
//                         product +0 changes no bit of a sum that started at +0.
//   moment_reduce_kernel  the tile partials added in ascending tile order from +0 (no atomics), mirrored below the
//                         diagonal; the float rounding beside it on request
//   jacobi_cols_kernel    a workgroup per pair of the step: the rotation from the pair's own a_pp, a_qq, a_pq (read by
//   jacobi_rows_kernel    every thread before the first write), its columns of A and V; then its rows of A and the two
//                         zeros.  Ordinary launches in stream order: no cooperative launch, no grid barrier, no flag.
// Compiled with -ffp-contract=off as every unit.
#include "vaq_train.h"

#include "train_plan.h"

namespace vaq {
namespace {

using train::MOMENT_TILE;
using train::Rot;
constexpr int MB = 32;  // edge of an output block
constexpr int MR = 64;  // rows staged per round

__device__ __forceinline__ void block_of(int b, int nb, int *bi, int *bj) {
  // b-th block of the upper triangle, row by row: (0,0) (0,1) .. (0,nb-1) (1,1) ..
  int i = 0, rem = b;
  while (rem >= nb - i) {
    rem -= nb - i;
    i++;
  }
  *bi = i;
  *bj = i + rem;
}

template <typename T>
__global__ __launch_bounds__(256) void moment_tile_kernel(const T *__restrict__ X, const int *__restrict__ rows, int64_t s,
                                                          int D, int64_t tile0, double *__restrict__ part) {
  __shared__ double xi[MR][MB], xj[MR][MB];
  const int nb = (D + MB - 1) / MB;
  int bi, bj;
  block_of((int)blockIdx.x, nb, &bi, &bj);
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int64_t pos0 = (tile0 + blockIdx.y) * MOMENT_TILE;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < MOMENT_TILE; r0 += MR) {
    if (pos0 + r0 >= s) break;  // (uniform: nothing but +0 follows)
    for (int e = tid; e < MR * MB; e += 256) {
      const int r = e / MB, c = e % MB;
      const int64_t pos = pos0 + r0 + r;
      double vi = 0.0, vj = 0.0;
      if (pos < s) {
        const int64_t row = rows ? (int64_t)rows[pos] : pos;
        if (bi * MB + c < D) vi = (double)X[row * D + bi * MB + c];
        if (bj * MB + c < D) vj = (double)X[row * D + bj * MB + c];
      }
      xi[r][c] = vi;
      xj[r][c] = vj;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < MR; r++) {
      const double b = xj[r][tx];
#pragma unroll
      for (int u = 0; u < 4; u++) acc[u] = acc[u] + xi[r][ty * 4 + u] * b;
    }
    __syncthreads();
  }
  const int j = bj * MB + tx;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = bi * MB + ty * 4 + u;
    if (i < D && j < D) part[((size_t)blockIdx.y * D + i) * D + j] = acc[u];
  }
}

__global__ __launch_bounds__(256) void moment_reduce_kernel(const double *__restrict__ part, int tiles, int D, int first,
                                                            double *__restrict__ out, float *__restrict__ out_f) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)D * D) return;
  const int i = (int)(e / D), j = (int)(e % D);
  if (j < i) return;  // (written by its mirror)
  double total = first ? 0.0 : out[e];
  for (int t = 0; t < tiles; t++) total = total + part[(size_t)t * D * D + e];
  out[e] = total;
  out[(size_t)j * D + i] = total;
  if (out_f) {
    out_f[e] = (float)total;
    out_f[(size_t)j * D + i] = (float)total;
  }
}

__global__ __launch_bounds__(256) void finite_kernel(const double *__restrict__ A, int64_t n, int *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  bool any = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    const double v = A[e];
    any = any || !(fabs(v) <= 1.7976931348623157e308);
  }
  if (any) atomicOr(bad, 1);
}

__global__ __launch_bounds__(256) void identity_kernel(double *__restrict__ V, int D) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)D * D) return;
  V[e] = (e / D == e % D) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void jacobi_cols_kernel(double *__restrict__ A, double *__restrict__ V, int D, int r,
                                                          Rot *__restrict__ rot, int *__restrict__ count) {
  int p = 0, q = 0;
  Rot R{1.0, 0.0, 0};
  const bool has = train::jacobi_pair(D, r, (int)blockIdx.x, &p, &q) != 0;  // (uniform over the workgroup)
  if (has) R = train::jacobi_rot(A[(size_t)p * D + p], A[(size_t)q * D + q], A[(size_t)p * D + q]);
  __syncthreads();  // every thread holds the rotation before a_pp, a_qq, a_pq are overwritten
  if (threadIdx.x == 0) {
    rot[blockIdx.x] = R;
    if (R.apply) atomicAdd(count, 1);
  }
  if (!R.apply) return;
  for (int k = threadIdx.x; k < D; k += 256) {
    train::jacobi_apply(R, &A[(size_t)k * D + p], &A[(size_t)k * D + q]);
    train::jacobi_apply(R, &V[(size_t)k * D + p], &V[(size_t)k * D + q]);
  }
}

__global__ __launch_bounds__(256) void jacobi_rows_kernel(double *__restrict__ A, int D, int r, const Rot *__restrict__ rot) {
  const Rot R = rot[blockIdx.x];
  int p = 0, q = 0;
  if (!R.apply || !train::jacobi_pair(D, r, (int)blockIdx.x, &p, &q)) return;
  for (int k = threadIdx.x; k < D; k += 256) {
    double x = A[(size_t)p * D + k], y = A[(size_t)q * D + k];
    train::jacobi_apply(R, &x, &y);
    A[(size_t)p * D + k] = k == q ? 0.0 : x;
    A[(size_t)q * D + k] = k == p ? 0.0 : y;
  }
}

}  // namespace

int moment_chunk_tiles(int D, int64_t tiles, size_t bytes) {
  const size_t per = (size_t)D * D * sizeof(double);
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(tiles, 32768), (int64_t)(bytes / per)));
}

hipError_t launch_train_moment(RowsRef X, const int *d_rows, int64_t s, int D, double *d_part, int chunk_tiles,
                               double *d_out, float *d_out_f, hipStream_t st) {
  const int nb = (D + MB - 1) / MB;
  const int64_t tiles = (s + MOMENT_TILE - 1) / MOMENT_TILE;
  const unsigned red_blocks = (unsigned)(((int64_t)D * D + 255) / 256);
  for (int64_t t0 = 0; t0 < tiles; t0 += chunk_tiles) {
    const int cnt = (int)std::min<int64_t>(chunk_tiles, tiles - t0);
    const dim3 grid((unsigned)(nb * (nb + 1) / 2), (unsigned)cnt);
    if (X.elem == 1)
      moment_tile_kernel<uint8_t><<<grid, 256, 0, st>>>(static_cast<const uint8_t *>(X.p), d_rows, s, D, t0, d_part);
    else
      moment_tile_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float *>(X.p), d_rows, s, D, t0, d_part);
    const bool last = t0 + cnt >= tiles;
    moment_reduce_kernel<<<red_blocks, 256, 0, st>>>(d_part, cnt, D, t0 == 0, d_out, last ? d_out_f : nullptr);
  }
  return hipGetLastError();
}

hipError_t launch_train_finite(const double *d_A, int64_t n, int *d_bad, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
  finite_kernel<<<blocks, 256, 0, st>>>(d_A, n, d_bad);
  return hipGetLastError();
}

hipError_t launch_train_identity(double *d_V, int D, hipStream_t st) {
  identity_kernel<<<(unsigned)(((int64_t)D * D + 255) / 256), 256, 0, st>>>(d_V, D);
  return hipGetLastError();
}

hipError_t launch_train_jacobi_step(double *d_A, double *d_V, int D, int r, Rot *d_rot, int *d_count, hipStream_t st) {
  const unsigned slots = (unsigned)train::jacobi_slots(D);
  jacobi_cols_kernel<<<slots, 256, 0, st>>>(d_A, d_V, D, r, d_rot, d_count);
  jacobi_rows_kernel<<<slots, 256, 0, st>>>(d_A, D, r, d_rot);
  return hipGetLastError();
}

}  // namespace vaq
