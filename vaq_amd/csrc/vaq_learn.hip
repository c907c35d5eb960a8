// vaq_learn.hip -- gfx950 kernels of learnQuantization's device forms (VAQ.cpp:1118-1187; host side in
// vaqhip_learn.cpp, the arithmetic in learn_plan.h):
//   learn_gather_kernel  the sampled rows, float or byte, as dense float rows (a byte widened where it is loaded)
//   learn_slice_kernel   a chunk's tables [m][M][ksub] -> the column group's [sample][Mc][ksub]
//   learn_keys_kernel    one column of the group as radix-sortable keys, in table order; flags non-finite values
//   learn_fetch_kernel   the few order statistics the percentiles read
//   learn_loss_kernel    the quantisation loss of 7 alphas x Mc columns.  The order of the additions is the contract
//                        (l += (double)(ideal * ideal) row after row, VAQ.cpp:1176): per (alpha, column) ONE chain of
//                        double additions in table order, no tree may replace it.  A workgroup owns a column: waves
//                        1..3 compute a tile's seven terms per value into LDS as doubles, lanes 0..6 of wave 0 add the
//                        tile before -- one v_add_f64 serves the seven chains -- and one barrier per tile orders the
//                        two LDS tiles.  The chain is latency-bound by design: rows dependent f64 additions.
// Compiled with -ffp-contract=off as every unit: the term's (x - off) * sc - quant must not fuse.
#include "vaq_learn.h"

#include "learn_plan.h"
#include "vaq_lutfit.h"

namespace vaq {
namespace {

using learn::N_ALPHA;

template <typename T>
__global__ __launch_bounds__(256) void learn_gather_kernel(const T *__restrict__ X, const int *__restrict__ rows, int m,
                                                           int D, float *__restrict__ out) {
  const int64_t total = (int64_t)m * D, stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t i = e / D;
    const int j = (int)(e - i * D);
    out[e] = (float)X[(int64_t)rows[i] * D + j];
  }
}

__global__ __launch_bounds__(256) void learn_slice_kernel(const float *__restrict__ tables, int m, int M, int ksub,
                                                          int s0, int Mc, int64_t i0, float *__restrict__ group) {
  const int w = Mc * ksub;  // floats of one row of the group
  const int64_t total = (int64_t)m * w, stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t i = e / w;
    const int j = (int)(e - i * w);
    group[(i0 + i) * w + j] = tables[(i * M + s0) * ksub + j];
  }
}

__global__ __launch_bounds__(256) void learn_keys_kernel(const float *__restrict__ group, int64_t rows, int Mc, int ksub,
                                                         int sl, uint32_t *__restrict__ keys, int *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  bool any_bad = false;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < rows; v += stride) {
    const int64_t i = v / ksub;
    const int c = (int)(v - i * ksub);
    const float x = group[(i * Mc + sl) * ksub + c];
    any_bad = any_bad || !lutfit::is_finite(x);
    keys[v] = lutfit::float_to_key(x);
  }
  if (any_bad) atomicOr(bad, 1);
}

__global__ __launch_bounds__(64) void learn_fetch_kernel(const uint32_t *__restrict__ sorted,
                                                         const int64_t *__restrict__ idx, int n_idx,
                                                         float *__restrict__ out) {
  const int j = threadIdx.x;
  if (j < n_idx) out[j] = lutfit::key_to_float(sorted[idx[j]]);
}

constexpr int LOSS_THREADS = 256, LOSS_PRODUCERS = LOSS_THREADS - 64;
constexpr int LOSS_TILE = 512;                                            // values of the column per LDS tile
constexpr int LOSS_PER = (LOSS_TILE + LOSS_PRODUCERS - 1) / LOSS_PRODUCERS;  // values a producer thread takes
// a row of terms per alpha; + 2 doubles keeps the 16-byte alignment of the adders' paired reads and sets the seven
// lanes 4 banks apart instead of on one
constexpr int LOSS_STRIDE = LOSS_TILE + 2;

__global__ __launch_bounds__(LOSS_THREADS) void learn_loss_kernel(const float *__restrict__ group, int64_t rows, int Mc,
                                                                  int ksub, const float *__restrict__ floors,
                                                                  const float *__restrict__ scales,
                                                                  double *__restrict__ loss) {
  __shared__ __attribute__((aligned(16))) double terms[2][N_ALPHA][LOSS_STRIDE];  // 57.6 KB
  const int sl = blockIdx.x, tid = threadIdx.x;
  const bool adder = tid < 64;
  const int pt = tid - 64;  // producer thread
  float fl[N_ALPHA], sc[N_ALPHA], r[LOSS_PER];
#pragma unroll
  for (int a = 0; a < N_ALPHA; a++) {
    fl[a] = floors[a * Mc + sl];
    sc[a] = scales[a * Mc + sl];
  }
  // the tile's values that this producer takes: v = pos + k * LOSS_PRODUCERS + pt, read where the table holds them
  auto load = [&](int64_t pos) {
#pragma unroll
    for (int k = 0; k < LOSS_PER; k++) {
      const int64_t v = pos + k * LOSS_PRODUCERS + pt;
      const int64_t i = v / ksub;
      const int c = (int)(v - i * ksub);
      r[k] = (k * LOSS_PRODUCERS + pt < LOSS_TILE && v < rows) ? group[(i * Mc + sl) * ksub + c] : 0.0f;
    }
  };
  auto produce = [&](int b) {
#pragma unroll
    for (int k = 0; k < LOSS_PER; k++) {
      const int j = k * LOSS_PRODUCERS + pt;
      if (j < LOSS_TILE) {
#pragma unroll
        for (int a = 0; a < N_ALPHA; a++) terms[b][a][j] = learn::loss_term(r[k], fl[a], sc[a]);
      }
    }
  };
  if (!adder) {
    load(0);
    produce(0);
    if (LOSS_TILE < rows) load(LOSS_TILE);
  }
  __syncthreads();
  double l = 0.0;
  int b = 0;
  for (int64_t pos = 0; pos < rows; pos += LOSS_TILE) {
    if (!adder) {
      if (pos + LOSS_TILE < rows) {  // the tile after this one, while the adders are on this one
        produce(b ^ 1);
        if (pos + 2 * (int64_t)LOSS_TILE < rows) load(pos + 2 * (int64_t)LOSS_TILE);
      }
    } else if (tid < N_ALPHA) {
      const int m = (int)(rows - pos < LOSS_TILE ? rows - pos : LOSS_TILE);
      const double *t = terms[b][tid];
      int j = 0;
      for (; j + 4 <= m; j += 4) {
        const double2 p = *reinterpret_cast<const double2 *>(t + j), q = *reinterpret_cast<const double2 *>(t + j + 2);
        l += p.x;
        l += p.y;
        l += q.x;
        l += q.y;
      }
      for (; j < m; j++) l += t[j];
    }
    __syncthreads();
    b ^= 1;
  }
  if (tid < N_ALPHA) loss[tid * Mc + sl] = l;
}

unsigned grid_for(int64_t elems) { return (unsigned)std::min<int64_t>(std::max<int64_t>((elems + 255) / 256, 1), 4096); }

}  // namespace

hipError_t launch_learn_gather(RowsRef X, const int *rows, int m, int D, float *out, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  if (X.elem == 1)
    hipLaunchKernelGGL(learn_gather_kernel<uint8_t>, dim3(grid_for((int64_t)m * D)), dim3(256), 0, st,
                       static_cast<const uint8_t *>(X.p), rows, m, D, out);
  else if (X.elem == 4)
    hipLaunchKernelGGL(learn_gather_kernel<float>, dim3(grid_for((int64_t)m * D)), dim3(256), 0, st,
                       static_cast<const float *>(X.p), rows, m, D, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_learn_slice(const float *tables, int m, int M, int ksub, int s0, int Mc, int64_t i0, float *group,
                              hipStream_t st) {
  if (m <= 0) return hipSuccess;
  if (s0 < 0 || Mc < 1 || s0 + Mc > M) return hipErrorInvalidValue;
  hipLaunchKernelGGL(learn_slice_kernel, dim3(grid_for((int64_t)m * Mc * ksub)), dim3(256), 0, st, tables, m, M, ksub, s0,
                     Mc, i0, group);
  return hipGetLastError();
}

hipError_t launch_learn_keys(const float *group, int64_t sample, int Mc, int ksub, int sl, uint32_t *keys, int *d_bad,
                             hipStream_t st) {
  if (sl < 0 || sl >= Mc) return hipErrorInvalidValue;
  const int64_t rows = sample * ksub;
  hipLaunchKernelGGL(learn_keys_kernel, dim3(grid_for(rows)), dim3(256), 0, st, group, rows, Mc, ksub, sl, keys, d_bad);
  return hipGetLastError();
}

hipError_t launch_learn_fetch(const uint32_t *sorted, const int64_t *idx, int n_idx, float *out, hipStream_t st) {
  if (n_idx < 0 || n_idx > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(learn_fetch_kernel, dim3(1), dim3(64), 0, st, sorted, idx, n_idx, out);
  return hipGetLastError();
}

hipError_t launch_learn_loss(const float *group, int64_t sample, int Mc, int ksub, const float *floors,
                             const float *scales, double *loss, hipStream_t st) {
  if (Mc < 1 || sample < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(learn_loss_kernel, dim3((unsigned)Mc), dim3(LOSS_THREADS), 0, st, group, sample * ksub, Mc, ksub,
                     floors, scales, loss);
  return hipGetLastError();
}

}  // namespace vaq
