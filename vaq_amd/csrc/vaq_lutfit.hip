// vaq_lutfit.hip -- gfx950 kernels that BUILD a queryLUT index: the per-dimension quantile codebooks and the
// encoder of BitVecEngine::binaryEncodingLUT (BitVecEngine.hpp:811-840, :889-932).  The arithmetic is in
// vaq_lutfit.h, shared with the host; here is how it is spread over the chip.
//
// Fit, one column at a time (workspace: two key buffers of n words and rocprim's scratch):
//   lutfit_extract_kernel     column d of the row-major rows -> sortable keys; flags non-finite values
//   lutfit_project_columns_kernel  the sharded fit's form of it: up to 16 columns of a shard's RAW rows at once,
//                             the projection fused (no projected copy of the rows exists there)
//   rocprim::radix_sort_keys  the column ascending
//   lutfit_quantiles_kernel   Q[0 .. N] and the bucket ends (one workgroup: <= 257 values)
//   lutfit_means_kernel       one workgroup per bucket: the bucket's values are staged through LDS in
//                             coalesced tiles and ONE lane adds them in ascending order -- the order is the
//                             contract (centroids[i] += Z[lastidx], :829), no tree may replace it
// Encode: lut_encode_kernel streams the rows; PM (prefix maxima of Q) and the centres of a tile of
// dimensions sit in LDS, packed (2N + 1 floats per dimension).
#include "vaq_lutfit.h"
#include "vaq_lutfit_dev.h"
#include "vaqhip_dev.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <vector>

namespace vaq {
namespace {

using namespace lutfit;

// T: the rows' element, float or uint8_t (RowsRef).  A byte is widened where it is loaded, (float)uint8 is exact.
template <typename T>
__global__ __launch_bounds__(256) void lutfit_extract_kernel(const T *__restrict__ Xp, int64_t n, int D, int d,
                                                             uint32_t *__restrict__ keys, int *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  bool any_bad = false;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
    const float x = (float)Xp[r * D + d];
    any_bad = any_bad || !is_finite(x);
    keys[r] = float_to_key(x);
  }
  if (any_bad) atomicOr(bad, 1);
}

// ---- rows -> column keys, projection fused (the sharded fit, vaqhip_multi_lutfit.cpp) ----
// A workgroup takes PC_ROWS rows at a time, lane = row, so each of the W column stores of a wave is 64 consecutive
// words.  The rows pass through LDS in tiles of PC_JT inner indices, loaded coalesced (32 consecutive floats of a
// row per half-wave) and read back one row per lane; the row stride PC_STRIDE = 33 words is odd, so the 32 lanes of
// a half-wave hit 32 different banks both ways (a stride of D = 128 would put them all on one).  A thread keeps W
// accumulators; E[j][d0 + w] is the same for the whole wave and comes in as scalar loads.  Each y is ONE fmaf chain
// over j ascending from acc = 0.0f: project_kernel's / project_tile_kernel's value bit for bit (vaq_front.hip).
// 16 accumulators, the tile value and the addresses stay far below the 128 VGPRs at which a SIMD still holds four
// waves; LDS (33 KB) allows four workgroups per CU.  Rows and offsets are 64-bit: a shard of 125M x 128 has 1.6e10
// elements.
// Byte rows (T = uint8_t): the tile load and the transposing extract widen each byte as they load it, the tile holds
// floats and everything behind the load is unchanged.  The loads stay one element per lane -- a half-wave reads 32
// consecutive bytes of a row -- so they need no alignment (D = 5 or 33 puts a row at any byte) and the LDS pattern,
// stride 33, is the float form's: the same instructions on a quarter of the bytes.
constexpr int PC_ROWS = 256, PC_JT = 32, PC_STRIDE = PC_JT + 1, PC_MAX_W = 16;

template <int W, typename T>
__global__ __launch_bounds__(PC_ROWS) void lutfit_project_columns_kernel(const T *__restrict__ X, int64_t n, int D,
                                                                         const float *__restrict__ E, int d0,
                                                                         uint32_t *__restrict__ keys,
                                                                         int *__restrict__ bad) {
  __shared__ float tile[PC_ROWS * PC_STRIDE];
  const int tid = threadIdx.x;
  const int c = tid & (PC_JT - 1), r8 = tid / PC_JT;
  bool any_bad = false;
  for (int64_t row0 = (int64_t)blockIdx.x * PC_ROWS; row0 < n; row0 += (int64_t)gridDim.x * PC_ROWS) {
    const int64_t row = row0 + tid;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; w++) acc[w] = 0.0f;
    if (!E) {  // a transposing extract: the row's own values
      if (row < n) {
#pragma unroll
        for (int w = 0; w < W; w++) acc[w] = (float)X[row * D + d0 + w];
      }
    } else {
      for (int j0 = 0; j0 < D; j0 += PC_JT) {
        __syncthreads();  // (the tile before has been read)
#pragma unroll 8
        for (int i = 0; i < PC_JT; i++) {  // (PC_ROWS x PC_JT values by PC_ROWS threads)
          const int r = i * (PC_ROWS / PC_JT) + r8;
          const int64_t src = row0 + r;
          tile[r * PC_STRIDE + c] = (src < n && j0 + c < D) ? (float)X[src * D + j0 + c] : 0.0f;
        }
        __syncthreads();
        const int jn = D - j0 < PC_JT ? D - j0 : PC_JT;
        const float *e = E + (size_t)j0 * D + d0;
        for (int jj = 0; jj < jn; jj++, e += D) {
          const float x = tile[tid * PC_STRIDE + jj];
#pragma unroll
          for (int w = 0; w < W; w++) acc[w] = __builtin_fmaf(x, e[w], acc[w]);
        }
      }
    }
    if (row < n) {
#pragma unroll
      for (int w = 0; w < W; w++) {
        any_bad = any_bad || !is_finite(acc[w]);
        keys[(int64_t)w * n + row] = float_to_key(acc[w]);
      }
    }
  }
  if (any_bad) atomicOr(bad, 1);
}

// Z: the sorted keys.  q_out[257] (entries past N: 0), ends[N + 1]: bucket i is Z[ends[i] .. ends[i + 1])
__global__ __launch_bounds__(256) void lutfit_quantiles_kernel(const uint32_t *__restrict__ Z, int64_t n, int N,
                                                               float *__restrict__ q_out, int64_t *__restrict__ ends) {
  __shared__ float sQ[MAX_Q];
  __shared__ int64_t sAbove[MAX_CENT];
  for (int q = threadIdx.x; q < MAX_Q; q += 256) {
    const float v = q <= N ? quantile_at(Z, n, N, q) : 0.0f;
    sQ[q] = v;
    q_out[q] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += 256) sAbove[i] = first_above(Z, n, sQ[i + 1]);
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t lastidx = 0;
    ends[0] = 0;
    for (int i = 0; i < N; i++) {
      lastidx = bucket_end(lastidx, sAbove[i]);
      ends[i + 1] = lastidx;
    }
  }
}

constexpr int MEANS_THREADS = 256, MEANS_PER_THREAD = 8, MEANS_TILE = MEANS_THREADS * MEANS_PER_THREAD;

// grid = N buckets.  Two LDS tiles: while lane 0 adds tile t, the loads of tile t + 1 are in flight; one
// barrier per tile orders both (tile t + 2 is written after the barrier lane 0 reaches once it has read t).
__global__ __launch_bounds__(MEANS_THREADS) void lutfit_means_kernel(const uint32_t *__restrict__ Z,
                                                                     const int64_t *__restrict__ ends,
                                                                     const float *__restrict__ Q,
                                                                     float *__restrict__ cent) {
  __shared__ __attribute__((aligned(16))) float tile[2][MEANS_TILE];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int64_t begin = ends[i], end = ends[i + 1];
  float r[MEANS_PER_THREAD];
  auto load = [&](int64_t pos) {
#pragma unroll
    for (int k = 0; k < MEANS_PER_THREAD; k++) {
      const int64_t j = pos + k * MEANS_THREADS + tid;
      r[k] = j < end ? key_to_float(Z[j]) : 0.0f;
    }
  };
  float sum = 0.0f;  // setZero(), :853
  int b = 0;
  if (begin < end) load(begin);
  for (int64_t pos = begin; pos < end; pos += MEANS_TILE) {
#pragma unroll
    for (int k = 0; k < MEANS_PER_THREAD; k++) tile[b][k * MEANS_THREADS + tid] = r[k];
    __syncthreads();
    if (pos + MEANS_TILE < end) load(pos + MEANS_TILE);
    if (tid == 0) {
      const int m = (int)(end - pos < MEANS_TILE ? end - pos : MEANS_TILE);
      for (int j = 0; j < m; j++) sum += tile[b][j];
    }
    b ^= 1;
  }
  if (tid == 0) cent[i] = bucket_centroid(sum, (int)(end - begin), Q[i], Q[i + 1]);
}

constexpr int ENC_LUT_THREADS = 1024, ENC_LUT_ROWS = 256, ENC_LUT_MAX_TILE = 128;
constexpr int ENC_LUT_LDS_FLOATS = 15360;  // 60 KB of tables per workgroup: two workgroups per CU

// Dimensions [d0, d0 + W) of rows [0, n): lane e of a chunk of ENC_LUT_ROWS rows takes (row e / W, dimension
// e % W), so a wave reads and writes runs of W consecutive values per row.
__global__ __launch_bounds__(ENC_LUT_THREADS) void lut_encode_kernel(const float *__restrict__ Xp, int64_t n, int D,
                                                                     int d0, int W, const SubDesc *__restrict__ sub,
                                                                     const float *__restrict__ pm,
                                                                     const float *__restrict__ cent,
                                                                     uint16_t *__restrict__ codes) {
  extern __shared__ float tab[];
  __shared__ int sOff[ENC_LUT_MAX_TILE], sN[ENC_LUT_MAX_TILE];
  const int tid = threadIdx.x;
  const int c0 = sub[d0].cent_off;
  for (int j = 0; j < W; j++) {
    const int N = sub[d0 + j].ncent, co = sub[d0 + j].cent_off;
    const int off = 2 * (co - c0) + j;
    if (tid == 0) {
      sOff[j] = off;
      sN[j] = N;
    }
    for (int t = tid; t < 2 * N + 1; t += ENC_LUT_THREADS)
      tab[off + t] = t <= N ? pm[co + d0 + j + t] : cent[co + t - (N + 1)];
  }
  __syncthreads();
  for (int64_t row0 = (int64_t)blockIdx.x * ENC_LUT_ROWS; row0 < n; row0 += (int64_t)gridDim.x * ENC_LUT_ROWS) {
    const int rows = (int)(n - row0 < ENC_LUT_ROWS ? n - row0 : ENC_LUT_ROWS);
    const unsigned cnt = (unsigned)rows * (unsigned)W;
    for (unsigned e = tid; e < cnt; e += ENC_LUT_THREADS) {
      const unsigned r = e / (unsigned)W, j = e - r * (unsigned)W;
      const int64_t at = (row0 + r) * D + d0 + j;
      const float *t = tab + sOff[j];
      const int N = sN[j];
      codes[at] = encode_value(Xp[at], N, t, t + N + 1);
    }
  }
}

#define LF_TRY(expr)                      \
  do {                                    \
    hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

}  // namespace

hipError_t launch_lut_encode(const float *Xp, int64_t n, int D, const SubDesc *h_sub, const SubDesc *d_sub,
                             const float *d_pm, const float *d_cent, uint16_t *codes, int n_cu, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const int64_t want = (n + ENC_LUT_ROWS - 1) / ENC_LUT_ROWS;
  const unsigned grid = (unsigned)std::min<int64_t>(want, (int64_t)2 * std::max(n_cu, 1));
  for (int d0 = 0; d0 < D;) {
    int W = 0, floats = 0;
    while (d0 + W < D && W < ENC_LUT_MAX_TILE && floats + 2 * h_sub[d0 + W].ncent + 1 <= ENC_LUT_LDS_FLOATS) {
      floats += 2 * h_sub[d0 + W].ncent + 1;
      W++;
    }
    if (W == 0) return hipErrorInvalidValue;  // (a column of more than 256 centres: the caller refuses it first)
    hipLaunchKernelGGL(lut_encode_kernel, dim3(grid), dim3(ENC_LUT_THREADS), (size_t)floats * sizeof(float), st, Xp, n,
                       D, d0, W, d_sub, d_pm, d_cent, codes);
    LF_TRY(hipGetLastError());
    d0 += W;
  }
  return hipSuccess;
}

namespace {
template <typename T>
hipError_t project_columns_as(const T *X, int64_t n, int D, const float *E, int d0, int W, uint32_t *keys, int *d_bad,
                              hipStream_t st) {
  if (n == 0 || W == 0) return hipSuccess;
  if (W < 0 || W > PC_MAX_W || d0 < 0 || d0 + W > D) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<int64_t>((n + PC_ROWS - 1) / PC_ROWS, 4096));
  switch (W) {
#define PC_CASE(w)                                                                                                   \
  case w:                                                                                                            \
    hipLaunchKernelGGL((lutfit_project_columns_kernel<w, T>), grid, dim3(PC_ROWS), 0, st, X, n, D, E, d0, keys, d_bad); \
    break;
    PC_CASE(1) PC_CASE(2) PC_CASE(3) PC_CASE(4) PC_CASE(5) PC_CASE(6) PC_CASE(7) PC_CASE(8)
    PC_CASE(9) PC_CASE(10) PC_CASE(11) PC_CASE(12) PC_CASE(13) PC_CASE(14) PC_CASE(15) PC_CASE(16)
#undef PC_CASE
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_lutfit_project_columns(RowsRef X, int64_t n, int D, const float *E, int d0, int W, uint32_t *keys,
                                         int *d_bad, hipStream_t st) {
  if (X.elem == 1) return project_columns_as(static_cast<const uint8_t *>(X.p), n, D, E, d0, W, keys, d_bad, st);
  if (X.elem != 4) return hipErrorInvalidValue;
  return project_columns_as(static_cast<const float *>(X.p), n, D, E, d0, W, keys, d_bad, st);
}

hipError_t LutFitColumnWork::ensure(int64_t n, hipStream_t st) {
  const size_t key_bytes = (size_t)n * sizeof(uint32_t);
  LF_TRY(keys.ensure(key_bytes));
  LF_TRY(sorted.ensure(key_bytes));
  LF_TRY(ends.ensure((MAX_CENT + 1) * sizeof(int64_t)));
  temp_bytes = 0;
  LF_TRY(rocprim::radix_sort_keys(nullptr, temp_bytes, keys.as<uint32_t>(), sorted.as<uint32_t>(), (size_t)n, 0u, 32u,
                                  st));
  return temp.ensure(temp_bytes ? temp_bytes : 16);
}

hipError_t lut_fit_column_from_keys(LutFitColumnWork &w, int64_t n, int bits, float *d_q, float *d_cent, hipEvent_t *e,
                                    hipStream_t st) {
  const int N = 1 << bits;
  if (e) LF_TRY(hipEventRecord(e[0], st));
  LF_TRY(rocprim::radix_sort_keys(w.temp.p, w.temp_bytes, w.keys.as<uint32_t>(), w.sorted.as<uint32_t>(), (size_t)n, 0u,
                                  32u, st));
  if (e) LF_TRY(hipEventRecord(e[1], st));
  hipLaunchKernelGGL(lutfit_quantiles_kernel, dim3(1), dim3(256), 0, st, w.sorted.as<uint32_t>(), n, N, d_q,
                     w.ends.as<int64_t>());
  LF_TRY(hipGetLastError());
  if (e) LF_TRY(hipEventRecord(e[2], st));
  hipLaunchKernelGGL(lutfit_means_kernel, dim3((unsigned)N), dim3(MEANS_THREADS), 0, st, w.sorted.as<uint32_t>(),
                     w.ends.as<int64_t>(), d_q, d_cent);
  LF_TRY(hipGetLastError());
  if (e) LF_TRY(hipEventRecord(e[3], st));
  return hipSuccess;
}

// d_cent_out [D][256] (= centroidsMat, 256 x D column-major), d_q_out [D][257], *d_bad: set when a value is not
// finite (zeroed here).  Enqueues on `st`; the scratch is freed on return, so the stream is synchronised first.
// phase_ms (optional) [4]: extract, sort, quantiles, means, summed over the columns (device events).
hipError_t lut_fit_columns(const float *d_Xp, int64_t n, int D, const int *bits, float *d_cent_out, float *d_q_out,
                           int *d_bad, float *phase_ms, hipStream_t st) {
  return lut_fit_columns(RowsRef{d_Xp, 4}, n, D, bits, d_cent_out, d_q_out, d_bad, phase_ms, st);
}

hipError_t lut_fit_columns(RowsRef d_Xp, int64_t n, int D, const int *bits, float *d_cent_out, float *d_q_out,
                           int *d_bad, float *phase_ms, hipStream_t st) {
  if (d_Xp.elem != 4 && d_Xp.elem != 1) return hipErrorInvalidValue;
  LutFitColumnWork w;
  LF_TRY(w.ensure(n, st));
  LF_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), st));
  LF_TRY(hipMemsetAsync(d_cent_out, 0, (size_t)D * MAX_CENT * sizeof(float), st));
  std::vector<hipEvent_t> ev;
  struct EvFree {
    std::vector<hipEvent_t> &v;
    ~EvFree() { for (auto e : v) if (e) (void)hipEventDestroy(e); }
  } ev_free{ev};
  if (phase_ms) {
    ev.resize((size_t)D * 5);
    for (auto &e : ev) e = nullptr;
    for (auto &e : ev) LF_TRY(hipEventCreate(&e));
  }
  const unsigned ex_grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  for (int d = 0; d < D; d++) {
    hipEvent_t *e = phase_ms ? ev.data() + (size_t)d * 5 : nullptr;
    if (e) LF_TRY(hipEventRecord(e[0], st));
    if (d_Xp.elem == 1)
      hipLaunchKernelGGL(lutfit_extract_kernel<uint8_t>, dim3(ex_grid), dim3(256), 0, st,
                         static_cast<const uint8_t *>(d_Xp.p), n, D, d, w.keys.as<uint32_t>(), d_bad);
    else
      hipLaunchKernelGGL(lutfit_extract_kernel<float>, dim3(ex_grid), dim3(256), 0, st,
                         static_cast<const float *>(d_Xp.p), n, D, d, w.keys.as<uint32_t>(), d_bad);
    LF_TRY(hipGetLastError());
    // (e[1], the end of the extract, is the column fit's first event)
    LF_TRY(lut_fit_column_from_keys(w, n, bits[d], d_q_out + (size_t)d * MAX_Q, d_cent_out + (size_t)d * MAX_CENT,
                                    e ? e + 1 : nullptr, st));
  }
  LF_TRY(hipStreamSynchronize(st));
  if (phase_ms) {
    for (int p = 0; p < 4; p++) phase_ms[p] = 0.0f;
    for (int d = 0; d < D; d++)
      for (int p = 0; p < 4; p++) {
        float ms = 0.0f;
        LF_TRY(hipEventElapsedTime(&ms, ev[(size_t)d * 5 + p], ev[(size_t)d * 5 + p + 1]));
        phase_ms[p] += ms;
      }
  }
  return hipSuccess;
}

}  // namespace vaq
