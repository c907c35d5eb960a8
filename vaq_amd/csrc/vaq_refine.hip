// vaq_refine.hip -- VAQ::refine (VAQ.cpp:849-876) over raw rows resident on the device, with the reference's own
// numbers: the distance is (XTest.row(q) - XTrain.row(l)).squaredNorm() in Eigen's summation order (sq_norm_eigen in
// vaq_restated.h is the specification), the k best are kept by the reference's heap on request.
//
// One workgroup per query, the query row staged in LDS.  A candidate row is read by 16 adjacent lanes, 64 contiguous
// bytes per step, four candidates per wave.  Lane j of the group IS Eigen's accumulator lane: a0[j] for j < 8,
// a1[j - 8] otherwise, adding (q[i + j] - y[i + j])^2 for i = 0, 16, 32, ... in that order.  Then, inside the 16 lanes:
// a0 += a1; the odd eighth packet (D mod 16 >= 8) is added to a0; predux = ((a0+a4)+(a2+a6)) + ((a1+a5)+(a3+a7)); the
// scalar tail is added element by element.  The shuffles move operands between lanes, they do not regroup the sums:
// every addition has the operands the specification gives it (fp add commutes, its grouping is what is fixed).
// Compiled with -ffp-contract=off like the rest: no FMA, no MFMA, no float atomics; plain vector stores.
//
// Rows are float or uint8 (RowsRef; a bvecs dataset kept as its bytes): the row type is a template argument of the two
// kernels that read rows, a byte is widened where it is loaded ((float)uint8 is exact) and nothing after the load
// differs -- the same instruction count, a quarter of the bytes.
//
// A label that is negative or outside [id_base, id_base + N) is skipped HERE, before its row's address is formed
// (the reference would read out of bounds): a device caller can hand over any list.
//
// The multi-device refiner (vaqhip_multi_refiner.cpp) runs the two halves apart: refine_dist_kernel on every shard
// (the same rf_group_sq_norm over the rows the shard holds), refine_select_kernel once over the gathered distances.
// A candidate's distance depends on its own row only and the selection on the R (distance, label) pairs in candidate
// order only, so the answer is refine_rows_kernel's slot for slot.
#include "refine_owner.h"
#include "vaq_refine_group.h"
#include "vaq_refine.h"
#include "vaq_restated.h"
#include "vaq_scan.h"

namespace vaq {

constexpr int RF_THREADS = 256;
constexpr int RF_CAP = 2048;    // candidates per query
constexpr int RF_GROUPS = RF_THREADS / RF_GROUP;

// One candidate slot of the selection's input: what refine_rows_kernel and refine_select_kernel both leave in sd / si.
template <bool EXACT>
__device__ __forceinline__ void rf_fill_slot(float *sd, int *si, int c, bool valid, float res, int lab) {
  if (EXACT) {
    sd[c] = valid ? res : INFINITY;
    si[c] = lab;
  } else {
    const bool in = valid && res < FLT_MAX;
    sd[c] = in ? res : INFINITY;
    si[c] = in ? lab : ID_SENTINEL;
  }
}

// The selection over the R slots of sd / si, the tail of both kernels.
// EXACT: the k best are what the reference's loop leaves (VAQ.cpp:863-872: heap_heapify, pop + push when
// heap_top > dist, heap_reorder), replayed by one thread over the R distances in candidate order.  Otherwise the k
// smallest by (distance, label).  Either way a distance that is not below FLT_MAX never enters (the heap starts from
// FLT_MAX: an infinite or NaN distance fails heap_top > dist), duplicates are kept, unfilled slots are -1 / FLT_MAX.
// The caller's writes to sd / si need no barrier before the call.
template <bool EXACT>
__device__ __forceinline__ void rf_select(float *sd, int *si, float *hv, int *hi, int *s_kept, int R, int k, int tid,
                                          int32_t *__restrict__ labels, float *__restrict__ dist, size_t o) {
  if (EXACT) {
    __syncthreads();
    if (tid == 0) {
      refheap::heapify(k, hv, hi);
      for (int i = 0; i < R; i++) {
        const float d = sd[i];
        if (hv[0] > d) {
          refheap::pop(k, hv, hi);
          refheap::push(k, hv, hi, d, si[i]);
        }
      }
      *s_kept = refheap::reorder(k, hv, hi);
    }
    __syncthreads();
    const int kept = *s_kept;
    for (int i = tid; i < k; i += RF_THREADS) {
      labels[o + i] = i < kept ? hi[k - kept + i] : -1;
      dist[o + i] = i < kept ? hv[k - kept + i] : FLT_MAX;
    }
  } else {
    int P = 2;
    while (P < R) P <<= 1;
    for (int i = R + tid; i < P; i += RF_THREADS) {
      sd[i] = INFINITY;
      si[i] = ID_SENTINEL;
    }
    __syncthreads();
    bitonic_sort<true>(sd, si, P, tid, RF_THREADS);
    for (int i = tid; i < k; i += RF_THREADS) {
      const bool ok = i < P && si[i] != ID_SENTINEL;
      labels[o + i] = ok ? si[i] : -1;
      dist[o + i] = ok ? sd[i] : FLT_MAX;
    }
  }
}

template <bool EXACT, typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_rows_kernel(const float *__restrict__ Q, int D,
                                                                 const T *__restrict__ rows, int64_t N,
                                                                 int64_t id_base, const int32_t *__restrict__ labels_in,
                                                                 int R, int k, int32_t *__restrict__ labels,
                                                                 float *__restrict__ dist) {
  __shared__ float sd[RF_CAP];
  __shared__ int si[RF_CAP];
  __shared__ float hv[EXACT ? RF_CAP : 1];
  __shared__ int hi[EXACT ? RF_CAP : 1];
  __shared__ int s_kept;
  extern __shared__ float qs[];
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += RF_THREADS) qs[j] = Q[(size_t)q * D + j];
  __syncthreads();
  const int g = tid / RF_GROUP, j = tid % RF_GROUP, gbase = (tid & 63) & ~(RF_GROUP - 1);
  for (int c0 = 0; c0 < R; c0 += RF_GROUPS) {  // (uniform trip count: the shuffles run in whole waves)
    const int c = c0 + g;
    const int lab = c < R ? labels_in[(size_t)q * R + c] : -1;
    const int64_t row = (int64_t)lab - id_base;
    const bool valid = lab >= 0 && row >= 0 && row < N;
    const T *y = rows + (valid ? (size_t)row * D : (size_t)0);
    const float res = rf_group_sq_norm(qs, y, D, valid, j, gbase);
    if (j == 0 && c < R) rf_fill_slot<EXACT>(sd, si, c, valid, res, lab);
  }
  rf_select<EXACT>(sd, si, hv, hi, &s_kept, R, k, tid, labels, dist, (size_t)q * k);
}

// The multi-device refiner, one shard's part: the distances of the candidates whose rows this shard holds (labels
// [lo_label, lo_label + n), row 0 of `rows` carrying lo_label), written to their own slots of the [nq][R] plane.  Every
// other slot is left alone: the select kernel reads a slot only from the plane of the shard that owns its label.
template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_dist_kernel(const float *__restrict__ Q, int D,
                                                                 const T *__restrict__ rows, int64_t n,
                                                                 int64_t lo_label, const int32_t *__restrict__ labels_in,
                                                                 int R, float *__restrict__ plane) {
  extern __shared__ float qs[];
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += RF_THREADS) qs[j] = Q[(size_t)q * D + j];
  __syncthreads();
  const int g = tid / RF_GROUP, j = tid % RF_GROUP, gbase = (tid & 63) & ~(RF_GROUP - 1);
  for (int c0 = 0; c0 < R; c0 += RF_GROUPS) {  // (uniform trip count, as above)
    const int c = c0 + g;
    const int lab = c < R ? labels_in[(size_t)q * R + c] : -1;
    const int64_t row = (int64_t)lab - lo_label;
    const bool valid = lab >= 0 && row >= 0 && row < n;
    const T *y = rows + (valid ? (size_t)row * D : (size_t)0);
    const float res = rf_group_sq_norm(qs, y, D, valid, j, gbase);
    if (j == 0 && valid) plane[(size_t)q * R + c] = res;
  }
}

// The multi-device refiner's selection, on the first device: slot c of query q takes its distance from the plane of
// the shard that owns its label (planes[owner * plane_stride + q * R + c]; refine_owner is the host's function too); a
// label nobody owns is skipped as refine_rows_kernel skips it.  Then the same selection over the same sd / si.
template <bool EXACT>
__global__ __launch_bounds__(RF_THREADS) void refine_select_kernel(const int32_t *__restrict__ labels_in,
                                                                   const float *__restrict__ planes, size_t plane_stride,
                                                                   RefineBounds bounds, int R, int k,
                                                                   int32_t *__restrict__ labels, float *__restrict__ dist) {
  __shared__ float sd[RF_CAP];
  __shared__ int si[RF_CAP];
  __shared__ float hv[EXACT ? RF_CAP : 1];
  __shared__ int hi[EXACT ? RF_CAP : 1];
  __shared__ int s_kept;
  __shared__ int64_t sb[RF_MAX_SHARDS + 1];
  const int q = blockIdx.x, tid = threadIdx.x;
  if (tid <= bounds.G) sb[tid] = bounds.b[tid];
  __syncthreads();
  for (int c = tid; c < R; c += RF_THREADS) {
    const int lab = labels_in[(size_t)q * R + c];
    const int owner = refine_owner(sb, bounds.G, lab);
    const bool valid = owner >= 0;
    const float res = valid ? planes[(size_t)owner * plane_stride + (size_t)q * R + c] : 0.0f;
    rf_fill_slot<EXACT>(sd, si, c, valid, res, lab);
  }
  rf_select<EXACT>(sd, si, hv, hi, &s_kept, R, k, tid, labels, dist, (size_t)q * k);
}

size_t refine_rows_max_dim() { return (size_t)(64 * 1024 - 4 * RF_CAP * sizeof(float) - 64) / sizeof(float); }

template <typename T>
static void rf_launch_rows(const float *Q, int nq, int D, const T *rows, int64_t N, int64_t id_base, const int32_t *labels_in,
                           int R, int k, int exact, int32_t *labels, float *dist, hipStream_t st) {
  const size_t lds = (size_t)D * sizeof(float);
  if (exact)
    hipLaunchKernelGGL((refine_rows_kernel<true, T>), dim3(nq), dim3(RF_THREADS), lds, st, Q, D, rows, N, id_base,
                       labels_in, R, k, labels, dist);
  else
    hipLaunchKernelGGL((refine_rows_kernel<false, T>), dim3(nq), dim3(RF_THREADS), lds, st, Q, D, rows, N, id_base,
                       labels_in, R, k, labels, dist);
}

hipError_t launch_refine_rows(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base,
                              const int32_t *labels_in, int R, int k, int exact, int32_t *labels, float *dist,
                              hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (R > RF_CAP || R < 1 || k < 1 || k > R || D < 1 || (size_t)D > refine_rows_max_dim() || N < 0 ||
      (rows.elem != 4 && rows.elem != 1))
    return hipErrorInvalidValue;
  if (rows.elem == 1)
    rf_launch_rows(Q, nq, D, static_cast<const uint8_t *>(rows.p), N, id_base, labels_in, R, k, exact, labels, dist, st);
  else
    rf_launch_rows(Q, nq, D, static_cast<const float *>(rows.p), N, id_base, labels_in, R, k, exact, labels, dist, st);
  return hipGetLastError();
}

hipError_t launch_refine_dist(const float *Q, int nq, int D, RowsRef rows, int64_t n, int64_t lo_label,
                              const int32_t *labels_in, int R, float *plane, hipStream_t st) {
  if (nq == 0 || n == 0) return hipSuccess;  // (a shard without rows owns no label)
  if (R > RF_CAP || R < 1 || D < 1 || (size_t)D > refine_rows_max_dim() || n < 0 || lo_label < 0 ||
      (rows.elem != 4 && rows.elem != 1))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)D * sizeof(float);
  if (rows.elem == 1)
    hipLaunchKernelGGL(refine_dist_kernel<uint8_t>, dim3(nq), dim3(RF_THREADS), lds, st, Q, D,
                       static_cast<const uint8_t *>(rows.p), n, lo_label, labels_in, R, plane);
  else
    hipLaunchKernelGGL(refine_dist_kernel<float>, dim3(nq), dim3(RF_THREADS), lds, st, Q, D,
                       static_cast<const float *>(rows.p), n, lo_label, labels_in, R, plane);
  return hipGetLastError();
}

// dst[i] = (float)src[i]: a chunk of byte rows as the encoders read it (vaqhip_multi_encode.cpp)
__global__ __launch_bounds__(RF_THREADS) void widen_rows_u8_kernel(const uint8_t *__restrict__ src, int64_t elems,
                                                                   float *__restrict__ dst) {
  const int64_t stride = (int64_t)gridDim.x * RF_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; i < elems; i += stride) dst[i] = (float)src[i];
}

hipError_t launch_widen_rows_u8(const uint8_t *src, int64_t elems, float *dst, hipStream_t st) {
  if (elems == 0) return hipSuccess;
  if (elems < 0 || !src || !dst) return hipErrorInvalidValue;
  const int64_t blocks = std::min<int64_t>((elems + RF_THREADS - 1) / RF_THREADS, 256 * 16);
  hipLaunchKernelGGL(widen_rows_u8_kernel, dim3((unsigned)blocks), dim3(RF_THREADS), 0, st, src, elems, dst);
  return hipGetLastError();
}

hipError_t launch_refine_select(const int32_t *labels_in, int nq, const float *planes, size_t plane_stride,
                                const RefineBounds &bounds, int R, int k, int exact, int32_t *labels, float *dist,
                                hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (R > RF_CAP || R < 1 || k < 1 || k > R || bounds.G < 1 || bounds.G > RF_MAX_SHARDS || plane_stride < (size_t)nq * R)
    return hipErrorInvalidValue;
  if (exact)
    hipLaunchKernelGGL(refine_select_kernel<true>, dim3(nq), dim3(RF_THREADS), 0, st, labels_in, planes, plane_stride,
                       bounds, R, k, labels, dist);
  else
    hipLaunchKernelGGL(refine_select_kernel<false>, dim3(nq), dim3(RF_THREADS), 0, st, labels_in, planes, plane_stride,
                       bounds, R, k, labels, dist);
  return hipGetLastError();
}

}  // namespace vaq
