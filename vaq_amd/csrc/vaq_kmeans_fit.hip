// vaq_kmeans_fit.hip -- the gfx950 kernels and the iteration loop of vaq_kmeans_fit.h ("Fitting
// the centres").
//
// An iteration is assign -> group -> update, all on one stream:
//   assign   vaq_cluster_index.hip's kernel with ROOT: lane = row, 64 running sums in registers, the root before the fold.
//   group    rocPRIM's stable radix sort of (belongs[i], i) by the bits of T - 1; kf_bounds_kernel finds every centre's
//            first grouped position by a binary search and the first row that no centre won.
//   update   kf_update_kernel.  A centre's sum over its rows is ONE chain per dimension in ascending row order, so the
//            parallelism is across centres and dimensions: a workgroup is one wave that owns one centre and 64
//            dimensions, lane = dimension.  A member row's 64 values are one coalesced run (256 bytes of floats, 64 of
//            bytes); the rows are read where the refiner has them, through member[].  The member numbers come through
//            LDS 256 at a time (one coalesced load a lane, then wave-uniform reads), the values of 8 rows are loaded
//            before the first is added, and they are added in member order into the lane's single accumulator.  The
//            wave then divides by the count, compares with the old centre and stamps the centre as changed;
//            kf_commit_kernel replaces the stamped centres whole, as the reference's vector `==` does (a per-element
//            replacement would keep a seed's -0.0f beside a new +0.0f that compares equal to it).
// No float atomics, no reassociation: every figure is the reference's sequential one.
#include "vaq_kmeans_fit.h"

#include <limits.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "vaq_cluster_index.h"

namespace vaq {

namespace {

constexpr int KF_DIMS = KMEANS_FIT_DIMS, KF_TILE = KMEANS_FIT_TILE, KF_LOADS = KMEANS_FIT_LOADS;
static_assert(KF_TILE % KF_DIMS == 0 && KF_TILE % KF_LOADS == 0, "a tile is staged by whole waves and walked in whole batches");

#define KF_TRY(expr)                  \
  do {                                \
    if ((e = (expr)) != hipSuccess) return e; \
  } while (0)

// the flags, the centres' stamps and the identity the sort permutes
__global__ void kf_init_kernel(KmeansFitFlags *__restrict__ flags, int32_t *__restrict__ stamp, int T,
                               uint32_t *__restrict__ rows_in, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *flags = KmeansFitFlags{0, INT32_MAX, INT32_MAX};
  if (i < T) stamp[i] = 0;
  if (i < n) rows_in[i] = (uint32_t)i;
}

// means[c] = (float) row seed_rows[c]; a seed outside [0, n) reads nothing, leaves zeros and its c in the flags
template <typename T>
__global__ void kf_seed_kernel(const T *__restrict__ rows, int64_t n, int D, const int32_t *__restrict__ seed_rows,
                               float *__restrict__ means, KmeansFitFlags *__restrict__ flags) {
  const int c = blockIdx.y, d = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t s = seed_rows[c];
  const bool ok = s >= 0 && s < n;
  if (!ok && d == 0) atomicMin(&flags->bad_seed, c);
  if (d < D) means[(size_t)c * D + d] = ok ? (float)rows[(size_t)s * D + d] : 0.0f;
}

// start[c] = the first grouped position whose centre is >= c (start[T] = n behind the last centre's rows; an empty
// centre starts where the next one does), and the first row whose assignment is -1
__global__ void kf_bounds_kernel(const int32_t *__restrict__ belongs, const uint32_t *__restrict__ keys_sorted, int64_t n, int T,
                                 int32_t *__restrict__ start, KmeansFitFlags *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && belongs[i] < 0) atomicMin(&flags->no_centre_row, (int32_t)i);
  if (i <= T) {
    int64_t lo = 0, hi = n;  // (lo, hi stay inside [0, n] whatever the keys are)
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys_sorted[mid] < (uint32_t)i) lo = mid + 1;
      else hi = mid;
    }
    start[i] = (int32_t)lo;
  }
}

// One wave: centre blockIdx.y, dimensions [64 blockIdx.x, +64).  next[c] = sum / count; stamp[c] = iter where an
// element is not == the old centre's.  Nothing happens once a row without a centre is on record.
template <typename T>
__global__ void __launch_bounds__(KF_DIMS)
kf_update_kernel(const T *__restrict__ rows, int D, const int32_t *__restrict__ start, const uint32_t *__restrict__ member,
                 const float *__restrict__ means, float *__restrict__ next, int32_t *__restrict__ stamp, int iter,
                 const KmeansFitFlags *__restrict__ flags) {
  __shared__ uint32_t tile[KF_TILE];
  if (flags->no_centre_row != INT32_MAX) return;
  const int lane = threadIdx.x, c = blockIdx.y, d = blockIdx.x * KF_DIMS + lane;
  const bool live = d < D;
  const T *col = rows + (live ? d : 0);
  const int g0 = start[c], g1 = start[c + 1];
  float acc = 0.0f;
  for (int t0 = g0; t0 < g1; t0 += KF_TILE) {
    const int m = min(KF_TILE, g1 - t0);
    __syncthreads();  // (the tile of the step before has been read)
#pragma unroll
    for (int i = lane; i < KF_TILE; i += KF_DIMS)
      if (i < m) tile[i] = member[t0 + i];
    __syncthreads();
    if (!live) continue;
    int i = 0;
    for (; i + KF_LOADS <= m; i += KF_LOADS) {
      float x[KF_LOADS];
#pragma unroll
      for (int u = 0; u < KF_LOADS; u++) x[u] = (float)col[(size_t)tile[i + u] * D];
#pragma unroll
      for (int u = 0; u < KF_LOADS; u++) acc += x[u];  // in member order
    }
    for (; i < m; i++) acc += (float)col[(size_t)tile[i] * D];
  }
  if (!live) return;
  const float nv = acc / (float)(g1 - g0);  // (no rows: 0 / 0, a NaN that never equals anything)
  next[(size_t)c * D + d] = nv;
  if (!(nv == means[(size_t)c * D + d])) stamp[c] = iter;
}

// means[c] = next[c] for the centres stamped in this iteration, which is then on record as one that changed
__global__ void kf_commit_kernel(float *__restrict__ means, const float *__restrict__ next, const int32_t *__restrict__ stamp,
                                 int T, int D, int iter, KmeansFitFlags *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)T * D) return;
  const int c = (int)(i / D);
  if (stamp[c] != iter) return;
  means[i] = next[i];
  if (i == (int64_t)c * D) flags->changed_iter = iter;
}

template <typename T>
hipError_t kf_seed(const void *rows, int64_t n, int D, int T_, const int32_t *d_seed_rows, KmeansFitWork &w, hipStream_t st) {
  hipLaunchKernelGGL(kf_seed_kernel<T>, dim3((unsigned)((D + 255) / 256), (unsigned)T_), dim3(256), 0, st,
                     static_cast<const T *>(rows), n, D, d_seed_rows, w.means.as<float>(), w.flags.as<KmeansFitFlags>());
  return hipGetLastError();
}

template <typename T>
hipError_t kf_update(const void *rows, int D, int T_, int iter, KmeansFitWork &w, hipStream_t st) {
  hipLaunchKernelGGL(kf_update_kernel<T>, dim3((unsigned)((D + KF_DIMS - 1) / KF_DIMS), (unsigned)T_), dim3(KF_DIMS), 0, st,
                     static_cast<const T *>(rows), D, w.start.as<int32_t>(), w.member.as<uint32_t>(), w.means.as<float>(),
                     w.next.as<float>(), w.stamp.as<int32_t>(), iter, w.flags.as<KmeansFitFlags>());
  return hipGetLastError();
}

struct KfEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~KfEvents() { vaqhost::destroy_events(e); }
};

}  // namespace

hipError_t kmeans_fit(RowsRef rows, int64_t n, int D, int T, const int32_t *d_seed_rows, int max_iter, KmeansFitWork &w,
                      KmeansFitResult *res, hipStream_t st) {
  if (n < 1 || n > 0x7fffffffLL || D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX || max_iter < 1 ||
      (rows.elem != 4 && rows.elem != 1) || !rows.p || !d_seed_rows || !res)
    return hipErrorInvalidValue;
  hipError_t e;
  const bool bytes = rows.elem == 1;
  unsigned key_bits = 1;  // the bits of T - 1
  while ((1 << key_bits) < T) key_bits++;
  const size_t cen_bytes = (size_t)T * D * sizeof(float);
  KF_TRY(w.means.ensure(cen_bytes));
  KF_TRY(w.next.ensure(cen_bytes));
  KF_TRY(w.stamp.ensure((size_t)T * sizeof(int32_t)));
  KF_TRY(w.start.ensure((size_t)(T + 1) * sizeof(int32_t)));
  KF_TRY(w.flags.ensure(sizeof(KmeansFitFlags)));
  for (vaqhost::DevBuf *b : {&w.belongs, &w.rows_in, &w.keys_out, &w.member}) KF_TRY(b->ensure((size_t)n * 4));
  uint32_t *keys_in = w.belongs.as<uint32_t>(), *keys_out = w.keys_out.as<uint32_t>();  // (an assignment of -1 ends the fit)
  uint32_t *rows_in = w.rows_in.as<uint32_t>(), *member = w.member.as<uint32_t>();
  KF_TRY(rocprim::radix_sort_pairs(nullptr, w.temp_bytes, keys_in, keys_out, rows_in, member, (size_t)n, 0u, key_bits, st));
  KF_TRY(w.temp.ensure(w.temp_bytes ? w.temp_bytes : 16));
  KfEvents ev;
  KF_TRY(vaqhost::ensure_events(ev.e));

  const unsigned over_n = (unsigned)((std::max<int64_t>(n, T + 1) + 255) / 256);
  hipLaunchKernelGGL(kf_init_kernel, dim3(over_n), dim3(256), 0, st, w.flags.as<KmeansFitFlags>(), w.stamp.as<int32_t>(), T,
                     rows_in, n);
  KF_TRY(hipGetLastError());
  KF_TRY(bytes ? kf_seed<uint8_t>(rows.p, n, D, T, d_seed_rows, w, st) : kf_seed<float>(rows.p, n, D, T, d_seed_rows, w, st));

  *res = KmeansFitResult{};
  for (int iter = 1; iter <= max_iter; iter++) {
    KF_TRY(hipEventRecord(ev.e[0], st));
    KF_TRY(launch_cluster_index_root(rows, n, D, w.means.as<float>(), T, w.belongs.as<int32_t>(), nullptr, st));
    KF_TRY(hipEventRecord(ev.e[1], st));
    KF_TRY(rocprim::radix_sort_pairs(w.temp.p, w.temp_bytes, keys_in, keys_out, rows_in, member, (size_t)n, 0u, key_bits, st));
    hipLaunchKernelGGL(kf_bounds_kernel, dim3(over_n), dim3(256), 0, st, w.belongs.as<int32_t>(), keys_out, n, T,
                       w.start.as<int32_t>(), w.flags.as<KmeansFitFlags>());
    KF_TRY(hipGetLastError());
    KF_TRY(hipEventRecord(ev.e[2], st));
    KF_TRY(bytes ? kf_update<uint8_t>(rows.p, D, T, iter, w, st) : kf_update<float>(rows.p, D, T, iter, w, st));
    hipLaunchKernelGGL(kf_commit_kernel, dim3((unsigned)(((int64_t)T * D + 255) / 256)), dim3(256), 0, st, w.means.as<float>(),
                       w.next.as<float>(), w.stamp.as<int32_t>(), T, D, iter, w.flags.as<KmeansFitFlags>());
    KF_TRY(hipGetLastError());
    KF_TRY(hipEventRecord(ev.e[3], st));
    // the one crossing of an iteration: did a centre change, did a row (or a seed) fail
    KF_TRY(hipMemcpyAsync(&res->flags, w.flags.p, sizeof(KmeansFitFlags), hipMemcpyDeviceToHost, st));
    KF_TRY(hipStreamSynchronize(st));
    float ms[3];
    for (int p = 0; p < 3; p++) KF_TRY(hipEventElapsedTime(&ms[p], ev.e[p], ev.e[p + 1]));
    res->assign_ms += ms[0], res->group_ms += ms[1], res->update_ms += ms[2];
    res->iterations = iter;
    if (res->flags.bad_seed != INT32_MAX || res->flags.no_centre_row != INT32_MAX || res->flags.changed_iter != iter) break;
  }
  return hipSuccess;
}

}  // namespace vaq
