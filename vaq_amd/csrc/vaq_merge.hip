// vaq_merge.hip -- the final k-min over the partial lists of a query: merge_kernel (heap_reorder's sorted output,
// utils/Heap.hpp:322-349), merge_compact_kernel (the first level over many mostly empty lists) and defer_merge_kernel
// (queries the best-first form cut in two).  (Numerics: vaq_common.h.)
// refine_kernel / launch_refine, the first-generation VAQ::refine over candidates the caller gathered, stay here: they
// are merge_kernel's fold with a distance in front -- the same MERGE_CAP slots of LDS, the same MERGE_THREADS, the
// same bitonic sort and the same -1 / FLT_MAX output rule -- and share nothing with vaq_refine.hip, whose kernels
// sum in Eigen's order and select by the reference's heap.
#include "vaq_merge.h"
#include "vaq_scan.h"  // bitonic_sort

#include <float.h>

namespace vaq {
// ---------------------------------------------------------------------------
// Final k-min over the candidate lists of one query, output in the order
// heap_reorder produces (ascending; utils/Heap.hpp:322-349), empty slots
// -1 / FLT_MAX.  One workgroup per query; candidates are folded through a
// 2048-entry LDS buffer: [kept | new chunk] -> bitonic sort -> keep k.
// ---------------------------------------------------------------------------
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_CAP = 2048;
constexpr int MERGE_FANIN = 16;  // lists folded by one workgroup (16 x k <= 2048 for k <= 128: one sort)

// grid = (query, group); group g folds lists [g*lists_per_group, ...).
//  final != 0 : write labels (+id_base) / distances with -1 / FLT_MAX in empty slots
//  final == 0 : write the group's k best as an intermediate list (raw ids, sentinels kept)
//  thr_out    : optional [nq] float bits; receives min(thr_out[q], k-th distance) when k rows exist
__global__ __launch_bounds__(MERGE_THREADS) void merge_kernel(
    const float *__restrict__ part_d, const int *__restrict__ part_id, int n_lists,
    int lists_per_group, int64_t list_stride, int64_t query_stride, int k, int64_t id_base,
    int in_final, int final, int32_t *__restrict__ out_id, float *__restrict__ out_d,
    unsigned *__restrict__ thr_out) {
  __shared__ float sd[MERGE_CAP];
  __shared__ int si[MERGE_CAP];
  const int q = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int l0 = g * lists_per_group;
  int l1 = l0 + lists_per_group;
  if (l1 > n_lists) l1 = n_lists;
  const int64_t total = (int64_t)(l1 > l0 ? l1 - l0 : 0) * k;
  int kept = 0;
  int64_t pos = 0;
  while (pos < total) {
    int take = MERGE_CAP - kept;
    if ((int64_t)take > total - pos) take = (int)(total - pos);
    for (int i = tid; i < take; i += MERGE_THREADS) {
      const int64_t c = pos + i;
      const int64_t l = c / k;
      const int j = (int)(c - l * k);
      const size_t a = (size_t)((l0 + l) * list_stride + (int64_t)q * query_stride + j);
      float d = part_d[a];
      int id = part_id[a];
      if (in_final && id < 0) { d = INFINITY; id = ID_SENTINEL; }
      sd[kept + i] = d;
      si[kept + i] = id;
    }
    const int n = kept + take;
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += MERGE_THREADS) { sd[i] = INFINITY; si[i] = ID_SENTINEL; }
    __syncthreads();
    bitonic_sort<true>(sd, si, P, tid, MERGE_THREADS);
    kept = n < k ? n : k;
    pos += take;
  }
  __syncthreads();
  const size_t o = ((size_t)q * gridDim.y + g) * k;
  for (int i = tid; i < k; i += MERGE_THREADS) {
    const bool ok = i < kept && si[i] != ID_SENTINEL;
    if (final) {
      out_id[o + i] = ok ? (int32_t)(si[i] + id_base) : -1;
      out_d[o + i] = ok ? sd[i] : FLT_MAX;
    } else {
      out_id[o + i] = ok ? si[i] : ID_SENTINEL;
      out_d[o + i] = ok ? sd[i] : INFINITY;
    }
  }
  if (thr_out && tid == 0 && kept >= k && si[k - 1] != ID_SENTINEL)
    atomicMin(&thr_out[q], __builtin_bit_cast(unsigned, sd[k - 1]));
}

// ---------------------------------------------------------------------------
// VAQ::refine, VAQ.cpp:849-876: exact squared L2 between the raw query and the
// raw dataset row of each of R candidates, then the same k-min.  The
// reference's squaredNorm order is Eigen's; here (and in the oracle) it is the
// sequential  dist = 0; dist += t*t.  One workgroup per query: thread t owns
// candidates t, t+256, ...; then a bitonic sort of the R (<= 2048) pairs.
// rows == nullptr: candidate vectors are read from `dataset` by label;
// otherwise `rows` holds them gathered as [nq][R][D].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MERGE_THREADS) void refine_kernel(
    const float *__restrict__ Q, int D, const float *__restrict__ dataset,
    const float *__restrict__ rows, const int32_t *__restrict__ labels_in, int R, int k,
    int32_t *__restrict__ labels, float *__restrict__ dist) {
  __shared__ float sd[MERGE_CAP];
  __shared__ int si[MERGE_CAP];
  extern __shared__ float qs[];
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += MERGE_THREADS) qs[j] = Q[(size_t)q * D + j];
  int P = 2;
  while (P < R) P <<= 1;
  __syncthreads();
  for (int i = tid; i < P; i += MERGE_THREADS) {
    float d = INFINITY;
    int id = ID_SENTINEL;
    if (i < R) {
      const int lab = labels_in[(size_t)q * R + i];
      if (lab >= 0) {
        const float *y = rows ? rows + ((size_t)q * R + i) * D : dataset + (size_t)lab * D;
        float acc = 0.0f;
        for (int j = 0; j < D; j++) {
          const float t = qs[j] - y[j];
          acc += t * t;
        }
        // heap admission rule (VAQ.cpp:867): heap_top > dist with the neutral FLT_MAX
        if (acc < FLT_MAX) { d = acc; id = lab; }
      }
    }
    sd[i] = d;
    si[i] = id;
  }
  __syncthreads();
  bitonic_sort<true>(sd, si, P, tid, MERGE_THREADS);
  for (int i = tid; i < k; i += MERGE_THREADS) {
    const bool ok = i < P && si[i] != ID_SENTINEL;
    labels[(size_t)q * k + i] = ok ? si[i] : -1;
    dist[(size_t)q * k + i] = ok ? sd[i] : FLT_MAX;
  }
}

hipError_t launch_refine(const float *Q, int nq, int D, const float *dataset, const float *rows,
                         const int32_t *labels_in, int R, int k, int32_t *labels, float *dist,
                         hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (R > MERGE_CAP || R < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(refine_kernel, dim3(nq), dim3(MERGE_THREADS), D * sizeof(float), st, Q, D, dataset,
                     rows, labels_in, R, k, labels, dist);
  return hipGetLastError();
}

// First merge level when the scan left MANY lists per query (one per row slice) that are
// mostly empty because the thresholds were tight: grid = (query, group of 256 lists), one
// thread per list; the per-list entry counts written by the scan let the workgroup gather
// only real candidates -- usually a single sort -- instead of reading 256 x k slots.
constexpr int MERGE_LPG = 256;

__global__ __launch_bounds__(MERGE_THREADS) void merge_compact_kernel(
    const float *__restrict__ part_d, const int *__restrict__ part_id,
    const int *__restrict__ part_cnt, int n_lists, int k, int32_t *__restrict__ out_id,
    float *__restrict__ out_d) {
  __shared__ float sd[MERGE_CAP];
  __shared__ int si[MERGE_CAP];
  __shared__ int pre[MERGE_LPG + 1];
  __shared__ int s_end;
  const int q = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int l0 = g * MERGE_LPG;
  const int nl = (n_lists - l0 < MERGE_LPG) ? n_lists - l0 : MERGE_LPG;
  const int my = (tid < nl) ? part_cnt[(size_t)q * n_lists + l0 + tid] : 0;
  // inclusive scan of the counts (Hillis-Steele over 256 entries)
  pre[tid + 1] = my;
  if (tid == 0) pre[0] = 0;
  __syncthreads();
  for (int off = 1; off < MERGE_LPG; off <<= 1) {
    const int v = (tid >= off) ? pre[tid + 1 - off] : 0;
    __syncthreads();
    pre[tid + 1] += v;
    __syncthreads();
  }
  int kept = 0, start = 0;
  while (start < nl) {
    const int room = MERGE_CAP - kept;
    if (tid == 0) s_end = start + 1;  // one list always fits: counts <= k <= 1024 <= room
    __syncthreads();
    if (tid >= start && tid < nl && pre[tid + 1] - pre[start] <= room) atomicMax(&s_end, tid + 1);
    __syncthreads();
    const int end = s_end;
    if (tid >= start && tid < end) {
      const size_t src = ((size_t)q * n_lists + l0 + tid) * k;
      const int dst = kept + pre[tid] - pre[start];
      for (int i = 0; i < my; i++) {
        sd[dst + i] = part_d[src + i];
        si[dst + i] = part_id[src + i];
      }
    }
    const int n = kept + pre[end] - pre[start];
    int P = 2;
    while (P < n) P <<= 1;
    __syncthreads();
    for (int i = n + tid; i < P; i += MERGE_THREADS) { sd[i] = INFINITY; si[i] = ID_SENTINEL; }
    __syncthreads();
    bitonic_sort<true>(sd, si, P, tid, MERGE_THREADS);
    kept = n < k ? n : k;
    start = end;
    __syncthreads();
  }
  const size_t o = ((size_t)q * gridDim.y + g) * k;
  for (int i = tid; i < k; i += MERGE_THREADS) {
    const bool ok = i < kept && si[i] != ID_SENTINEL;
    out_id[o + i] = ok ? si[i] : ID_SENTINEL;
    out_d[o + i] = ok ? sd[i] : INFINITY;
  }
}

size_t merge_scratch_elems(int n_lists, int nq, int k) {
  size_t lists = 1;  // room for one discarded result list (labels == nullptr)
  // worst case of either first level (compacting groups of 256, or plain groups of 16)
  for (size_t n = (size_t)n_lists; n > (size_t)MERGE_FANIN;) {
    n = (n + MERGE_FANIN - 1) / MERGE_FANIN;
    lists += n;
  }
  return lists * (size_t)nq * k;
}

// ---------------------------------------------------------------------------
// Queries the best-first form cut in two (ScanParams::defer_*).  The first launch wrote the k best
// of the buckets it scanned to labels/dist (the API's format: ascending, -1 / FLT_MAX in empty
// slots, labels with id_base added); the second launch's workgroups wrote n_lists partial lists
// (local labels) of the other buckets -- disjoint rows, so every (distance, label) pair is distinct.
// One workgroup per handed-over query: each thread counts the pairs below its own, compared as one
// 64-bit key, and writes its pair at that position if it is among the k best (VAQ::searchHeap's
// result is the k smallest pairs whatever the order they were met in, VAQ.cpp:1729-1758).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void defer_merge_kernel(const unsigned *__restrict__ defer_count, int defer_cap,
                                                          const DeferRec *__restrict__ defer_list, int n_lists, int k,
                                                          const float *__restrict__ part_d,
                                                          const int *__restrict__ part_id,
                                                          const int *__restrict__ part_cnt, int64_t id_base,
                                                          int32_t *labels, float *dist) {
  extern __shared__ unsigned long long dk[];  // [(1 + n_lists) * k] keys, ~0 = empty
  __shared__ unsigned n_valid;
  const unsigned asked = *defer_count;
  const int cnt = asked < (unsigned)defer_cap ? (int)asked : defer_cap;
  const int e = blockIdx.x;
  if (e >= cnt) return;
  const int q = defer_list[e].q;
  const int total = (1 + n_lists) * k;
  if (threadIdx.x == 0) n_valid = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int l = i / k, t = i - l * k;
    unsigned long long key = ~0ull;
    if (l == 0) {
      const int32_t lab = labels[(size_t)q * k + t];
      if (lab >= 0) key = ((unsigned long long)__float_as_uint(dist[(size_t)q * k + t]) << 32) | (unsigned)((int64_t)lab - id_base);
    } else {
      const size_t li = (size_t)e * n_lists + (l - 1);
      if (t < part_cnt[li])
        key = ((unsigned long long)__float_as_uint(part_d[li * k + t]) << 32) | (unsigned)part_id[li * k + t];
    }
    dk[i] = key;
    mine += key != ~0ull ? 1u : 0u;
  }
  if (mine) atomicAdd(&n_valid, mine);
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const unsigned long long ki = dk[i];
    if (ki == ~0ull) continue;
    int rank = 0;
    for (int j = 0; j < total; j++) rank += dk[j] < ki ? 1 : 0;
    if (rank < k) {
      labels[(size_t)q * k + rank] = (int32_t)((int64_t)(int)(unsigned)(ki & 0xffffffffull) + id_base);
      dist[(size_t)q * k + rank] = __uint_as_float((unsigned)(ki >> 32));
    }
  }
  for (int i = (int)n_valid + (int)threadIdx.x; i < k; i += blockDim.x) {
    labels[(size_t)q * k + i] = -1;
    dist[(size_t)q * k + i] = FLT_MAX;
  }
}

hipError_t launch_defer_merge(const unsigned *defer_count, int defer_cap, const DeferRec *defer_list, int n_lists, int k,
                              const float *part_d, const int *part_id, const int *part_cnt, int64_t id_base,
                              int32_t *labels, float *dist, hipStream_t st) {
  const size_t lds = (size_t)(1 + n_lists) * k * sizeof(unsigned long long);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(defer_merge_kernel, dim3(defer_cap), dim3(256), lds, st, defer_count, defer_cap, defer_list, n_lists,
                     k, part_d, part_id, part_cnt, id_base, labels, dist);
  return hipGetLastError();
}

hipError_t launch_merge(const float *part_d, const int *part_id, const int *part_cnt, int n_lists,
                        int64_t list_stride, int64_t query_stride, int nq, int k, int64_t id_base,
                        int in_final, int32_t *labels, float *dist, unsigned *thr_out,
                        float *scratch_d, int *scratch_id, hipStream_t st) {
  if (nq == 0 || k == 0) return hipSuccess;
  const float *cur_d = part_d;
  const int *cur_id = part_id;
  float *sd = scratch_d;
  int *si = scratch_id;
  if (!labels && (!sd || !si)) return hipErrorInvalidValue;
  if (part_cnt && n_lists > MERGE_FANIN && list_stride == k && query_stride == (int64_t)n_lists * k) {
    // scan partials with per-list counts: compact 256 lists per workgroup first
    const int groups = (n_lists + MERGE_LPG - 1) / MERGE_LPG;
    if (!sd || !si) return hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_compact_kernel, dim3(nq, groups), dim3(MERGE_THREADS), 0, st, cur_d, cur_id,
                       part_cnt, n_lists, k, si, sd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cur_d = sd;
    cur_id = si;
    sd += (size_t)nq * groups * k;
    si += (size_t)nq * groups * k;
    n_lists = groups;
    list_stride = k;
    query_stride = (int64_t)groups * k;
    in_final = 0;
  }
  // fold 64 lists at a time into intermediate lists until one workgroup can finish
  while (n_lists > MERGE_FANIN) {
    const int groups = (n_lists + MERGE_FANIN - 1) / MERGE_FANIN;
    if (!sd || !si) return hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_kernel, dim3(nq, groups), dim3(MERGE_THREADS), 0, st, cur_d, cur_id,
                       n_lists, MERGE_FANIN, list_stride, query_stride, k, (int64_t)0, in_final, 0, si,
                       sd, (unsigned *)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cur_d = sd;
    cur_id = si;
    sd += (size_t)nq * groups * k;
    si += (size_t)nq * groups * k;
    n_lists = groups;
    list_stride = k;
    query_stride = (int64_t)groups * k;
    in_final = 0;
  }
  hipLaunchKernelGGL(merge_kernel, dim3(nq, 1), dim3(MERGE_THREADS), 0, st, cur_d, cur_id, n_lists,
                     n_lists > 0 ? n_lists : 1, list_stride, query_stride, k, id_base, in_final,
                     labels ? 1 : 0, labels ? labels : si, labels ? dist : sd, thr_out);
  return hipGetLastError();
}

} // namespace vaq
