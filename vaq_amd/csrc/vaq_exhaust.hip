// vaq_exhaust.hip -- the exhaustive form of VAQ::refine (VAQ.cpp:849-876): every resident row is a candidate, in row
// order.  Distances are Eigen's (q - y).squaredNorm() bit for bit (vaq_exhaust.h, vaq_refine_group.h), the k best are
// the k smallest by (distance, label) or, with "exact_ties", what the reference's heap leaves (vaq::refheap).
//
// xs_tile_kernel<NP>   rows of up to XS_MAX_DIM columns.  ONE THREAD OWNS ONE ROW and keeps it in registers; the
//                      workgroup's 256 rows then meet every query the workgroup owns, the query's elements being
//                      wave-uniform (read through the scalar cache).  Per pair: sub, mul, add per element, unfused, in
//                      the sixteen accumulators of xs_pair_sq_norm -- no cross-lane traffic, no LDS in the inner loop.
// xs_wide_kernel       any width the refiner accepts: the same workgroup geometry and selection, the distance by
//                      sixteen lanes per row (rf_group_sq_norm), the query staged in LDS.
// Selection is streaming: workgroup (split s, query group g) owns the (query, split) lists of its queries.  A list is
// `cap` slots in global memory (its first entries the sorted best so far), its count and its threshold -- the k-th
// best (distance, label) as one 64-bit key, FLT_MAX / 0 before k rows were seen -- live in LDS.  A row enters when its
// key is below the threshold; a list that could overflow on the next tile is folded: sorted in LDS (bitonic_sort),
// its k best kept.  Which rows were ever appended depends on the geometry, the k smallest keys do not.  At the end
// every list is folded once more and written as [split][query][k] in the API's format (-1 / FLT_MAX in empty slots);
// launch_merge folds the splits.
// xs_replay_kernel     "exact_ties": one workgroup per LISTED query (launch_exact_flag lists the queries whose merged
//                      k + 1 list holds two equal distances) walks rows 0..N-1 in order: 1024 distances into LDS, then
//                      wave 0 tests 64 rows at a time against the heap top by ballot and lane 0 applies the
//                      reference's statements to the admitted rows in row order; heap_reorder at the end.  It is one
//                      link of a chain: across the shards of a multi-device refiner the raw heap arrays go from
//                      shard to shard and only the last link reorders (xs_scatter_kernel places its slots).
// Rows are float or uint8 (RowsRef): the row type is a template argument of the three kernels that read rows.  A byte
// is widened to the float it stands for where it is loaded -- in the register form once per tile, outside the query
// loop -- and nothing after the load differs.
// Compiled with -ffp-contract=off like the rest: no FMA, no MFMA, no float atomics; plain vector stores.
#include "vaq_exhaust.h"
#include "vaq_exhaust_launch.h"
#include "vaq_refine.h"
#include "vaq_refine_group.h"
#include "vaq_scan.h"

namespace vaq {

constexpr int XS_THREADS = 256;
constexpr int XS_QB = 8;           // queries between two barriers of the register form
constexpr int XS_SORT_CAP = 2048;  // slots of the fold's sort: cap <= this
constexpr int XR_CHUNK = 1024;     // rows per chunk of the replay (a multiple of 64)
static_assert(XS_TILE == XS_THREADS, "one row per thread");
static_assert(XS_MAX_K1 + XS_TILE <= XS_SORT_CAP, "a list of k + 1 and one tile of appends fit the sort");

struct XsShared {
  unsigned long long thr[XS_MAX_QG];
  int cnt[XS_MAX_QG];
  float sd[XS_SORT_CAP];
  int si[XS_SORT_CAP];
};

__device__ __forceinline__ unsigned long long xs_key(float d, int label) {
  return ((unsigned long long)float_to_bits(d) << 32) | (unsigned)label;
}

// the workgroup's part of the plan: its queries [q0, q0 + nqg), its rows [r0, r1)
struct XsPart {
  int s, q0, nqg;
  int64_t r0, r1;
};
__device__ __forceinline__ XsPart xs_part(const XsParams &p) {
  XsPart w;
  w.s = blockIdx.x % p.S;
  const int g = blockIdx.x / p.S;
  w.q0 = g * p.qg;
  w.nqg = min(p.qg, p.nq - w.q0);
  w.r0 = min(p.N, (int64_t)w.s * p.split_rows);
  w.r1 = min(p.N, w.r0 + p.split_rows);
  return w;
}

__device__ __forceinline__ void xs_init(XsShared &sh, int nqg, int tid) {
  for (int i = tid; i < nqg; i += XS_THREADS) {
    sh.thr[i] = xs_key(FLT_MAX, 0);  // heap_heapify's neutral element: a distance >= FLT_MAX never enters
    sh.cnt[i] = 0;
  }
  __syncthreads();
}

// one row against query ql of the workgroup (any thread, any time between two barriers)
__device__ __forceinline__ void xs_offer(const XsParams &p, XsShared &sh, const XsPart &w, int ql, float d, int label) {
  if (!(d < FLT_MAX)) return;
  const unsigned long long key = xs_key(d, label);
  if (key < sh.thr[ql]) {
    const int pos = atomicAdd(&sh.cnt[ql], 1);  // (below cap: the list had room for a whole tile)
    const size_t o = ((size_t)(w.q0 + ql) * p.S + w.s) * p.cap + pos;
    p.buf_d[o] = d;
    p.buf_id[o] = label;
  }
}

// Fold list ql: sort its entries, keep the k best, tighten the threshold.  All threads, between barriers; ends
// past a barrier.  Afterwards sd / si [0, returned count) hold the kept entries.
__device__ __forceinline__ int xs_fold(const XsParams &p, XsShared &sh, const XsPart &w, int ql, int tid) {
  const int n = sh.cnt[ql];
  const size_t o = ((size_t)(w.q0 + ql) * p.S + w.s) * p.cap;
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += XS_THREADS) {
    sh.sd[i] = i < n ? p.buf_d[o + i] : INFINITY;
    sh.si[i] = i < n ? p.buf_id[o + i] : ID_SENTINEL;
  }
  __syncthreads();
  bitonic_sort<true>(sh.sd, sh.si, P, tid, XS_THREADS);
  const int keep = n < p.k ? n : p.k;
  for (int i = tid; i < keep; i += XS_THREADS) {
    p.buf_d[o + i] = sh.sd[i];
    p.buf_id[o + i] = sh.si[i];
  }
  if (tid == 0) {
    sh.cnt[ql] = keep;
    if (n >= p.k) sh.thr[ql] = xs_key(sh.sd[p.k - 1], sh.si[p.k - 1]);
  }
  __syncthreads();
  return keep;
}

// every list folded and written out as the split's k best, in the API's format
__device__ __forceinline__ void xs_emit(const XsParams &p, XsShared &sh, const XsPart &w, int tid) {
  for (int ql = 0; ql < w.nqg; ql++) {
    const int keep = xs_fold(p, sh, w, ql, tid);
    const size_t o = ((size_t)w.s * p.nq + w.q0 + ql) * p.k;
    for (int i = tid; i < p.k; i += XS_THREADS) {
      p.part_id[o + i] = i < keep ? sh.si[i] : -1;
      p.part_d[o + i] = i < keep ? sh.sd[i] : FLT_MAX;
    }
    __syncthreads();
  }
}

template <int NP, typename T>
__global__ __launch_bounds__(XS_THREADS) void xs_tile_kernel(const XsParams p, const float *__restrict__ Q,
                                                             const T *__restrict__ rows) {
  __shared__ XsShared sh;
  const int tid = threadIdx.x;
  const XsPart w = xs_part(p);
  const int D = p.D;
  xs_init(sh, w.nqg, tid);
  for (int64_t t0 = w.r0; t0 < w.r1; t0 += XS_TILE) {
    const int64_t row = t0 + tid;
    const bool valid = row < w.r1;
    const T *yp = rows + (size_t)(valid ? row : w.r0) * D;
    constexpr bool REST = NP < XS_MAX_NP;  // (the widest form has no columns past its packets)
    float y[XsRow<NP, REST>::SLOTS];
    if constexpr (sizeof(T) == 1) {
      xs_widen_row<NP, REST>(y, yp, D);
    } else {
#pragma unroll
      for (int e = 0; e < XsRow<NP, REST>::SLOTS; e++) y[e] = (e < NP * 16 || e < D) ? yp[e] : 0.0f;
    }
    const int label = (int)(p.id_base + row);
    for (int qb = 0; qb < w.nqg; qb += XS_QB) {
      const int nb = min(XS_QB, w.nqg - qb);
      for (int qi = 0; qi < nb; qi++) {
        const float d = xs_pair_sq_norm<NP, REST>(Q + (size_t)(w.q0 + qb + qi) * D, y, D);
        if (valid) xs_offer(p, sh, w, qb + qi, d, label);
      }
      __syncthreads();
      for (int qi = 0; qi < nb; qi++)
        if (sh.cnt[qb + qi] + XS_TILE > p.cap) xs_fold(p, sh, w, qb + qi, tid);
      __syncthreads();  // (nobody appends to a list while another thread still reads its count)
    }
  }
  xs_emit(p, sh, w, tid);
}

template <typename T>
__global__ __launch_bounds__(XS_THREADS) void xs_wide_kernel(const XsParams p, const float *__restrict__ Q,
                                                             const T *__restrict__ rows) {
  __shared__ XsShared sh;
  extern __shared__ float qs[];
  const int tid = threadIdx.x;
  const XsPart w = xs_part(p);
  const int D = p.D;
  const int g = tid / RF_GROUP, j = tid % RF_GROUP, gbase = (tid & 63) & ~(RF_GROUP - 1);
  xs_init(sh, w.nqg, tid);
  for (int64_t t0 = w.r0; t0 < w.r1; t0 += XS_TILE) {
    for (int ql = 0; ql < w.nqg; ql++) {
      for (int e = tid; e < D; e += XS_THREADS) qs[e] = Q[(size_t)(w.q0 + ql) * D + e];
      __syncthreads();
      for (int c0 = 0; c0 < XS_TILE; c0 += XS_THREADS / RF_GROUP) {  // (uniform trip count: the shuffles run in whole waves)
        const int64_t row = t0 + c0 + g;
        const bool valid = row < w.r1;
        const T *y = rows + (size_t)(valid ? row : w.r0) * D;
        const float res = rf_group_sq_norm(qs, y, D, valid, j, gbase);
        if (j == 0 && valid) xs_offer(p, sh, w, ql, res, (int)(p.id_base + row));
      }
      __syncthreads();
      if (sh.cnt[ql] + XS_TILE > p.cap) xs_fold(p, sh, w, ql, tid);
      __syncthreads();
    }
  }
  xs_emit(p, sh, w, tid);
}

// VAQ.cpp:863-872 over rows [0, N) of `rows` in row order, for the listed queries.  A block beyond the device-side
// count exits at once: no host round trip decides anything.  One LINK of a chain over shards (the single refiner's
// call is the chain of one link): entry e starts from the raw heap arrays hin_v / hin_i [e][k] as the link before
// left them (nullptr: heap_heapify of nothing), and
//   finish == 0   leaves its raw arrays in hout_v / hout_i [e][k] for the next link;
//   finish != 0   applies heap_reorder and writes the k slots: to labels / dist [query][k], or, when labels is
//                 nullptr, to hout_v / hout_i [e][k] (xs_scatter_kernel places them on the first device).
// The heap's statements see the rows of all links in order with nothing in between.
template <typename T>
__global__ __launch_bounds__(XS_THREADS) void xs_replay_kernel(const float *__restrict__ Q, int D,
                                                               const T *__restrict__ rows, int64_t N, int64_t id_base,
                                                               int k, const int *__restrict__ list,
                                                               const unsigned *__restrict__ count,
                                                               const float *__restrict__ hin_v,
                                                               const int *__restrict__ hin_i, float *__restrict__ hout_v,
                                                               int *__restrict__ hout_i, int finish,
                                                               int32_t *__restrict__ labels, float *__restrict__ dist) {
  __shared__ float hv[XS_MAX_K1];
  __shared__ int hi[XS_MAX_K1];
  __shared__ float cd[XR_CHUNK];
  __shared__ int s_kept;
  extern __shared__ float qs[];
  if (blockIdx.x >= *count) return;
  const int q = list[blockIdx.x], tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < D; e += XS_THREADS) qs[e] = Q[(size_t)q * D + e];
  const size_t eo = (size_t)blockIdx.x * k;  // this entry's slots of the chain's state
  for (int i = tid; i < k; i += XS_THREADS) {  // heap_heapify of nothing, or the heap as the link before left it
    hv[i] = hin_v ? hin_v[eo + i] : FLT_MAX;
    hi[i] = hin_i ? hin_i[eo + i] : -1;
  }
  __syncthreads();
  const int g = tid / RF_GROUP, j = tid % RF_GROUP, gbase = lane & ~(RF_GROUP - 1);
  for (int64_t c0 = 0; c0 < N; c0 += XR_CHUNK) {
    for (int i0 = 0; i0 < XR_CHUNK; i0 += XS_THREADS / RF_GROUP) {  // (uniform trip count)
      const int64_t row = c0 + i0 + g;
      const bool valid = row < N;
      const T *y = rows + (size_t)(valid ? row : 0) * D;
      const float res = rf_group_sq_norm(qs, y, D, valid, j, gbase);
      if (j == 0) cd[i0 + g] = valid ? res : INFINITY;
    }
    __syncthreads();
    if (tid < 64) {
      const int n = (int)min((int64_t)XR_CHUNK, N - c0);
      for (int b = 0; b < n; b += 64) {
        const float d = cd[b + lane];
        // the top only falls: a row the reference admits is below the top read here
        unsigned long long m = __ballot(hv[0] > d);
        if (lane == 0) {
          while (m) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            const float di = cd[b + i];
            if (hv[0] > di) {
              refheap::pop(k, hv, hi);
              refheap::push(k, hv, hi, di, (int)(id_base + c0 + b + i));
            }
          }
        }
        wave_lds_sync();
      }
    }
    __syncthreads();
  }
  if (!finish) {  // (the chunk loop ended past a barrier: hv / hi are lane 0's last)
    for (int i = tid; i < k; i += XS_THREADS) {
      hout_v[eo + i] = hv[i];
      hout_i[eo + i] = hi[i];
    }
    return;
  }
  if (tid == 0) s_kept = refheap::reorder(k, hv, hi);
  __syncthreads();
  const int kept = s_kept;
  int32_t *ol = labels ? labels + (size_t)q * k : hout_i + eo;
  float *od = labels ? dist + (size_t)q * k : hout_v + eo;
  for (int i = tid; i < k; i += XS_THREADS) {
    ol[i] = i < kept ? hi[k - kept + i] : -1;
    od[i] = i < kept ? hv[k - kept + i] : FLT_MAX;
  }
}

// the k slots the chain's last link wrote per ENTRY, brought to the first device: entry e is query list[e]
__global__ __launch_bounds__(XS_THREADS) void xs_scatter_kernel(int k, const int *__restrict__ list,
                                                                const unsigned *__restrict__ count,
                                                                const float *__restrict__ src_v,
                                                                const int *__restrict__ src_i,
                                                                int32_t *__restrict__ labels, float *__restrict__ dist) {
  if (blockIdx.x >= *count) return;
  const size_t eo = (size_t)blockIdx.x * k, qo = (size_t)list[blockIdx.x] * k;
  for (int i = threadIdx.x; i < k; i += XS_THREADS) {
    labels[qo + i] = src_i[eo + i];
    dist[qo + i] = src_v[eo + i];
  }
}

int exhaust_list_cap(int k) {
  int cap = 512;
  while (cap < k + XS_TILE) cap <<= 1;
  return cap;
}

size_t exhaust_register_max_dim() { return XS_MAX_DIM; }

template <int NP, typename T>
static int xs_tile_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, xs_tile_kernel<NP, T>, XS_THREADS, 0) != hipSuccess) n = 0;
  return n;
}

template <typename T>
static int xs_blocks_per_cu(int D) {
  int n = 0;
  if (D > XS_MAX_DIM) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, xs_wide_kernel<T>, XS_THREADS, (size_t)D * sizeof(float)) != hipSuccess) n = 0;
    return n;
  }
  switch (D / 16) {
    case 0: return xs_tile_blocks_per_cu<0, T>();
    case 1: return xs_tile_blocks_per_cu<1, T>();
    case 2: return xs_tile_blocks_per_cu<2, T>();
    case 3: return xs_tile_blocks_per_cu<3, T>();
    case 4: return xs_tile_blocks_per_cu<4, T>();
    case 5: return xs_tile_blocks_per_cu<5, T>();
    case 6: return xs_tile_blocks_per_cu<6, T>();
    case 7: return xs_tile_blocks_per_cu<7, T>();
    default: return xs_tile_blocks_per_cu<8, T>();
  }
}

// workgroups of launch_exhaust_select's kernel for rows of D columns that one CU holds at a time (>= 1): the plan
// sizes its grid to ONE round of them -- a second, partly filled round runs at a fraction of the issue rate
int exhaust_blocks_per_cu(int D, int elem) {
  const int n = elem == 1 ? xs_blocks_per_cu<uint8_t>(D) : xs_blocks_per_cu<float>(D);
  return n < 1 ? 1 : (n > 8 ? 8 : n);
}

template <int NP, typename T>
static void xs_launch_tile(const XsParams &p, const float *Q, const T *rows, hipStream_t st) {
  hipLaunchKernelGGL((xs_tile_kernel<NP, T>), dim3(p.S * p.G), dim3(XS_THREADS), 0, st, p, Q, rows);
}

template <typename T>
static void xs_launch_select(const XsParams &p, const float *Q, const T *rows, hipStream_t st) {
  if (p.D > XS_MAX_DIM) {
    hipLaunchKernelGGL(xs_wide_kernel<T>, dim3(p.S * p.G), dim3(XS_THREADS), (size_t)p.D * sizeof(float), st, p, Q, rows);
    return;
  }
  switch (p.D / 16) {
    case 0: xs_launch_tile<0>(p, Q, rows, st); break;
    case 1: xs_launch_tile<1>(p, Q, rows, st); break;
    case 2: xs_launch_tile<2>(p, Q, rows, st); break;
    case 3: xs_launch_tile<3>(p, Q, rows, st); break;
    case 4: xs_launch_tile<4>(p, Q, rows, st); break;
    case 5: xs_launch_tile<5>(p, Q, rows, st); break;
    case 6: xs_launch_tile<6>(p, Q, rows, st); break;
    case 7: xs_launch_tile<7>(p, Q, rows, st); break;
    default: xs_launch_tile<8>(p, Q, rows, st); break;
  }
}

hipError_t launch_exhaust_select(const XsParams &p, const float *Q, RowsRef rows, hipStream_t st) {
  if (p.nq == 0) return hipSuccess;
  if (p.nq < 0 || p.D < 1 || (size_t)p.D > refine_rows_max_dim() || p.N < 0 || p.k < 1 || p.k > XS_MAX_K1 ||
      p.cap != exhaust_list_cap(p.k) || p.cap > XS_SORT_CAP || p.S < 1 || p.qg < 1 || p.qg > XS_MAX_QG ||
      p.G != (p.nq + p.qg - 1) / p.qg || p.split_rows < 0 || (p.N > 0 && (p.N + p.S - 1) / p.S > p.split_rows) ||
      p.id_base < 0 || p.id_base + p.N > 0x7fffffffLL || (rows.elem != 4 && rows.elem != 1))
    return hipErrorInvalidValue;
  if (rows.elem == 1) {
    // (xs_widen_row's wide loads need the allocation's own alignment)
    if (reinterpret_cast<uintptr_t>(rows.p) % 16 != 0) return hipErrorInvalidValue;
    xs_launch_select(p, Q, static_cast<const uint8_t *>(rows.p), st);
  } else {
    xs_launch_select(p, Q, static_cast<const float *>(rows.p), st);
  }
  return hipGetLastError();
}

hipError_t launch_exhaust_replay_link(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base, int k,
                                      const int *list, const unsigned *count, const float *hin_v, const int *hin_i,
                                      float *hout_v, int *hout_i, int finish, int32_t *labels, float *dist,
                                      hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (nq < 0 || D < 1 || (size_t)D > refine_rows_max_dim() || N < 0 || k < 1 || k > XS_MAX_K1 || id_base < 0 ||
      id_base + N > 0x7fffffffLL || !list || !count || (hin_v == nullptr) != (hin_i == nullptr) ||
      (hout_v == nullptr) != (hout_i == nullptr) || (labels == nullptr) != (dist == nullptr) ||
      (finish ? !labels && !hout_v : !hout_v) || (rows.elem != 4 && rows.elem != 1))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)D * sizeof(float);
  if (rows.elem == 1)
    hipLaunchKernelGGL(xs_replay_kernel<uint8_t>, dim3(nq), dim3(XS_THREADS), lds, st, Q, D,
                       static_cast<const uint8_t *>(rows.p), N, id_base, k, list, count, hin_v, hin_i, hout_v, hout_i, finish,
                       labels, dist);
  else
    hipLaunchKernelGGL(xs_replay_kernel<float>, dim3(nq), dim3(XS_THREADS), lds, st, Q, D,
                       static_cast<const float *>(rows.p), N, id_base, k, list, count, hin_v, hin_i, hout_v, hout_i, finish,
                       labels, dist);
  return hipGetLastError();
}

hipError_t launch_exhaust_replay(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base, int k,
                                 const int *list, const unsigned *count, int32_t *labels, float *dist, hipStream_t st) {
  if (!labels || !dist) return nq == 0 ? hipSuccess : hipErrorInvalidValue;
  return launch_exhaust_replay_link(Q, nq, D, rows, N, id_base, k, list, count, nullptr, nullptr, nullptr, nullptr, 1, labels,
                                    dist, st);
}

hipError_t launch_exhaust_scatter(int nq, int k, const int *list, const unsigned *count, const float *src_v,
                                  const int *src_i, int32_t *labels, float *dist, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (nq < 0 || k < 1 || k > XS_MAX_K1 || !list || !count || !src_v || !src_i || !labels || !dist)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(xs_scatter_kernel, dim3(nq), dim3(XS_THREADS), 0, st, k, list, count, src_v, src_i, labels, dist);
  return hipGetLastError();
}

}  // namespace vaq
