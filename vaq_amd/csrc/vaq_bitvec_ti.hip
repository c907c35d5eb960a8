// vaq_bitvec_ti.hip -- the gfx950 kernels of the triangle-inequality form (vaq_bitvec_ti.h, DESIGN.md section 4h,
// "Triangle-inequality form").
//
// Group.  The cluster index kernel has given every row its centre and squared distance.  A key per row,
// (cluster << 32) | ~bits(sqrtf(dist)), a stable rocPRIM radix sort of (key, row), and one pass over the sorted keys
// for start[] and xcc[]: the rows cluster after cluster, the farthest from its centre first.
//
// Plan.  One workgroup per query, lane = centre over the dimension-major centres; the keys (bits(qcc) << 32) | c are
// sorted in LDS (bitonic), so a query's centres come out in ascending distance with the distance beside them.
//
// Scan.  One workgroup of 256 threads per query, one lane per candidate row (the sum over D is a serial chain).  A tile
// is 256 consecutive positions of the walk and goes through LDS as in the exact cluster form (vaq_bitvec_tile.h).  The
// walk is what is new: the clusters are taken in plan order; the 64 lanes of a wave look at 64 clusters at once and
// drop those that are empty or whose whole xcc range lies outside the annulus of the present threshold; inside a
// cluster that stays, xcc descends, so the rows inside the annulus are one range [lo, hi), found by two 64-ary
// searches of the wave over xcc[] before any row is loaded.  Only positions inside the ranges are dealt to lanes, across
// cluster boundaries.  Every wave runs the same searches over the same values, so the walk's state is the same in all
// four waves with no exchange through LDS.
//
// Selection.  Keys are (bits(sqrtf(sum)) << 32) | row: unique, and ordered as unsigned integers by (distance, row).
// Until min(k, n) candidates exist every one is kept; then the pool is sorted (bitonic), the key of slot kk - 1 is the
// threshold, and later candidates below it are appended (a ballot and a prefix per wave, one LDS counter).  The pool
// is compacted again before a tile that might not fit, after `refresh` admissions, and at the end.  A stale threshold
// is only looser.
#include "vaq_bitvec_ti.h"

#include <float.h>

#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "vaq_bitvec_tile.h"

namespace vaq {

namespace {

constexpr int TI_POOL = BITVEC_TI_POOL;
constexpr int TI_PER_THREAD = BITVEC_CLUSTERS_MAX / EX_THREADS;  // centres a thread of the plan keeps
static_assert(TI_POOL >= BITVEC_RERANK_MAX + EX_THREADS && (TI_POOL & (TI_POOL - 1)) == 0, "k keys and a tile must fit");
static_assert((size_t)BITVEC_CLUSTERS_MAX_DIM * sizeof(float) <= (size_t)BITVEC_CLUSTERS_MAX * sizeof(uint64_t),
              "the plan stages the query row where its keys go");

__global__ void __launch_bounds__(EX_THREADS)
ti_keys_kernel(const int32_t *__restrict__ assign, const float *__restrict__ dist2, int64_t n, uint64_t *__restrict__ keys,
               uint32_t *__restrict__ vals, int32_t *__restrict__ first_bad) {
  const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (i >= n) return;
  if (assign[i] < 0) atomicMin(first_bad, (int32_t)i);  // (the host refuses the build; this key is never used)
  keys[i] = ((uint64_t)(uint32_t)assign[i] << 32) | (uint64_t)(~__float_as_uint(sqrtf(dist2[i])));
  vals[i] = (uint32_t)i;
}

// position i closes the clusters between its predecessor's and its own; the last position (or, with no rows, thread 0)
// closes the rest, start[T] = n among them
__global__ void __launch_bounds__(EX_THREADS)
ti_bounds_kernel(const uint64_t *__restrict__ keys, int64_t n, int T, int32_t *__restrict__ start, float *__restrict__ xcc) {
  const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
  if (n == 0) {
    if (i == 0)
      for (int c = 0; c <= T; c++) start[c] = 0;
    return;
  }
  if (i >= n) return;
  const int c = min((int)(keys[i] >> 32), T - 1);
  const int prev = i == 0 ? -1 : min((int)(keys[i - 1] >> 32), T - 1);
  for (int cc = prev + 1; cc <= c; cc++) start[cc] = (int32_t)i;
  if (i == n - 1)
    for (int cc = c + 1; cc <= T; cc++) start[cc] = (int32_t)n;
  xcc[i] = __uint_as_float(~(uint32_t)keys[i]);
}

// the first n <= P keys ascending, by the whole workgroup; every thread calls it with the same n
template <int THREADS>
__device__ __forceinline__ void ti_sort_keys(uint64_t *keys, int n, int cap) {
  const int tid = threadIdx.x;
  n = min(n, cap);
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += THREADS) keys[i] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const uint64_t a = keys[i], b = keys[o];
          if ((a > b) == ((i & size) == 0)) {
            keys[i] = b;
            keys[o] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(EX_THREADS)
ti_plan_kernel(const float *__restrict__ Q, int D, const float *__restrict__ centres_t, int T, int32_t *__restrict__ order,
               float *__restrict__ qcc) {
  __shared__ uint64_t key[BITVEC_CLUSTERS_MAX];  // the query row first, then a key per centre
  float *qs = reinterpret_cast<float *>(key);
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += EX_THREADS) qs[j] = Q[(size_t)q * D + j];
  __syncthreads();
  // euclideanDistNoSQRT per centre: distance += (a - b) * (a - b) in dimension order from 0.0f
  float acc[TI_PER_THREAD];
#pragma unroll
  for (int j = 0; j < TI_PER_THREAD; j++) acc[j] = 0.0f;
  const int nj = (T + EX_THREADS - 1) / EX_THREADS;
  for (int i = 0; i < D; i++) {
    const float a = qs[i];
    const float *row = centres_t + (size_t)i * T;
#pragma unroll
    for (int j = 0; j < TI_PER_THREAD; j++) {
      const int c = tid + j * EX_THREADS;
      if (j < nj && c < T) {
        const float t = a - row[c];
        acc[j] += t * t;
      }
    }
  }
  __syncthreads();  // (every thread is done with the query row)
#pragma unroll
  for (int j = 0; j < TI_PER_THREAD; j++) {
    const int c = tid + j * EX_THREADS;
    if (c < T) key[c] = ((uint64_t)__float_as_uint(sqrtf(acc[j])) << 32) | (uint32_t)c;
  }
  __syncthreads();
  ti_sort_keys<EX_THREADS>(key, T, BITVEC_CLUSTERS_MAX);
  for (int i = tid; i < T; i += EX_THREADS) {
    order[(size_t)q * T + i] = (int32_t)(uint32_t)key[i];
    qcc[(size_t)q * T + i] = __uint_as_float((uint32_t)(key[i] >> 32));
  }
}

// How many leading elements of x[0, len) satisfy pred, where pred holds for a prefix and for nothing behind it.  The
// 64 lanes of the wave probe 64 places at once; every wave of the workgroup calls it with the same arguments and gets
// the same count.  Where pred is no prefix (a NaN among x) the count is some value in [0, len].
template <class P>
__device__ __forceinline__ int ti_leading(const float *__restrict__ x, int len, P pred) {
  const int lane = threadIdx.x & (EX_WAVE - 1);
  int a = 0, b = len;  // pred holds before a and fails from b on
  while (b - a > EX_WAVE) {
    const int step = (b - a + EX_WAVE - 1) / EX_WAVE;
    const int64_t p = (int64_t)a + (int64_t)(lane + 1) * step - 1;  // the last element of this lane's piece
    const bool t = p < b && pred(x[p]);
    const int cnt = __popcll(__ballot(t));  // whole pieces inside the prefix
    const int64_t na = (int64_t)a + (int64_t)cnt * step;
    b = (int)min(na + step - 1, (int64_t)b);  // (piece cnt's last element failed, or lies behind b)
    a = (int)min(na, (int64_t)b);
  }
  const int p = a + lane;
  const bool t = p < b && pred(x[p]);
  return __builtin_amdgcn_readfirstlane(a + __popcll(__ballot(t)));
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(EX_THREADS)
ti_select_kernel(const float *__restrict__ Q, int D, const T *__restrict__ rows, int n, const int32_t *__restrict__ start,
                 const int32_t *__restrict__ member, const float *__restrict__ xcc, int nT,
                 const int32_t *__restrict__ order, const float *__restrict__ qcc, int k, int refresh, float slack,
                 int64_t id_base, int32_t *__restrict__ labels, float *__restrict__ out_dist, int64_t *__restrict__ evaluated) {
  __shared__ float tile[EX_THREADS * EX_STRIDE];
  __shared__ uint64_t keys[TI_POOL];     // (bits(distance) << 32) | row
  __shared__ int32_t s_row[EX_THREADS];  // the raw rows of the tile
  __shared__ int s_count;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (EX_WAVE - 1);
  const int32_t *ord = order + (size_t)q * nT;
  const float *qc = qcc + (size_t)q * nT;
  const float *qp = Q + (size_t)q * D;
  int32_t *lab = labels + (size_t)q * k;
  float *dis = out_dist + (size_t)q * k;
  const int kk = min(k, n);
  for (int i = max(kk, 0) + tid; i < k; i += EX_THREADS) {
    lab[i] = -1;
    dis[i] = FLT_MAX;
  }
  if (kk <= 0) {  // (the same for every thread)
    if (evaluated && tid == 0) evaluated[q] = 0;
    return;
  }
  if (tid == 0) s_count = 0;
  __syncthreads();
  uint64_t thr = ~0ull;  // no threshold yet: no key is all ones (a row is below 2^31)
  float thr_d = 0.0f;
  bool have = false;
  // the walk: the present place in the plan, the next position and the end of its cluster's range (cut: they are set;
  // cur == 0 with cut unset: no cluster is open)
  int wv = 0, cur = 0, end = 0, total = 0;
  bool cut = false;
  // The pool's fill, in a register and the same for every thread: s_count read behind the barrier that ended the last
  // tile, or kk after a compaction.  s_count itself is never read between thread 0's write after a compaction and the
  // barriers of the next tile, so the walk's end, which may follow a compaction with no tile between, reads the register.
  int fill = 0;

  for (;;) {
    fill = __builtin_amdgcn_readfirstlane(s_count);
    if (fill >= kk && (!have || fill + EX_THREADS > TI_POOL || fill - kk >= refresh)) {  // keep the kk smallest
      ti_sort_keys<EX_THREADS>(keys, fill, TI_POOL);
      thr = keys[kk - 1];
      thr_d = __uint_as_float((uint32_t)(thr >> 32));
      have = true;
      cut = false;  // the open cluster's range is cut again under the tighter threshold
      if (tid == 0) s_count = kk;  // (the appends of the next tile start there, behind its first barrier)
      fill = kk;
    }
    // this lane's position: the tile's 256 places are dealt out range after range
    int g = -1, filled = 0;
    while (filled < EX_THREADS && wv < nT) {
      if (!cut) {
        if (cur == 0) {  // skip the clusters that are empty or wholly outside their annulus, 64 at a time
          while (wv < nT) {
            const int i = wv + lane;
            bool alive = false;
            if (i < nT) {
              const int c = ord[i];
              const int s = start[c], e = start[c + 1];
              alive = e > s;
              if (alive && have) {
                const TiAnnulus an = bitvec_ti_annulus(qc[i], thr_d, slack);
                alive = !(xcc[e - 1] > an.hi) && !(xcc[s] < an.lo);
              }
            }
            const unsigned long long b = __ballot(alive);
            if (b != 0) {
              wv += __ffsll((long long)b) - 1;
              break;
            }
            wv += EX_WAVE;
          }
          wv = __builtin_amdgcn_readfirstlane(wv);
          if (wv >= nT) break;
        }
        const int c = ord[wv];
        const int s = start[c], e = start[c + 1];
        int lo = s, hi = e;
        if (have) {  // xcc descends: [lo, hi) are the positions with an.lo <= xcc <= an.hi
          const TiAnnulus an = bitvec_ti_annulus(qc[wv], thr_d, slack);
          lo = s + ti_leading(xcc + s, e - s, [&](float x) { return x > an.hi; });
          hi = s + ti_leading(xcc + s, e - s, [&](float x) { return !(x < an.lo); });
        }
        cur = max(cur, lo);
        end = hi;
        cut = true;
      }
      const int take = max(min(end - cur, EX_THREADS - filled), 0);
      if (tid >= filled && tid < filled + take) g = cur + (tid - filled);
      filled += take;
      cur += take;
      if (cur >= end) {  // the range is dealt: the next cluster
        wv++;
        cur = 0;
        cut = false;
        if (!have && fill + filled >= kk) break;  // kk candidates: the threshold comes before another cluster is opened
      }
    }
    filled = __builtin_amdgcn_readfirstlane(filled);
    if (filled == 0) break;  // (the same for every thread)
    total += filled;
    const int32_t row = g >= 0 ? member[g] : -1;
    s_row[tid] = row;
    __syncthreads();

    // euclideanDistNoSQRT per candidate, the tile staged DC dimensions at a time
    float distance = 0.0f;
    float v[EX_DC];
    ex_fetch<T, VEC>(rows, D, s_row, 0, v);
    for (int d0 = 0; d0 < D; d0 += EX_DC) {
      ex_stage<VEC>(tile, v);
      __syncthreads();
      if (d0 + EX_DC < D) ex_fetch<T, VEC>(rows, D, s_row, d0 + EX_DC, v);
      const float *mine = tile + tid * EX_STRIDE;
      if (g >= 0) {
        if (d0 + EX_DC <= D) {
#pragma unroll
          for (int j = 0; j < EX_DC; j++) {
            const float t = qp[d0 + j] - mine[j];
            distance += t * t;
          }
        } else {
          for (int j = 0; j < D - d0; j++) {
            const float t = qp[d0 + j] - mine[j];
            distance += t * t;
          }
        }
      }
      __syncthreads();
    }

    const uint64_t key = ((uint64_t)__float_as_uint(sqrtf(distance)) << 32) | (uint32_t)row;
    const bool admit = g >= 0 && key < thr;
    const unsigned long long b = __ballot(admit);
    int base = 0;
    if (lane == 0 && b != 0) base = atomicAdd(&s_count, __popcll(b));
    base = __shfl(base, 0);
    const int slot = base + __popcll(b & ((1ull << lane) - 1ull));
    if (admit && slot < TI_POOL) keys[slot] = key;  // (s_count + 256 <= TI_POOL before every tile)
    __syncthreads();
  }

  // (without a threshold every row was kept, with one kk keys at least stay: the pool holds kk keys)
  ti_sort_keys<EX_THREADS>(keys, fill, TI_POOL);
  for (int i = tid; i < kk; i += EX_THREADS) {
    lab[i] = (int32_t)((int64_t)(uint32_t)keys[i] + id_base);
    dis[i] = __uint_as_float((uint32_t)(keys[i] >> 32));
  }
  if (evaluated && tid == 0) evaluated[q] = total;
}

template <typename T>
hipError_t ti_select_t(bool vec, int nq, hipStream_t st, const float *queries, int D, const void *rows, int n,
                       const int32_t *start, const int32_t *member, const float *xcc, int T_, const int32_t *order,
                       const float *qcc, int k, int refresh, int64_t id_base, int32_t *labels, float *out_dist,
                       int64_t *evaluated) {
  const float slack = bitvec_ti_slack(D);
  if (vec)
    hipLaunchKernelGGL((ti_select_kernel<T, true>), dim3(nq), dim3(EX_THREADS), 0, st, queries, D, static_cast<const T *>(rows),
                       n, start, member, xcc, T_, order, qcc, k, refresh, slack, id_base, labels, out_dist, evaluated);
  else
    hipLaunchKernelGGL((ti_select_kernel<T, false>), dim3(nq), dim3(EX_THREADS), 0, st, queries, D, static_cast<const T *>(rows),
                       n, start, member, xcc, T_, order, qcc, k, refresh, slack, id_base, labels, out_dist, evaluated);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bitvec_ti_keys(const int32_t *assign, const float *dist2, int64_t n, uint64_t *keys, uint32_t *vals,
                                 int32_t *first_bad, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ti_keys_kernel, dim3((unsigned)((n + EX_THREADS - 1) / EX_THREADS)), dim3(EX_THREADS), 0, st, assign, dist2,
                     n, keys, vals, first_bad);
  return hipGetLastError();
}

hipError_t bitvec_ti_sort(void *temp, size_t &temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                          int32_t *member_out, int64_t n, int T, hipStream_t st) {
  unsigned cbits = 1;
  while ((1u << cbits) < (unsigned)T) cbits++;
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, reinterpret_cast<uint32_t *>(member_out),
                                   (size_t)n, 0u, 32u + cbits, st);
}

hipError_t launch_bitvec_ti_bounds(const uint64_t *keys_sorted, int64_t n, int T, int32_t *start, float *xcc, hipStream_t st) {
  if (n < 0 || n > 0x7fffffffLL || T < 1 || T > BITVEC_CLUSTERS_MAX) return hipErrorInvalidValue;
  const int64_t blocks = std::max<int64_t>((n + EX_THREADS - 1) / EX_THREADS, 1);
  hipLaunchKernelGGL(ti_bounds_kernel, dim3((unsigned)blocks), dim3(EX_THREADS), 0, st, keys_sorted, n, T, start, xcc);
  return hipGetLastError();
}

hipError_t launch_bitvec_ti_plan(const float *ori_queries, int nq, int D, const float *centres_t, int T, int32_t *order_out,
                                 float *qcc_out, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ti_plan_kernel, dim3(nq), dim3(EX_THREADS), 0, st, ori_queries, D, centres_t, T, order_out, qcc_out);
  return hipGetLastError();
}

hipError_t launch_bitvec_ti_select(const float *queries, int nq, int D, RowsRef rows, int64_t n, const int32_t *start,
                                   const int32_t *member, const float *xcc, int T, const int32_t *order, const float *qcc,
                                   int k, int refresh, int64_t id_base, int32_t *labels, float *out_dist, int64_t *evaluated,
                                   hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX || k < 1 || k > BITVEC_RERANK_MAX || n < 0 ||
      n > 0x7fffffffLL || refresh < 1 || (rows.elem != 4 && rows.elem != 1) || (n > 0 && !rows.p))
    return hipErrorInvalidValue;
  // whole aligned pieces of four elements: 16 bytes of floats, 4 of bytes
  const bool vec = D % 4 == 0 && reinterpret_cast<uintptr_t>(rows.p) % (size_t)(4 * rows.elem) == 0;
  if (rows.elem == 1)
    return ti_select_t<uint8_t>(vec, nq, st, queries, D, rows.p, (int)n, start, member, xcc, T, order, qcc, k, refresh, id_base,
                                labels, out_dist, evaluated);
  return ti_select_t<float>(vec, nq, st, queries, D, rows.p, (int)n, start, member, xcc, T, order, qcc, k, refresh, id_base,
                            labels, out_dist, evaluated);
}

}  // namespace vaq
