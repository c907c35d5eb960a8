// vaq_bitvec_naive.hip -- the gfx950 kernel of the exact cluster form (vaq_bitvec_naive.h, DESIGN.md section 4h,
// "Exact cluster form").
//
// One workgroup of 256 threads per query walks the query's visit list once.  A tile is 256 consecutive positions of
// the walk (it runs across cluster boundaries), lane = position: the sum over D is a serial chain, so a thread owns a
// candidate.  The raw rows stay in the refiner's order and are reached through member[g]; a lane reading its own row
// would touch 64 rows per load, so the tile goes through LDS in chunks of DC = 32 dimensions: eight adjacent lanes
// load the eight 16-byte pieces of a row's chunk (thirty-two adjacent lanes its elements one by one where the row is
// not a whole number of aligned pieces), the chunk lies in LDS with a row stride of 33 dwords, and each lane then
// walks its own row against the query's values, which are the same for every lane and arrive as scalar operands.  The
// next chunk's loads are issued before the sums of the present one, so their latency hides behind the arithmetic.
//
// Selection.  Keys are (dist bits << 32) | seq: a sum of squares from +0.0f is never negative, so the float's bits
// order as an unsigned integer (+inf behind every finite value, NaN behind that).  The first kk candidates are the
// head: thread 0 runs the restated std::sort over their (dist, row) pairs, seq becomes the slot, and the key of slot
// kk - 1 is the threshold.  Every later candidate below the threshold is appended to the pool (a ballot and a prefix
// per wave, one LDS counter).  Before a tile that might not fit, and at the end, the pool is sorted (bitonic), its kk
// smallest stay and the threshold tightens.  Keys are unique, so the sort has no tie rule of its own.
#include "vaq_bitvec_naive.h"

#include <float.h>

#include "vaq_bitvec_tile.h"

namespace vaq {

namespace {

// (the tile's shape and its loaders, ex_fetch and ex_stage: vaq_bitvec_tile.h)
constexpr int EX_POOL = BITVEC_EXACT_POOL;
static_assert(EX_POOL >= BITVEC_RERANK_MAX + EX_THREADS && (EX_POOL & (EX_POOL - 1)) == 0, "the head and a tile must fit");

// the pool's first n slots by key, by the whole workgroup; every thread calls it with the same n <= EX_POOL
__device__ __forceinline__ void ex_sort_pool(uint64_t *keys, int32_t *pool_g, int n) {
  const int tid = threadIdx.x;
  n = min(n, EX_POOL);
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += EX_THREADS) keys[i] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += EX_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const uint64_t a = keys[i], b = keys[o];
          if ((a > b) == ((i & size) == 0)) {
            keys[i] = b;
            keys[o] = a;
            const int32_t r = pool_g[i];
            pool_g[i] = pool_g[o];
            pool_g[o] = r;
          }
        }
      }
      __syncthreads();
    }
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(EX_THREADS)
cluster_exact_select_kernel(const float *__restrict__ Q, int D, const T *__restrict__ rows, const int32_t *__restrict__ start,
                            const int32_t *__restrict__ member, int nT, const int32_t *__restrict__ visit_lists,
                            const BitvecClusterPlan *__restrict__ plans, int k, int64_t id_base, int32_t *__restrict__ labels,
                            float *__restrict__ out_dist) {
  __shared__ float tile[EX_THREADS * EX_STRIDE];
  __shared__ uint64_t keys[EX_POOL];    // the head's (dist, g) pairs while it gathers, then (dist bits << 32) | seq
  __shared__ int32_t pool_g[EX_POOL];   // their image rows
  __shared__ int32_t s_row[EX_THREADS];  // the raw rows of the tile
  __shared__ stdsort::Frame s_stack[stdsort::frames(10)];  // of the head's std::sort: kk <= 1024
  __shared__ int s_count;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (EX_WAVE - 1);
  const int visit = min(plans[q].visit, nT);
  const int32_t *vis = visit_lists + (size_t)q * nT;
  const float *qp = Q + (size_t)q * D;
  int32_t *lab = labels + (size_t)q * k;
  float *dis = out_dist + (size_t)q * k;
  // C_q: the members of the visited clusters (the same scalar walk in every thread)
  int C = 0;
  for (int v = 0; v < visit; v++) {
    const int c = vis[v];
    if ((unsigned)c < (unsigned)nT) C += max(start[c + 1] - start[c], 0);
  }
  const int kk = min(k, C);
  for (int i = max(kk, 0) + tid; i < k; i += EX_THREADS) {
    lab[i] = -1;
    dis[i] = FLT_MAX;
  }
  if (kk <= 0) return;  // (the same for every thread)
  if (tid == 0) s_count = 0;
  uint64_t thr = 0;
  int wv = 0, woff = 0;  // the walk: the next cluster of the list and the members of it already taken

  for (int p0 = 0; p0 < C; p0 += EX_THREADS) {
    // the pool's fill is the same for every thread: the barrier that ended the last tile stands before this read
    const int fill = __builtin_amdgcn_readfirstlane(s_count);
    if (p0 >= kk && fill + EX_THREADS > EX_POOL) {  // the tile might not fit: keep the kk smallest
      ex_sort_pool(keys, pool_g, fill);
      thr = keys[kk - 1];
      if (tid == 0) s_count = kk;  // (read again behind this tile's barriers)
    }
    // this lane's image row: the tile's 256 positions are dealt out cluster after cluster
    int g = -1;
    for (int filled = 0; filled < EX_THREADS && wv < visit;) {
      const int c = vis[wv];
      int s = 0, e = 0;
      if ((unsigned)c < (unsigned)nT) s = start[c] + woff, e = start[c + 1];
      const int take = max(min(e - s, EX_THREADS - filled), 0);
      if (tid >= filled && tid < filled + take) g = s + (tid - filled);
      filled += take;
      if (s + take >= e) wv++, woff = 0;
      else woff += take;
    }
    s_row[tid] = g >= 0 ? member[g] : -1;
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

    const int p = p0 + tid;
    const uint32_t bits = __float_as_uint(distance);
    if (p0 < kk) {  // the head: (dist, g) pairs in candidate order, as RerankPair lays them out
      if (g >= 0 && p < kk) keys[p] = ((uint64_t)(uint32_t)g << 32) | bits;
      if (p0 + EX_THREADS >= kk) {  // complete with this tile: KNNFromDistsIndicesSupplied's std::sort
        __syncthreads();
        if (tid == 0) {  // rerank_sort's walk, its stack in LDS: the one sorting thread is no reason for scratch memory
          stdsort::sort_by_on<true>(reinterpret_cast<RerankPair *>(keys), kk, RerankLt{}, s_stack);
          s_count = kk;
        }
        __syncthreads();
        for (int s = tid; s < kk; s += EX_THREADS) {
          const uint64_t pair = keys[s];
          keys[s] = ((uint64_t)(uint32_t)pair << 32) | (uint32_t)s;
          pool_g[s] = (int32_t)(pair >> 32);
        }
        __syncthreads();
        thr = keys[kk - 1];
      }
    }
    if (p0 + EX_THREADS > kk) {  // positions behind the head: admitted below the threshold
      const uint64_t key = ((uint64_t)bits << 32) | (uint32_t)p;
      const bool admit = g >= 0 && p >= kk && key < thr;
      const unsigned long long b = __ballot(admit);
      int base = 0;
      if (lane == 0 && b != 0) base = atomicAdd(&s_count, __popcll(b));
      base = __shfl(base, 0);
      const int slot = base + __popcll(b & ((1ull << lane) - 1ull));
      if (admit && slot < EX_POOL) {  // (s_count + 256 <= EX_POOL before every tile)
        keys[slot] = key;
        pool_g[slot] = g;
      }
    }
    __syncthreads();
  }

  ex_sort_pool(keys, pool_g, __builtin_amdgcn_readfirstlane(s_count));
  for (int i = tid; i < kk; i += EX_THREADS) {
    lab[i] = (int32_t)(member[pool_g[i]] + id_base);
    dis[i] = __uint_as_float((uint32_t)(keys[i] >> 32));
  }
}

template <typename T>
hipError_t exact_select_t(const float *queries, int nq, int D, const void *rows, bool vec, const int32_t *start,
                          const int32_t *member, int T_, const int32_t *visit, const BitvecClusterPlan *plan, int k,
                          int64_t id_base, int32_t *labels, float *out_dist, hipStream_t st) {
  if (vec)
    hipLaunchKernelGGL((cluster_exact_select_kernel<T, true>), dim3(nq), dim3(EX_THREADS), 0, st, queries, D,
                       static_cast<const T *>(rows), start, member, T_, visit, plan, k, id_base, labels, out_dist);
  else
    hipLaunchKernelGGL((cluster_exact_select_kernel<T, false>), dim3(nq), dim3(EX_THREADS), 0, st, queries, D,
                       static_cast<const T *>(rows), start, member, T_, visit, plan, k, id_base, labels, out_dist);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bitvec_cluster_exact_select(const float *queries, int nq, int D, RowsRef rows, int64_t N,
                                              const int32_t *start, const int32_t *member, int T, const int32_t *visit,
                                              const BitvecClusterPlan *plan, int k, int64_t id_base, int32_t *labels,
                                              float *out_dist, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX || k < 1 || k > BITVEC_RERANK_MAX || N < 0 ||
      N > 0x7fffffffLL || (rows.elem != 4 && rows.elem != 1) || (N > 0 && !rows.p))
    return hipErrorInvalidValue;
  // whole aligned pieces of four elements: 16 bytes of floats, 4 of bytes
  const bool vec = D % 4 == 0 && reinterpret_cast<uintptr_t>(rows.p) % (size_t)(4 * rows.elem) == 0;
  if (rows.elem == 1)
    return exact_select_t<uint8_t>(queries, nq, D, rows.p, vec, start, member, T, visit, plan, k, id_base, labels, out_dist, st);
  return exact_select_t<float>(queries, nq, D, rows.p, vec, start, member, T, visit, plan, k, id_base, labels, out_dist, st);
}

}  // namespace vaq
