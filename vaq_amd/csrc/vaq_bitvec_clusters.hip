// vaq_bitvec_clusters.hip -- gfx950 kernels of the cluster form of the Hamming queries (vaq_bitvec_clusters.h,
// DESIGN.md section 4h, "Cluster form").
//
// Plan.  One workgroup per query, the query row staged in LDS.  Lane = centre: the centres lie dimension-major, so a
// wave reads 64 adjacent floats per dimension, and a thread keeps the running sums of its (at most 16) centres in
// registers.  The (dist, c) pairs then take the query's place in LDS.  Every centre counts the pairs ahead of it by
// (dist, c): with all distances distinct that is std::sort's order.  Where two distances are equal (or one is NaN)
// the order inside the run is std::sort's own business, so thread 0 runs the restated std::sort over the pairs in
// their original order instead.  Thread 0 then walks the order until the members number k and the clusters atleast.
//
// Select.  One workgroup of 256 threads per query walks the query's visit list twice over the cluster-major image of
// the bit rows: consecutive lanes take consecutive image rows, a row is 2 W dwords in registers, and the query words
// are the same for every lane (scalar operands, as in the scan).  Pass A histograms the distances in LDS and keeps
// the first kk = min(k, C_q) candidates, the head KNNFromDistsIndicesSupplied sorts; the cut t and the number of
// candidates still needed at distance t come from a prefix sum over the bins.  Thread 0 runs FAST's std::sort over
// the head.  Pass B recomputes the distances and collects every candidate below the cut and, at the cut, the first
// `need` by seq: head members by the slot std::sort left them at, then the others in position order (a ballot and a
// prefix per tile of 256 positions).  The kk collected items are sorted by (dist, seq) in LDS (bitonic) and written.
// No nq x n array exists on this path.
#include "vaq_bitvec_clusters.h"

#include <float.h>

#include <algorithm>

namespace vaq {

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVE = 64;
constexpr int CP_PER_THREAD = BITVEC_CLUSTERS_MAX / CL_THREADS;  // centres a thread of the plan keeps

__global__ void __launch_bounds__(CL_THREADS)
cluster_gather_kernel(const uint64_t *__restrict__ rows, const int32_t *__restrict__ member, int64_t n, int64_t n_pad, int W,
                      uint64_t *__restrict__ image) {
  const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n_pad * W) return;
  const int64_t g = i / W;
  const int w = (int)(i - g * W);
  image[i] = g < n ? rows[(int64_t)member[g] * W + w] : 0;
}

// bytes of the plan's first LDS region: the query row, then the pairs
__host__ __device__ inline size_t plan_region_bytes(int D, int T) {
  const size_t a = (size_t)D * sizeof(float), b = (size_t)T * sizeof(ClusterPair);
  return ((a > b ? a : b) + 7) & ~(size_t)7;
}

__global__ void __launch_bounds__(CL_THREADS)
cluster_plan_kernel(const float *__restrict__ Q, int D, const float *__restrict__ centres_t, int T,
                    const int32_t *__restrict__ start, int k, int atleast, int32_t *__restrict__ visit_out,
                    BitvecClusterPlan *__restrict__ plan_out) {
  extern __shared__ unsigned char cp_lds[];
  __shared__ int s_tie, s_visit;
  float *qs = reinterpret_cast<float *>(cp_lds);
  ClusterPair *pairs = reinterpret_cast<ClusterPair *>(cp_lds);  // (takes the query's place once the sums are done)
  int *sorted = reinterpret_cast<int *>(cp_lds + plan_region_bytes(D, T));
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += CL_THREADS) qs[j] = Q[(size_t)q * D + j];
  if (tid == 0) s_tie = 0;
  __syncthreads();
  // euclideanDistNoSQRT per centre: distance += (a - b) * (a - b) in dimension order from 0.0f
  float acc[CP_PER_THREAD];
#pragma unroll
  for (int j = 0; j < CP_PER_THREAD; j++) acc[j] = 0.0f;
  const int nj = (T + CL_THREADS - 1) / CL_THREADS;
  for (int i = 0; i < D; i++) {
    const float a = qs[i];
    const float *row = centres_t + (size_t)i * T;
#pragma unroll
    for (int j = 0; j < CP_PER_THREAD; j++) {
      const int c = tid + j * CL_THREADS;
      if (j < nj && c < T) {
        const float t = a - row[c];
        acc[j] += t * t;
      }
    }
  }
  __syncthreads();  // (every thread is done with the query row)
#pragma unroll
  for (int j = 0; j < CP_PER_THREAD; j++) {
    const int c = tid + j * CL_THREADS;
    if (c < T) pairs[c] = ClusterPair{acc[j], c};
  }
  __syncthreads();
  // the position of each centre among the pairs by (dist, c); an equal or NaN distance anywhere: std::sort decides
#pragma unroll
  for (int j = 0; j < CP_PER_THREAD; j++) {
    const int c = tid + j * CL_THREADS;
    if (c >= T) continue;
    const float di = acc[j];
    int rank = 0;
    bool tie = di != di;
    for (int o = 0; o < T; o++) {
      const float dj = pairs[o].dist;
      rank += (dj < di || (dj == di && o < c)) ? 1 : 0;
      tie |= dj == di && o != c;
    }
    sorted[rank] = c;  // (rank <= T - 1: the centre does not count itself)
    if (tie) s_tie = 1;
  }
  __syncthreads();
  const bool fallback = s_tie != 0;
  if (fallback) {
    if (tid == 0) stdsort::sort_by<12, true>(pairs, T, ClusterLt{});
    __syncthreads();
    for (int c = tid; c < T; c += CL_THREADS) sorted[c] = pairs[c].idx;
    __syncthreads();
  }
  if (tid == 0) {
    int visit = 0, cum = 0;
    while (visit < T) {
      const int c = sorted[visit++];
      cum += start[c + 1] - start[c];
      if (cum >= k) break;
    }
    while (visit < atleast) {  // (atleast <= T)
      const int c = sorted[visit++];
      cum += start[c + 1] - start[c];
    }
    s_visit = visit;
    plan_out[q] = BitvecClusterPlan{visit, cum, fallback ? 1 : 0, 0};
  }
  __syncthreads();
  const int visit = s_visit;
  for (int i = tid; i < visit; i += CL_THREADS) visit_out[(size_t)q * T + i] = sorted[i];
}

// hammingDist of image row g to the query's words: 8-byte loads where a row starts on 8 bytes only (W odd)
template <int W>
__device__ __forceinline__ uint32_t cluster_row_dist(const uint32_t *__restrict__ image, int64_t g, const uint32_t (&qw)[2 * W]) {
  uint32_t d = 0;
  if constexpr (W % 2 == 0) {
    const uint4 *p = reinterpret_cast<const uint4 *>(image + g * (2 * W));
#pragma unroll
    for (int i = 0; i < W / 2; i++) {
      const uint4 v = p[i];
      d += __builtin_popcount(v.x ^ qw[4 * i]) + __builtin_popcount(v.y ^ qw[4 * i + 1]) +
           __builtin_popcount(v.z ^ qw[4 * i + 2]) + __builtin_popcount(v.w ^ qw[4 * i + 3]);
    }
  } else {
    const uint2 *p = reinterpret_cast<const uint2 *>(image + g * (2 * W));
#pragma unroll
    for (int i = 0; i < W; i++) {
      const uint2 v = p[i];
      d += __builtin_popcount(v.x ^ qw[2 * i]) + __builtin_popcount(v.y ^ qw[2 * i + 1]);
    }
  }
  return d;
}

// The candidates of one query in visiting order, a tile of CL_THREADS positions at a time: f(valid, p, g, d) is
// called by every thread of the workgroup together (it may hold barriers); p is the position, carried across
// clusters and tiles, g the image row, d its distance.
template <int W, class F>
__device__ __forceinline__ void cluster_walk(const uint32_t *__restrict__ image, const int32_t *__restrict__ start, int T,
                                             const int32_t *__restrict__ vis, int visit, const uint32_t (&qw)[2 * W], F &&f) {
  int base = 0;
  for (int v = 0; v < visit; v++) {
    const int c = vis[v];  // the same for every lane
    if ((unsigned)c >= (unsigned)T) continue;
    const int s = start[c], e = start[c + 1];
    for (int r0 = s; r0 < e; r0 += CL_THREADS) {
      const int64_t g = (int64_t)r0 + threadIdx.x;
      const bool valid = g < e;
      const uint32_t d = valid ? cluster_row_dist<W>(image, g, qw) : 0u;
      f(valid, base + (r0 - s) + (int)threadIdx.x, g, d);
    }
    base += e - s;
  }
}

template <int W>
__global__ void __launch_bounds__(CL_THREADS)
cluster_select_kernel(const uint32_t *__restrict__ image, const int32_t *__restrict__ start, const int32_t *__restrict__ member,
                      int T, const uint32_t *__restrict__ queries, const int32_t *__restrict__ visit_lists,
                      const BitvecClusterPlan *__restrict__ plans, int k, int64_t id_base, int32_t *__restrict__ labels,
                      float *__restrict__ out_dist) {
  constexpr int W2 = 2 * W, BINS = 64 * W + 1, PER = (BINS + CL_THREADS - 1) / CL_THREADS;
  __shared__ uint32_t hist[BINS];
  __shared__ uint32_t head[BITVEC_RERANK_MAX];  // (dist << 16) | p of the first kk candidates
  __shared__ uint16_t inv[BITVEC_RERANK_MAX];   // the slot std::sort left position p at
  __shared__ uint64_t keys[BITVEC_RERANK_MAX];  // (dist << 32) | seq of the collected
  __shared__ int32_t rows_g[BITVEC_RERANK_MAX];  // their image rows
  __shared__ uint32_t scan[CL_THREADS];
  __shared__ int s_wave[CL_THREADS / CL_WAVE];
  __shared__ int s_t, s_need, s_lo, s_ht, s_ncol;
  const int q = blockIdx.x, tid = threadIdx.x;
  const BitvecClusterPlan plan = plans[q];
  const int visit = min(plan.visit, T);
  const int kk = min(k, plan.cand);
  const int32_t *vis = visit_lists + (size_t)q * T;
  int32_t *lab = labels + (size_t)q * k;
  float *dis = out_dist + (size_t)q * k;
  for (int i = max(kk, 0) + tid; i < k; i += CL_THREADS) {
    lab[i] = -1;
    dis[i] = FLT_MAX;
  }
  if (kk <= 0) return;  // (the same for every thread)
  uint32_t qw[W2];
#pragma unroll
  for (int w = 0; w < W2; w++) qw[w] = queries[(size_t)q * W2 + w];  // wave-uniform
  for (int b = tid; b < BINS; b += CL_THREADS) hist[b] = 0;
  if (tid == 0) s_t = 0, s_need = 0, s_lo = 0, s_ht = 0, s_ncol = 0;
  __syncthreads();

  // pass A: the histogram and the head
  cluster_walk<W>(image, start, T, vis, visit, qw, [&](bool valid, int p, int64_t, uint32_t d) {
    if (!valid) return;
    atomicAdd(&hist[d], 1u);
    if (p < kk) head[p] = (d << 16) | (uint32_t)p;
  });
  __syncthreads();

  // the cut: count(< t) < kk <= count(<= t), need = kk - count(< t); a thread owns PER adjacent bins
  uint32_t own = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int b = tid * PER + i;
    own += b < BINS ? hist[b] : 0u;
  }
  scan[tid] = own;
  __syncthreads();
  for (int off = 1; off < CL_THREADS; off <<= 1) {
    const uint32_t v = tid >= off ? scan[tid - off] : 0u;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  uint32_t run = scan[tid] - own;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int b = tid * PER + i;
    const uint32_t cnt = b < BINS ? hist[b] : 0u;
    if (run < (uint32_t)kk && (uint32_t)kk <= run + cnt) {
      s_t = b;
      s_need = kk - (int)run;
    }
    run += cnt;
  }
  // KNNFromDistsIndicesSupplied's std::sort of the first kk pairs by distance alone
  if (tid == 0) stdsort::sort(head, kk);
  __syncthreads();
  const int t = s_t, need = s_need;
  for (int i = tid; i < kk; i += CL_THREADS) {
    const uint32_t item = head[i];
    inv[item & 0xffffu] = (uint16_t)i;
    const int d = (int)(item >> 16);
    if (d < t) atomicAdd(&s_lo, 1);
    if (d == t) atomicAdd(&s_ht, 1);
  }
  __syncthreads();
  // head members at the cut lie at slots lo .. lo + ht - 1 and precede every other candidate at the cut
  const int lo = s_lo, nh_need = need - min(s_ht, need);
  int nh_taken = 0;

  // pass B: collect
  cluster_walk<W>(image, start, T, vis, visit, qw, [&](bool valid, int p, int64_t g, uint32_t d) {
    bool take = false;
    uint32_t seq = (uint32_t)p;
    if (valid) {
      if (p < kk) {
        seq = inv[p];
        take = (int)d < t || ((int)d == t && (int)seq - lo < need);
      } else {
        take = (int)d < t;
      }
    }
    if (nh_taken < nh_need) {  // (the same for every thread)
      const bool tie = valid && p >= kk && (int)d == t;
      const unsigned long long b = __ballot(tie);
      const int lane = tid & (CL_WAVE - 1), wave = tid / CL_WAVE;
      if (lane == 0) s_wave[wave] = __popcll(b);
      __syncthreads();
      int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < CL_THREADS / CL_WAVE; w++) {
        const int n = s_wave[w];
        before += w < wave ? n : 0;
        total += n;
      }
      if (tie && nh_taken + before < nh_need) take = true;
      __syncthreads();  // (s_wave is written again by the next tile)
      nh_taken += total;
    }
    if (take) {
      const int slot = atomicAdd(&s_ncol, 1);
      if (slot < BITVEC_RERANK_MAX) {
        keys[slot] = ((uint64_t)d << 32) | seq;
        rows_g[slot] = (int32_t)g;
      }
    }
  });
  __syncthreads();

  // the collected, kk of them, by (dist, seq)
  const int n = min(s_ncol, kk);
  int P = 1;
  while (P < kk) P <<= 1;
  for (int i = n + tid; i < P; i += CL_THREADS) {
    keys[i] = ~0ull;
    rows_g[i] = -1;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += CL_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const uint64_t a = keys[i], b = keys[o];
          if ((a > b) == ((i & size) == 0)) {
            keys[i] = b;
            keys[o] = a;
            const int32_t r = rows_g[i];
            rows_g[i] = rows_g[o];
            rows_g[o] = r;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < kk; i += CL_THREADS) {
    const int32_t g = rows_g[i];
    lab[i] = g >= 0 ? (int32_t)(member[g] + id_base) : -1;
    dis[i] = g >= 0 ? (float)(uint32_t)(keys[i] >> 32) : FLT_MAX;
  }
}

template <int W>
hipError_t select_w(const uint64_t *image, const int32_t *start, const int32_t *member, int T, const uint64_t *queries,
                    int nq, const int32_t *visit, const BitvecClusterPlan *plan, int k, int64_t id_base, int32_t *labels,
                    float *out_dist, hipStream_t st) {
  hipLaunchKernelGGL(cluster_select_kernel<W>, dim3(nq), dim3(CL_THREADS), 0, st, reinterpret_cast<const uint32_t *>(image),
                     start, member, T, reinterpret_cast<const uint32_t *>(queries), visit, plan, k, id_base, labels, out_dist);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bitvec_cluster_gather(const uint64_t *rows, const int32_t *member, int64_t n, int64_t n_pad, int W,
                                        uint64_t *image, hipStream_t st) {
  if (n_pad <= 0) return hipSuccess;
  if (n < 0 || n > n_pad || W < 1 || W > BITVEC_MAX_WORDS) return hipErrorInvalidValue;
  const int64_t blocks = (n_pad * W + CL_THREADS - 1) / CL_THREADS;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cluster_gather_kernel, dim3((unsigned)blocks), dim3(CL_THREADS), 0, st, rows, member, n, n_pad, W, image);
  return hipGetLastError();
}

hipError_t launch_bitvec_cluster_plan(const float *ori_queries, int nq, int D, const float *centres_t, int T,
                                      const int32_t *start, int k, int atleast, int32_t *visit_out,
                                      BitvecClusterPlan *plan_out, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX || k < 1 || atleast < 1 || atleast > T)
    return hipErrorInvalidValue;
  const size_t lds = plan_region_bytes(D, T) + (size_t)T * sizeof(int);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(cluster_plan_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_plan_kernel, dim3(nq), dim3(CL_THREADS), lds, st, ori_queries, D, centres_t, T, start, k, atleast,
                     visit_out, plan_out);
  return hipGetLastError();
}

hipError_t launch_bitvec_cluster_select(const uint64_t *image, int W, const int32_t *start, const int32_t *member,
                                        int T, const uint64_t *queries, int nq, const int32_t *visit,
                                        const BitvecClusterPlan *plan, int k, int64_t id_base, int32_t *labels,
                                        float *out_dist, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (T < 1 || T > BITVEC_CLUSTERS_MAX || k < 1 || k > BITVEC_RERANK_MAX) return hipErrorInvalidValue;
  switch (W) {
#define VAQ_BITVEC_CASE(w) \
  case w: return select_w<w>(image, start, member, T, queries, nq, visit, plan, k, id_base, labels, out_dist, st);
    VAQ_BITVEC_CASE(1) VAQ_BITVEC_CASE(2) VAQ_BITVEC_CASE(3) VAQ_BITVEC_CASE(4) VAQ_BITVEC_CASE(5) VAQ_BITVEC_CASE(6)
    VAQ_BITVEC_CASE(7) VAQ_BITVEC_CASE(8) VAQ_BITVEC_CASE(9) VAQ_BITVEC_CASE(10) VAQ_BITVEC_CASE(11) VAQ_BITVEC_CASE(12)
    VAQ_BITVEC_CASE(13) VAQ_BITVEC_CASE(14) VAQ_BITVEC_CASE(15) VAQ_BITVEC_CASE(16)
#undef VAQ_BITVEC_CASE
  }
  return hipErrorInvalidValue;
}

}  // namespace vaq
