// vaq_bitvec.hip -- gfx950 kernels of the Hamming queries of BitVecEngine (vaq_bitvec.h).
//
// Scan.  A thread keeps two adjacent rows in registers (4 W dwords, at most 64) and meets the BITVEC_QT queries of
// its workgroup's tile one after the other.  A query word is the same for every lane: its address depends on the
// workgroup and the loop counters only, so it is fetched by a scalar load and is the scalar operand of the XOR; a
// 32-bit word of a pair then costs one v_xor_b32 and one v_bcnt_u32_b32, which adds to the running sum.  The rows
// are read once per query tile (16-byte loads, a thread's two rows are contiguous), never once per query.  The two
// distances of a thread go out as one dword, adjacent lanes adjacent: 256 contiguous bytes per wave and query.
//
// Rerank.  One workgroup per query, the query row staged in LDS.  A thread computes one candidate's distance by the
// reference's own loop (one accumulator, dimension order); thread 0 runs std::sort over the first kk pairs; then
// every candidate counts the pairs ahead of it by (dist, position) and the first kk are written.
#include "vaq_bitvec.h"

#include <float.h>

#include <algorithm>

namespace vaq {

namespace {

template <int W>
__global__ void __launch_bounds__(BITVEC_THREADS)
bitvec_scan_kernel(const uint32_t *__restrict__ rows, int64_t n_pad, const uint32_t *__restrict__ queries, int nq,
                   uint16_t *__restrict__ dist) {
  constexpr int W2 = 2 * W;  // dwords per row
  const int64_t r0 = ((int64_t)blockIdx.x * BITVEC_THREADS + threadIdx.x) * BITVEC_ROWS_PER_THREAD;
  if (r0 >= n_pad) return;  // (n_pad is even: both rows of a thread are inside or neither; no barrier follows)
  uint32_t x[2 * W2];
  const uint4 *p = reinterpret_cast<const uint4 *>(rows + r0 * W2);  // 8 W bytes a row: two rows start on 16 bytes
#pragma unroll
  for (int i = 0; i < W; i++) {
    const uint4 v = p[i];
    x[4 * i] = v.x;
    x[4 * i + 1] = v.y;
    x[4 * i + 2] = v.z;
    x[4 * i + 3] = v.w;
  }
  const int q0 = blockIdx.y * BITVEC_QT;
  const int qn = min(BITVEC_QT, nq - q0);
  const uint32_t *qp = queries + (int64_t)q0 * W2;
  uint32_t *out = reinterpret_cast<uint32_t *>(dist + (int64_t)q0 * n_pad + r0);
  const int64_t stride = n_pad / 2;  // dwords between the same rows of two queries
  for (int t = 0; t < qn; t++) {
    uint32_t d0 = 0, d1 = 0;
#pragma unroll
    for (int w = 0; w < W2; w++) {
      const uint32_t qw = qp[t * W2 + w];  // wave-uniform
      d0 += __builtin_popcount(x[w] ^ qw);
      d1 += __builtin_popcount(x[W2 + w] ^ qw);
    }
    out[(int64_t)t * stride] = d0 | (d1 << 16);
  }
}

constexpr int RR_THREADS = 256;

__device__ __forceinline__ void rr_load4(const float *y, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4 *>(y);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void rr_load4(const uint8_t *y, float (&v)[4]) {
  const uint32_t t = *reinterpret_cast<const uint32_t *>(y);
  v[0] = (float)(t & 255u); v[1] = (float)((t >> 8) & 255u); v[2] = (float)((t >> 16) & 255u); v[3] = (float)(t >> 24);
}

// euclideanDistNoSQRT(query, row): one accumulator from 0.0f, distance += (a - b) * (a - b) in dimension order
template <typename T>
__device__ __forceinline__ float rr_dist(const float *qs, const T *y, int D) {
  float distance = 0.0f;
  int i = 0;
  if ((D & 3) == 0) {  // rows of 4 j elements start on 4 (bytes) or 16 (floats) bytes: the same additions, wider loads
    for (; i < D; i += 4) {
      float v[4];
      rr_load4(y + i, v);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float t = qs[i + j] - v[j];
        distance += t * t;
      }
    }
  }
  for (; i < D; i++) {
    const float t = qs[i] - (float)y[i];
    distance += t * t;
  }
  return distance;
}

template <typename T>
__global__ void __launch_bounds__(RR_THREADS)
bitvec_rerank_kernel(const float *__restrict__ Q, int D, const T *__restrict__ rows, int64_t N, int64_t id_base,
                     const int32_t *__restrict__ cand, int64_t cand_stride, int R, int k, int32_t *__restrict__ labels,
                     float *__restrict__ out_dist) {
  __shared__ RerankPair items[BITVEC_RERANK_MAX];
  extern __shared__ float rr_qs[];
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < D; j += RR_THREADS) rr_qs[j] = Q[(size_t)q * D + j];
  __syncthreads();
  for (int c = tid; c < R; c += RR_THREADS) {
    const int lab = cand[(int64_t)q * cand_stride + c];
    const int64_t row = (int64_t)lab - id_base;
    const bool valid = lab >= 0 && row >= 0 && row < N;  // (checked before the row's address is formed)
    RerankPair it;
    it.dist = valid ? rr_dist(rr_qs, rows + (size_t)(valid ? row : 0) * D, D) : INFINITY;
    it.idx = valid ? lab : -1;
    items[c] = it;
  }
  __syncthreads();
  const int kk = min(k, R);
  if (tid == 0) rerank_sort(items, kk);
  __syncthreads();
  // positions are the seq of the (dist, seq) order: the head lies as std::sort left it, the others behind it in
  // candidate order
  for (int c = tid; c < R; c += RR_THREADS) {
    const float di = items[c].dist;
    int rank = 0;
    for (int j = 0; j < R; j++) {
      const float dj = items[j].dist;
      rank += (dj < di || (dj == di && j < c)) ? 1 : 0;
    }
    if (rank < kk) {
      labels[(size_t)q * k + rank] = items[c].idx;
      out_dist[(size_t)q * k + rank] = di;
    }
  }
  for (int i = kk + tid; i < k; i += RR_THREADS) {
    labels[(size_t)q * k + i] = -1;
    out_dist[(size_t)q * k + i] = FLT_MAX;
  }
}

template <int W>
hipError_t scan_w(const uint64_t *rows, int64_t n_pad, const uint64_t *queries, int nq, uint16_t *dist, hipStream_t st) {
  const int64_t blocks = (n_pad + BITVEC_ROW_TILE - 1) / BITVEC_ROW_TILE;
  const int qtiles = (nq + BITVEC_QT - 1) / BITVEC_QT;
  hipLaunchKernelGGL(bitvec_scan_kernel<W>, dim3((unsigned)blocks, (unsigned)qtiles), dim3(BITVEC_THREADS), 0, st,
                     reinterpret_cast<const uint32_t *>(rows), n_pad, reinterpret_cast<const uint32_t *>(queries), nq, dist);
  return hipGetLastError();
}

template <typename T>
hipError_t rerank_t(const float *queries, int nq, int D, const void *rows, int64_t N, int64_t id_base, const int32_t *cand,
                    int64_t cand_stride, int R, int k, int32_t *labels, float *out_dist, hipStream_t st) {
  const size_t lds = (size_t)D * sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(bitvec_rerank_kernel<T>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bitvec_rerank_kernel<T>, dim3(nq), dim3(RR_THREADS), lds, st, queries, D, static_cast<const T *>(rows), N,
                     id_base, cand, cand_stride, R, k, labels, out_dist);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bitvec_scan(const uint64_t *rows, int64_t n_pad, int W, const uint64_t *queries, int nq,
                              uint16_t *dist, hipStream_t st) {
  if (nq <= 0 || n_pad <= 0) return hipSuccess;
  if (n_pad % FAST_ROW_PAD != 0 || W < 1 || W > BITVEC_MAX_WORDS) return hipErrorInvalidValue;
  if ((nq + BITVEC_QT - 1) / BITVEC_QT > 65535 || (n_pad + BITVEC_ROW_TILE - 1) / BITVEC_ROW_TILE > 0x7fffffffLL)
    return hipErrorInvalidValue;
  switch (W) {
#define VAQ_BITVEC_CASE(w) case w: return scan_w<w>(rows, n_pad, queries, nq, dist, st);
    VAQ_BITVEC_CASE(1) VAQ_BITVEC_CASE(2) VAQ_BITVEC_CASE(3) VAQ_BITVEC_CASE(4) VAQ_BITVEC_CASE(5) VAQ_BITVEC_CASE(6)
    VAQ_BITVEC_CASE(7) VAQ_BITVEC_CASE(8) VAQ_BITVEC_CASE(9) VAQ_BITVEC_CASE(10) VAQ_BITVEC_CASE(11) VAQ_BITVEC_CASE(12)
    VAQ_BITVEC_CASE(13) VAQ_BITVEC_CASE(14) VAQ_BITVEC_CASE(15) VAQ_BITVEC_CASE(16)
#undef VAQ_BITVEC_CASE
  }
  return hipErrorInvalidValue;
}

size_t bitvec_rerank_max_dim() { return (size_t)(64 * 1024 - sizeof(RerankPair) * BITVEC_RERANK_MAX - 256) / sizeof(float); }

hipError_t launch_bitvec_rerank(const float *queries, int nq, int D, RowsRef rows, int64_t N, int64_t id_base,
                                const int32_t *cand, int64_t cand_stride, int R, int k, int32_t *labels,
                                float *out_dist, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (D < 1 || (size_t)D > bitvec_rerank_max_dim() || R < 1 || R > BITVEC_RERANK_MAX || k < 1 || cand_stride < R ||
      (rows.elem != 4 && rows.elem != 1))
    return hipErrorInvalidValue;
  if (rows.elem == 1)
    return rerank_t<uint8_t>(queries, nq, D, rows.p, N, id_base, cand, cand_stride, R, k, labels, out_dist, st);
  return rerank_t<float>(queries, nq, D, rows.p, N, id_base, cand, cand_stride, R, k, labels, out_dist, st);
}

}  // namespace vaq
