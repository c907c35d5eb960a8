// vaq_cluster_index.hip -- the gfx950 kernel of vaq_cluster_index.h ("Cluster index").
//
// Lane = row: a row's sum against one centre is a serial chain in dimension order, so a thread owns a row and keeps
// the running sums of a block of TC = 64 centres in registers.  A workgroup of 256 threads owns 256 consecutive rows.
// Centre blocks are the outer loop, chunks of DC = 32 dimensions the inner one: a (row, centre) sum is carried through
// all D before the lane folds its 64 sums into (nearestDist, nearestIdx) in centre order with the strict `<`.
//
// Both operands go through LDS.  The rows' chunk lies there as floats with a row stride of 33 dwords (a lane reading
// its own row meets its own bank); it is loaded from the row-major rows by eight adjacent lanes per row in 16-byte
// pieces (4-byte pieces of a byte row) where D % 4 == 0 and the base is aligned, by thirty-two adjacent lanes element
// by element otherwise, and a byte is widened on the way.  The centres' DC x TC tile lies beside it dimension-major
// (stride 68 dwords: 16-byte aligned, and the staging writes of adjacent dimensions land four banks apart): per
// dimension a lane reads its own element once and the 64 centre values at a wave-uniform address, four to a
// ds_read_b128, then spends 3 x 64 vector operations on them.  The next step's global loads are issued before the
// present step's sums, across the block boundary too.  Rows are read again for every centre block.
#include "vaq_cluster_index.h"

#include <float.h>

namespace vaq {

namespace {

constexpr int CI_THREADS = 256;
constexpr int CI_DC = CLUSTER_INDEX_DC;
constexpr int CI_TC = CLUSTER_INDEX_TC;
constexpr int CI_ROW_STRIDE = CI_DC + 1;  // dwords between two rows of the tile: odd
constexpr int CI_CEN_STRIDE = CI_TC + 4;  // dwords between two dimensions of the centre tile: a multiple of 4
constexpr int CI_CEN_PER = CI_DC * CI_TC / CI_THREADS;  // centre values a thread stages per step
static_assert(CI_DC == 32, "a thread carries 8 pieces of 4, or 32 elements, of a chunk: 256 rows x 32 over 256 threads");
static_assert(CI_TC % 4 == 0 && CI_CEN_PER * CI_THREADS == CI_DC * CI_TC && CI_THREADS / CI_DC * CI_CEN_PER == CI_TC,
              "the centre tile is dealt out dimension = tid % 32, centres tid / 32 + 8 i");

__device__ __forceinline__ void ci_load4(const float *y, float *v) {
  const float4 t = *reinterpret_cast<const float4 *>(y);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ci_load4(const uint8_t *y, float *v) {
  const uint32_t t = *reinterpret_cast<const uint32_t *>(y);
  v[0] = (float)(t & 255u); v[1] = (float)((t >> 8) & 255u); v[2] = (float)((t >> 16) & 255u); v[3] = (float)(t >> 24);
}

// The elements [d0, d0 + DC) of rows [r0, r0 + 256) into a thread's registers.  VEC: thread = piece tid % 8 of rows
// tid / 8 + 32 i; otherwise element tid % 32 of rows tid / 32 + 8 i.  Nothing is read past row n - 1 or past a row's D
// elements: those slots are 0.
template <typename T, bool VEC>
__device__ __forceinline__ void ci_fetch_rows(const T *__restrict__ rows, int64_t n, int D, int64_t r0, int d0, float (&v)[CI_DC]) {
  const int tid = threadIdx.x;
  if constexpr (VEC) {
    const int e = d0 + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int64_t row = r0 + i * 32 + (tid >> 3);
      if (row < n && e < D) {  // (D % 4 == 0: the piece is inside the row)
        ci_load4(rows + (size_t)row * D + e, &v[4 * i]);
      } else {
        v[4 * i] = v[4 * i + 1] = v[4 * i + 2] = v[4 * i + 3] = 0.0f;
      }
    }
  } else {
    const int e = d0 + (tid & 31);
#pragma unroll
    for (int i = 0; i < 32; i++) {
      const int64_t row = r0 + i * 8 + (tid >> 5);
      v[i] = (row < n && e < D) ? (float)rows[(size_t)row * D + e] : 0.0f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void ci_stage_rows(float *tile, const float (&v)[CI_DC]) {
  const int tid = threadIdx.x;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      float *t = tile + (i * 32 + (tid >> 3)) * CI_ROW_STRIDE + (tid & 7) * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = v[4 * i + j];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 32; i++) tile[(i * 8 + (tid >> 5)) * CI_ROW_STRIDE + (tid & 31)] = v[i];
  }
}

// dimension d0 + tid % 32 of centres c0 + tid / 32 + 8 i; 0 past centre T - 1 and past dimension D - 1
__device__ __forceinline__ void ci_fetch_centres(const float *__restrict__ centroids, int T, int D, int c0, int d0,
                                                 float (&cv)[CI_CEN_PER]) {
  const int tid = threadIdx.x, e = d0 + (tid & 31);
#pragma unroll
  for (int i = 0; i < CI_CEN_PER; i++) {
    const int c = c0 + (tid >> 5) + 8 * i;
    cv[i] = (c < T && e < D) ? centroids[(size_t)c * D + e] : 0.0f;
  }
}

__device__ __forceinline__ void ci_stage_centres(float *cen, const float (&cv)[CI_CEN_PER]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < CI_CEN_PER; i++) cen[(tid & 31) * CI_CEN_STRIDE + (tid >> 5) + 8 * i] = cv[i];
}

// one dimension of the lane's row against the block's centres: dist += (x - c) * (x - c), every step on its own
__device__ __forceinline__ void ci_dimension(float x, const float *cen, float (&acc)[CI_TC]) {
#pragma unroll
  for (int i = 0; i < CI_TC / 4; i++) {
    const float4 c = *reinterpret_cast<const float4 *>(cen + 4 * i);  // the same address in every lane
    const float t0 = x - c.x, t1 = x - c.y, t2 = x - c.z, t3 = x - c.w;
    acc[4 * i] += t0 * t0;
    acc[4 * i + 1] += t1 * t1;
    acc[4 * i + 2] += t2 * t2;
    acc[4 * i + 3] += t3 * t3;
  }
}

// ROOT (the k-means fit's assign, vaq_kmeans_fit.h): a finished sum becomes its square root before it meets the fold,
// so two sums whose roots round to one float keep the earlier centre.  Nothing else differs.
template <typename T, bool VEC, bool ROOT>
__global__ void __launch_bounds__(CI_THREADS)
cluster_index_kernel(const T *__restrict__ rows, int64_t n, int D, const float *__restrict__ centroids, int nT,
                     int32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
  __shared__ float tile[CI_THREADS * CI_ROW_STRIDE];
  __shared__ __attribute__((aligned(16))) float cen[CI_DC * CI_CEN_STRIDE];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CI_THREADS;
  const float *mine = tile + tid * CI_ROW_STRIDE;
  float nearest = FLT_MAX;
  int nearest_c = -1;
  float v[CI_DC], cv[CI_CEN_PER];
  ci_fetch_rows<T, VEC>(rows, n, D, r0, 0, v);
  ci_fetch_centres(centroids, nT, D, 0, 0, cv);

  for (int c0 = 0; c0 < nT; c0 += CI_TC) {
    float acc[CI_TC];
#pragma unroll
    for (int i = 0; i < CI_TC; i++) acc[i] = 0.0f;
    for (int d0 = 0; d0 < D; d0 += CI_DC) {
      ci_stage_rows<VEC>(tile, v);
      ci_stage_centres(cen, cv);
      __syncthreads();
      // the next step's operands: the next chunk of this block, or the first chunk of the next block
      const bool last_chunk = d0 + CI_DC >= D;
      const int nc0 = last_chunk ? c0 + CI_TC : c0, nd0 = last_chunk ? 0 : d0 + CI_DC;
      if (nc0 < nT) {
        ci_fetch_rows<T, VEC>(rows, n, D, r0, nd0, v);
        ci_fetch_centres(centroids, nT, D, nc0, nd0, cv);
      }
      if (!last_chunk || D - d0 == CI_DC) {
#pragma unroll 4
        for (int j = 0; j < CI_DC; j++) ci_dimension(mine[j], cen + j * CI_CEN_STRIDE, acc);
      } else {
        for (int j = 0; j < D - d0; j++) ci_dimension(mine[j], cen + j * CI_CEN_STRIDE, acc);
      }
      __syncthreads();
    }
    // the fold, in centre order; a centre past T - 1 holds the sum against zeros and is left out
#pragma unroll
    for (int i = 0; i < CI_TC; i++) {
      if constexpr (ROOT) acc[i] = sqrtf(acc[i]);
      if (c0 + i < nT && acc[i] < nearest) {
        nearest = acc[i];
        nearest_c = c0 + i;
      }
    }
  }
  if (r0 + tid < n) {
    idx_out[r0 + tid] = nearest_c;
    if (dist_out) dist_out[r0 + tid] = nearest;
  }
}

template <typename T, bool ROOT>
hipError_t cluster_index_t(const void *rows, bool vec, int64_t n, int D, const float *centroids, int T_, int32_t *idx_out,
                           float *dist_out, hipStream_t st) {
  const dim3 grid((unsigned)((n + CI_THREADS - 1) / CI_THREADS));
  if (vec)
    hipLaunchKernelGGL((cluster_index_kernel<T, true, ROOT>), grid, dim3(CI_THREADS), 0, st, static_cast<const T *>(rows), n, D,
                       centroids, T_, idx_out, dist_out);
  else
    hipLaunchKernelGGL((cluster_index_kernel<T, false, ROOT>), grid, dim3(CI_THREADS), 0, st, static_cast<const T *>(rows), n, D,
                       centroids, T_, idx_out, dist_out);
  return hipGetLastError();
}

template <bool ROOT>
hipError_t cluster_index_any(RowsRef rows, int64_t n, int D, const float *centroids, int T, int32_t *idx_out, float *dist_out,
                             hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (D < 1 || D > BITVEC_CLUSTERS_MAX_DIM || T < 1 || T > BITVEC_CLUSTERS_MAX || n < 0 || n > 0x7fffffffLL ||
      (rows.elem != 4 && rows.elem != 1) || !rows.p || !centroids || !idx_out)
    return hipErrorInvalidValue;
  // whole aligned pieces of four elements: 16 bytes of floats, 4 of bytes
  const bool vec = D % 4 == 0 && reinterpret_cast<uintptr_t>(rows.p) % (size_t)(4 * rows.elem) == 0;
  if (rows.elem == 1) return cluster_index_t<uint8_t, ROOT>(rows.p, vec, n, D, centroids, T, idx_out, dist_out, st);
  return cluster_index_t<float, ROOT>(rows.p, vec, n, D, centroids, T, idx_out, dist_out, st);
}

}  // namespace

hipError_t launch_cluster_index(RowsRef rows, int64_t n, int D, const float *centroids, int T, int32_t *idx_out,
                                float *dist_out, hipStream_t st) {
  return cluster_index_any<false>(rows, n, D, centroids, T, idx_out, dist_out, st);
}

hipError_t launch_cluster_index_root(RowsRef rows, int64_t n, int D, const float *centroids, int T, int32_t *idx_out,
                                     float *dist_out, hipStream_t st) {
  return cluster_index_any<true>(rows, n, D, centroids, T, idx_out, dist_out, st);
}

}  // namespace vaq
