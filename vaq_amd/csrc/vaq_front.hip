// vaq_front.hip -- the query front end: what a search does with its queries before the scan starts.
// (Numerics: vaq_common.h.  Wavefront = 64 lanes everywhere.)
//
// Kernels
//   project_kernel, project_tile_kernel      VAQ::ProjectOnEigenVectors   VAQ.hpp:198-201
//   lut_build_kernel, lut_build_batch_kernel VAQ::CreateLUT<maxbit>       VAQ.hpp:128-167
//   lut_expand_kernel                        packed tables -> the reference's LUTType (test hook)
//   slice_order_kernel, query_order_kernel   the order of a multi-slice scan's slices and of a pass's queries
//   query_cost_kernel, cost_scatter_kernel   expensive queries first (best-first form, one workgroup per query)
#include "vaq_front.h"
#include "vaq_scan.h"  // HOT_MAX_BUCKETS, float_to_bits, bits_to_float

#include <float.h>

namespace vaq {
// ---------------------------------------------------------------------------
// VAQ::ProjectOnEigenVectors, VAQ.hpp:198-201: out = (X * mEigenVectors).real()
// One workgroup per row; thread c owns output column c; fmaf chain over the
// inner index ascending (the reference leaves the order to Eigen's GEMM).
// ---------------------------------------------------------------------------
// checked: BitVecEngine::ProjectOnEigenVectors(Z, withChecking = true) (BitVecEngine.hpp:53-71, called
// by queryLUT at :1226): a coordinate that comes out NaN or infinite is replaced by 0.  E == nullptr
// stands for the identity matrix: the product z * I is then NaN in EVERY column as soon as one
// component of z is not finite (NaN * 0 and inf * 0 are NaN), i.e. the whole row becomes 0.
// T: the rows' element, float or uint8_t (RowsRef).  A byte is widened where it is loaded ((float)uint8 is exact) and
// sits in LDS as the float the float form would have loaded: nothing after the load differs.
template <typename T>
__global__ void project_kernel(const T *__restrict__ X, int D,
                               const float *__restrict__ E, float *__restrict__ out, int checked) {
  extern __shared__ float xs[];
  __shared__ int bad;
  const int64_t r = blockIdx.x;
  if (threadIdx.x == 0) bad = 0;
  for (int j = threadIdx.x; j < D; j += blockDim.x) xs[j] = (float)X[r * D + j];
  __syncthreads();
  if (!E) {
    for (int j = threadIdx.x; j < D; j += blockDim.x)
      if (!(fabsf(xs[j]) <= FLT_MAX)) bad = 1;
    __syncthreads();
    const bool zero = checked && bad;
    for (int c = threadIdx.x; c < D; c += blockDim.x) out[r * D + c] = zero ? 0.0f : xs[c];
    return;
  }
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float acc = 0.0f;
    for (int j = 0; j < D; j++) acc = __builtin_fmaf(xs[j], E[(size_t)j * D + c], acc);
    if (checked && !(fabsf(acc) <= FLT_MAX)) acc = 0.0f;
    out[r * D + c] = acc;
  }
}

// Many rows (the encoder's input: VAQ::encode projects the whole dataset, VAQ.cpp:294): a workgroup
// takes RPT * (256 / D) rows, thread (h, c) keeps RPT outputs of column c in registers, the rows sit in
// LDS and are read four inner indices at a time (one ds_read_b128, the same address for the whole
// wave: a broadcast).  Every output is still ONE fmaf chain over the inner index ascending from 0,
// so the result is bit for bit the one-row-per-workgroup kernel's; per four inner steps a thread
// issues 4 loads of E, RPT LDS reads and 4 RPT FMAs.
// Byte rows (T = uint8_t) are widened on the way INTO LDS, so the FMA loop below reads the floats it always read.  Four
// consecutive bytes come in as one dword where the source is 4-byte aligned (PACKED; a tile starts at a multiple of D_
// bytes, so that is the alignment of X itself) and as four byte loads where it is not: a quarter of the float form's
// bytes either way, and no misaligned dword load.
template <bool PACKED>
__device__ __forceinline__ float4 project_load4(const float *p) {
  return *reinterpret_cast<const float4 *>(p);
}
template <bool PACKED>
__device__ __forceinline__ float4 project_load4(const uint8_t *p) {
  if (PACKED) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
    return make_float4((float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24));
  }
  return make_float4((float)p[0], (float)p[1], (float)p[2], (float)p[3]);
}

template <int D_, int RPT, typename T, bool PACKED>
__global__ __launch_bounds__(256) void project_tile_kernel(const T *__restrict__ X, int64_t n,
                                                           const float *__restrict__ E, float *__restrict__ out,
                                                           int checked) {
  constexpr int G = 256 / D_, R = G * RPT;
  __shared__ __attribute__((aligned(16))) float xs[R * D_];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  for (int i = tid; i < R * D_ / 4; i += 256) {
    const int64_t row = row0 + (i * 4) / D_;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row < n) v = project_load4<PACKED>(X + row0 * D_ + (int64_t)i * 4);
    reinterpret_cast<float4 *>(xs)[i] = v;
  }
  __syncthreads();
  const int c = tid % D_, h = tid / D_;
  float acc[RPT];
#pragma unroll
  for (int r = 0; r < RPT; r++) acc[r] = 0.0f;
  for (int j = 0; j < D_; j += 4) {
    const float e0 = E[(size_t)(j + 0) * D_ + c], e1 = E[(size_t)(j + 1) * D_ + c];
    const float e2 = E[(size_t)(j + 2) * D_ + c], e3 = E[(size_t)(j + 3) * D_ + c];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
      const float4 xv = *reinterpret_cast<const float4 *>(&xs[(h * RPT + r) * D_ + j]);
      acc[r] = __builtin_fmaf(xv.x, e0, acc[r]);
      acc[r] = __builtin_fmaf(xv.y, e1, acc[r]);
      acc[r] = __builtin_fmaf(xv.z, e2, acc[r]);
      acc[r] = __builtin_fmaf(xv.w, e3, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < RPT; r++) {
    const int64_t row = row0 + h * RPT + r;
    float a = acc[r];
    if (checked && !(fabsf(a) <= FLT_MAX)) a = 0.0f;
    if (row < n) out[row * D_ + c] = a;
  }
}

// The tiled kernel from this many rows on: a query batch too (10 k rows: 0.025 -> 0.013 ms with 8 rows per
// thread, C2 step 0.491 -> 0.480 ms); the encoder's millions of rows take 16 per thread.
#ifndef VAQ_PROJECT_TILE_MIN
#define VAQ_PROJECT_TILE_MIN 2048
#endif
#ifndef VAQ_PROJECT_TILE_RPT_SMALL
#define VAQ_PROJECT_TILE_RPT_SMALL 8
#endif
constexpr int64_t PROJECT_TILE_MIN_ROWS = VAQ_PROJECT_TILE_MIN;
constexpr int64_t PROJECT_TILE_BIG_ROWS = 65536;

template <int RPT, typename T, bool PACKED>
static hipError_t launch_project_tile_as(const T *X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked) {
  const int R = (256 / D) * RPT;
  const dim3 grid((unsigned)((n + R - 1) / R));
  if (D == 64) hipLaunchKernelGGL((project_tile_kernel<64, RPT, T, PACKED>), grid, dim3(256), 0, st, X, n, E, out, checked);
  else if (D == 128) hipLaunchKernelGGL((project_tile_kernel<128, RPT, T, PACKED>), grid, dim3(256), 0, st, X, n, E, out, checked);
  else hipLaunchKernelGGL((project_tile_kernel<256, RPT, T, PACKED>), grid, dim3(256), 0, st, X, n, E, out, checked);
  return hipGetLastError();
}

template <int RPT>
static hipError_t launch_project_tile(const float *X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked) {
  return launch_project_tile_as<RPT, float, true>(X, n, D, E, out, st, checked);
}
// byte rows: a device caller may hand over any address (a view that starts at an odd byte)
template <int RPT>
static hipError_t launch_project_tile(const uint8_t *X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked) {
  if ((reinterpret_cast<uintptr_t>(X) & 3u) == 0) return launch_project_tile_as<RPT, uint8_t, true>(X, n, D, E, out, st, checked);
  return launch_project_tile_as<RPT, uint8_t, false>(X, n, D, E, out, st, checked);
}

template <typename T>
static hipError_t launch_project_rows(const T *X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked) {
  if (n == 0) return hipSuccess;
  if (E && n >= PROJECT_TILE_MIN_ROWS && (D == 64 || D == 128 || D == 256)) {
    if (n >= PROJECT_TILE_BIG_ROWS) return launch_project_tile<16>(X, n, D, E, out, st, checked);
    return launch_project_tile<VAQ_PROJECT_TILE_RPT_SMALL>(X, n, D, E, out, st, checked);
  }
  // (one workgroup per row: batching 8 rows per workgroup, as the LUT build does with queries,
  //  was measured slower here -- 0.044 vs 0.030 ms for 10 k rows: too few workgroups to fill the chip)
  int threads = D < 256 ? ((D + 63) / 64) * 64 : 256;
  hipLaunchKernelGGL(project_kernel<T>, dim3((unsigned)n), dim3(threads), D * sizeof(float), st, X, D,
                     E, out, checked);
  return hipGetLastError();
}

hipError_t launch_project(const float *X, int64_t n, int D, const float *E, float *out,
                          hipStream_t st, int checked) {
  return launch_project_rows(X, n, D, E, out, st, checked);
}

hipError_t launch_project(RowsRef X, int64_t n, int D, const float *E, float *out, hipStream_t st, int checked) {
  if (X.elem == 1) return launch_project_rows(static_cast<const uint8_t *>(X.p), n, D, E, out, st, checked);
  if (X.elem != 4) return hipErrorInvalidValue;
  return launch_project_rows(static_cast<const float *>(X.p), n, D, E, out, st, checked);
}

// ---------------------------------------------------------------------------
// VAQ::CreateLUT<maxbit>, VAQ.hpp:128-167.  grid = (query, subspace); one
// thread per centroid.
//   ncent >= 8 (:134-159): acc = fma(diff, diff, acc) for j ascending, from 0.
//   ncent <  8 (:161-165): fvec_L2sqr_ny, utils/Math.hpp:147-171, with the
//       SSE reduction orders of :38-128 for L in {1,2,4,8,12}; sequential
//       multiply-then-add otherwise (:8-19).
// Output is the packed LUT (no zero tails): lut[q][lut_off[s] + c].
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sqdiff(float x, float y) {
  float t = x - y;
  return t * t;
}

__global__ void lut_build_kernel(const float *__restrict__ qproj, int D, int L,
                                 const SubDesc *__restrict__ sub,
                                 const float *__restrict__ cent_t, int lut_floats,
                                 float *__restrict__ lut, int only_small) {
  extern __shared__ float qs[];
  const int q = blockIdx.x, s = blockIdx.y;
  const SubDesc sd = sub[s];
  if ((int)(blockIdx.z * blockDim.x) >= sd.ncent) return;  // chunk beyond this subspace's codebook
  if (only_small && sd.ncent >= 8) return;                 // (the batched kernel did those)
  for (int j = threadIdx.x; j < L; j += blockDim.x) qs[j] = qproj[(size_t)q * D + (size_t)s * L + j];
  __syncthreads();
  float *out = lut + (size_t)q * lut_floats + sd.lut_off;
  // dimension-major codebook: y(j) of centroid c at cs[j * K + c], so a wave reads 64
  // consecutive floats per dimension
  const float *cs = cent_t + sd.cent_off;
  const int K = sd.ncent;
#define Y(j) cs[(size_t)(j) * K + c]
  for (int c = blockIdx.z * blockDim.x + threadIdx.x; c < K; c += gridDim.z * blockDim.x) {
    float r;
    if (K >= 8) {
      float acc = 0.0f;
      for (int j = 0; j < L; j++) {
        float diff = qs[j] - Y(j);
        acc = __builtin_fmaf(diff, diff, acc);
      }
      r = acc;
    } else if (L == 1) {
      r = sqdiff(qs[0], Y(0));
    } else if (L == 2) {
      r = sqdiff(qs[0], Y(0)) + sqdiff(qs[1], Y(1));
    } else if (L == 4) {
      r = (sqdiff(qs[0], Y(0)) + sqdiff(qs[1], Y(1))) + (sqdiff(qs[2], Y(2)) + sqdiff(qs[3], Y(3)));
    } else if (L == 8) {
      float a0 = sqdiff(qs[0], Y(0)) + sqdiff(qs[4], Y(4));
      float a1 = sqdiff(qs[1], Y(1)) + sqdiff(qs[5], Y(5));
      float a2 = sqdiff(qs[2], Y(2)) + sqdiff(qs[6], Y(6));
      float a3 = sqdiff(qs[3], Y(3)) + sqdiff(qs[7], Y(7));
      r = (a0 + a1) + (a2 + a3);
    } else if (L == 12) {
      float a0 = (sqdiff(qs[0], Y(0)) + sqdiff(qs[4], Y(4))) + sqdiff(qs[8], Y(8));
      float a1 = (sqdiff(qs[1], Y(1)) + sqdiff(qs[5], Y(5))) + sqdiff(qs[9], Y(9));
      float a2 = (sqdiff(qs[2], Y(2)) + sqdiff(qs[6], Y(6))) + sqdiff(qs[10], Y(10));
      float a3 = (sqdiff(qs[3], Y(3)) + sqdiff(qs[7], Y(7))) + sqdiff(qs[11], Y(11));
      r = (a0 + a1) + (a2 + a3);
    } else {
      float res = 0.0f;
      for (int j = 0; j < L; j++) {
        float t = qs[j] - Y(j);
        res += t * t;
      }
      r = res;
    }
    out[c] = r;
  }
#undef Y
}

// The same for codebooks of >= 8 centroids (VAQ.hpp:134-159), LUT_QT queries per workgroup: a
// thread owns one centroid and reads each of its coordinates ONCE for the whole batch of queries
// (the per-query kernel above spends its time launching 80 000 workgroups of 16 FMAs a thread
// at C2).  Per (query, centroid) the chain is unchanged: acc = fma(diff, diff, acc), j ascending.
// With `keys` (the ranking of the queries by cost, further down) the workgroups of subspace 0 also make each of
// their queries' cost key, from the entries they have just computed: a table 0 of up to
// COST_KEY_LDS_ENTRIES entries goes to the key through LDS, a larger one (whose key samples a part of it) is read
// back by the workgroup that wrote it.  One wave per query, the key of query_cost_kernel bit for bit.
constexpr int LUT_QT = 8;
constexpr int COST_KEY_LDS_ENTRIES = 256;
template <int NREG>
__device__ __forceinline__ unsigned cost_key_bits(const float *l, int n0, int shift, int lane);
__device__ __forceinline__ void cost_key_emit(unsigned kb, int q, unsigned long long *__restrict__ keys);

__global__ __launch_bounds__(256) void lut_build_batch_kernel(const float *__restrict__ qproj, int nq, int D, int L,
                                                              const SubDesc *__restrict__ sub,
                                                              const float *__restrict__ cent_t, int lut_floats,
                                                              float *__restrict__ lut,
                                                              unsigned long long *__restrict__ keys, int shift) {
  extern __shared__ float qs[];  // [LUT_QT][L]; with keys, for a small table 0: then [LUT_QT][K]
  const int q0 = blockIdx.x * LUT_QT, s = blockIdx.y;
  const SubDesc sd = sub[s];
  const int K = sd.ncent;
  if (K < 8) return;  // (those subspaces are the per-query kernel's)
  for (int i = threadIdx.x; i < LUT_QT * L; i += blockDim.x) {
    const int qt = i / L, j = i - qt * L;
    qs[i] = q0 + qt < nq ? qproj[(size_t)(q0 + qt) * D + (size_t)s * L + j] : 0.0f;
  }
  __syncthreads();
  const bool rank = keys != nullptr && s == 0;
  const bool rank_lds = rank && K <= COST_KEY_LDS_ENTRIES;
  float *t0 = qs + LUT_QT * L;
  const float *cs = cent_t + sd.cent_off;
  for (int c = threadIdx.x; c < K; c += blockDim.x) {
    float acc[LUT_QT];
#pragma unroll
    for (int qt = 0; qt < LUT_QT; qt++) acc[qt] = 0.0f;
    for (int j = 0; j < L; j++) {
      const float y = cs[(size_t)j * K + c];
#pragma unroll
      for (int qt = 0; qt < LUT_QT; qt++) {
        const float diff = qs[qt * L + j] - y;
        acc[qt] = __builtin_fmaf(diff, diff, acc[qt]);
      }
    }
#pragma unroll
    for (int qt = 0; qt < LUT_QT; qt++) {
      if (q0 + qt < nq) lut[(size_t)(q0 + qt) * lut_floats + sd.lut_off + c] = acc[qt];
      if (rank_lds) t0[qt * K + c] = acc[qt];
    }
  }
  if (!rank) return;
  __threadfence_block();  // (the read-back form: this workgroup's stores before its own loads)
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int qt = threadIdx.x >> 6; qt < LUT_QT && q0 + qt < nq; qt += blockDim.x >> 6) {
    const int q = q0 + qt;
    const unsigned kb = rank_lds ? cost_key_bits<4>(t0 + qt * K, K, shift, lane)
                                 : cost_key_bits<4>(lut + (size_t)q * lut_floats + sd.lut_off, K, shift, lane);
    if (lane == 0) cost_key_emit(kb, q, keys);
  }
}

static bool cost_order_shape_ok(int nq, int n0, int shift);  // (with the ranking, further down)

hipError_t launch_lut_build(const float *qproj, int nq, int D, int M, int L, const SubDesc *sub,
                            const float *cent_t, int lut_floats, int max_ncent, float *lut,
                            hipStream_t st, int min_ncent, const CostKeys *ck) {
  if (nq == 0) return hipSuccess;
  (void)max_ncent;
  // (keys come from the batched kernel's subspace-0 workgroups alone: the caller asks only where those run)
  if (ck && !(nq >= 2 * LUT_QT && ck->n0 >= 8 && cost_order_shape_ok(nq, ck->n0, ck->shift))) return hipErrorInvalidValue;
  if (nq >= 2 * LUT_QT && max_ncent >= 8) {
    size_t lds = LUT_QT * L * sizeof(float);
    if (ck && ck->n0 <= COST_KEY_LDS_ENTRIES) lds += (size_t)LUT_QT * ck->n0 * sizeof(float);
    hipLaunchKernelGGL(lut_build_batch_kernel, dim3((nq + LUT_QT - 1) / LUT_QT, M), dim3(256), lds, st, qproj, nq, D, L,
                       sub, cent_t, lut_floats, lut, ck ? ck->keys : nullptr, ck ? ck->shift : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || min_ncent >= 8) return e;
    // codebooks of fewer than 8 centroids (the reference's scalar branch) go through the per-query kernel
    hipLaunchKernelGGL(lut_build_kernel, dim3(nq, M, 1), dim3(64), L * sizeof(float), st, qproj, D, L, sub, cent_t,
                       lut_floats, lut, 1);
    return hipGetLastError();
  }
  // one workgroup per (query, subspace): splitting big codebooks over blockIdx.z was measured
  // slower (the extra, mostly empty workgroups cost more than the 16-iteration loop they save)
  hipLaunchKernelGGL(lut_build_kernel, dim3(nq, M, 1), dim3(256), L * sizeof(float), st, qproj, D, L,
                     sub, cent_t, lut_floats, lut, 0);
  return hipGetLastError();
}

// packed LUT -> the reference's LUTType (ksub x M column-major, zero tails; VAQ.cpp:780,
// VAQ.hpp:130).  Test hook only.
__global__ void lut_expand_kernel(const float *__restrict__ lp, int M,
                                  const SubDesc *__restrict__ sub, int lut_floats, int ksub,
                                  float *__restrict__ lr) {
  const int q = blockIdx.x, s = blockIdx.y;
  const SubDesc sd = sub[s];
  for (int c = threadIdx.x; c < ksub; c += blockDim.x)
    lr[((size_t)q * M + s) * ksub + c] =
        c < sd.ncent ? lp[(size_t)q * lut_floats + sd.lut_off + c] : 0.0f;
}

hipError_t launch_lut_expand(const float *lut_packed, int nq, int M, const SubDesc *sub,
                             int lut_floats, int ksub, float *lut_ref, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(lut_expand_kernel, dim3(nq, M), dim3(256), 0, st, lut_packed, M, sub,
                     lut_floats, ksub, lut_ref);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Best-first order of the row slices of a multi-slice scan, one list per query
// batch: slices are ranked by the smallest first LUT term (or its per-bucket
// lower bound) that any query of the batch sees in any bucket the slice touches.
// Workgroups are dispatched in blockIdx order, so with this table the first
// ones scan the most promising rows, publish tight thresholds, and the rest
// skip their buckets unread -- it replaces the sampling pre-pass.
// grid = query batches; n_slices <= SLICE_ORDER_MAX (packed-key sort in LDS).
// ---------------------------------------------------------------------------
constexpr int SLICE_ORDER_MAX = 4096;

__global__ __launch_bounds__(256) void slice_order_kernel(
    const float *__restrict__ lut, int lut_floats, int nq, int qb, const int *__restrict__ bstart,
    int n_buckets, int bucket_shift, int64_t slice_rows, int n_slices, int64_t n_rows,
    int *__restrict__ order) {
  __shared__ unsigned key[SLICE_ORDER_MAX];
  __shared__ float lbk[HOT_MAX_BUCKETS];
  const int batch = blockIdx.x, tid = threadIdx.x;
  // per-bucket bound over the batch's queries
  for (int b = tid; b < n_buckets; b += 256) {
    float m = INFINITY;
    for (int q = 0; q < qb; q++) {
      int x = batch * qb + q;
      if (x >= nq) x = nq - 1;
      for (int c = b << bucket_shift; c < ((b + 1) << bucket_shift); c++) {
        const float v = lut[(size_t)x * lut_floats + c];
        m = v < m ? v : m;
      }
    }
    lbk[b] = m;
  }
  __syncthreads();
  int P = 2;
  while (P < n_slices) P <<= 1;
  const unsigned idx_mask = (unsigned)P - 1u;
  for (int s = tid; s < P; s += 256) {
    unsigned k = 0xffffffffu;
    if (s < n_slices) {
      const int64_t r0 = (int64_t)s * slice_rows;
      int64_t r1 = r0 + slice_rows;
      if (r1 > n_rows) r1 = n_rows;
      int lo = 0, hi = n_buckets;  // bucket of r0
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bstart[mid] <= r0) lo = mid; else hi = mid;
      }
      float m = INFINITY;
      for (int b = lo; b < n_buckets && bstart[b] < r1; b++)
        if (bstart[b + 1] > r0 && lbk[b] < m) m = lbk[b];
      k = m == m ? ((__builtin_bit_cast(unsigned, m) & ~idx_mask) | (unsigned)s) : (0xffffffffu & ~idx_mask) | (unsigned)s;
    }
    key[s] = k;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += 256) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const unsigned a = key[i], c = key[j];
        if ((a > c) == ((i & size) == 0)) { key[i] = c; key[j] = a; }
      }
      __syncthreads();
    }
  // padding keys (0xffffffff) sort last; real ones carry their slice index in the low bits
  for (int r = tid; r < n_slices; r += 256) order[(size_t)batch * n_slices + r] = (int)(key[r] & idx_mask);
}

hipError_t launch_slice_order(const float *lut, int lut_floats, int nq, int qb, const int *bstart,
                              int n_buckets, int bucket_shift, int64_t slice_rows, int n_slices,
                              int64_t n_rows, int *order, hipStream_t st) {
  if (n_slices > SLICE_ORDER_MAX || n_buckets > HOT_MAX_BUCKETS) return hipErrorInvalidValue;
  const int nqb = (nq + qb - 1) / qb;
  if (nqb == 0) return hipSuccess;
  hipLaunchKernelGGL(slice_order_kernel, dim3(nqb), dim3(256), 0, st, lut, lut_floats, nq, qb, bstart,
                     n_buckets, bucket_shift, slice_rows, n_slices, n_rows, order);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------
// Query grouping for multi-query passes over a streamed database.  A pass of Qb queries skips a
// bucket only when EVERY query of the pass can skip it, so a pass costs the UNION of its queries'
// buckets.  Queries whose nearest first and second codes agree have nearly the same buckets in
// reach: ordering the queries by (nearest first code, nearest second code) before cutting them
// into passes shrinks that union (125M x 16 B, 1024 queries, Qb = 4: 35.5 -> 28.0 ms).  Results
// are written to the queries' own slots, so the caller sees no difference.
// query_order_kernel: one workgroup; keys = (argmin of LUT table 0) << 16 | (argmin of table 1),
// then a bitonic sort of key << 32 | query in LDS (nq <= 16384: 128 KB); order[i] = i-th query.
// ---------------------------------------------------------------------------
constexpr int QORDER_THREADS = 1024;
constexpr int QORDER_MAX = 16384;
__global__ __launch_bounds__(QORDER_THREADS) void query_order_kernel(const float *__restrict__ lut, int lut_floats, int nq,
                                                                     int n0, int off1, int n1, int *__restrict__ order) {
  extern __shared__ unsigned long long qk[];  // [P], P = power of two >= nq
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = QORDER_THREADS / 64;
  int P = 2;
  while (P < nq) P <<= 1;
  for (int q = wave; q < P; q += nwaves) {
    unsigned long long key = ~0ull;
    if (q < nq) {
      const float *l = lut + (size_t)q * lut_floats;
      unsigned a[2];
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const int off = t == 0 ? 0 : off1, n = t == 0 ? n0 : n1;
        // packed (value bits, index): entries are >= 0, so bit order == value order; NaN sorts last
        unsigned long long best = ~0ull;
        for (int e = lane; e < n; e += 64) {
          const float x = l[off + e];
          const unsigned long long c = ((unsigned long long)(x == x ? float_to_bits(x) : 0xffffffffu) << 32) | (unsigned)e;
          best = c < best ? c : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long x = __shfl_xor(best, o);
          best = x < best ? x : best;
        }
        a[t] = (unsigned)(best & 0xffffu);
      }
      key = ((unsigned long long)((a[0] << 16) | a[1]) << 32) | (unsigned)q;
    }
    if (lane == 0) qk[q] = key;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += QORDER_THREADS) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const unsigned long long x = qk[i], y = qk[j];
        if ((x > y) == ((i & size) == 0)) { qk[i] = y; qk[j] = x; }
      }
      __syncthreads();
    }
  for (int i = tid; i < nq; i += QORDER_THREADS) order[i] = (int)(qk[i] & 0xffffffffu);
}

hipError_t launch_query_order(const float *lut, int lut_floats, int nq, int n0, int off1, int n1, int *order,
                              hipStream_t st) {
  if (nq <= 0 || nq > QORDER_MAX) return hipErrorInvalidValue;
  int P = 2;
  while (P < nq) P <<= 1;
  const size_t lds = (size_t)P * sizeof(unsigned long long);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(query_order_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(query_order_kernel, dim3(1), dim3(QORDER_THREADS), lds, st, lut, lut_floats, nq, n0, off1, n1, order);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Dispatch order of the best-first form with one workgroup per query: expensive queries first.
// A query's cost spans 6x (C2: 318 wave steps on average, 1857 for the top 1 %) and a launch ends
// with its most expensive workgroups; started first they end inside the bulk (C2 scan 0.75 -> 0.55 ms
// with this predictor, 0.50 with the exact costs: tools/exp_cost_predictor.py).  What makes a
// query expensive is the number of buckets in its reach, i.e. how FLAT its first lookup table is
// near the minimum: cost key = (sum of the 16 smallest - 16 x the smallest) of the per-bucket minima of
// table 0 (of 256 of them, sampled, when there are more),
// ascending (Spearman 0.72 with a workgroup's lifetime, 0.83 with its steps).
//   cost_key_bits        one wave per query -> key bits; cost_key_emit: keys[q] = key bits << 32 | query.  Run where
//                        table 0 is made (lut_build_batch_kernel) or, over tables that are there already, by
//                        query_cost_kernel
//   cost_scatter_kernel  counting sort by the key's top bits -> order[b] = query of block b
// Block b serves order[b]: blocks are dealt round-robin over the XCDs and dispatched in order, so
// every XCD gets every 8th query of the ranking.  Speed only: any order is correct.
// ---------------------------------------------------------------------------
// `l`: the query's table 0 (n0 entries), in LDS or in global memory; all 64 lanes of the wave call it
template <int NREG>  // per-bucket minima a lane holds: buckets at the level of the first code <= 64 NREG
__device__ __forceinline__ unsigned cost_key_bits(const float *l, int n0, int shift, int lane) {
  // (more than 256 buckets at the level of the first code: every stride-th one is sampled -- the
  //  statistic is a ranking aid, and reading a 4096-entry table per query costs more than it saves)
  const int nb_all = n0 >> shift;
  const int stride = nb_all > 64 * NREG ? nb_all / (64 * NREG) : 1;
  const int nb = nb_all / stride;
  unsigned v[NREG];
  unsigned vmin = 0xffffffffu, vmax = 0u;
#pragma unroll
  for (int i = 0; i < NREG; i++) {
    const int b = i * 64 + lane;
    unsigned m = 0xffffffffu;  // (absent or NaN: never counted)
    if (b < nb) {
      // (sampled in runs of one 64-byte line of the table, so that the unsampled lines are never read)
      const int g = (16 >> shift) > 0 ? (16 >> shift) : 1;
      const int bb = (b / g) * g * stride + (b % g);
      for (int c = bb << shift; c < ((bb + 1) << shift); c++) {
        const float x = l[c];
        const unsigned xb = x == x ? float_to_bits(x) : 0xffffffffu;  // entries are >= 0: bit order == value order
        m = xb < m ? xb : m;
      }
    }
    v[i] = m;
    vmin = m < vmin ? m : vmin;
    vmax = (m != 0xffffffffu && m > vmax) ? m : vmax;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned x = (unsigned)__shfl_xor((int)vmin, o), y = (unsigned)__shfl_xor((int)vmax, o);
    vmin = x < vmin ? x : vmin;
    vmax = y > vmax ? y : vmax;
  }
  int J = 16 / stride;
  J = J < 2 ? 2 : J;
  J = nb < J ? nb : J;
  unsigned lo = vmin, hi = vmax;  // smallest t with count(v <= t) >= J (vmax: all of them, unless NaNs leave fewer)
  if (lo > hi) lo = hi;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    int c = 0;
#pragma unroll
    for (int i = 0; i < NREG; i++) c += __popcll(__ballot(v[i] <= mid));
    if (c >= J) hi = mid;
    else lo = mid + 1u;
  }
  // key = sum of the J smallest minima - J x the smallest: how flat the table is near its minimum
  // (tools/exp_cost_predictor.py: the batch in this order 0.532 ms, by the J-th smallest alone 0.556)
  float part = 0.0f;
  int below = 0;
#pragma unroll
  for (int i = 0; i < NREG; i++) {
    const bool lt = v[i] < lo;
    part += lt ? bits_to_float(v[i]) : 0.0f;
    below += __popcll(__ballot(lt));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  const float v0 = bits_to_float(vmin < 0x7f800000u ? vmin : 0x7f800000u);
  const float spread = (part + (float)(J - below) * bits_to_float(lo)) - (float)J * v0;
  return (spread == spread && spread >= 0.0f) ? float_to_bits(spread) : (spread < 0.0f ? 0u : 0x7f800000u);  // (inf - inf: last)
}

// The queries are sorted by the top 12 value bits of their cost key (sign 0, exponent, 4 mantissa bits: 6 % steps
// -- the ranking only has to put expensive queries ahead of cheap ones), a counting sort over COST_CLASSES classes.
constexpr int COST_CLASSES = 4096;

__device__ __forceinline__ unsigned cost_class(unsigned long long key) { return (unsigned)(key >> 51) & (COST_CLASSES - 1); }

__device__ __forceinline__ void cost_key_emit(unsigned kb, int q, unsigned long long *__restrict__ keys) {
  keys[q] = ((unsigned long long)kb << 32) | (unsigned)q;
}

// over tables that are already there (no table build in front, or a table 0 the batched build does not make)
template <int NREG>
__global__ __launch_bounds__(256) void query_cost_kernel(const float *__restrict__ lut, int lut_floats, int nq, int n0,
                                                         int shift, unsigned long long *__restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const unsigned kb = cost_key_bits<NREG>(lut + (size_t)q * lut_floats, n0, shift, lane);
  if (lane == 0) cost_key_emit(kb, q, keys);
}

// QORDER_THREADS queries per workgroup, and no word shared between the workgroups: each counts ALL the keys for
// itself in LDS (nq x 8 bytes out of L2) -- per class the queries there are (low half of the word) and those of
// them that belong to earlier workgroups (high half; nq <= QORDER_MAX keeps both inside 16 bits) --, takes the
// exclusive prefix over the classes, and places its own queries from where the earlier workgroups' end.  Inside a
// class the queries stand in the order of their workgroups, inside a workgroup in the order of its LDS atomics.
// (Counting the classes in global memory while the keys are made, and handing places out with returning global
//  atomics, was measured: the 10 k same-word atomics of a C2 batch add 69 us to the kernel that makes the keys and
//  take 23 us in the scatter.)
static_assert(QORDER_MAX < (1 << 16), "a class's two counts share one word");
__global__ __launch_bounds__(QORDER_THREADS) void cost_scatter_kernel(const unsigned long long *__restrict__ keys, int nq,
                                                                      int *__restrict__ order) {
  __shared__ unsigned cnt[COST_CLASSES];
  __shared__ unsigned wave_tot[QORDER_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mine0 = blockIdx.x * QORDER_THREADS;  // this workgroup's first query
  for (int i = tid; i < COST_CLASSES; i += QORDER_THREADS) cnt[i] = 0u;
  __syncthreads();
  for (int i = tid; i < nq; i += QORDER_THREADS) atomicAdd(&cnt[cost_class(keys[i])], i < mine0 ? 0x10001u : 1u);
  __syncthreads();
  // exclusive prefix over the classes: 4 per thread, then a wave scan, then the waves' totals
  constexpr int PER = COST_CLASSES / QORDER_THREADS;
  unsigned c[PER], sum = 0u;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    c[j] = cnt[tid * PER + j];
    sum += c[j] & 0xffffu;
  }
  unsigned inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = (unsigned)__shfl_up((int)inc, o);
    if (lane >= o) inc += x;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  unsigned base = inc - sum;
  for (int w = 0; w < wave; w++) base += wave_tot[w];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    cnt[tid * PER + j] = base + (c[j] >> 16);  // the class's first place, then the earlier workgroups' queries
    base += c[j] & 0xffffu;
  }
  __syncthreads();
  const int i = mine0 + tid;
  if (i >= nq) return;
  const unsigned long long kq = keys[i];
  const unsigned pos = atomicAdd(&cnt[cost_class(kq)], 1u);
  if (pos < (unsigned)nq) order[pos] = (int)(kq & 0xffffffffu);  // (always: the counts are these keys')
}

static bool cost_order_shape_ok(int nq, int n0, int shift) {
  return nq > 0 && nq <= QORDER_MAX && (n0 >> shift) <= 1024 && (n0 >> shift) >= 1;
}

hipError_t launch_cost_scatter(const unsigned long long *keys, int nq, int *order, hipStream_t st) {
  if (nq <= 0 || nq > QORDER_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cost_scatter_kernel, dim3((nq + QORDER_THREADS - 1) / QORDER_THREADS), dim3(QORDER_THREADS), 0, st,
                     keys, nq, order);
  return hipGetLastError();
}

hipError_t launch_cost_order(const float *lut, int lut_floats, int nq, int n0, int shift, unsigned long long *keys,
                             int *order, hipStream_t st) {
  if (!cost_order_shape_ok(nq, n0, shift)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(query_cost_kernel<4>, dim3((nq + 3) / 4), dim3(256), 0, st, lut, lut_floats, nq, n0, shift, keys);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_cost_scatter(keys, nq, order, st);
}

} // namespace vaq
