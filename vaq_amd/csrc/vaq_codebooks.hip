// vaq_codebooks.hip -- the subspace codebooks mCentroidsPerSubs on gfx950: KMeans::staticFitSampling (KMeans.hpp:487-616)
// as VAQ.cpp:644-649 calls it, once per subspace on XTrain.block(0, s * L, n, L), for ALL subspaces in one launch per
// phase and iteration.  The arithmetic is vaq_kmeans.hip's (the same reference function), statement for statement:
//   assign      sqrt((x - mean).squaredNorm()) in Eigen's summation order over the L floats of the slice
//               (sq_norm_eigen, vaq_restated.h), centres ascending, strict `<`
//   accumulate  per (half, centre, column) a float sum from +0 in ascending row order: a stable sort of the rows by
//               run_off[s] + half * k_s + centre and one thread per (run, column) walking its run
//   update      new = ((0 + p0) + p1) / float(count); a centre whose new row is not elementwise == the old one is
//               replaced (an empty cluster: 0 / 0 = NaN, unequal for ever)
// Every call of the reference samples for itself (KMeans.hpp:489-503): subspace s works on all n rows in their own
// order when n <= max(256 k_s, 65536), else on the first max(256 k_s, 65536) rows of randomPermutation(n).  So a batch
// has up to two sources, and cbfit::Sub::full says which one a subspace reads: the full matrix (all rows projected, or
// widened, whole), or the gathered sample (the head of the permutation as long as the largest sampling subspace needs;
// a smaller one takes a prefix).  A row's projection does not depend on other rows, so where both are needed the
// sample is gathered from the projected full matrix.
// Batching cannot change a bit: no value of subspace s is computed from another subspace's -- the slices are
// disjoint columns of the subspace's source, the keys of s lie in its own range [run_off, run_off + 2 k_s), its pairs
// enter the sort in ascending row order and the sort is stable, so every run is the run the single fit would walk.
// A subspace whose centres stopped changing is a fixed point: its assign step is skipped (its pairs are still there
// from the iteration before), the rest recomputes the same centres.
// The kernels address a fit through cbfit::Fit (source matrix, row stride, column, first row), so the same phases run
// the hierarchical form's batches (codebooks_fit_hier below): 128-centre fits beside the flat subspaces, then the
// K2-centre fits of all groups over a compact regrouped matrix, the assign kernel walking a table of row tiles.
// No float atomics, no MFMA, no reassociation; compiled with -ffp-contract=off like every file of the library.
#include "fit_codebooks_bin_plan.h"
#include "fit_codebooks_hier_plan.h"
#include "kmeans_sample.h"
#include "vaq_codebooks.h"
#include "vaq_front.h"
#include "vaq_refine.h"
#include "vaq_restated.h"
#include "vaqhip_dev.h"

#include <chrono>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>

#include <float.h>
#include <math.h>

namespace vaq {

namespace {
// floats of centres a workgroup of the assign kernel stages in LDS at a time
constexpr int CB_STAGE_FLOATS = 4096;
// (the LDS its tile of slices may take, and with it the rows per workgroup: cbfit::assign_tile_rows)
}  // namespace

// out[i][j] = (float)X[rows[i]][j]: the sample in the reference's order, a byte widened where it is loaded
template <typename T>
__global__ void cb_gather_kernel(const T *__restrict__ X, int D, const int *__restrict__ rows, int64_t S,
                                 float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * D) return;
  const int64_t r = i / D;
  out[i] = (float)X[(int64_t)rows[r] * D + (i - r * D)];
}

// the source matrices of a batch (cbfit::Fit::src indexes them; unused ones are null)
struct CbSources {
  const float *p[cbfit::N_SOURCES];
};
// the first float of a fit's slice of its row 0
__device__ __forceinline__ const float *cb_fit_base(const CbSources &src, const cbfit::Fit &f) {
  return src.p[f.src] + (size_t)f.row0 * f.stride + f.col;
}

// out[i][j] = src[rows[i] (or i, rows null)][col + j], i < cnt, j < L: a column slice, gathered compactly
__global__ void cb_slice_kernel(const float *__restrict__ src, int stride, int col, const int *__restrict__ rows, int64_t cnt,
                                int L, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt * L) return;
  const int64_t r = i / L;
  out[i] = src[(size_t)(rows ? rows[r] : r) * stride + col + (i - r * L)];
}

// means[c] = the slice of row seed_rows[c] of the fit's rows (KMeans.hpp:516-520); grid.y = fit
__global__ void cb_seed_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits, const int *__restrict__ seed_rows,
                               float *__restrict__ means) {
  const cbfit::Fit fd = fits[blockIdx.y];
  const float *P = cb_fit_base(src, fd);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fd.k * L) return;
  const int c = i / L, j = i % L;
  means[(size_t)(fd.cent_off + c) * L + j] = P[(size_t)seed_rows[fd.cent_off + c] * fd.stride + j];
}

// One row per thread.  Which rows a workgroup takes: with `tiles`, rows [row0, row0 + blockDim.x) of fit tiles[blockIdx.x]
// (fits of very different sizes: no workgroup is launched to find itself past its fit's end); without, grid = (row
// tile, fit).  X_LDS: the workgroup's slices sit in LDS as [column][row] (each thread reads its own column,
// conflict-free); else every thread reads its slice from global memory.  The fit's centres pass through LDS `stage` at
// a time and are read with wave-uniform addresses (broadcast).
// Lloyd (MEMBER false): the distance is sqrt(squaredNorm), row r of fit f: keys[pair_off + r] = run_off + half * k +
// centre, vals[pair_off + r] = r.  MEMBER: the hierarchical fit's split of R_s by nearest stage-1 centre
// (getBelongsToCluster, VAQ.cpp:1272-1292): the squaredNorm itself is compared, NO sqrt -- two distinct squares whose
// roots round to one float choose differently --, and the key is run_off + centre.
template <bool X_LDS, bool MEMBER>
__global__ void cb_assign_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits, const cbfit::Tile *__restrict__ tiles,
                                 const float *__restrict__ means, int stage, const int *__restrict__ active,
                                 unsigned *__restrict__ keys, unsigned *__restrict__ vals, int *__restrict__ no_centre) {
  extern __shared__ float cb_lds[];
  const int R = blockDim.x, tid = threadIdx.x;
  const int f = tiles ? tiles[blockIdx.x].fit : (int)blockIdx.y;
  const int64_t r0 = tiles ? (int64_t)tiles[blockIdx.x].row0 : (int64_t)blockIdx.x * R;
  const cbfit::Fit fd = fits[f];
  if (r0 >= fd.rows || (active && !active[f])) return;  // (the whole workgroup)
  float *cs = cb_lds;                        // [stage][L]
  float *xt = cb_lds + (size_t)stage * L;    // [L][R]
  const int64_t r = r0 + tid;
  const int64_t rr = r < fd.rows ? r : fd.rows - 1;  // (rows past the end work on the last row and store nothing)
  const float *slice0 = cb_fit_base(src, fd);
  const int D = fd.stride;
  if (X_LDS) {
    for (int i = tid; i < R * L; i += R) {
      const int row = i / L, col = i % L;
      xt[(size_t)col * R + row] = r0 + row < fd.rows ? slice0[(size_t)(r0 + row) * D + col] : 0.0f;
    }
  }
  const float *m = means + (size_t)fd.cent_off * L;
  float best = FLT_MAX;
  int idx = -1;
  for (int c0 = 0; c0 < fd.k; c0 += stage) {
    const int cn = min(stage, fd.k - c0);
    __syncthreads();  // the last stage is read, the tile is written
    for (int i = tid; i < cn * L; i += R) cs[i] = m[(size_t)c0 * L + i];
    __syncthreads();
    for (int c = 0; c < cn; c++) {
      const float d2 = X_LDS ? sq_norm_eigen<false>(xt + tid, R, cs + (size_t)c * L, L)
                             : sq_norm_eigen<true>(slice0 + (size_t)rr * D, 1, cs + (size_t)c * L, L);
      const float dist = MEMBER ? d2 : sqrtf(d2);
      if (dist < best) {
        best = dist;
        idx = c0 + c;
      }
    }
  }
  if (r < fd.rows) {
    if (idx < 0) no_centre[f] = 1;  // the reference indexes row -1 here
    keys[fd.pair_off + r] = (unsigned)(fd.run_off + (!MEMBER && r >= fd.half ? fd.k : 0) + max(idx, 0));
    vals[fd.pair_off + r] = (unsigned)r;
  }
}

// run [start, end) of every key in the sorted keys (both preset to 0: keys that do not occur are empty)
__global__ void cb_bounds_kernel(const unsigned *__restrict__ keys, int n, int *__restrict__ start,
                                 int *__restrict__ end) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i];
  if (i == 0 || keys[i - 1] != k) start[k] = i;
  if (i == n - 1 || keys[i + 1] != k) end[k] = i + 1;
}

// part[run * L + col] = the rows of that run added from +0 in ascending row order; grid.y = fit, neighbouring
// threads take neighbouring columns of the same run
__global__ void cb_accumulate_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits,
                                     const unsigned *__restrict__ rows_sorted, const int *__restrict__ start,
                                     const int *__restrict__ end, float *__restrict__ part) {
  const cbfit::Fit fd = fits[blockIdx.y];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * fd.k * L) return;
  const int g = fd.run_off + t / L, col = t % L;
  const float *x = cb_fit_base(src, fd) + col;
  float sum = 0.0f;
  for (int i = start[g], e = end[g]; i < e; i++) sum += x[(size_t)rows_sorted[i] * fd.stride];
  part[(size_t)g * L + col] = sum;
}

// cb_accumulate_kernel's sums for long runs (the binary fit's batches: two centres make a run a quarter of a node): one
// wavefront per run, grid = (run of the fit, fit).  The wavefront stages a tile of the run's rows through LDS -- first the
// row numbers, then the slices, 64 loads in flight per instruction and none of them on the add chain -- and lane c
// adds column c of the staged rows in ascending order, the sum carried in a register from tile to tile.  Per (run,
// column) that is cb_accumulate_kernel's chain exactly: from +0.0f, one row after the other, nothing reassociated.
// The tile is [row][column] for CB_SUMS_COLS columns at a time: the adding lanes read neighbouring words (no bank
// conflict), the staging lanes write neighbouring words.  An empty run writes +0.
constexpr int CB_SUMS_COLS = 64, CB_SUMS_TILE_FLOATS = 4096, CB_SUMS_MAX_ROWS = 256;

__global__ __launch_bounds__(64) void cb_sums_staged_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits,
                                                           const unsigned *__restrict__ rows_sorted,
                                                           const int *__restrict__ start, const int *__restrict__ end,
                                                           float *__restrict__ part) {
  __shared__ float tile[CB_SUMS_TILE_FLOATS];
  __shared__ unsigned tile_row[CB_SUMS_MAX_ROWS];
  const cbfit::Fit fd = fits[blockIdx.y];
  if ((int)blockIdx.x >= 2 * fd.k) return;  // (the whole wavefront)
  const int g = fd.run_off + (int)blockIdx.x, lane = threadIdx.x;
  const int s = start[g], e = end[g];
  const float *x = cb_fit_base(src, fd);
  for (int c0 = 0; c0 < L; c0 += CB_SUMS_COLS) {
    const int cw = min(CB_SUMS_COLS, L - c0);
    const int T = min(CB_SUMS_MAX_ROWS, CB_SUMS_TILE_FLOATS / cw);
    float sum = 0.0f;
    for (int t0 = s; t0 < e; t0 += T) {
      const int tn = min(T, e - t0);
      __syncthreads();  // (the tile before has been added)
      for (int i = lane; i < tn; i += 64) tile_row[i] = rows_sorted[t0 + i];
      __syncthreads();
      for (int i = lane; i < tn * cw; i += 64) {
        const int r = i / cw;
        tile[i] = x[(size_t)tile_row[r] * fd.stride + c0 + (i - r * cw)];
      }
      __syncthreads();
      if (lane < cw)
        for (int r = 0; r < tn; r++) sum += tile[r * cw + lane];
    }
    if (lane < cw) part[(size_t)g * L + c0 + lane] = sum;
  }
}

// The binary fit's split of a node's rows between its two centres (getBelongsToBinaryCluster, VAQ.cpp:1293-1310): one
// row per thread, rows [row0, row0 + blockDim.x) of fit tiles[blockIdx.x].fit, the two centres in LDS (every lane reads
// the same word: a broadcast).  left = (x - C0).squaredNorm(), right = (x - C1).squaredNorm() in Eigen's order, no
// sqrt; the row goes left iff left < right -- a tie and a NaN on either side go right, and there is no row without a
// centre.  keys[pair_off + r] = run_off + side, vals[pair_off + r] = r.
__global__ void cb_split_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits, const cbfit::Tile *__restrict__ tiles,
                                const float *__restrict__ means, unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
  extern __shared__ float cb_lds[];  // [2][L]
  const cbfit::Tile t = tiles[blockIdx.x];
  const cbfit::Fit fd = fits[t.fit];
  for (int i = threadIdx.x; i < 2 * L; i += blockDim.x) cb_lds[i] = means[(size_t)fd.cent_off * L + i];
  __syncthreads();
  const int64_t r = (int64_t)t.row0 + threadIdx.x;
  if (r >= fd.rows) return;
  const float *x = cb_fit_base(src, fd) + (size_t)r * fd.stride;
  const float left = sq_norm_eigen<true>(x, 1, cb_lds, L);
  const float right = sq_norm_eigen<true>(x, 1, cb_lds + L, L);
  keys[fd.pair_off + r] = (unsigned)(fd.run_off + (left < right ? 0 : 1));
  vals[fd.pair_off + r] = (unsigned)r;
}

// The regroup behind the split: sorted pair p belongs to fit keys_sorted[p] / 2 and is row rows_sorted[p] of it; where
// that node has children (dest >= 0) its slice becomes row dest + (p - pair_off) of the next level's compact matrix.
__global__ void cb_regroup_kernel(CbSources src, int L, const cbfit::Fit *__restrict__ fits, const int64_t *__restrict__ dest,
                                  const unsigned *__restrict__ keys_sorted, const unsigned *__restrict__ rows_sorted,
                                  int64_t n_pairs, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs * L) return;
  const int64_t p = i / L;
  const int f = (int)(keys_sorted[p] >> 1);
  const int64_t d = dest[f];
  if (d < 0) return;
  const cbfit::Fit fd = fits[f];
  out[(size_t)(d + (p - fd.pair_off)) * L + (i - p * L)] = cb_fit_base(src, fd)[(size_t)rows_sorted[p] * fd.stride + (i - p * L)];
}

// one wavefront per (centre, fit) (KMeans.hpp:586-604); changed[f] is set when a centre of fit f was replaced
__global__ __launch_bounds__(64) void cb_update_kernel(const float *__restrict__ part, const int *__restrict__ start,
                                                      const int *__restrict__ end, int L,
                                                      const cbfit::Fit *__restrict__ fits, float *__restrict__ means,
                                                      int *__restrict__ changed) {
  const int f = blockIdx.y;
  const cbfit::Fit fd = fits[f];
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c >= fd.k) return;
  const int g0 = fd.run_off + c, g1 = g0 + fd.k;
  const int count = (end[g0] - start[g0]) + (end[g1] - start[g1]);
  const float *p0 = part + (size_t)g0 * L, *p1 = part + (size_t)g1 * L;
  float *m = means + (size_t)(fd.cent_off + c) * L;
  bool differs = false;
  for (int j = lane; j < L; j += 64) {
    const float v = ((0.0f + p0[j]) + p1[j]) / (float)count;
    if (!(v == m[j])) differs = true;
  }
  if (!__any(differs)) return;
  for (int j = lane; j < L; j += 64) m[j] = ((0.0f + p0[j]) + p1[j]) / (float)count;
  if (lane == 0) changed[f] = 1;
}

// ---- the sharded fit's shard step (vaqhip_multi_codebooks.cpp, DESIGN.md section 4f "Across shards") ----
// out[i][c], i < cnt, c < D_w: compact column c of ONE owner (column subs[c / L] * L + c % L of the rows) for the i-th
// row a shard contributes -- local row rows[i], or first + i where rows is null.  Without E the value is the row's
// own, a byte widened where it is loaded.  With E it is ONE fmaf chain over the row's D inputs ascending from
// acc = 0.0f: project_kernel's value bit for bit (vaq_front.hip), computed for the owner's columns only.
// A workgroup is tc column threads by tr = 256 / tc row groups (tc: the power of two from 16 to 256 that covers D_w,
// blockIdx.y the column block where D_w > 256) and takes CC_RPT * tr rows at a time, CC_RPT accumulators per thread.
// The rows pass through LDS in tiles of CC_JT inner indices, each element loaded once per workgroup: a half-wave loads
// 32 consecutive elements of a row, and the row stride CC_STRIDE = 33 words is odd, so the loader's 32 lanes and the
// row groups of a half-wave (at most 16, rows rg apart) hit different banks; lanes of one row group read one address
// (a broadcast).  E[j][column] is read by neighbouring lanes at neighbouring addresses inside a subspace's L columns.
// 8.4 KB of LDS and a handful of VGPRs: occupancy is bounded by waves, not by either.  Rows and offsets are 64-bit.
constexpr int CC_THREADS = 256, CC_JT = 32, CC_STRIDE = CC_JT + 1, CC_RPT = 4, CC_MIN_TC_LOG2 = 4;
constexpr int CC_TILE_ROWS = CC_RPT * (CC_THREADS >> CC_MIN_TC_LOG2);

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cb_columns_kernel(const T *__restrict__ X, int D, const float *__restrict__ E,
                                                                const int *__restrict__ rows, int64_t first, int64_t cnt,
                                                                const int *__restrict__ subs, int L, int D_w, int tc_log2,
                                                                float *__restrict__ out) {
  __shared__ float tile[CC_TILE_ROWS * CC_STRIDE];
  const int tid = threadIdx.x;
  const int tc = 1 << tc_log2, tr = CC_THREADS >> tc_log2;
  const int rg = tid >> tc_log2;
  const int c = blockIdx.y * tc + (tid & (tc - 1));
  const bool col_ok = c < D_w;
  const int gc = col_ok ? subs[c / L] * L + c % L : 0;
  const int tile_rows = tr * CC_RPT;
  const int lc = tid & (CC_JT - 1), lr = tid / CC_JT;
  for (int64_t row0 = (int64_t)blockIdx.x * tile_rows; row0 < cnt; row0 += (int64_t)gridDim.x * tile_rows) {
    float acc[CC_RPT];
#pragma unroll
    for (int i = 0; i < CC_RPT; i++) acc[i] = 0.0f;
    if (!E) {
#pragma unroll
      for (int i = 0; i < CC_RPT; i++) {
        const int64_t r = row0 + rg + i * tr;
        if (col_ok && r < cnt) acc[i] = (float)X[(rows ? (int64_t)rows[r] : first + r) * D + gc];
      }
    } else {
      for (int j0 = 0; j0 < D; j0 += CC_JT) {
        __syncthreads();  // (the tile before has been read)
        for (int r = lr; r < tile_rows; r += CC_THREADS / CC_JT) {
          const int64_t i = row0 + r;
          float v = 0.0f;
          if (i < cnt && j0 + lc < D) v = (float)X[(rows ? (int64_t)rows[i] : first + i) * D + j0 + lc];
          tile[r * CC_STRIDE + lc] = v;
        }
        __syncthreads();
        if (col_ok) {
          const int jn = D - j0 < CC_JT ? D - j0 : CC_JT;
          const float *e = E + (size_t)j0 * D + gc;
          for (int jj = 0; jj < jn; jj++, e += D) {
            const float ev = *e;
#pragma unroll
            for (int i = 0; i < CC_RPT; i++) acc[i] = __builtin_fmaf(tile[(rg + i * tr) * CC_STRIDE + jj], ev, acc[i]);
          }
        }
      }
    }
    if (col_ok) {
#pragma unroll
      for (int i = 0; i < CC_RPT; i++) {
        const int64_t r = row0 + rg + i * tr;
        if (r < cnt) out[r * D_w + c] = acc[i];
      }
    }
  }
}

// the owner's side of the exchange: staging row i goes to row pos[i] of the sample matrix (the sample is in
// permutation order, so a shard's rows are scattered in it)
__global__ void cb_place_kernel(const float *__restrict__ stage, const int *__restrict__ pos, int64_t rows, int D_w,
                                float *__restrict__ Ps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * D_w) return;
  const int64_t r = i / D_w;
  Ps[(int64_t)pos[r] * D_w + (i - r * D_w)] = stage[i];
}

hipError_t launch_codebook_columns(RowsRef X, int D, const float *d_eig, const int *d_rows, int64_t first, int64_t cnt,
                                   const int *d_subs, int L, int D_w, float *out, hipStream_t st) {
  if (cnt < 1 || D_w < 1) return hipSuccess;
  int tc_log2 = CC_MIN_TC_LOG2;
  while (tc_log2 < 8 && (1 << tc_log2) < D_w) tc_log2++;
  const int tc = 1 << tc_log2, tile_rows = CC_RPT * (CC_THREADS >> tc_log2);
  const dim3 grid((unsigned)std::min<int64_t>((cnt + tile_rows - 1) / tile_rows, 1 << 16), (unsigned)((D_w + tc - 1) / tc));
  if (X.elem == 1)
    hipLaunchKernelGGL(cb_columns_kernel<uint8_t>, grid, dim3(CC_THREADS), 0, st, static_cast<const uint8_t *>(X.p), D, d_eig,
                       d_rows, first, cnt, d_subs, L, D_w, tc_log2, out);
  else
    hipLaunchKernelGGL(cb_columns_kernel<float>, grid, dim3(CC_THREADS), 0, st, static_cast<const float *>(X.p), D, d_eig,
                       d_rows, first, cnt, d_subs, L, D_w, tc_log2, out);
  return hipGetLastError();
}

hipError_t launch_codebook_place(const float *d_stage, const int *d_pos, int64_t rows, int D_w, float *d_Ps, hipStream_t st) {
  if (rows < 1) return hipSuccess;
  hipLaunchKernelGGL(cb_place_kernel, dim3((unsigned)((rows * D_w + 255) / 256)), dim3(256), 0, st, d_stage, d_pos, rows,
                     D_w, d_Ps);
  return hipGetLastError();
}

hipError_t launch_codebook_gather(const float *d_Pf, int D_w, const int *d_rows, int64_t S, float *d_Ps, hipStream_t st) {
  if (S < 1) return hipSuccess;
  hipLaunchKernelGGL(cb_gather_kernel<float>, dim3((unsigned)((S * D_w + 255) / 256)), dim3(256), 0, st, d_Pf, D_w, d_rows, S,
                     d_Ps);
  return hipGetLastError();
}

namespace {
double cb_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

#define CB_TRY(expr)                          \
  do {                                        \
    if ((e = (expr)) != hipSuccess) return e; \
  } while (0)

// (buffers are freed on return, after the stream is synchronised)
struct CbSync {
  hipStream_t st;
  bool armed;
  ~CbSync() {
    if (armed) (void)hipStreamSynchronize(st);
  }
};

// The two sources of a fit and the buffers that hold them.  full: all n rows projected (or widened) once, for the
// readers of all rows in their own order.  sample: the first S rows of randomPermutation(n), projected, every reader
// of it working on a prefix -- gathered here (`gather`), or the caller's rows are the sample already.
struct CbPrepared {
  vaqhost::DevBuf rows, gathered, proj, all;
  const float *full = nullptr, *sample = nullptr;
};

hipError_t cb_prepare(RowsRef d_X, int64_t n, int D, const float *d_eig, bool need_full, int64_t S, bool gather,
                      CbPrepared &out, hipStream_t st) {
  hipError_t e;
  // rows x D of src as floats, projected where there is a rotation: in place when nothing is to be done, else in buf
  auto projected = [&](RowsRef src, int64_t rows, vaqhost::DevBuf &buf, const float **res) -> hipError_t {
    *res = static_cast<const float *>(src.p);
    if (!d_eig && src.elem != 1) return hipSuccess;
    hipError_t pe = buf.ensure((size_t)rows * D * sizeof(float));
    if (pe != hipSuccess) return pe;
    *res = buf.as<float>();
    if (d_eig) return launch_project(src, rows, D, d_eig, buf.as<float>(), st, 0);  // unchecked, as VAQ::train projects
    return launch_widen_rows_u8(static_cast<const uint8_t *>(src.p), rows * D, buf.as<float>(), st);
  };
  // ---- the full matrix, for the subspaces that do not sample: all n rows projected (or widened) once ----
  if (need_full) CB_TRY(projected(d_X, n, out.all, &out.full));
  // ---- the sample, for those that do: gathered once, every one of them works on a prefix of it ----
  if (S > 0 && !gather) {
    CB_TRY(projected(d_X, S, out.proj, &out.sample));  // (the caller's rows are the sample)
  } else if (S > 0) {
    const std::vector<int> rows = permutation_head(n, S);
    CB_TRY(out.rows.ensure((size_t)S * sizeof(int)));
    CB_TRY(out.gathered.ensure((size_t)S * D * sizeof(float)));
    CB_TRY(hipMemcpyAsync(out.rows.p, rows.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)((S * D + 255) / 256);
    if (out.full || d_X.elem != 1)  // from the projected full matrix where there is one: a row's projection is its own
      hipLaunchKernelGGL(cb_gather_kernel<float>, dim3(grid), dim3(256), 0, st,
                         out.full ? out.full : static_cast<const float *>(d_X.p), D, out.rows.as<int>(), S,
                         out.gathered.as<float>());
    else
      hipLaunchKernelGGL(cb_gather_kernel<uint8_t>, dim3(grid), dim3(256), 0, st, static_cast<const uint8_t *>(d_X.p), D,
                         out.rows.as<int>(), S, out.gathered.as<float>());
    CB_TRY(hipGetLastError());
    CB_TRY(hipStreamSynchronize(st));  // (rows is the host's)
    out.sample = out.gathered.as<float>();
    if (!out.full && d_eig) CB_TRY(projected(RowsRef{out.gathered.p, 4}, S, out.proj, &out.sample));
  }
  return hipSuccess;
}

// launch shape of the assign kernel for slices of L floats and at most k_max centres per fit
struct CbAssignShape {
  int R, stage;
  bool x_lds;
  size_t lds;
};
CbAssignShape cb_assign_shape(int L, int k_max) {
  CbAssignShape a;
  a.R = cbfit::assign_tile_rows(L);
  a.x_lds = (size_t)a.R * L * sizeof(float) <= (size_t)cbfit::TILE_BYTES;
  a.stage = std::max(1, std::min(k_max, CB_STAGE_FLOATS / L));
  a.lds = ((size_t)a.stage * L + (a.x_lds ? (size_t)a.R * L : 0)) * sizeof(float);
  return a;
}

// the assign kernel over a batch: by its tile table (d_tiles, n_tiles) or, without one, over (row tile, fit)
template <bool MEMBER>
hipError_t cb_launch_assign(const CbSources &src, int L, const cbfit::Batch &b, const cbfit::Fit *d_fits,
                            const cbfit::Tile *d_tiles, const float *d_means, const int *d_active, unsigned *keys,
                            unsigned *vals, int *d_no_centre, hipStream_t st) {
  const CbAssignShape a = cb_assign_shape(L, b.k_max);
  const dim3 grid = d_tiles ? dim3((unsigned)b.tile.size()) : dim3((unsigned)((b.rows_max + a.R - 1) / a.R), (unsigned)b.fit.size());
  if (a.x_lds)
    hipLaunchKernelGGL((cb_assign_kernel<true, MEMBER>), grid, dim3(a.R), a.lds, st, src, L, d_fits, d_tiles, d_means, a.stage,
                       d_active, keys, vals, d_no_centre);
  else
    hipLaunchKernelGGL((cb_assign_kernel<false, MEMBER>), grid, dim3(a.R), a.lds, st, src, L, d_fits, d_tiles, d_means, a.stage,
                       d_active, keys, vals, d_no_centre);
  return hipGetLastError();
}

// One fit that samples for itself (KMeans.hpp:489-503 over the rows it is handed): rows
// randomPermutation(node_rows)[0 .. rows) of the matrix at src (rows `stride` floats apart, the slice from column `col`
// on) become rows [off, off + rows) of a compact [.][L] matrix.
struct CbResample {
  const float *src;
  int stride, col, node_rows, rows;
  int64_t off;
};

// The buffers the passes of ONE call share.  The call's entry point (codebooks_lloyd, codebooks_fit_hier,
// codebooks_fit_bin; codebooks_fit through codebooks_lloyd) owns it and hands it to every pass: a run of the Lloyd
// phases (cb_lloyd_batch), the hierarchical fit's membership pass, the binary fit's split pass.  The buffers only grow,
// so a level of the binary fit allocates what no pass before it needed and nothing else.
// The one rule: DevBuf::ensure drops the contents when it grows, and a pass ensures what it needs as it begins.  So
// NOTHING a pass left in here -- tables, pairs sorted or not, bounds -- may be read once the next pass has begun.  Who
// needs it longer launches the readers and synchronises first.  There are two such readers: the hierarchical fit's
// cb_slice_kernel over vals_out (the bounds' copy to the host synchronises behind it, before stage 2), and the binary
// fit's cb_regroup_kernel over keys_out, vals_out and the split's fit table (launched and synchronised before the cut
// fits).  A source matrix a later pass reads (the resamples, the compact matrices) is not kept in here.
struct CbWork {
  hipStream_t st;
  vaqhost::DevBuf b_keys_in, b_keys_out, b_vals_in, b_vals_out, b_bounds, b_temp, b_fit, b_tile, b_part, b_flags, b_seed, b_perm;
  unsigned *keys_in = nullptr, *keys_out = nullptr, *vals_in = nullptr, *vals_out = nullptr;  // of the last pairs()
  int *start = nullptr, *end = nullptr;  // run [start[k], end[k]) of key k, of the last sort_and_bound()
  size_t temp_bytes = 0, sized_pairs = 0;  // rocprim's temporary storage for (sized_pairs, sized_bits)
  unsigned sized_bits = 0;

  struct Tables {
    const cbfit::Fit *fits = nullptr;
    const cbfit::Tile *tiles = nullptr;  // null: the batch has no tile table
  };
  // the batch's fit table and, where there is one, its tile table, on the stream (the batch is the host's until it is
  // synchronised)
  hipError_t upload(const cbfit::Batch &b, Tables *t) {
    hipError_t e;
    CB_TRY(b_fit.ensure(b.fit.size() * sizeof(cbfit::Fit)));
    CB_TRY(hipMemcpyAsync(b_fit.p, b.fit.data(), b.fit.size() * sizeof(cbfit::Fit), hipMemcpyHostToDevice, st));
    *t = Tables{b_fit.as<cbfit::Fit>(), nullptr};
    if (b.tile.empty()) return hipSuccess;
    CB_TRY(b_tile.ensure(b.tile.size() * sizeof(cbfit::Tile)));
    CB_TRY(hipMemcpyAsync(b_tile.p, b.tile.data(), b.tile.size() * sizeof(cbfit::Tile), hipMemcpyHostToDevice, st));
    t->tiles = b_tile.as<cbfit::Tile>();
    return hipSuccess;
  }
  // room for n_pairs (key, row) pairs, unsorted (keys_in, vals_in) and sorted
  hipError_t pairs(int n_pairs) {
    hipError_t e;
    for (vaqhost::DevBuf *b : {&b_keys_in, &b_keys_out, &b_vals_in, &b_vals_out}) CB_TRY(b->ensure((size_t)n_pairs * 4));
    keys_in = b_keys_in.as<unsigned>(), keys_out = b_keys_out.as<unsigned>();
    vals_in = b_vals_in.as<unsigned>(), vals_out = b_vals_out.as<unsigned>();
    return hipSuccess;
  }
  // (keys_in, vals_in) sorted by the low key_bits of the key into (keys_out, vals_out) -- stable: pairs of equal key stay
  // in the order they were emitted in -- and the run of every key below n_runs (a key that does not occur: empty)
  hipError_t sort_and_bound(int n_pairs, unsigned key_bits, int n_runs) {
    hipError_t e;
    if ((size_t)n_pairs != sized_pairs || key_bits != sized_bits) {
      CB_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n_pairs, 0u, key_bits, st));
      CB_TRY(b_temp.ensure(temp_bytes ? temp_bytes : 16));
      sized_pairs = (size_t)n_pairs, sized_bits = key_bits;
    }
    CB_TRY(b_bounds.ensure((size_t)2 * n_runs * sizeof(int)));
    start = b_bounds.as<int>(), end = start + n_runs;
    CB_TRY(hipMemsetAsync(start, 0, (size_t)2 * n_runs * sizeof(int), st));
    CB_TRY(rocprim::radix_sort_pairs(b_temp.p, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n_pairs, 0u, key_bits, st));
    hipLaunchKernelGGL(cb_bounds_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, keys_out, n_pairs, start, end);
    return hipGetLastError();
  }
  // the compact matrix of the fits that sample for themselves: ONE upload of their permutation heads back to back, one
  // cb_slice_kernel each, one synchronisation (the heads are the host's)
  hipError_t gather_resamples(const std::vector<CbResample> &rs, int L, float *out) {
    hipError_t e;
    std::vector<int> perm;
    std::vector<size_t> at;
    for (const CbResample &r : rs) {
      const std::vector<int> rows = permutation_head(r.node_rows, r.rows);
      at.push_back(perm.size());
      perm.insert(perm.end(), rows.begin(), rows.end());
    }
    CB_TRY(b_perm.ensure(perm.size() * sizeof(int)));
    CB_TRY(hipMemcpyAsync(b_perm.p, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    for (size_t i = 0; i < rs.size(); i++) {
      const CbResample &r = rs[i];
      hipLaunchKernelGGL(cb_slice_kernel, dim3((unsigned)(((int64_t)r.rows * L + 255) / 256)), dim3(256), 0, st, r.src, r.stride,
                         r.col, b_perm.as<int>() + at[i], (int64_t)r.rows, L, out + (size_t)r.off * L);
      CB_TRY(hipGetLastError());
    }
    return hipStreamSynchronize(st);
  }
};

// The Lloyd loop over a batch of fits: seeds from permutation_head(rows, k) of every fit's own rows, then one launch per
// phase and iteration for ALL fits until every fit's centres stopped changing or max_iter.  The sources are complete on
// w.st; d_means spans b.n_cent centres.  iters_out[fits] (host).  began: when the caller started preparing the
// sources, for phases->gather_ms (null phases: no per-phase synchronisation).  Synchronises the stream.
// staged_sums (the binary fit's batches): the sums by cb_sums_staged_kernel, the same bits.
hipError_t cb_lloyd_batch(CbWork &w, const CbSources &src, int L, const cbfit::Batch &b, int max_iter, float *d_means,
                          int *iters_out, int *no_centre_out, CodebookPhases *phases,
                          std::chrono::steady_clock::time_point began, bool staged_sums = false) {
  const int F = (int)b.fit.size();
  if (F < 1 || b.rows_max < 1 || b.n_pairs > 0x7fffffff || F > 65535) return hipErrorInvalidValue;
  const int n_pairs = (int)b.n_pairs, n_runs = b.n_runs;
  const hipStream_t st = w.st;
  hipError_t e;
  auto t0 = began;

  // ---- the batch's tables and the seeds ----
  std::vector<int> seeds((size_t)b.n_cent, 0);
  for (const cbfit::Fit &fd : b.fit) {
    const std::vector<int> head = permutation_head(fd.rows, fd.k);
    std::copy(head.begin(), head.end(), seeds.begin() + fd.cent_off);
  }
  CbWork::Tables t;
  CB_TRY(w.upload(b, &t));
  CB_TRY(w.pairs(n_pairs));
  CB_TRY(w.b_seed.ensure(seeds.size() * sizeof(int)));
  CB_TRY(w.b_part.ensure((size_t)n_runs * L * sizeof(float)));
  CB_TRY(w.b_flags.ensure((size_t)3 * F * sizeof(int)));
  int *flags = w.b_flags.as<int>();  // changed[2][F] (this iteration's and the one before), then no_centre[F]
  float *part = w.b_part.as<float>();
  std::vector<int> host_flags((size_t)3 * F, 0);
  for (int f = 0; f < F; f++) host_flags[(size_t)f] = 1;  // every fit starts active
  CB_TRY(hipMemcpyAsync(w.b_seed.p, seeds.data(), seeds.size() * sizeof(int), hipMemcpyHostToDevice, st));
  CB_TRY(hipMemcpyAsync(flags, host_flags.data(), host_flags.size() * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(cb_seed_kernel, dim3((unsigned)((b.k_max * L + 255) / 256), (unsigned)F), dim3(256), 0, st, src, L,
                     t.fits, w.b_seed.as<int>(), d_means);
  CB_TRY(hipGetLastError());
  CB_TRY(hipStreamSynchronize(st));  // (the tables are the host's)
  if (phases) phases->gather_ms += cb_ms_since(t0);

  const dim3 acc_grid((unsigned)((2 * (int64_t)b.k_max * L + 255) / 256), (unsigned)F);

  auto phase_end = [&](double *acc) -> hipError_t {
    if (!phases) return hipSuccess;
    const hipError_t pe = hipStreamSynchronize(st);
    *acc += cb_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    return pe;
  };
  std::vector<char> done((size_t)F, 0);
  for (int f = 0; f < F; f++) iters_out[f] = 0;
  int no_centre = 0, n_done = 0;
  t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < max_iter && n_done < F && !no_centre; it++) {
    int *prev = flags + (size_t)(it & 1) * F, *now = flags + (size_t)((it + 1) & 1) * F;
    CB_TRY(hipMemsetAsync(now, 0, (size_t)F * sizeof(int), st));
    CB_TRY(cb_launch_assign<false>(src, L, b, t.fits, t.tiles, d_means, prev, w.keys_in, w.vals_in, flags + 2 * F, st));
    CB_TRY(phase_end(phases ? &phases->assign_ms : nullptr));
    // stable: rows of equal (fit, half, centre) stay in ascending order
    CB_TRY(w.sort_and_bound(n_pairs, b.key_bits, n_runs));
    if (staged_sums)
      hipLaunchKernelGGL(cb_sums_staged_kernel, dim3((unsigned)(2 * b.k_max), (unsigned)F), dim3(64), 0, st, src, L, t.fits,
                         w.vals_out, w.start, w.end, part);
    else
      hipLaunchKernelGGL(cb_accumulate_kernel, acc_grid, dim3(256), 0, st, src, L, t.fits, w.vals_out, w.start, w.end, part);
    CB_TRY(hipGetLastError());
    CB_TRY(phase_end(phases ? &phases->accumulate_ms : nullptr));
    hipLaunchKernelGGL(cb_update_kernel, dim3((unsigned)b.k_max, (unsigned)F), dim3(64), 0, st, part, w.start, w.end, L, t.fits,
                       d_means, now);
    CB_TRY(hipGetLastError());
    CB_TRY(hipMemcpyAsync(host_flags.data(), flags, host_flags.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    CB_TRY(hipStreamSynchronize(st));
    CB_TRY(phase_end(phases ? &phases->update_ms : nullptr));
    for (int f = 0; f < F; f++) {
      no_centre |= host_flags[(size_t)2 * F + f];
      if (done[(size_t)f]) continue;
      iters_out[f] = it + 1;  // the reference's iter_count: the iteration that changes nothing is counted
      if (!host_flags[(size_t)((it + 1) & 1) * F + f]) {
        done[(size_t)f] = 1;
        n_done++;
      }
    }
  }
  *no_centre_out = no_centre;
  return hipStreamSynchronize(st);
}
}  // namespace

hipError_t codebooks_fit(RowsRef d_X, int64_t n, int D, int L, const cbfit::Plan &plan, const float *d_eig,
                         int max_iter, float *d_means, int *iters_out, int *no_centre_out, CodebookPhases *phases,
                         hipStream_t st) {
  const int M = (int)plan.sub.size();
  const int64_t S = plan.gathered;
  if (M < 1 || plan.sample < 1 || plan.n_pairs > 0x7fffffff) return hipErrorInvalidValue;
  if (plan.n_full ? (S > 0 && !plan.gather) : S < 1) return hipErrorInvalidValue;
  hipError_t e;
  CbPrepared src;
  CbSync sync_on_return{st, true};
  if (phases) *phases = CodebookPhases{};
  auto t0 = std::chrono::steady_clock::now();
  CB_TRY(cb_prepare(d_X, n, D, d_eig, plan.n_full > 0, S, plan.gather, src, st));
  sync_on_return.armed = false;  // (codebooks_lloyd synchronises before it returns, and the sources are freed behind it)
  return codebooks_lloyd(src.sample, src.full, D, L, plan, max_iter, d_means, iters_out, no_centre_out, phases, t0, st);
}

// The fit from its two sources on: Ps the sample (plan.gathered x D, the subspaces with full == 0 read prefixes of
// it), Pf the full matrix (n x D, those with full == 1), either null when no subspace reads it; both complete on `st`.
// codebooks_fit above ends in it; the owners of the sharded fit (vaqhip_multi_codebooks.cpp) call it over their
// compact matrices.  began: when the caller started preparing the sources, for phases->gather_ms.
hipError_t codebooks_lloyd(const float *Ps, const float *Pf, int D, int L, const cbfit::Plan &plan, int max_iter,
                           float *d_means, int *iters_out, int *no_centre_out, CodebookPhases *phases,
                           std::chrono::steady_clock::time_point began, hipStream_t st) {
  if (plan.sub.empty() || plan.sample < 1) return hipErrorInvalidValue;
  CbWork work{st};
  CbSync sync_on_return{st, true};  // (a failed launch: the workspace is freed behind what still runs)
  return cb_lloyd_batch(work, CbSources{{Ps, Pf, nullptr}}, L, cbfit::make_batch(plan, D, L), max_iter, d_means, iters_out,
                        no_centre_out, phases, began);
}

// ---- the hierarchical fit (DESIGN.md section 4f "Hierarchical"; fit_codebooks_hier_plan.h) ----
// Stage 1: the flat subspaces and the 128-centre fits of the hierarchical ones in ONE run of the Lloyd phases.  Then the
// membership of every row of R_s (nearest stage-1 centre by squaredNorm, no sqrt), a stable sort of the rows by
// (subspace, group) and a gather into one compact [rows_s][L] matrix per subspace whose groups are contiguous and in
// R_s order -- the stable order is what makes the stage-2 sums the reference's.  Stage 2: the K2-centre fits of ALL
// groups of ALL hierarchical subspaces as one more run of the same phases over the compact matrices, the assign kernel
// walking the plan's tile table.  d_means: plan.n_cent + 128 per hierarchical subspace centres (the stage-1 centres
// behind the final ones).  On a refusal (*refusal, or *no_centre_out) the centres are not to be used.
hipError_t codebooks_fit_hier(RowsRef d_X, int64_t n, int D, int L, const cbhier::Plan &plan, const float *d_eig,
                              int max_iter, float *d_means, int *iters_out, int *no_centre_out, cbhier::Refusal *refusal,
                              CodebookHierStats *stats, CodebookPhases *phases, hipStream_t st) {
  const int M = (int)plan.flat.sub.size(), H = (int)plan.hsub.size();
  if (M < 1 || H < 1 || plan.gathered < 1 || plan.n_pairs > 0x7fffffff) return hipErrorInvalidValue;
  hipError_t e;
  CbPrepared src;
  CbWork work{st};
  vaqhost::DevBuf b_resample, b_compact;
  CbSync sync_on_return{st, true};
  *refusal = cbhier::Refusal{};
  *no_centre_out = 0;
  *stats = CodebookHierStats{};
  CodebookPhases ph;
  auto t0 = std::chrono::steady_clock::now();
  const auto began = t0;

  // ---- the sources: all rows for the flat subspaces that read them, and ONE head of randomPermutation(n) ----
  CB_TRY(cb_prepare(d_X, n, D, d_eig, plan.n_full > 0, plan.gathered, true, src, st));
  // stage 1 of a subspace with more than 65536 rows samples for itself: rows randomPermutation(rows_s)[0 .. 65536) of R_s
  if (plan.resample_rows > 0) {
    std::vector<CbResample> rs;
    for (const cbhier::HSub &h : plan.hsub)
      if (h.resampled) rs.push_back(CbResample{src.sample, D, h.s * L, h.rows, h.stage1_rows, h.resample_off});
    CB_TRY(b_resample.ensure((size_t)plan.resample_rows * L * sizeof(float)));
    CB_TRY(work.gather_resamples(rs, L, b_resample.as<float>()));
  }

  // ---- stage 1 ----
  std::vector<int> it1((size_t)M, 0);
  CB_TRY(cb_lloyd_batch(work, CbSources{{src.sample, src.full, b_resample.as<float>()}}, L, plan.stage1, max_iter, d_means,
                        it1.data(), no_centre_out, phases ? &ph : nullptr, began));
  for (int s = 0; s < M; s++) iters_out[s] = it1[(size_t)s];
  stats->stage1_ms = cb_ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (*no_centre_out) return hipSuccess;
  std::vector<float> c1((size_t)H * cbhier::K1 * L);
  CB_TRY(hipMemcpyAsync(c1.data(), d_means + (size_t)plan.n_cent * L, c1.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  CB_TRY(hipStreamSynchronize(st));
  for (int h = 0; h < H; h++)
    for (int g = 0; g < cbhier::K1; g++)
      if (nan_rows(c1.data() + ((size_t)h * cbhier::K1 + g) * L, 1, L)) {
        refusal->kind = cbhier::NAN_CENTRE;
        refusal->s = plan.hsub[(size_t)h].s;
        refusal->group = g;
        return hipSuccess;
      }

  // ---- membership and regroup ----
  const int n_pairs = (int)plan.n_pairs, n_groups = H * cbhier::K1;
  CbWork::Tables member;
  CB_TRY(work.upload(plan.member, &member));
  CB_TRY(work.pairs(n_pairs));
  CB_TRY(work.b_flags.ensure((size_t)H * sizeof(int)));
  CB_TRY(b_compact.ensure((size_t)n_pairs * L * sizeof(float)));
  CB_TRY(hipMemsetAsync(work.b_flags.p, 0, (size_t)H * sizeof(int), st));
  const CbSources member_src{{src.sample, nullptr, nullptr}};
  CB_TRY(cb_launch_assign<true>(member_src, L, plan.member, member.fits, nullptr, d_means, nullptr, work.keys_in, work.vals_in,
                                work.b_flags.as<int>(), st));
  // stable: the rows of a group stay in ascending position within R_s
  CB_TRY(work.sort_and_bound(n_pairs, plan.member.key_bits, n_groups));
  for (const cbhier::HSub &h : plan.hsub) {  // the sorted rows of subspace h are pairs [pair_off, pair_off + rows)
    hipLaunchKernelGGL(cb_slice_kernel, dim3((unsigned)(((int64_t)h.rows * L + 255) / 256)), dim3(256), 0, st, src.sample, D,
                       h.s * L, reinterpret_cast<const int *>(work.vals_out) + h.pair_off, (int64_t)h.rows, L,
                       b_compact.as<float>() + (size_t)h.pair_off * L);
    CB_TRY(hipGetLastError());
  }
  std::vector<int> bounds((size_t)2 * n_groups), counts((size_t)n_groups), unreached((size_t)H);
  CB_TRY(hipMemcpyAsync(bounds.data(), work.start, bounds.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  CB_TRY(hipMemcpyAsync(unreached.data(), work.b_flags.p, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, st));
  CB_TRY(hipStreamSynchronize(st));  // (and the slices have read vals_out: stage 2 may take the workspace)
  stats->groups = n_groups;
  stats->min_group = 0x7fffffff;
  for (int g = 0; g < n_groups; g++) {
    counts[(size_t)g] = bounds[(size_t)n_groups + g] - bounds[(size_t)g];
    stats->min_group = std::min(stats->min_group, counts[(size_t)g]);
    stats->max_group = std::max(stats->max_group, counts[(size_t)g]);
  }
  stats->regroup_ms = cb_ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  for (int h = 0; h < H; h++)
    if (unreached[(size_t)h]) {
      refusal->kind = cbhier::NO_CENTRE;
      refusal->s = plan.hsub[(size_t)h].s;
      return hipSuccess;
    }
  *refusal = cbhier::check_groups(plan, counts.data());
  if (refusal->kind != cbhier::OK) return hipSuccess;

  // ---- stage 2: every group of every hierarchical subspace, one batch ----
  const cbfit::Batch stage2 = cbhier::make_stage2(plan, counts.data(), L, cbfit::assign_tile_rows(L));
  std::vector<int> it2(stage2.fit.size(), 0);
  CB_TRY(cb_lloyd_batch(work, CbSources{{b_compact.as<float>(), nullptr, nullptr}}, L, stage2, max_iter, d_means, it2.data(),
                        no_centre_out, phases ? &ph : nullptr, t0));
  for (int h = 0; h < H; h++)
    for (int g = 0; g < cbhier::K1; g++) {
      int &out = iters_out[plan.hsub[(size_t)h].s];
      out = std::max(out, it2[(size_t)h * cbhier::K1 + g]);
      stats->stage2_iters = std::max(stats->stage2_iters, it2[(size_t)h * cbhier::K1 + g]);
    }
  for (int s = 0; s < M; s++) stats->stage1_iters = std::max(stats->stage1_iters, it1[(size_t)s]);
  stats->stage2_ms = cb_ms_since(t0);
  if (phases) *phases = ph;
  sync_on_return.armed = false;
  return hipStreamSynchronize(st);
}

// ---- the binary-tree fit (DESIGN.md section 4f "Binary form"; fit_codebooks_bin_plan.h) ----
// Level by level over the trees of ALL binary subspaces.  Per level: the 2-centre fits of every live node as one run
// of the Lloyd phases (the first level's carries the call's flat subspaces); unless the level is a subspace's last,
// the split of all rows of its nodes, a stable sort by 2 * node + side and the run bounds, which come back to the
// host; the flat fits of the nodes the sizes cut, as one more run over the same matrix; then the rows of the nodes
// that go on are gathered, in sorted order, into the other compact [rows][L] matrix -- left child, right child, node
// after node, every child's rows in ascending position within its parent.  A fit over more rows than
// staticFitSampling takes works on rows randomPermutation(m)[0 .. sample) of its node, gathered into `extra`.  Every
// fit writes its centres where the node's block of the output begins: a split node's two centres are overwritten by
// its descendants, which tile the block.  On *no_centre_out the centres are not to be used.
hipError_t codebooks_fit_bin(RowsRef d_X, int64_t n, int D, int L, const cbbin::Plan &plan, const float *d_eig, int max_iter,
                             bool staged_sums, float *d_means, int *iters_out, int *no_centre_out, CodebookBinStats *stats,
                             CodebookPhases *phases, hipStream_t st) {
  const int M = (int)plan.flat.sub.size();
  if (M < 1 || plan.bsub.empty() || plan.gathered < 1 || plan.n_pairs > 0x7fffffff) return hipErrorInvalidValue;
  hipError_t e;
  CbPrepared src;
  CbWork work{st};
  vaqhost::DevBuf b_extra, b_dest, b_level[2];
  CbSync sync_on_return{st, true};
  *no_centre_out = 0;
  *stats = CodebookBinStats{};
  stats->min_leaf_rows = 0x7fffffff;
  CodebookPhases ph;
  const auto began = std::chrono::steady_clock::now();
  for (int s = 0; s < M; s++) iters_out[s] = 0;

  CB_TRY(cb_prepare(d_X, n, D, d_eig, plan.n_full > 0, plan.gathered, true, src, st));
  const int tile_rows = cbfit::assign_tile_rows(L);

  CbSources cur{{src.sample, src.full, nullptr}};
  // one kind of fits of a level: the samples of those that sample, then chunk after chunk of the Lloyd phases
  auto run_fits = [&](const std::vector<cbbin::Node> &level, const cbbin::Fits &f, std::chrono::steady_clock::time_point t0) -> hipError_t {
    if (!f.resample.empty()) {
      std::vector<CbResample> rs;
      for (const cbbin::Resample &r : f.resample) {
        const cbbin::Node &nd = level[(size_t)r.node];
        rs.push_back(CbResample{cur.p[nd.src] + (size_t)nd.row0 * nd.stride, nd.stride, nd.col, nd.rows, r.rows, r.off});
      }
      CB_TRY(b_extra.ensure((size_t)f.extra_rows * L * sizeof(float)));
      CB_TRY(work.gather_resamples(rs, L, b_extra.as<float>()));
      stats->resampled_fits += (int)f.resample.size();
    }
    const CbSources fit_src{{cur.p[0], cur.p[1], b_extra.as<float>()}};
    for (size_t c = 0; c < f.chunk.size(); c++) {
      std::vector<int> its(f.chunk[c].fit.size(), 0);
      int nc = 0;
      CB_TRY(cb_lloyd_batch(work, fit_src, L, f.chunk[c], max_iter, d_means, its.data(), &nc, phases ? &ph : nullptr, t0, staged_sums));
      *no_centre_out |= nc;
      for (size_t i = 0; i < its.size(); i++) {
        const int o = f.owner[c][i];
        int &out = iters_out[o < 0 ? -1 - o : plan.bsub[(size_t)level[(size_t)o].b].s];
        out = std::max(out, its[i]);
        stats->max_iters = std::max(stats->max_iters, its[i]);
      }
      t0 = std::chrono::steady_clock::now();
    }
    return hipSuccess;
  };

  std::vector<cbbin::Node> level = cbbin::root_level(plan, D, L);
  for (int depth = 1; !level.empty(); depth++) {
    // ---- the 2-centre fits of every live node ----
    auto t0 = std::chrono::steady_clock::now();
    std::vector<int> all(level.size()), inner;
    for (size_t i = 0; i < level.size(); i++) {
      all[i] = (int)i;
      const cbbin::Node &nd = level[i];
      if (nd.depth < plan.bsub[(size_t)nd.b].bits) {
        inner.push_back((int)i);
        continue;
      }
      stats->leaf_nodes++;
      stats->min_leaf_rows = std::min(stats->min_leaf_rows, nd.rows);
      stats->max_leaf_rows = std::max(stats->max_leaf_rows, nd.rows);
    }
    stats->levels = depth;
    stats->nodes += (int)level.size();
    CB_TRY(run_fits(level, cbbin::make_fits(plan, level, all, false, depth == 1, D, L, tile_rows), depth == 1 ? began : t0));
    stats->fit_ms += cb_ms_since(t0);
    if (*no_centre_out || inner.empty()) break;

    // ---- the split of the nodes that are no leaves ----
    t0 = std::chrono::steady_clock::now();
    const cbfit::Batch split = cbbin::make_split(plan, level, inner, tile_rows);
    const int F = (int)split.fit.size(), sp = (int)split.n_pairs;
    CbWork::Tables tabs;
    CB_TRY(work.upload(split, &tabs));
    CB_TRY(work.pairs(sp));
    CB_TRY(b_dest.ensure((size_t)F * sizeof(int64_t)));
    hipLaunchKernelGGL(cb_split_kernel, dim3((unsigned)split.tile.size()), dim3(tile_rows), (size_t)2 * L * sizeof(float), st, cur, L,
                       tabs.fits, tabs.tiles, d_means, work.keys_in, work.vals_in);
    CB_TRY(hipGetLastError());
    // stable: each side of a node keeps its rows in ascending position within the node
    CB_TRY(work.sort_and_bound(sp, split.key_bits, 2 * F));
    std::vector<int> bounds((size_t)4 * F), left((size_t)F), right((size_t)F), cut;
    CB_TRY(hipMemcpyAsync(bounds.data(), work.start, bounds.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    CB_TRY(hipStreamSynchronize(st));
    std::vector<cbbin::Kind> kind((size_t)F);
    for (int i = 0; i < F; i++) {
      left[(size_t)i] = bounds[(size_t)2 * F + 2 * i] - bounds[(size_t)2 * i];
      right[(size_t)i] = bounds[(size_t)2 * F + 2 * i + 1] - bounds[(size_t)2 * i + 1];
      const cbbin::Node &nd = level[(size_t)inner[(size_t)i]];
      kind[(size_t)i] = cbbin::decide(plan.bsub[(size_t)nd.b], nd, left[(size_t)i], right[(size_t)i]);
      if (kind[(size_t)i] == cbbin::CUT) cut.push_back(inner[(size_t)i]);
    }
    std::vector<int64_t> dest;
    int64_t next_rows = 0;
    std::vector<cbbin::Node> next = cbbin::next_level(level, inner, kind, left.data(), right.data(), L, &dest, &next_rows);
    float *out = nullptr;
    if (next_rows > 0) {  // (before the cut fits: they read `cur` as well, nothing writes it -- and they take the workspace)
      vaqhost::DevBuf &nb = b_level[depth & 1];
      CB_TRY(nb.ensure((size_t)next_rows * L * sizeof(float)));
      out = nb.as<float>();
      CB_TRY(hipMemcpyAsync(b_dest.p, dest.data(), (size_t)F * sizeof(int64_t), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(cb_regroup_kernel, dim3((unsigned)(((int64_t)sp * L + 255) / 256)), dim3(256), 0, st, cur, L,
                         tabs.fits, b_dest.as<int64_t>(), work.keys_out, work.vals_out, (int64_t)sp, out);
      CB_TRY(hipGetLastError());
      CB_TRY(hipStreamSynchronize(st));  // (dest is the host's; the sorted pairs and the fit table have been read)
    }
    stats->split_ms += cb_ms_since(t0);

    // ---- the nodes the sizes cut: a flat fit of tempK centres each, over the matrix the level was fitted on ----
    if (!cut.empty()) {
      t0 = std::chrono::steady_clock::now();
      stats->cut_nodes += (int)cut.size();
      CB_TRY(run_fits(level, cbbin::make_fits(plan, level, cut, true, false, D, L, tile_rows), t0));
      stats->cut_ms += cb_ms_since(t0);
      if (*no_centre_out) break;
    }
    level.swap(next);
    cur = CbSources{{out, nullptr, nullptr}};
  }
  if (!stats->leaf_nodes) stats->min_leaf_rows = 0;
  stats->total_ms = cb_ms_since(began);
  if (phases) *phases = ph;
  sync_on_return.armed = false;
  return hipStreamSynchronize(st);
}
#undef CB_TRY

}  // namespace vaq
