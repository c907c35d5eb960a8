// vaq_fast.hip -- gfx950 kernels of the FAST search method (vaq_fast.h, DESIGN.md section "FAST").
//
// Per query chunk: smallQuantize the lookup tables to uint8, compute every row's integer distance as an
// int8 GEMM on the matrix cores (A = the rows' codes one-hot, B = the quantised tables - 128), then pick
// the k best by (dist, seq) with an exact histogram of the distances (they are integers <= 255 * M).
#include "vaq_fast.h"

#include <float.h>

namespace vaq {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

__global__ void fast_pack_kernel(const uint16_t *__restrict__ codes, int64_t row_begin, int64_t row_end, int M,
                                 uint32_t *__restrict__ out) {
  const int cw = fast_code_words(M);
  const int per_row = 4 * cw;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = row_begin + i / per_row;
  if (r >= row_end) return;
  const int h = (int)(i % per_row) / cw, w = (int)(i % per_row) % cw;
  const uint16_t *row = codes + (r - row_begin) * M;
  uint32_t x = 0;
  for (int n = 0; n < 8; n++) {
    const int s = 4 * (8 * w + n) + h;
    if (s < M) x |= (uint32_t)(row[s] & 15u) << (4 * n);
  }
  out[r * per_row + h * cw + w] = x;
}

__global__ void fast_quantize_kernel(const float *__restrict__ lut, int nq, int M, int ksub,
                                     const float *__restrict__ off, const float *__restrict__ scale,
                                     uint8_t *__restrict__ small) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nq * M * 16) return;
  const int c = (int)(i & 15);
  const int64_t qs = i >> 4;
  const int s = (int)(qs % M);
  uint8_t v = 0;
  if (c < ksub) {
    // (lut - off).max(0) * scale, floor, min 255, cast: four separate float32 steps (-ffp-contract=off)
    float x = lut[qs * ksub + c] - off[s];
    x = fmaxf(x, 0.0f);
    x = x * scale[s];
    x = fminf(floorf(x), 255.0f);
    v = (uint8_t)x;
  }
  small[i] = v;
}

// One workgroup: QT x 16 queries (their B fragments staged in LDS, lane-linear so that a wave reads them
// with conflict-free ds_read_b128) against a range of rows; each wave takes 2 x 16 rows at a time.
// v_mfma_i32_16x16x64_i8: lane l holds 16 bytes of A row (l & 15) and of B column (l & 15) for the same
// 16 k indices (group l >> 4); the result has col = l & 15, row = 4 (l >> 4) + reg.  Lane group h carries
// subspace 4t + h of step t: A = one-hot of the row's code, B = that query's 16 table entries - 128, so
// the step's sum over k is sum_h (small[4t + h][code] - 128) whichever order the bytes are in.
constexpr int FAST_QT = 4;
constexpr int FAST_RT = 2;
constexpr int FAST_WAVES = 4;

template <int CW>
__global__ void __launch_bounds__(64 * FAST_WAVES)
fast_scan_kernel(const uint32_t *__restrict__ codes, int64_t n_pad, int M, const uint8_t *__restrict__ small,
                 int nq, uint16_t *__restrict__ dist, int64_t rows_per_block) {
  extern __shared__ uint4 bimg[];  // [qt][t][lane] 16 bytes
  const int T = M / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.y * (FAST_QT * 16);
  // stage B: entry (qt, t, lane) = small[q0 + 16 qt + (lane & 15)][4t + (lane >> 4)][0..15] ^ 0x80 (= q - 128)
  for (int e = threadIdx.x; e < FAST_QT * T * 64; e += blockDim.x) {
    const int ln = e & 63, t = (e >> 6) % T, qt = (e >> 6) / T;
    const int q = q0 + qt * 16 + (ln & 15);
    uint4 v = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);  // absent query: zero table
    if (q < nq) v = *reinterpret_cast<const uint4 *>(small + ((int64_t)q * M + 4 * t + (ln >> 4)) * 16);
    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
    bimg[e] = v;
  }
  __syncthreads();
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r_end = r_begin + rows_per_block < n_pad ? r_begin + rows_per_block : n_pad;
  const int r16 = lane & 15, h = lane >> 4;
  const int bias = 128 * M;
  for (int64_t r0 = r_begin + (int64_t)wave * 16 * FAST_RT; r0 < r_end; r0 += (int64_t)FAST_WAVES * 16 * FAST_RT) {
    uint32_t cw[FAST_RT][CW];
#pragma unroll
    for (int rt = 0; rt < FAST_RT; rt++) {
      const uint32_t *p = codes + (r0 + rt * 16 + r16) * (4 * CW) + h * CW;
#pragma unroll
      for (int w = 0; w < CW; w++) cw[rt][w] = p[w];
    }
    v4i acc[FAST_QT][FAST_RT];
#pragma unroll
    for (int qt = 0; qt < FAST_QT; qt++)
#pragma unroll
      for (int rt = 0; rt < FAST_RT; rt++) acc[qt][rt] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < CW; w++) {
#pragma unroll
      for (int n = 0; n < 8; n++) {
        const int t = 8 * w + n;
        if (t >= T) break;  // uniform
        v4i a[FAST_RT];
#pragma unroll
        for (int rt = 0; rt < FAST_RT; rt++) {
          const uint32_t c = (cw[rt][w] >> (4 * n)) & 15u;
          const uint32_t one = 1u << ((c & 3u) << 3);
          const uint32_t d = c >> 2;
          a[rt] = v4i{(int)(d == 0 ? one : 0u), (int)(d == 1 ? one : 0u), (int)(d == 2 ? one : 0u),
                      (int)(d == 3 ? one : 0u)};
        }
#pragma unroll
        for (int qt = 0; qt < FAST_QT; qt++) {
          const uint4 bv = bimg[(qt * T + t) * 64 + lane];
          const v4i b = v4i{(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
#pragma unroll
          for (int rt = 0; rt < FAST_RT; rt++)
            acc[qt][rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rt], b, acc[qt][rt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int qt = 0; qt < FAST_QT; qt++) {
      const int q = q0 + qt * 16 + r16;
      if (q >= nq) continue;
#pragma unroll
      for (int rt = 0; rt < FAST_RT; rt++) {
        const int64_t row = r0 + rt * 16 + 4 * h;
        const uint32_t d0 = (uint32_t)(acc[qt][rt][0] + bias), d1 = (uint32_t)(acc[qt][rt][1] + bias);
        const uint32_t d2 = (uint32_t)(acc[qt][rt][2] + bias), d3 = (uint32_t)(acc[qt][rt][3] + bias);
        *reinterpret_cast<uint2 *>(dist + (int64_t)q * n_pad + row) = make_uint2(d0 | (d1 << 16), d2 | (d3 << 16));
      }
    }
  }
}

__global__ void fast_head_sort_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int nq, int kk,
                                      uint32_t *__restrict__ scratch, int64_t scratch_stride,
                                      uint16_t *__restrict__ order, int64_t order_stride) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  uint32_t *f = scratch + (int64_t)q * scratch_stride;
  for (int i = 0; i < kk; i++) f[i] = ((uint32_t)dist[(int64_t)q * n_pad + i] << 16) | (uint32_t)i;
  stdsort::sort(f, kk);
  for (int i = 0; i < kk; i++) order[(int64_t)q * order_stride + i] = (uint16_t)(f[i] & 0xffffu);
}

constexpr int SEL_THREADS = 1024;
constexpr int SEL_CAND = 4096;  // >= 3 * VAQHIP_MAX_K: rows below the cut + ties among rows < kk + ties after

// inclusive block-wide prefix sum of one int per thread (SEL_THREADS threads); returns the total too
__device__ inline int block_scan(int v, int *wsum, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int before = 0, tot = 0;
  for (int w = 0; w < SEL_THREADS / 64; w++) {
    const int s = wsum[w];
    if (w < wave) before += s;
    tot += s;
  }
  total = tot;
  return x + before;
}

// One workgroup per query.  Distances are integers in [0, 255 M]: a histogram in LDS gives tau, the
// kk-th smallest distance, and how many rows lie below it.  Only these rows can be among the kk best by
// (dist, seq): every row below tau, the rows < kk at tau (seq < kk), and the first rows >= kk at tau in
// row order (seq = row there).  They are sorted by (dist, seq) and the first kk written.
// TAIL (one shard of a sharded index): rows < skip are left out of all three passes, there is no `order`,
// every row's seq is the row, and kk = min(k, n - skip).
template <bool TAIL>
__global__ void __launch_bounds__(SEL_THREADS)
fast_select_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int64_t n, int k, int nbins,
                   const uint16_t *__restrict__ order, int kk, int64_t skip, int64_t id_base,
                   int32_t *__restrict__ labels, float *__restrict__ out_dist) {
  // the histogram and, once tau is known, the candidate keys (dist << 32 | seq) share the LDS
  extern __shared__ unsigned long long sel_smem[];
  unsigned *hist = reinterpret_cast<unsigned *>(sel_smem);
  unsigned long long *cand = sel_smem;
  __shared__ uint16_t inv[1024];  // row < kk -> its position in std::sort's output
  __shared__ int wsum[SEL_THREADS / 64];
  __shared__ int s_tau, s_below, s_count;
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  const uint16_t *d = dist + (int64_t)q * n_pad;
  const uint16_t *ord = TAIL ? nullptr : order + (int64_t)q * kk;
  const int hk = TAIL ? 0 : kk;  // rows whose seq comes from `order`
  int32_t *lab_out = labels + (int64_t)q * k;
  float *dist_out = out_dist + (int64_t)q * k;
  for (int i = kk + tid; i < k; i += SEL_THREADS) {
    lab_out[i] = -1;
    dist_out[i] = FLT_MAX;
  }
  if (kk == 0) return;
  for (int i = tid; i < nbins; i += SEL_THREADS) hist[i] = 0;
  if (!TAIL)
    for (int i = tid; i < kk; i += SEL_THREADS) inv[ord[i]] = (uint16_t)i;
  if (tid == 0) s_count = 0;
  __syncthreads();
  // 8 distances per 16-byte load (rows are padded to FAST_ROW_PAD, the row start is 64-byte aligned)
  const uint4 *d8 = reinterpret_cast<const uint4 *>(d);
  const int64_t n8 = (n + 7) / 8;
  // four loads in flight per lane before their values are used: the pass is latency-bound otherwise
  // (counters)
  for (int64_t v0 = tid; v0 < n8; v0 += 4 * SEL_THREADS) {
    uint4 w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t v = v0 + (int64_t)u * SEL_THREADS;
      w[u] = v < n8 ? d8[v] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t v = v0 + (int64_t)u * SEL_THREADS;
      const uint32_t ws[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (v * 8 + j < n && (!TAIL || v * 8 + j >= skip)) atomicAdd(&hist[min((int)((ws[j >> 1] >> (16 * (j & 1))) & 0xffffu), nbins - 1)], 1u);
    }
  }
  __syncthreads();
  const int per = (nbins + SEL_THREADS - 1) / SEL_THREADS;
  const int b0 = min(nbins, tid * per), b1 = min(nbins, b0 + per);
  int mine = 0;
  for (int b = b0; b < b1; b++) mine += (int)hist[b];
  int total;
  const int incl = block_scan(mine, wsum, total);
  int run = incl - mine;
  if (run < kk && incl >= kk) {  // exactly one thread
    for (int b = b0; b < b1; b++) {
      if (run + (int)hist[b] >= kk) {
        s_tau = b;
        s_below = run;
        break;
      }
      run += (int)hist[b];
    }
  }
  __syncthreads();  // the histogram is dead from here on: cand overwrites it
  const int tau = s_tau, need = kk - s_below;
  for (int64_t v0 = tid; v0 < n8; v0 += 4 * SEL_THREADS) {
    uint4 w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t v = v0 + (int64_t)u * SEL_THREADS;
      w[u] = v < n8 ? d8[v] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 32; j++) {
      const int64_t i = (v0 + (int64_t)(j >> 3) * SEL_THREADS) * 8 + (j & 7);
      const uint32_t ws[4] = {w[j >> 3].x, w[j >> 3].y, w[j >> 3].z, w[j >> 3].w};
      const int di = (int)((ws[(j & 7) >> 1] >> (16 * (j & 1))) & 0xffffu);
      if (i < n && (!TAIL || i >= skip) && (di < tau || (di == tau && i < hk))) {
        const unsigned seq = i < hk ? (unsigned)inv[i] : (unsigned)i;
        const int slot = atomicAdd(&s_count, 1);
        if (slot < 2 * kk) cand[slot] = ((unsigned long long)di << 32) | seq;
      }
    }
  }
  __syncthreads();
  int count = min(s_count, 2 * kk);  // < kk rows below tau + <= kk rows < kk at tau
  // the first `need` rows >= kk at tau, in row order
  int taken = 0;
  for (int64_t base = TAIL ? skip : (int64_t)kk; base < n && taken < need; base += SEL_THREADS) {
    const int64_t i = base + tid;
    const int flag = (i < n && d[i] == tau) ? 1 : 0;
    int tot;
    const int pos = block_scan(flag, wsum, tot) - flag;
    if (flag && taken + pos < need) cand[count + taken + pos] = ((unsigned long long)tau << 32) | (unsigned)i;
    taken += tot;  // uniform
  }
  count += min(taken, need);
  __syncthreads();
  int P = 1;
  while (P < count) P <<= 1;
  for (int i = count + tid; i < P; i += SEL_THREADS) cand[i] = ~0ull;
  __syncthreads();
  // bitonic sort of P <= SEL_CAND keys
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P / 2; i += SEL_THREADS) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = cand[lo], b = cand[hi];
        if ((a > b) == up) {
          cand[lo] = b;
          cand[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < kk; i += SEL_THREADS) {
    const unsigned long long key = cand[i];
    const unsigned seq = (unsigned)key;
    const int64_t row = seq < (unsigned)hk ? (int64_t)ord[seq] : (int64_t)seq;
    lab_out[i] = (int32_t)(id_base + row);
    dist_out[i] = (float)(unsigned)(key >> 32);
  }
}

__global__ void fast_head_copy_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int nq, int h,
                                      uint16_t *__restrict__ out, int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nq * h) return;
  const int64_t q = i / h, p = i % h;
  out[q * out_stride + p] = dist[q * n_pad + p];
}

__global__ void fast_head_gather_kernel(const uint16_t *__restrict__ planes, int64_t plane_stride, FastHeadParts parts,
                                        int nq, int kk, uint16_t *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nq * kk) return;
  const int p = (int)(i % kk);
  int g = 0;
  while (g + 1 < parts.n_parts && p >= parts.start[g + 1]) g++;  // (a part without head rows owns nothing)
  head[i] = planes[(int64_t)g * plane_stride + i];
}

// One workgroup per query (a few KiB of LDS at k = 100: eight workgroups, 32 waves, per CU).  The lists'
// distances sit in LDS as uint16, 0xffff = no entry, every list padded to k slots; the lists are ascending, so
// the place of entry p of list l in the stable merge is p + the entries of earlier lists <= its distance + the
// entries of later lists < it: one binary search per other list.  The places are a permutation, so every
// output slot below the number of entries is written exactly once, and equal distances need no special case.
constexpr int MERGE_THREADS = 256;
__global__ void __launch_bounds__(MERGE_THREADS)
fast_merge_kernel(const uint32_t *head_sorted, int64_t head_stride, int kk, int64_t head_label_base,
                  const float *__restrict__ dist_lists, const int32_t *__restrict__ label_lists, int n_lists,
                  int64_t list_stride, int64_t query_stride, int k, int32_t *labels, float *out_dist) {
  extern __shared__ uint16_t mg_d[];  // [1 + n_lists][k] distances, then the head rows [kk]
  __shared__ int s_total;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int L = n_lists + 1;
  uint16_t *hrow = mg_d + (size_t)L * k;
  if (tid == 0) s_total = 0;
  int mine = 0;
  for (int i = tid; i < k; i += MERGE_THREADS) {
    uint16_t d = 0xffffu;
    if (i < kk) {
      const uint32_t item = head_sorted[(int64_t)q * head_stride + i];
      d = (uint16_t)(item >> 16);
      hrow[i] = (uint16_t)(item & 0xffffu);
      mine++;
    }
    mg_d[i] = d;
  }
  for (int e = tid; e < n_lists * k; e += MERGE_THREADS) {
    const int l = e / k, i = e % k;
    const int64_t at = (int64_t)l * list_stride + (int64_t)q * query_stride + i;
    uint16_t d = 0xffffu;
    if (label_lists[at] >= 0) {
      d = (uint16_t)fminf(fmaxf(dist_lists[at], 0.0f), 65534.0f);
      mine++;
    }
    mg_d[k + e] = d;
  }
  __syncthreads();  // head_sorted (which may be this query's row of `labels`) is not read after this point
  if (mine) atomicAdd(&s_total, mine);
  for (int e = tid; e < L * k; e += MERGE_THREADS) {
    const int l = e / k, p = e % k;
    const uint32_t d = mg_d[e];
    if (d == 0xffffu) continue;
    int place = p;
    for (int l2 = 0; l2 < L && place < k; l2++) {
      if (l2 == l) continue;
      const uint16_t *a = mg_d + (size_t)l2 * k;
      const uint32_t t = d + (l2 < l ? 1u : 0u);  // entries below t: <= d in an earlier list, < d in a later one
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < t) lo = mid + 1;
        else hi = mid;
      }
      place += lo;
    }
    if (place < k) {
      labels[(int64_t)q * k + place] =
          l == 0 ? (int32_t)(head_label_base + hrow[p])
                 : label_lists[(int64_t)(l - 1) * list_stride + (int64_t)q * query_stride + p];
      out_dist[(int64_t)q * k + place] = (float)d;
    }
  }
  __syncthreads();
  for (int i = min(s_total, k) + tid; i < k; i += MERGE_THREADS) {
    labels[(int64_t)q * k + i] = -1;
    out_dist[(int64_t)q * k + i] = FLT_MAX;
  }
}

}  // namespace

hipError_t launch_fast_pack_codes(const uint16_t *codes_u16, int64_t row_begin, int64_t row_end, int M,
                                  uint32_t *out, hipStream_t st) {
  const int64_t n = (row_end - row_begin) * 4 * fast_code_words(M);
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fast_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, codes_u16, row_begin,
                     row_end, M, out);
  return hipGetLastError();
}

hipError_t launch_fast_quantize(const float *lut_ref, int nq, int M, int ksub, const float *offsets,
                                const float *scale, uint8_t *small, hipStream_t st) {
  const int64_t n = (int64_t)nq * M * 16;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fast_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, lut_ref, nq, M,
                     ksub, offsets, scale, small);
  return hipGetLastError();
}

template <int CW>
static hipError_t scan_cw(const uint32_t *codes, int64_t n_pad, int M, const uint8_t *small, int nq,
                          uint16_t *dist, int n_cu, hipStream_t st) {
  const int qgroups = (nq + FAST_QT * 16 - 1) / (FAST_QT * 16);
  const size_t lds = (size_t)FAST_QT * (M / 4) * 64 * 16;
  // about four workgroups per CU in all, each a multiple of one workgroup step of rows
  const int64_t step = 16 * FAST_RT * FAST_WAVES;
  int64_t blocks = std::max<int64_t>(1, (int64_t)4 * n_cu / qgroups);
  int64_t rows = (n_pad + blocks - 1) / blocks;
  rows = std::max<int64_t>(step, (rows + step - 1) / step * step);
  blocks = (n_pad + rows - 1) / rows;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fast_scan_kernel<CW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fast_scan_kernel<CW>, dim3((unsigned)blocks, (unsigned)qgroups), dim3(64 * FAST_WAVES), lds, st,
                     codes, n_pad, M, small, nq, dist, rows);
  return hipGetLastError();
}

hipError_t launch_fast_scan(const uint32_t *codes, int64_t n_pad, int M, const uint8_t *small, int nq,
                            uint16_t *dist, int n_cu, hipStream_t st) {
  if (nq <= 0 || n_pad <= 0) return hipSuccess;
  if (n_pad % FAST_ROW_PAD != 0 || M % 4 != 0 || M > 128) return hipErrorInvalidValue;
  switch (fast_code_words(M)) {
    case 1: return scan_cw<1>(codes, n_pad, M, small, nq, dist, n_cu, st);
    case 2: return scan_cw<2>(codes, n_pad, M, small, nq, dist, n_cu, st);
    case 3: return scan_cw<3>(codes, n_pad, M, small, nq, dist, n_cu, st);
    default: return scan_cw<4>(codes, n_pad, M, small, nq, dist, n_cu, st);
  }
}

hipError_t launch_fast_head_sort(const uint16_t *dist, int64_t n_pad, int nq, int kk, uint32_t *scratch,
                                 uint16_t *order, hipStream_t st) {
  if (nq <= 0 || kk <= 0) return hipSuccess;
  if (kk > 1024) return hipErrorInvalidValue;
  return launch_fast_head_sort_strided(dist, n_pad, nq, kk, scratch, kk, order, kk, st);
}

hipError_t launch_fast_head_sort_strided(const uint16_t *dist, int64_t dist_stride, int nq, int kk, uint32_t *scratch,
                                         int64_t scratch_stride, uint16_t *order, int64_t order_stride, hipStream_t st) {
  if (nq <= 0 || kk <= 0) return hipSuccess;
  if (kk > 1024 || scratch_stride < kk || order_stride < kk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fast_head_sort_kernel, dim3((nq + 63) / 64), dim3(64), 0, st, dist, dist_stride, nq, kk, scratch,
                     scratch_stride, order, order_stride);
  return hipGetLastError();
}

hipError_t launch_fast_select(const uint16_t *dist, int64_t n_pad, int64_t n, int nq, int k, int M,
                              const uint16_t *order, int64_t id_base, int32_t *labels, float *out_dist,
                              hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (k > 1024 || 3 * k > SEL_CAND) return hipErrorInvalidValue;
  const int kk = (int)std::min<int64_t>(k, n);
  const int nbins = 255 * M + 1;
  const size_t lds = std::max<size_t>((size_t)nbins * 4, (size_t)SEL_CAND * 8);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fast_select_kernel<false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fast_select_kernel<false>, dim3(nq), dim3(SEL_THREADS), lds, st, dist, n_pad, n, k, nbins, order,
                     kk, (int64_t)0, id_base, labels, out_dist);
  return hipGetLastError();
}

hipError_t launch_fast_select_tail(const uint16_t *dist, int64_t n_pad, int64_t n, int64_t head_rows, int nq, int k,
                                   int M, int64_t id_base, int32_t *labels, float *out_dist, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (k <= 0 || k > 1024 || 3 * k > SEL_CAND || head_rows < 0 || head_rows > n) return hipErrorInvalidValue;
  const int kk = (int)std::min<int64_t>(k, n - head_rows);
  const int nbins = 255 * M + 1;
  const size_t lds = std::max<size_t>((size_t)nbins * 4, (size_t)SEL_CAND * 8);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fast_select_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fast_select_kernel<true>, dim3(nq), dim3(SEL_THREADS), lds, st, dist, n_pad, n, k, nbins,
                     (const uint16_t *)nullptr, kk, head_rows, id_base, labels, out_dist);
  return hipGetLastError();
}

hipError_t launch_fast_head_copy(const uint16_t *dist, int64_t n_pad, int nq, int h, uint16_t *out,
                                 int64_t out_stride, hipStream_t st) {
  if (nq <= 0 || h <= 0) return hipSuccess;
  if (h > n_pad || out_stride < h) return hipErrorInvalidValue;
  const int64_t n = (int64_t)nq * h;
  hipLaunchKernelGGL(fast_head_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dist, n_pad, nq, h, out,
                     out_stride);
  return hipGetLastError();
}

hipError_t launch_fast_head_gather(const uint16_t *planes, int64_t plane_stride, FastHeadParts parts, int nq, int kk,
                                   uint16_t *head, hipStream_t st) {
  if (nq <= 0 || kk <= 0) return hipSuccess;
  if (parts.n_parts < 1 || parts.n_parts > FAST_MAX_LISTS || parts.start[0] != 0 || parts.start[parts.n_parts] != kk)
    return hipErrorInvalidValue;
  for (int g = 0; g < parts.n_parts; g++)
    if (parts.start[g] > parts.start[g + 1]) return hipErrorInvalidValue;
  const int64_t n = (int64_t)nq * kk;
  hipLaunchKernelGGL(fast_head_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, planes, plane_stride,
                     parts, nq, kk, head);
  return hipGetLastError();
}

hipError_t launch_fast_merge(const uint32_t *head_sorted, int64_t head_stride, int kk, int64_t head_label_base,
                             const float *dist_lists, const int32_t *label_lists, int n_lists, int64_t list_stride,
                             int64_t query_stride, int nq, int k, int32_t *labels, float *out_dist, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (k <= 0 || k > 1024 || kk < 0 || kk > k || n_lists < 0 || n_lists > FAST_MAX_LISTS) return hipErrorInvalidValue;
  const size_t lds = ((size_t)(n_lists + 1) * k + kk) * sizeof(uint16_t);  // <= 36 KiB
  hipLaunchKernelGGL(fast_merge_kernel, dim3(nq), dim3(MERGE_THREADS), lds, st, head_sorted, head_stride, kk,
                     head_label_base, dist_lists, label_lists, n_lists, list_stride, query_stride, k, labels, out_dist);
  return hipGetLastError();
}

}  // namespace vaq
