// vaq_exact.hip -- the reference's own choice among rows of EQUAL distance (option "exact_ties").
//
// VAQ::searchHeap (VAQ.cpp:1729-1758) keeps its k best in a binary max-heap (utils/Heap.hpp:115-169:
// pop takes the RIGHT child on equal children, push sifts up on strict >) and admits row i iff
// heap_top > dist_i, rows in ORIGINAL order.  Which of several rows tying at the k-th distance
// survive, and the order heap_reorder (:322-349) returns equal distances in, depend on the heap's
// shape, i.e. on every row it ever admitted -- a rule of the form "smallest label wins" (the scan
// kernels' order) cannot reproduce it.  So for the queries that HAVE ties the admission sequence is
// replayed:
//   exact_flag_kernel    the scan ran with k + 1: a query whose k + 1 smallest distances are all
//                        distinct has a unique answer, already in heap_reorder's order -- copied out.
//                        Any two equal neighbours (inside the top k, or the k-th and the (k+1)-th:
//                        a boundary tie) put the query on the replay list.
//   exact_replay_kernel  one workgroup per listed query walks the rows in ORIGINAL order (through the
//                        inverse of the bucketed order's permutation).  Waves 1.. evaluate a chunk of
//                        consecutive rows -- the complete row sum in the reference's order, abandoned
//                        once a partial sum reaches the heap top (VAQ::searchEarlyAbandon's test, :1708)
//                        -- into an LDS buffer; wave 0 meanwhile replays the PREVIOUS chunk: 64 rows at
//                        a time, ballot of dist < top, and for each set bit in row order the reference's
//                        own statements: if (top > dist) { heap_pop; heap_push }.  The top the evaluating
//                        waves abandon against is always one the heap had BEFORE the rows they look at,
//                        so nothing the reference would admit is ever dropped.  At the end heap_reorder.
// Across the shards of a multi-device index (vaqhip_multi_search.cpp) the replay is a CHAIN: shards are
// contiguous label ranges in label order, so the reference's heap after the rows of shards 0..g is shard
// g's replay started from the heap (values and ids, raw layout) shards 0..g-1 left behind.  A chain link
// (ExactParams::chain) takes that state instead of heap_heapify's neutral one, pushes GLOBAL row numbers
// (the state travels), and writes the raw heap out again; exact_finish_kernel runs heap_reorder on the
// state the last shard left.  The bucket-bound skip and the early abandon test against a top that is
// never below the reference's at that row -- the inherited top IS the reference's top there.
// The heap functions are the reference's (utils/Heap.hpp), statement for statement: refheap:: in
// vaq_restated.h, pinned on the CPU against oracle/vaq_oracle.c's (tests/cpp/refheap_test.cpp) -- which is
// pinned against the compiled reference heap (tests/test_oracle_golden.py).
//
// Sequential-sum indexes (BitVecEngine::queryLUT, BitVecEngine.hpp:1282-1317) keep their k best under
// libstdc++'s heap functions instead: with pairs empty and bsfK = FLT_MAX, row i (ORIGINAL order, dist the
// sequential column sum) is taken iff dist < bsfK: emplace_back + std::push_heap, and for i >= k also
// std::pop_heap + pop_back + bsfK = front().dist; std::sort_heap at the end.  The first k rows enter
// unconditionally, row k meets a full heap (k + 1 slots are needed), i is the row's position in the WHOLE
// database.  The same pipeline replays it (template argument SEQ): the heap is k + 1 pairs under
// stdheap:: (vaq_restated.h, pinned against the real functions by tests/cpp/stdheap_test.cpp), the state of a
// chain link is the raw heap, its length and bsfK, and the links count i from ExactParams::row0.  The
// loop's partial-sum abandon only drops rows the test dist < bsfK drops (table entries are >= 0), so the
// evaluating waves abandon and skip buckets against bsfK exactly as they do against the heap top.
#include "vaq_exact.h"
#include "vaq_restated.h"
#include "vaq_scan.h"

namespace vaq {

constexpr int EX_THREADS = 512;
constexpr int EX_CHUNK = 2048;  // rows per chunk (a multiple of 64)

// the block's threads write query q's k output slots: the kept entries hval / hid[first, first + kept) with
// id_add added to the ids, then the -1 / FLT_MAX tail
__device__ __forceinline__ void ex_write_out(int32_t *labels, float *dist, const int q, const int k, const float *hval,
                                             const int *hid, const int first, const int kept, const int64_t id_add,
                                             const int tid, const int nthreads) {
  for (int i = tid; i < k; i += nthreads) {
    const bool ok = i < kept;
    labels[(size_t)q * k + i] = ok ? (int32_t)(hid[first + i] + id_add) : -1;
    dist[(size_t)q * k + i] = ok ? hval[first + i] : FLT_MAX;
  }
}

// heap_reorder by thread 0, then the output slots (the tail is refilled with FLT_MAX / -1).  Ends with the
// block's threads past a barrier on *s_kept.
__device__ __forceinline__ void ex_reorder_out(int32_t *labels, float *dist, const int q, const int k, float *hval,
                                               int *hid, const int64_t id_add, int *s_kept, const int tid,
                                               const int nthreads) {
  if (tid == 0) *s_kept = refheap::reorder(k, hval, hid);
  __syncthreads();
  const int kept = *s_kept;
  ex_write_out(labels, dist, q, k, hval, hid, k - kept, kept, id_add, tid, nthreads);
}

// std::sort_heap (BitVecEngine.hpp:1316) by thread 0: ascending from slot 0; at most k pairs are left
__device__ __forceinline__ void ex_sort_out(int32_t *labels, float *dist, const int q, const int k, float *hval, int *hid,
                                            const int len, const int64_t id_add, const int tid, const int nthreads) {
  if (tid == 0) stdheap::sort_heap(hval, hid, len);
  __syncthreads();
  ex_write_out(labels, dist, q, k, hval, hid, 0, len, id_add, tid, nthreads);
}

// A list entry's state in a chain (ExactParams::chain) into the heap's slots, by the block's threads; sin ==
// nullptr: heap_heapify's neutral state (utils/Heap.hpp:211-235: FLT_MAX, ids -1; sequential sum: `pairs` empty
// and bsfK = FLT_MAX, BitVecEngine.hpp:1287-1290 -- slots past the length are never read).
template <bool SEQ>
__device__ __forceinline__ void ex_state_load(const int32_t *sin, const int k, float *hval, int *hid, const int tid,
                                              const int nthreads, int *len, float *bsf) {
  const int hs = SEQ ? k + 1 : k;
  for (int i = tid; i < hs; i += nthreads) {
    hval[i] = sin ? bits_to_float((unsigned)sin[i]) : FLT_MAX;
    hid[i] = sin ? sin[hs + i] : -1;
  }
  // (the clamp is defensive only: a length outside [0, k] can only come from a bug in an earlier link, and
  //  it keeps such a bug from writing outside the heap's slots -- it does not make the answer right)
  *len = SEQ && sin ? min(max(sin[2 * hs], 0), k) : 0;                      // pairs.size()
  *bsf = SEQ && sin ? bits_to_float((unsigned)sin[2 * hs + 1]) : FLT_MAX;  // bsfK
}

// ... and the raw heap back out
template <bool SEQ>
__device__ __forceinline__ void ex_state_store(int32_t *sout, const int k, const float *hval, const int *hid,
                                               const int tid, const int nthreads, const int len, const float bsf) {
  const int hs = SEQ ? k + 1 : k;
  for (int i = tid; i < hs; i += nthreads) {
    sout[i] = (int32_t)float_to_bits(hval[i]);
    sout[hs + i] = hid[i];
  }
  if (SEQ && tid == 0) {
    sout[2 * hs] = len;
    sout[2 * hs + 1] = (int32_t)float_to_bits(bsf);
  }
}

__global__ __launch_bounds__(256) void exact_flag_kernel(const int nq, const int k, const int32_t *__restrict__ in_labels,
                                                          const float *__restrict__ in_dist, int32_t *__restrict__ labels,
                                                          float *__restrict__ dist, int *__restrict__ list,
                                                          unsigned *__restrict__ count) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= nq) return;
  const int k1 = k + 1;
  const int32_t *il = in_labels + (size_t)q * k1;
  const float *id = in_dist + (size_t)q * k1;
  bool tie = false;
  for (int i = lane; i < k; i += 64) {
    const int32_t a = il[i], b = il[i + 1];
    tie = tie || (a >= 0 && b >= 0 && id[i] == id[i + 1]);
    labels[(size_t)q * k + i] = a;
    dist[(size_t)q * k + i] = id[i];
  }
  if (__ballot(tie) != 0ull && lane == 0) list[atomicAdd(count, 1u)] = q;
}

// complete sum of sorted row r, abandoned (-> +inf) once a partial sum is no longer below t: in the
// reference's order (groups of four, each added to the sum and tested, VAQ.cpp:1737-1748), or with SEQ the
// sequential sum (BitVecEngine.hpp:1295-1300: dist += luts[code], column by column, tested after each as the
// loop's own condition does)
template <bool BYTES, bool SEQ>
__device__ __forceinline__ float ex_row_dist(const ExactParams &p, const float *lut, const int64_t r, const float t) {
  float dist = 0.0f;
  if (BYTES) {
    const int WPR = p.M / 4;
    const uint32_t *rp = p.codes + r * WPR;
    for (int g = 0; g < WPR; g++) {
      const uint32_t c4 = rp[g];
      float dism = lut[(g * 4 + 0) * 256 + (c4 & 0xffu)];
      dism += lut[(g * 4 + 1) * 256 + ((c4 >> 8) & 0xffu)];
      dism += lut[(g * 4 + 2) * 256 + ((c4 >> 16) & 0xffu)];
      dism += lut[(g * 4 + 3) * 256 + (c4 >> 24)];
      dist = g == 0 ? dism : dist + dism;
      if (!(dist < t)) return INFINITY;
    }
    return dist;
  }
  const int W = p.W;
  const uint32_t *tp = p.codes + (r / TILE_ROWS) * (int64_t)(TILE_ROWS * W) + (r % TILE_ROWS);
  float dism = 0.0f;
  for (int s = 0; s < p.M; s++) {
    const SubDesc d = p.sub[s];
    const uint32_t lo = tp[(int64_t)d.word * TILE_ROWS];
    const uint32_t hi = d.word + 1 < W ? tp[(int64_t)(d.word + 1) * TILE_ROWS] : 0u;
    const uint32_t c = __builtin_amdgcn_alignbit(hi, lo, (unsigned)d.shift) & ((1u << d.bits) - 1u);
    const float l = lut[d.lut_off + c];
    if (SEQ) {
      dist = s == 0 ? l : dist + l;
      if (!(dist < t)) return INFINITY;
    } else {
      dism = (s & 3) == 0 ? l : dism + l;
      if ((s & 3) == 3) {
        dist = s == 3 ? dism : dist + dism;
        if (!(dist < t)) return INFINITY;
      }
    }
  }
  return dist;
}

template <bool BYTES, bool SEQ>
__global__ __launch_bounds__(EX_THREADS) void exact_replay_kernel(ExactParams p) {
  static_assert(!(BYTES && SEQ), "sequential-sum rows are always bit-packed");
  extern __shared__ __attribute__((aligned(16))) unsigned char ex_smem[];
  const int e = p.e0 + blockIdx.x;
  if ((unsigned)e >= *p.count) return;
  const int q = p.list[e];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = p.k;
  const int hs = SEQ ? k + 1 : k;  // heap slots
  // LDS: heap values, heap ids, two chunk buffers, [the query's lookup tables]
  float *hval = reinterpret_cast<float *>(ex_smem);
  int *hid = reinterpret_cast<int *>(hval + hs);
  float *buf = reinterpret_cast<float *>(hid + hs);  // [2][EX_CHUNK]
  float *lbound = buf + 2 * EX_CHUNK;              // [n_buckets] lower bound of the row sums of each bucket (row_bucket)
  float *lds_lut = lbound + (p.row_bucket ? p.n_buckets : 0);
  const float *glut = p.lut + (size_t)q * p.lut_floats;
  const float *lut = glut;
  if (p.lut_in_lds && p.n_rows > 0) {  // (an empty shard has built no tables)
    for (int i = tid; i < p.lut_floats; i += EX_THREADS) lds_lut[i] = glut[i];
    lut = lds_lut;
  }
  // the neutral heap -- or the one the earlier shards left
  const int32_t *sin = p.chain && p.state_in ? p.state_in + (size_t)e * exact_state_words(k, SEQ) : nullptr;
  int len;    // pairs.size()
  float bsf;  // bsfK
  ex_state_load<SEQ>(sin, k, hval, hid, tid, EX_THREADS, &len, &bsf);
  // ids pushed: rows of this index (id_base is added on the way out), or global row numbers in a chain
  const int64_t push_base = p.chain ? p.id_base : 0;
  // the heap top after the last COMPLETE pop + push, for the evaluating waves (the root itself passes
  // through values below the new top while a pop is under way)
  __shared__ float s_top;
  __shared__ unsigned s_gmin[1 << GMIN_MAX_BITS];
  if (tid == 0) s_top = SEQ ? bsf : (sin ? bits_to_float((unsigned)sin[0]) : FLT_MAX);
  if (p.row_bucket) {
    // Per bucket the smallest sum its rows can have -- the first table term, plus the smallest second
    // term of the bucket's group of second codes, or the minimum over a coarse bucket's first codes:
    // the bound the scan kernels order the buckets by.  A row whose bucket's bound is not below the
    // heap top cannot be admitted (every further term is >= 0 and fp32 addition is monotone), so its
    // codes are not even read.
    const int bt = p.bucket_t, bsh = p.bucket_shift;
    if (tid < (1 << GMIN_MAX_BITS)) s_gmin[tid] = 0x7f800000u;
    __syncthreads();
    if (bt > 0) {
      const int off1 = p.sub[1].lut_off, n1 = p.sub[1].ncent;
      const int w = 31 - __builtin_clz((unsigned)n1) - bt;
      for (int e = tid; e < n1; e += EX_THREADS) atomicMin(&s_gmin[e >> w], float_to_bits(glut[off1 + e]));
      __syncthreads();
    }
    for (int b = tid; b < p.n_buckets; b += EX_THREADS) {
      float m;
      if (bt > 0) {
        m = glut[b >> bt] + bits_to_float(s_gmin[b & ((1 << bt) - 1)]);
      } else {
        m = INFINITY;
        for (int c = b << bsh; c < ((b + 1) << bsh); c++) {
          const float x = glut[c];
          m = x < m ? x : m;
        }
      }
      lbound[b] = m == m ? m : -INFINITY;  // (a NaN table: never prune by it)
    }
  }
  __syncthreads();
  const int64_t N = p.n_rows;
  const int64_t nchunks = (N + EX_CHUNK - 1) / EX_CHUNK;
  for (int64_t c = 0; c <= nchunks; c++) {
    if (wave > 0) {
      if (c < nchunks) {
        // (the top as it is NOW: the heap has only seen rows before this chunk, so it is at least the
        //  top any row of the chunk will meet -- an admissible row is never abandoned)
        const float t = __hip_atomic_load(&s_top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        float *out = buf + (c & 1) * EX_CHUNK;
        constexpr int RPT = (EX_CHUNK + EX_THREADS - 64 - 1) / (EX_THREADS - 64);
        // first the cheap test for all of the thread's rows (one coalesced halfword + one LDS word each),
        // then the gathers of the survivors, all issued before the first sum
        bool live[RPT];
        int64_t src[RPT];
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const int j = tid - 64 + i * (EX_THREADS - 64);
          const int64_t row = c * EX_CHUNK + j;
          live[i] = j < EX_CHUNK && row < N;
          if (live[i] && p.row_bucket) live[i] = lbound[p.row_bucket[row]] < t;
        }
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const int64_t row = c * EX_CHUNK + (tid - 64 + i * (EX_THREADS - 64));
          src[i] = live[i] ? (p.inv ? (int64_t)p.inv[row] : row) : 0;
        }
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const int j = tid - 64 + i * (EX_THREADS - 64);
          if (j < EX_CHUNK)
            out[j] = !live[i] ? INFINITY : ex_row_dist<BYTES, SEQ>(p, lut, src[i], t);
        }
      }
    } else if (c > 0) {
      // wave 0: the previous chunk through the reference's loop (VAQ.cpp:1750-1753), 64 rows at a time
      const float *in = buf + ((c - 1) & 1) * EX_CHUNK;
      const int64_t base = (c - 1) * EX_CHUNK;
      if constexpr (SEQ) {
        for (int j0 = 0; j0 < EX_CHUNK; j0 += 64) {
          // BitVecEngine.hpp:1301-1311: rows past the end and abandoned rows are +inf, never below bsfK
          const float d = in[j0 + lane];
          unsigned long long m = __ballot(d < bsf);
          while (m != 0ull) {
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            const float dv = bits_to_float((unsigned)__builtin_amdgcn_readlane((int)float_to_bits(d), src));
            if (dv < bsf) {  // if (dist < bsfK)
              const bool full = p.row0 + base + j0 + src >= k;  // if (dataIndex >= k)
              if (lane == 0) {
                hval[len] = dv;
                hid[len] = (int)(push_base + base + j0 + src);
                stdheap::push_heap(hval, hid, len + 1);
                if (full) stdheap::pop_heap(hval, hid, len + 1);  // (pop_back: the length stays)
              }
              wave_lds_sync();
              if (full) {
                bsf = hval[0];
                if (lane == 0) __hip_atomic_store(&s_top, bsf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                m &= __ballot(d < bsf);  // (rows the new bsfK already excludes)
              } else {
                len++;
              }
            }
          }
        }
      } else {
        for (int j0 = 0; j0 < EX_CHUNK; j0 += 64) {
          const float d = in[j0 + lane];
          float top = hval[0];
          unsigned long long m = __ballot(d < top);
          while (m != 0ull) {
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            const float dv = bits_to_float((unsigned)__builtin_amdgcn_readlane((int)float_to_bits(d), src));
            if (top > dv) {  // if (heap_dis[0] > dist)
              if (lane == 0) {
                refheap::pop(k, hval, hid);
                refheap::push(k, hval, hid, dv, (int)(push_base + base + j0 + src));
                __hip_atomic_store(&s_top, hval[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              }
              wave_lds_sync();
              top = hval[0];
              m &= __ballot(d < top);  // (rows the new top already excludes)
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (SEQ) {
    // the length and bsfK live in wave 0; the chunk buffers are free (the loop above ended with a barrier)
    if (tid == 0) {
      reinterpret_cast<int *>(buf)[0] = len;
      buf[1] = bsf;
    }
    __syncthreads();
    len = reinterpret_cast<int *>(buf)[0];
    bsf = buf[1];
    __syncthreads();
  }
  if (p.chain) {
    // a link hands the raw heap on (the loop above ended with a barrier)
    ex_state_store<SEQ>(p.state_out + (size_t)e * exact_state_words(k, SEQ), k, hval, hid, tid, EX_THREADS, len, bsf);
    return;
  }
  if (SEQ) ex_sort_out(p.labels, p.dist, q, k, hval, hid, len, p.id_base, tid, EX_THREADS);
  else ex_reorder_out(p.labels, p.dist, q, k, hval, hid, p.id_base, reinterpret_cast<int *>(buf), tid, EX_THREADS);
}

// End of a chain: heap_reorder on the state the last shard left, into the caller's slots of the listed
// queries.  One wave per list entry; the ids are global already.
template <bool SEQ>
__global__ __launch_bounds__(64) void exact_finish_kernel(const int32_t *__restrict__ state, const int *__restrict__ list,
                                                          const unsigned *__restrict__ count, int k,
                                                          int32_t *__restrict__ labels, float *__restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ex_smem[];
  const int e = blockIdx.x, lane = threadIdx.x;
  if ((unsigned)e >= *count) return;
  const int q = list[e];
  const int hs = SEQ ? k + 1 : k;
  float *hval = reinterpret_cast<float *>(ex_smem);
  int *hid = reinterpret_cast<int *>(hval + hs);
  int len;
  float bsf;
  ex_state_load<SEQ>(state + (size_t)e * exact_state_words(k, SEQ), k, hval, hid, lane, 64, &len, &bsf);
  __shared__ int s_nel;
  __syncthreads();
  if (SEQ) ex_sort_out(labels, dist, q, k, hval, hid, len, 0, lane, 64);
  else ex_reorder_out(labels, dist, q, k, hval, hid, 0, &s_nel, lane, 64);
}

// inv[original row] = row of the bucketed order; row_bucket[original row] = its bucket (optional)
__global__ void inverse_perm_kernel(const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ inv,
                                    const int *__restrict__ bucket_start, int n_buckets,
                                    unsigned short *__restrict__ row_bucket) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t lab = perm ? perm[r] : (uint32_t)r;
  inv[lab] = (uint32_t)r;
  if (row_bucket) {
    int lo = 0, hi = n_buckets;  // largest b with bucket_start[b] <= r
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)bucket_start[mid] <= r) lo = mid;
      else hi = mid;
    }
    row_bucket[lab] = (unsigned short)lo;
  }
}

hipError_t launch_inverse_perm(const uint32_t *perm, int64_t n, uint32_t *inv, const int *bucket_start, int n_buckets,
                               unsigned short *row_bucket, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(inverse_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, perm, n, inv, bucket_start,
                     n_buckets, row_bucket);
  return hipGetLastError();
}

// a launch with dynamic LDS beyond the default limit
template <class... P, class... A>
static hipError_t launch_lds(void (*kernel)(P...), int grid, int threads, size_t lds, hipStream_t st, const A &...args) {
  const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
  return hipGetLastError();
}

// `fixed` bytes of LDS, plus the query's lookup tables if both fit in 96 KiB (*lut_in_lds)
static size_t lds_with_tables(size_t fixed, int lut_floats, int *lut_in_lds) {
  const size_t tables = (size_t)lut_floats * 4;
  *lut_in_lds = tables + fixed <= 96 * 1024 ? 1 : 0;
  return *lut_in_lds ? fixed + tables : fixed;
}

hipError_t launch_exact_flag(int nq, int k, const int32_t *in_labels, const float *in_dist, int32_t *labels, float *dist,
                             int *list, unsigned *count, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(exact_flag_kernel, dim3((nq + 3) / 4), dim3(256), 0, st, nq, k, in_labels, in_dist, labels, dist, list,
                     count);
  return hipGetLastError();
}

hipError_t launch_exact_replay(const ExactParams &params, int n_entries, hipStream_t st) {
  if (n_entries <= 0) return hipSuccess;
  ExactParams p = params;
  if (p.seq && p.layout == LAYOUT_BYTES) return hipErrorInvalidValue;  // (sequential-sum rows are always bit-packed)
  const size_t lds = lds_with_tables((size_t)(p.seq ? p.k + 1 : p.k) * 8 + (size_t)2 * EX_CHUNK * 4 +
                                         (p.row_bucket ? (size_t)p.n_buckets * 4 : 0),
                                     p.lut_floats, &p.lut_in_lds);
  if (p.seq) return launch_lds(exact_replay_kernel<false, true>, n_entries, EX_THREADS, lds, st, p);
  if (p.layout == LAYOUT_BYTES) return launch_lds(exact_replay_kernel<true, false>, n_entries, EX_THREADS, lds, st, p);
  return launch_lds(exact_replay_kernel<false, false>, n_entries, EX_THREADS, lds, st, p);
}

hipError_t launch_exact_finish(const int32_t *state, const int *list, const unsigned *count, int n_entries, int seq, int k,
                               int32_t *labels, float *dist, hipStream_t st) {
  if (n_entries <= 0) return hipSuccess;
  if (seq) return launch_lds(exact_finish_kernel<true>, n_entries, 64, (size_t)(k + 1) * 8, st, state, list, count, k, labels, dist);
  return launch_lds(exact_finish_kernel<false>, n_entries, 64, (size_t)k * 8, st, state, list, count, k, labels, dist);
}

// ---------------------------------------------------------------------------------------------------
// TI indexes: VAQ::searchTriangleInequality (VAQ.cpp:1540-1692) replayed, EVERY query (there is no "queries
// that have ties" shortcut: the 1-ulp cases of the unslacked bound are part of what is reproduced).
// The walk of a query: the clusters in the order of launch_ti_plan(exact = 1), the first nvisit of them
// ((ccIdxIdx < maxClusterVisit) || (!retrievedEnough && ccIdxIdx < T), :1555), empty ones skipped, inside a
// cluster the reference's member order (ti_build_walk).  Walk position w is row w of that concatenation when
// nothing is pruned; a `break` (:1566-1569) makes the cursor jump to the first position of the next cluster.
//   - heap_heapify; bsfK = 0, bsfKSquared = 0
//   - positions < k (counter < k; no break can precede them) enter unconditionally: heap_pop, heap_push of
//     sqrt(dist), if (dist > bsfK) { bsfK = dist; [EA: bsfKSquared = bsfK * bsfK] }  (:1591-1613)
//   - from position k on: break at the first member with bsfK <= qToCCDist[c] - mCodeToCCDist[row] (plain
//     fp32 subtraction); else admit iff dist < bsfKSquared on the un-rooted sum: heap_pop, heap_push(sqrt(dist)),
//     bsfK = heap_dis[0], bsfKSquared = bsfK * bsfK (one rounded multiply)  (:1565-1590)
//   - without EA bsfKSquared stays 0 (:1624-1658): nothing is admitted after position k - 1, so the walk ends
//     there -- labels and distances are final
//   - heap_reorder
// The EA branch's partial-sum abandon (:1574) only drops rows dist < bsfKSquared drops (table entries >= 0).
// Waves 1.. evaluate a chunk of consecutive walk positions into LDS -- the complete row sum, the bound
// qcc - xcc, the row's label --, wave 0 replays the previous chunk: per 64 positions a ballot of the break
// test and one of the admission test over the lanes at or after the cursor; the first set lane of either is
// the next event (the break test comes first in the loop body, so it wins a shared lane), handled with the
// reference's statements, after which both ballots are taken again.  After the first k positions bsfK and
// bsfKSquared never rise as long as bsfK * bsfK is a normal number (sqrt(fl(x * x)) == x then), so the
// evaluating waves may abandon against the published bsfKSquared and skip rows whose bound the published bsfK
// already excludes: both are never below the reference's at that row, and an excluded row lies at or behind
// its cluster's break.  Where bsfK * bsfK is subnormal or underflows (bsfK below about 1.1e-19) the identity
// fails and an admission can RAISE heap_dis[0]: +inf is published there instead (tix_publish), i.e. nothing is
// skipped or abandoned -- and a value published earlier, from the normal range, stays above all of these.  When the cursor jumps
// past whole chunks they are not evaluated at all.
constexpr int TIX_THREADS = 512;
constexpr int TIX_CHUNK = 1024;  // walk positions per chunk (a multiple of 64)

// what the evaluating waves may test against (above)
__device__ __forceinline__ void tix_publish(float *s_bsfk, float *s_bsf2, const float bsfK, const float bsf2) {
  const bool mono = bsf2 >= FLT_MIN;
  __hip_atomic_store(s_bsfk, mono ? bsfK : INFINITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_store(s_bsf2, mono ? bsf2 : INFINITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool BYTES>
__global__ __launch_bounds__(TIX_THREADS) void ti_exact_replay_kernel(TiExactParams tp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ex_smem[];
  const ExactParams &p = tp.x;
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = p.k, T = tp.T;
  // LDS: heap values, heap ids, two chunk buffers of (row sum, bound, label), the walk position of every
  // visited cluster's first member, [the query's lookup tables]
  float *hval = reinterpret_cast<float *>(ex_smem);
  int *hid = reinterpret_cast<int *>(hval + k);
  float *bufd = reinterpret_cast<float *>(hid + k);      // [2][TIX_CHUNK]
  float *bufb = bufd + 2 * TIX_CHUNK;                    // [2][TIX_CHUNK]
  int *bufl = reinterpret_cast<int *>(bufb + 2 * TIX_CHUNK);  // [2][TIX_CHUNK]
  int *cum = bufl + 2 * TIX_CHUNK;                       // [T + 1]
  float *lds_lut = reinterpret_cast<float *>(cum + T + 1);
  const float *glut = p.lut + (size_t)q * p.lut_floats;
  const float *lut = glut;
  if (p.lut_in_lds) {
    for (int i = tid; i < p.lut_floats; i += TIX_THREADS) lds_lut[i] = glut[i];
    lut = lds_lut;
  }
  const int *order = tp.order + (size_t)q * T;
  const float *qcc = tp.qcc + (size_t)q * T;
  const int nv = min(max(tp.nvisit[q], 0), T);
  for (int i = tid; i < k; i += TIX_THREADS) {  // heap_heapify (utils/Heap.hpp:211-235)
    hval[i] = FLT_MAX;
    hid[i] = -1;
  }
  // cum[i] = members of the first i clusters of the order (wave 0: a segment per lane, then the lanes' totals)
  if (wave == 0) {
    const int seg = (nv + 63) / 64;
    const int i0 = min(lane * seg, nv), i1 = min(i0 + seg, nv);
    int sum = 0;
    for (int i = i0; i < i1; i++) {
      const int c = order[i];
      sum += tp.start[c + 1] - tp.start[c];
    }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    int run = incl - sum;
    for (int i = i0; i < i1; i++) {
      const int c = order[i];
      cum[i] = run;
      run += tp.start[c + 1] - tp.start[c];
    }
    if (lane == 63) cum[nv] = incl;
  }
  // what the evaluating waves test against: +inf until k rows have entered (nothing is skipped before)
  __shared__ float s_bsfk, s_bsf2;
  __shared__ int s_cur[2];
  if (tid == 0) {
    s_bsfk = INFINITY;
    s_bsf2 = INFINITY;
  }
  __syncthreads();
  // without EA the walk ends with the k-th row that enters
  const int wend = tp.ea ? cum[nv] : min(cum[nv], k);
  const int nchunks = (wend + TIX_CHUNK - 1) / TIX_CHUNK;
  float bsfK = 0.0f, bsf2 = 0.0f;
  int cur = 0;  // wave 0: the walk position the reference's loops stand at
  int ec = 0, pc = -1;  // chunk the waves evaluate in this round, chunk wave 0 replays
  for (int it = 0;; it++) {
    if (wave > 0) {
      if (ec < nchunks) {
        const float t2 = __hip_atomic_load(&s_bsf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const float tk = __hip_atomic_load(&s_bsfk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int scur = it > 0 ? s_cur[(it - 1) & 1] : 0;  // (the cursor after the round before: never ahead)
        float *od = bufd + (it & 1) * TIX_CHUNK, *ob = bufb + (it & 1) * TIX_CHUNK;
        int *ol = bufl + (it & 1) * TIX_CHUNK;
        for (int j = tid - 64; j < TIX_CHUNK; j += TIX_THREADS - 64) {
          const int w = ec * TIX_CHUNK + j;
          float dv = INFINITY, bv = 0.0f;
          int lab = -1;
          if (w < wend && w >= scur) {
            int lo = 0, hi = nv;  // largest i with cum[i] <= w: its cluster (w < cum[nv]; empty ones skipped)
            while (hi - lo > 1) {
              const int mid = (lo + hi) >> 1;
              if (cum[mid] <= w) lo = mid;
              else hi = mid;
            }
            const int c = order[lo];
            const int64_t row = tp.walk[tp.start[c] + (w - cum[lo])];
            bv = qcc[lo] - tp.xcc[row];
            lab = (int)tp.perm[row];
            const bool uncond = w < k;
            if (uncond || !(tk <= bv)) dv = ex_row_dist<BYTES, false>(p, lut, row, uncond ? INFINITY : t2);
          }
          od[j] = dv;
          ob[j] = bv;
          ol[j] = lab;
        }
      }
    } else if (pc >= 0) {
      const float *id = bufd + ((it - 1) & 1) * TIX_CHUNK, *ib = bufb + ((it - 1) & 1) * TIX_CHUNK;
      const int *il = bufl + ((it - 1) & 1) * TIX_CHUNK;
      const int base = pc * TIX_CHUNK;
      for (int j0 = 0; j0 < TIX_CHUNK; j0 += 64) {
        const int g0 = base + j0, g1 = min(g0 + 64, wend);
        if (g0 >= wend) break;
        if (cur >= g1) continue;
        const float d = id[j0 + lane], b = ib[j0 + lane];
        const int lab = il[j0 + lane];
        const int w = g0 + lane;
        if (cur < k) {
          // counter < k (:1591-1613 / :1659-1679): (cur >= g0 here: nothing jumps before k rows have entered)
          const int e = min(k, g1);
          for (int w1 = cur; w1 < e; w1++) {
            const float dv = bits_to_float((unsigned)__builtin_amdgcn_readlane((int)float_to_bits(d), w1 - g0));
            const int lb = __builtin_amdgcn_readlane(lab, w1 - g0);
            const float r = sqrtf(dv);
            if (lane == 0) {
              refheap::pop(k, hval, hid);
              refheap::push(k, hval, hid, r, lb);
            }
            if (r > bsfK) {
              bsfK = r;
              if (tp.ea) bsf2 = bsfK * bsfK;
            }
          }
          wave_lds_sync();
          cur = e;
          if (cur >= k && lane == 0) tix_publish(&s_bsfk, &s_bsf2, bsfK, bsf2);
        }
        while (cur < g1) {
          // counter >= k (:1565-1590): the next event among the positions at or after the cursor
          const bool act = w >= cur && w < g1;
          const unsigned long long brk = __ballot(act && bsfK <= b);
          const unsigned long long adm = __ballot(act && d < bsf2);
          const int fb = brk != 0ull ? __builtin_ctzll(brk) : 64, fa = adm != 0ull ? __builtin_ctzll(adm) : 64;
          if (fb == 64 && fa == 64) {
            cur = g1;
          } else if (fb <= fa) {
            // break: on to the first member of the next cluster
            const int wb = g0 + fb;
            int lo = 0, hi = nv;
            while (hi - lo > 1) {
              const int mid = (lo + hi) >> 1;
              if (cum[mid] <= wb) lo = mid;
              else hi = mid;
            }
            cur = cum[lo + 1];
          } else {
            const float dv = bits_to_float((unsigned)__builtin_amdgcn_readlane((int)float_to_bits(d), fa));
            const int lb = __builtin_amdgcn_readlane(lab, fa);
            if (lane == 0) {
              refheap::pop(k, hval, hid);
              refheap::push(k, hval, hid, sqrtf(dv), lb);
            }
            wave_lds_sync();
            bsfK = hval[0];
            bsf2 = bsfK * bsfK;
            if (lane == 0) tix_publish(&s_bsfk, &s_bsf2, bsfK, bsf2);
            cur = g0 + fa + 1;
          }
        }
      }
    }
    // (two slots: a wave still reading this round's cursor is at most one barrier behind wave 0)
    if (tid == 0) s_cur[it & 1] = cur;
    __syncthreads();
    const int cc = s_cur[it & 1];
    if (ec >= nchunks || cc >= wend) break;  // the last chunk has been replayed / the walk is over
    pc = ec;
    ec = max(ec + 1, cc / TIX_CHUNK);
  }
  __shared__ int s_nel;
  ex_reorder_out(p.labels, p.dist, q, k, hval, hid, p.id_base, &s_nel, tid, TIX_THREADS);
}

hipError_t launch_ti_exact_replay(const TiExactParams &params, int nq, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  TiExactParams tp = params;
  const size_t lds = lds_with_tables((size_t)tp.x.k * 8 + (size_t)6 * TIX_CHUNK * 4 + (size_t)(tp.T + 1) * 4,
                                     tp.x.lut_floats, &tp.x.lut_in_lds);
  if (tp.x.layout == LAYOUT_BYTES) return launch_lds(ti_exact_replay_kernel<true>, nq, TIX_THREADS, lds, st, tp);
  return launch_lds(ti_exact_replay_kernel<false>, nq, TIX_THREADS, lds, st, tp);
}

} // namespace vaq
