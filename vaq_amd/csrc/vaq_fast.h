// vaq_fast.h -- the FAST search method (VAQ::searchFast, VAQ.cpp:1778-1834): uint8 lookup tables
// over codes of at most 4 bits, integer row sums, top-k by KNNFromDists (utils/Experiment.hpp:40-56).
// DESIGN.md section "FAST" has the specification and the (dist, seq) argument.
#ifndef VAQ_FAST_H_
#define VAQ_FAST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vaq {

// rows of the FAST code image are padded to this (the reference pads mCodebookCMajor to 32, VAQ.cpp:666-670)
constexpr int FAST_ROW_PAD = 32;
// dwords per (row, lane group) of the FAST code image: code s = 4t + h sits in group h, nibble t
__host__ __device__ inline int fast_code_words(int M) { return (M / 4 + 7) / 8; }

// FAST code image: row r, group h (s % 4), dword w holds the codes of subspaces 4(8w + i) + h in nibble i.
// Rows [row_begin, row_end) of `out` are written from codes_u16 (CodebookType rows, first = row_begin).
hipError_t launch_fast_pack_codes(const uint16_t *codes_u16, int64_t row_begin, int64_t row_end, int M,
                                  uint32_t *out, hipStream_t st);
// smallQuantize (utils/Math.hpp:215-224) of the reference LUTType lut_ref[q][s][ksub] (rows >= 1 << bits[s]
// zero, as CreateLUT leaves them): small[q][s][c] = min(floor(max(lut - off[s], 0) * scale[s]), 255) for
// c < ksub, 0 for ksub <= c < 16
hipError_t launch_fast_quantize(const float *lut_ref, int nq, int M, int ksub, const float *offsets,
                                const float *scale, uint8_t *small, hipStream_t st);
// dist[q][r] = sum_s small[q][s][code(r, s)] for rows [0, n_pad) (n_pad a multiple of FAST_ROW_PAD) as an
// int8 GEMM on the matrix cores: A = one-hot rows, B = small - 128
hipError_t launch_fast_scan(const uint32_t *codes, int64_t n_pad, int M, const uint8_t *small, int nq,
                            uint16_t *dist, int n_cu, hipStream_t st);
// KNNFromDists' std::sort of the first kk = min(k, n) rows by distance only (libstdc++ introsort, one
// thread per query): order[q][p] = row at position p, for p < kk
hipError_t launch_fast_head_sort(const uint16_t *dist, int64_t n_pad, int nq, int kk, uint32_t *scratch,
                                 uint16_t *order, hipStream_t st);
// the same with explicit element strides per query for all three arrays; scratch[q * scratch_stride + p] is
// left holding the sorted items themselves, (dist << 16) | row
hipError_t launch_fast_head_sort_strided(const uint16_t *dist, int64_t dist_stride, int nq, int kk, uint32_t *scratch,
                                         int64_t scratch_stride, uint16_t *order, int64_t order_stride, hipStream_t st);
// the k smallest rows by (dist, seq) per query: seq = position in `order` for rows < kk, the row itself after.
// Slots >= min(k, n) are -1 / FLT_MAX.
hipError_t launch_fast_select(const uint16_t *dist, int64_t n_pad, int64_t n, int nq, int k, int M,
                              const uint16_t *order, int64_t id_base, int32_t *labels, float *out_dist,
                              hipStream_t st);
// One shard's part of a sharded FAST search ("FAST across shards"): the first
// head_rows rows are left out, the others are ranked by (dist, row); slots >= min(k, n - head_rows) are
// -1 / FLT_MAX.  head_rows = 0 is a plain (dist, row) top-k.
hipError_t launch_fast_select_tail(const uint16_t *dist, int64_t n_pad, int64_t n, int64_t head_rows, int nq, int k,
                                   int M, int64_t id_base, int32_t *labels, float *out_dist, hipStream_t st);
// out[q * out_stride + i] = dist[q * n_pad + i] for i < h: a shard's head distances into its exchange buffer
hipError_t launch_fast_head_copy(const uint16_t *dist, int64_t n_pad, int nq, int h, uint16_t *out,
                                 int64_t out_stride, hipStream_t st);
// head[q][p] for p < kk from the gathered planes of n_parts shards: part g owns positions
// [start[g], start[g + 1]) and holds them at planes[g * plane_stride + q * kk + p]
constexpr int FAST_MAX_LISTS = 16;
struct FastHeadParts {
  int n_parts;
  int start[FAST_MAX_LISTS + 1];
};
hipError_t launch_fast_head_gather(const uint16_t *planes, int64_t plane_stride, FastHeadParts parts, int nq, int kk,
                                   uint16_t *head, hipStream_t st);
// The first k of the stable merge by distance alone of: the head list -- head_sorted[q * head_stride + p] =
// (dist << 16) | head row, p < kk, in the order launch_fast_head_sort_strided left them -- then n_lists <=
// FAST_MAX_LISTS lists of k slots each, ascending, empty slots label < 0 (candidate i of list l of query q at
// l * list_stride + q * query_stride + i).  Ties go to the earlier list, then to the earlier position.  Labels of
// head rows are head_label_base + row.  head_sorted may be the query's own row of `labels` (it is read whole
// before anything is written); slots past the number of entries are -1 / FLT_MAX.
hipError_t launch_fast_merge(const uint32_t *head_sorted, int64_t head_stride, int kk, int64_t head_label_base,
                             const float *dist_lists, const int32_t *label_lists, int n_lists, int64_t list_stride,
                             int64_t query_stride, int nq, int k, int32_t *labels, float *out_dist, hipStream_t st);

// ---------------------------------------------------------------------------------------------------
// libstdc++'s std::sort (bits/stl_algo.h, bits/stl_heap.h) restated over an element type T and a
// comparator `lt` (a strict "comes before", as std::sort takes it).  The permutation std::sort makes of
// elements that compare equal is a function of the sequence of comparison results alone, so this
// reproduces it item for item -- also under a comparator that is no strict weak order (float keys with
// NaNs: every comparison with one is false): the walk is the same, and it stays inside [0, n) for the
// same reason std::sort's does NOT have to, so such a comparator is only passed where the caller guards
// for it (sort_by's `guarded` argument below).
// FAST's instantiation: uint32 items compared by the top 16 bits (the distance; the low 16 bits are the
// row and ride along), n <= 1024.
namespace stdsort {
template <class T, class Lt>
struct Impl {
  Lt lt;
  __host__ __device__ static inline void swp(T *a, T *b) { T t = *a; *a = *b; *b = t; }

  __host__ __device__ inline void push_heap(T *f, int hole, int top, T v) const {
    int parent = (hole - 1) / 2;
    while (hole > top && lt(f[parent], v)) {
      f[hole] = f[parent];
      hole = parent;
      parent = (hole - 1) / 2;
    }
    f[hole] = v;
  }
  __host__ __device__ inline void adjust_heap(T *f, int hole, int len, T v) const {
    const int top = hole;
    int second = hole;
    while (second < (len - 1) / 2) {
      second = 2 * (second + 1);
      if (lt(f[second], f[second - 1])) second--;
      f[hole] = f[second];
      hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
      second = 2 * (second + 1);
      f[hole] = f[second - 1];
      hole = second - 1;
    }
    push_heap(f, hole, top, v);
  }
  // __partial_sort(first, last, last): __make_heap then __sort_heap
  __host__ __device__ inline void heap_sort(T *f, int len) const {
    if (len >= 2) {
      for (int parent = (len - 2) / 2;; parent--) {
        adjust_heap(f, parent, len, f[parent]);
        if (parent == 0) break;
      }
    }
    for (int last = len - 1; last > 0; last--) {
      const T v = f[last];
      f[last] = f[0];
      adjust_heap(f, 0, last, v);
    }
  }
  __host__ __device__ inline void move_median_to_first(T *r, T *a, T *b, T *c) const {
    if (lt(*a, *b)) {
      if (lt(*b, *c)) swp(r, b);
      else if (lt(*a, *c)) swp(r, c);
      else swp(r, a);
    } else if (lt(*a, *c)) swp(r, a);
    else if (lt(*b, *c)) swp(r, c);
    else swp(r, b);
  }
  // [lo, hi): the sub-range; with GUARDED the two scans also stop at its ends (see sort_by)
  template <bool GUARDED>
  __host__ __device__ inline int unguarded_partition_pivot(T *f, int lo, int hi) const {
    const int mid = lo + (hi - lo) / 2;
    move_median_to_first(f + lo, f + lo + 1, f + mid, f + hi - 1);
    int first = lo + 1, last = hi;
    const T *pivot = f + lo;
    while (true) {
      while ((!GUARDED || first < hi) && lt(f[first], *pivot)) ++first;
      --last;
      while ((!GUARDED || last > lo) && lt(*pivot, f[last])) --last;
      if (!(first < last)) return first;
      swp(f + first, f + last);
      ++first;
    }
  }
  template <bool GUARDED>
  __host__ __device__ inline void unguarded_linear_insert(T *f, int last) const {
    const T v = f[last];
    int next = last - 1;
    while ((!GUARDED || next >= 0) && lt(v, f[next])) {
      f[last] = f[next];
      last = next;
      --next;
    }
    f[last] = v;
  }
  template <bool GUARDED>
  __host__ __device__ inline void insertion_sort(T *f, int lo, int hi) const {
    if (lo == hi) return;
    for (int i = lo + 1; i != hi; ++i) {
      if (lt(f[i], f[lo])) {
        const T v = f[i];
        for (int j = i; j > lo; --j) f[j] = f[j - 1];
        f[lo] = v;
      } else {
        unguarded_linear_insert<GUARDED>(f, i);
      }
    }
  }
};
constexpr int THRESHOLD = 16;
// std::__introsort_loop with its tail recursion (on the right part) made an explicit stack: the
// depth limit bounds the stack at 2 * log2(n) frames, so LG_MAX >= log2(n) rounded down.
// GUARDED: under a strict weak order the "unguarded" scans of std::sort stop by themselves inside the
// range (the pivot is a median of three, the first 16 elements hold the minimum); under another
// comparator (NaN keys) the real function may run past an end of the sequence and read whatever lies
// there.  With GUARDED the scans stop at the ends of the range instead -- the same walk wherever the
// real function stays inside, and defined where it does not.
template <int LG_MAX, bool GUARDED, class T, class Lt>
__host__ __device__ inline void sort_by(T *f, int n, Lt lt) {
  if (n <= 1) return;
  const Impl<T, Lt> s{lt};
  int lg = 0;
  while ((2 << lg) <= n) lg++;  // std::__lg(n)
  struct Frame { int lo, hi, depth; };
  Frame stack[2 * (LG_MAX + 1) + 2];
  int sp = 0;
  stack[sp++] = {0, n, 2 * lg};
  while (sp > 0) {
    Frame fr = stack[--sp];
    int lo = fr.lo, hi = fr.hi, depth = fr.depth;
    // the loop body of __introsort_loop(lo, hi, depth): recurse right, continue left
    while (hi - lo > THRESHOLD) {
      if (depth == 0) {
        s.heap_sort(f + lo, hi - lo);
        break;
      }
      --depth;
      const int cut = s.template unguarded_partition_pivot<GUARDED>(f, lo, hi);
      // __introsort_loop(cut, hi, depth) runs to completion before the left part is continued;
      // the two parts are disjoint, so finishing the left part first gives the same result
      stack[sp++] = {cut, hi, depth};
      hi = cut;
    }
  }
  // __final_insertion_sort
  if (n > THRESHOLD) {
    s.template insertion_sort<GUARDED>(f, 0, THRESHOLD);
    for (int i = THRESHOLD; i < n; ++i) s.template unguarded_linear_insert<GUARDED>(f, i);
  } else {
    s.template insertion_sort<GUARDED>(f, 0, n);
  }
}

// FAST: KNNFromDists' items, n <= 1024 (VAQHIP_MAX_K): depth <= 2 * 10 frames below the root
__host__ __device__ inline bool lt(uint32_t a, uint32_t b) { return (a >> 16) < (b >> 16); }
struct Lt16 {
  __host__ __device__ inline bool operator()(uint32_t a, uint32_t b) const { return lt(a, b); }
};
__host__ __device__ inline void sort(uint32_t *f, int n) { sort_by<10, false>(f, n, Lt16{}); }
}  // namespace stdsort

// ---------------------------------------------------------------------------------------------------
// libstdc++'s std::push_heap / std::pop_heap / std::sort_heap (bits/stl_heap.h) restated over (dist, id)
// pairs held as two arrays and compared by dist alone -- BitVecEngine::queryLUT's k best
// (BitVecEngine.hpp:1283-1316: std::vector<IdxDistPairFloat> under a.dist < b.dist).  The same
// __push_heap / __adjust_heap as stdsort's above, over another element; which of several equal
// distances ends where is a function of the sequence of calls alone.  Used by option "exact_ties" on
// sequential-sum indexes (vaq_exact.hip).
namespace stdheap {
// std::__push_heap(first, hole, top, value, comp)
__host__ __device__ inline void sift_up(float *d, int *id, int hole, int top, float vd, int vi) {
  int parent = (hole - 1) / 2;
  while (hole > top && d[parent] < vd) {
    d[hole] = d[parent];
    id[hole] = id[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  d[hole] = vd;
  id[hole] = vi;
}
// std::__adjust_heap(first, hole, len, value, comp)
__host__ __device__ inline void adjust_heap(float *d, int *id, int hole, int len, float vd, int vi) {
  const int top = hole;
  int second = hole;
  while (second < (len - 1) / 2) {
    second = 2 * (second + 1);
    if (d[second] < d[second - 1]) second--;
    d[hole] = d[second];
    id[hole] = id[second];
    hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) {
    second = 2 * (second + 1);
    d[hole] = d[second - 1];
    id[hole] = id[second - 1];
    hole = second - 1;
  }
  sift_up(d, id, hole, top, vd, vi);
}
// std::push_heap(first, first + len): the new element is the last one
__host__ __device__ inline void push_heap(float *d, int *id, int len) {
  sift_up(d, id, len - 1, 0, d[len - 1], id[len - 1]);
}
// std::__pop_heap(first, last, result = last): the maximum goes to slot `last`, the element that was there
// is sifted down from the root of the remaining `last` elements
__host__ __device__ inline void pop_to(float *d, int *id, int last) {
  const float vd = d[last];
  const int vi = id[last];
  d[last] = d[0];
  id[last] = id[0];
  adjust_heap(d, id, 0, last, vd, vi);
}
// std::pop_heap(first, first + len): the maximum goes to the last slot
__host__ __device__ inline void pop_heap(float *d, int *id, int len) {
  if (len > 1) pop_to(d, id, len - 1);
}
// std::sort_heap(first, first + len): ascending
__host__ __device__ inline void sort_heap(float *d, int *id, int len) {
  while (len > 1) {
    --len;
    pop_to(d, id, len);
  }
}
}  // namespace stdheap

}  // namespace vaq
#endif  // VAQ_FAST_H_
