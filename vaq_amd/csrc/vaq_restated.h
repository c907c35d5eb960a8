// vaq_restated.h -- library functions whose behaviour on EQUAL keys is part of the reference's answers,
// restated so that host and device run the same statements: libstdc++'s std::sort (stdsort) and heap
// functions (stdheap), the reference's own heap, utils/Heap.hpp (refheap), and the summation order of Eigen's
// squaredNorm (sq_norm_eigen).  Each is pinned on the CPU against the real thing: tests/cpp/stdsort_test.cpp,
// stdsort_generic_test.cpp, stdheap_test.cpp, refheap_test.cpp and refine_order_test.cpp.
#ifndef VAQ_RESTATED_H_
#define VAQ_RESTATED_H_

#include <hip/hip_runtime.h>
#include <float.h>
#include <stddef.h>
#include <stdint.h>

namespace vaq {

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

// ---------------------------------------------------------------------------------------------------
// The reference's own heap (utils/Heap.hpp, CMax<float, int>: a binary max-heap over k (value, id) slots held
// as two arrays), statement for statement, as restated in oracle/vaq_oracle.c -- which is pinned against the
// compiled reference heap (tests/test_oracle_golden.py); tests/cpp/refheap_test.cpp compares the two after
// every call.  VAQ::searchHeap and VAQ::searchTriangleInequality keep their k best in it, so it decides option
// "exact_ties" on byte-code and TI indexes (vaq_exact.hip).
namespace refheap {
// heap_heapify (utils/Heap.hpp:211-235) of nothing, by ONE thread: neutral FLT_MAX, ids -1
__host__ __device__ inline void heapify(const int k, float *val, int *ids) {
  for (int i = 0; i < k; i++) {
    val[i] = FLT_MAX;
    ids[i] = -1;
  }
}

// utils/Heap.hpp:115-144 (1-based sift-down of the last element from the root; on equal children the
// comparison is false, so the RIGHT child is taken)
__host__ __device__ inline void pop(const int k, float *val0, int *ids0) {
  float *val = val0 - 1;
  int *ids = ids0 - 1;
  const float v = val[k];
  int i = 1;
  for (;;) {
    const int i1 = i << 1, i2 = i1 + 1;
    if (i1 > k) break;
    if (i2 == k + 1 || val[i1] > val[i2]) {
      if (v > val[i1]) break;
      val[i] = val[i1];
      ids[i] = ids[i1];
      i = i1;
    } else {
      if (v > val[i2]) break;
      val[i] = val[i2];
      ids[i] = ids[i2];
      i = i2;
    }
  }
  val[i] = val[k];
  ids[i] = ids[k];
}

// utils/Heap.hpp:151-169 (sift-up from slot k)
__host__ __device__ inline void push(const int k, float *val0, int *ids0, const float v, const int id) {
  float *val = val0 - 1;
  int *ids = ids0 - 1;
  int i = k;
  while (i > 1) {
    const int f = i >> 1;
    if (!(v > val[f])) break;
    val[i] = val[f];
    ids[i] = ids[f];
    i = f;
  }
  val[i] = v;
  ids[i] = id;
}

// heap_reorder (utils/Heap.hpp:322-349) by ONE thread: pop the maxima into the tail -> ascending; entries
// of id -1 are dropped.  Returns the number kept: they sit in [k - kept, k).  (The memmove of the kept
// entries to the front and the neutral tail are left to the copy that follows.)
__host__ __device__ inline int reorder(const int k, float *hval, int *hid) {
  int ii = 0;
  for (int i = 0; i < k; i++) {
    const float v = hval[0];
    const int id = hid[0];
    pop(k - i, hval, hid);
    hval[k - ii - 1] = v;
    hid[k - ii - 1] = id;
    if (id != -1) ii++;
  }
  return ii;
}
}  // namespace refheap

// ---------------------------------------------------------------------------------------------------
// Eigen's (x - m).squaredNorm() over float rows (Eigen/src/Core/Redux.h, redux_impl<.., LinearVectorizedTraversal,
// NoUnrolling>: 8-float packets, two accumulators, predux, scalar tail; fewer than 8 columns: the plain sequential
// sum), as the k-means of clusterTI (vaq_kmeans.hip) and VAQ::refine (VAQ.cpp:866; vaq_refine.hip spreads the same
// additions over 16 lanes) evaluate it.  Pinned against the compiled reference by tests/golden/kmeans and
// tests/golden/refine (tests/cpp/refine_order_test.cpp runs this very function on the host).
__host__ __device__ __forceinline__ float km_sq(float x, float m) {
  const float t = x - m;
  return t * t;
}

// (x - m).squaredNorm() as Eigen reduces it; x[j] is read at xs[j * xstride] (UNIT: at xs[j])
template <bool UNIT>
__host__ __device__ __forceinline__ float sq_norm_eigen(const float *xs, int xstride, const float *__restrict__ m, int d) {
#define T_(j) km_sq(xs[UNIT ? (size_t)(j) : (size_t)(j) * xstride], m[j])
  if (d < 8) {  // too small to vectorise: res = coeff(0); res += coeff(i)
    float res = T_(0);
    for (int j = 1; j < d; j++) res += T_(j);
    return res;
  }
  const int end1 = (d / 8) * 8, end2 = (d / 16) * 16;
  float a0[8], a1[8];
#pragma unroll
  for (int l = 0; l < 8; l++) a0[l] = T_(l);
  if (end1 > 8) {
#pragma unroll
    for (int l = 0; l < 8; l++) a1[l] = T_(8 + l);
    for (int i = 16; i < end2; i += 16) {
#pragma unroll
      for (int l = 0; l < 8; l++) a0[l] += T_(i + l);
#pragma unroll
      for (int l = 0; l < 8; l++) a1[l] += T_(i + 8 + l);
    }
#pragma unroll
    for (int l = 0; l < 8; l++) a0[l] += a1[l];
    if (end1 > end2) {
#pragma unroll
      for (int l = 0; l < 8; l++) a0[l] += T_(end2 + l);
    }
  }
  // predux<Packet8f>: the halves added, then (b0 + b2) + (b1 + b3)
  float res = ((a0[0] + a0[4]) + (a0[2] + a0[6])) + ((a0[1] + a0[5]) + (a0[3] + a0[7]));
  for (int j = end1; j < d; j++) res += T_(j);
  return res;
#undef T_
}

}  // namespace vaq
#endif  // VAQ_RESTATED_H_
