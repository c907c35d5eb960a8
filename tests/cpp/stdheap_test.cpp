// stdheap_test.cpp -- vaq::stdheap (vaq_amd/csrc/vaq_restated.h) against the real libstdc++ std::push_heap /
// std::pop_heap / std::sort_heap on the host.  BitVecEngine::queryLUT (BitVecEngine.hpp:1282-1317) keeps its k
// best in a std::vector<IdxDistPairFloat> under those functions with a distance-only comparator, so where equal
// distances end up is part of its answer; the restatement works on two arrays (dist, idx) and must agree with the
// vector element for element after EVERY call.
//
//   stdheap_test IN OUT
// IN:  int32 count, then per sequence int32 n, int32 k (>= 1) and n float32 keys (n <= 4096)
// OUT: per sequence int32 m = min(k, n) and the m int32 row indices queryLUT's loop returns for these row
//      distances, in its order
// Per sequence: (1) n pushes, (2) n / 2 pops, (3) sort_heap of what is left, (4) the queryLUT loop as a whole:
// the first k rows pushed, then push + pop while dist < bsfK, then sort_heap.
// Built by tests/test_seq_exact_cpu.py with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include); it may also
// be built with -fsanitize=address,undefined and run on its own.
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vaq_restated.h"

struct IdxDistPairFloat {  // the element of queryLUT's vector
  int idx;
  float dist;
  IdxDistPairFloat(int i, float d) : idx(i), dist(d) {}
};

static bool comparator(IdxDistPairFloat const &a, IdxDistPairFloat const &b) { return a.dist < b.dist; }

static void read_exact(void *p, size_t bytes, FILE *f) {
  if (bytes && std::fread(p, 1, bytes, f) != bytes) {
    std::fprintf(stderr, "stdheap_test: short input\n");
    std::exit(2);
  }
}

// the restatement's heap beside the vector: len elements in use
struct Mine {
  std::vector<float> d;
  std::vector<int> id;
  int len = 0;
  explicit Mine(size_t cap) : d(cap), id(cap) {}
};

static bool same(const std::vector<IdxDistPairFloat> &ref, const Mine &m, const char *what, int c, int step) {
  bool ok = (int)ref.size() == m.len;
  for (int i = 0; ok && i < m.len; i++) ok = ref[(size_t)i].idx == m.id[(size_t)i] && ref[(size_t)i].dist == m.d[(size_t)i];
  if (!ok) std::fprintf(stderr, "stdheap_test: sequence %d differs after %s %d\n", c, what, step);
  return ok;
}

static bool one_sequence(int c, const std::vector<float> &keys, int k, std::vector<int32_t> *loop_ids) {
  const int n = (int)keys.size();
  std::vector<IdxDistPairFloat> ref;
  Mine m((size_t)n + 1);
  // (1) pushes
  for (int i = 0; i < n; i++) {
    ref.emplace_back(i, keys[(size_t)i]);
    std::push_heap(ref.begin(), ref.end(), comparator);
    m.d[(size_t)m.len] = keys[(size_t)i];
    m.id[(size_t)m.len] = i;
    m.len++;
    vaq::stdheap::push_heap(m.d.data(), m.id.data(), m.len);
    if (!same(ref, m, "push", c, i)) return false;
  }
  // (2) pops
  for (int i = 0; i < n / 2; i++) {
    std::pop_heap(ref.begin(), ref.end(), comparator);
    ref.pop_back();
    vaq::stdheap::pop_heap(m.d.data(), m.id.data(), m.len);
    m.len--;
    if (!same(ref, m, "pop", c, i)) return false;
  }
  // (3) sort_heap
  std::sort_heap(ref.begin(), ref.end(), comparator);
  vaq::stdheap::sort_heap(m.d.data(), m.id.data(), m.len);
  if (!same(ref, m, "sort_heap", c, 0)) return false;
  // (4) queryLUT's loop over the row distances `keys`, side by side: `best` under the real functions, `w` under
  // the restatement.  A row below the bound is appended and pushed; from row k on the maximum of the k + 1
  // is popped off again and the bound becomes the new maximum; sort_heap at the end.
  std::vector<IdxDistPairFloat> best;
  best.reserve((size_t)k + 1);
  float bound = FLT_MAX;
  Mine w((size_t)k + 1);
  float my_bound = FLT_MAX;
  for (int row = 0; row < n; row++) {
    const float dist = keys[(size_t)row];
    if (dist < bound) {
      best.emplace_back(row, dist);
      std::push_heap(best.begin(), best.end(), comparator);
      if (row >= k) {
        std::pop_heap(best.begin(), best.end(), comparator);
        best.pop_back();
        bound = best.front().dist;
      }
    }
    if (dist < my_bound) {
      w.d[(size_t)w.len] = dist;
      w.id[(size_t)w.len] = row;
      vaq::stdheap::push_heap(w.d.data(), w.id.data(), w.len + 1);
      if (row >= k) {
        vaq::stdheap::pop_heap(w.d.data(), w.id.data(), w.len + 1);
        my_bound = w.d[0];
      } else {
        w.len++;
      }
    }
    if (!same(best, w, "loop row", c, row) || bound != my_bound) return false;
  }
  std::sort_heap(best.begin(), best.end(), comparator);
  vaq::stdheap::sort_heap(w.d.data(), w.id.data(), w.len);
  if (!same(best, w, "the loop's sort_heap", c, 0)) return false;
  for (const IdxDistPairFloat &p : best) loop_ids->push_back(p.idx);
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: stdheap_test IN OUT\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  FILE *out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "stdheap_test: cannot open files\n");
    return 2;
  }
  int32_t count;
  read_exact(&count, sizeof count, in);
  int bad = 0;
  for (int c = 0; c < count; c++) {
    int32_t nk[2];
    read_exact(nk, sizeof nk, in);
    if (nk[0] < 0 || nk[0] > 4096 || nk[1] < 1 || nk[1] > 4096) {
      std::fprintf(stderr, "stdheap_test: sequence %d has n=%d k=%d\n", c, nk[0], nk[1]);
      return 2;
    }
    std::vector<float> keys((size_t)nk[0]);
    read_exact(keys.data(), keys.size() * sizeof(float), in);
    std::vector<int32_t> ids;
    if (!one_sequence(c, keys, nk[1], &ids)) bad++;
    const int32_t m = (int32_t)ids.size();
    std::fwrite(&m, sizeof m, 1, out);
    if (m) std::fwrite(ids.data(), sizeof(int32_t), (size_t)m, out);
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  if (bad) {
    std::fprintf(stderr, "stdheap_test: %d of %d sequences differ\n", bad, count);
    return 1;
  }
  std::printf("stdheap_test: ok (%d sequences)\n", count);
  return 0;
}
