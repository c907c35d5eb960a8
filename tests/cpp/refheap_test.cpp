// refheap_test.cpp -- vaq::refheap (vaq_amd/csrc/vaq_restated.h), the restatement of the reference's heap
// (utils/Heap.hpp) that the replay kernels of option "exact_ties" run, against vo_heap_* of oracle/vaq_oracle.c
// on the host -- which tests/test_oracle_golden.py pins against the compiled reference heap.  VAQ::searchHeap
// and VAQ::searchTriangleInequality keep their k best in this heap, so where equal distances end up is part of
// their answer: the two heaps must agree slot for slot (distances bit for bit, ids exactly) after EVERY call.
//
//   refheap_test IN
// IN: int32 count, then per sequence int32 n, int32 k (>= 1) and n float32 keys (n, k <= 4096)
// Per sequence, in this order: (1) heapify, (2) VAQ::searchHeap's loop (VAQ.cpp:1750-1753) over the keys as row
// distances: if (top > key) { pop; push }, (3) reorder: the kept count, and the kept range [k - kept, k) against
// the entries vo_heap_reorder has moved to the front (whose tail must be neutral).
// Built by tests/test_seq_exact_cpu.py with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include -Ivaq_amd/csrc
// -Ioracle) and linked with oracle/vaq_oracle.c compiled as C; it is also built with
// -fsanitize=address,undefined and run on its own.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vaq_oracle.h"
#include "vaq_restated.h"

static void read_exact(void *p, size_t bytes, FILE *f) {
  if (bytes && std::fread(p, 1, bytes, f) != bytes) {
    std::fprintf(stderr, "refheap_test: short input\n");
    std::exit(2);
  }
}

struct Heap {
  std::vector<float> val;
  std::vector<int> ids;
  explicit Heap(size_t k) : val(k), ids(k) {}
};

// slots [a0, a0 + n) of a against [b0, b0 + n) of b
static bool same(const Heap &a, size_t a0, const Heap &b, size_t b0, size_t n, const char *what, int c, int step) {
  const bool ok = std::memcmp(a.val.data() + a0, b.val.data() + b0, n * sizeof(float)) == 0 &&
                  std::memcmp(a.ids.data() + a0, b.ids.data() + b0, n * sizeof(int)) == 0;
  if (!ok) std::fprintf(stderr, "refheap_test: sequence %d differs after %s %d\n", c, what, step);
  return ok;
}

static bool one_sequence(int c, const std::vector<float> &keys, int k) {
  const size_t K = (size_t)k;
  Heap mine(K), ref(K);
  vaq::refheap::heapify(k, mine.val.data(), mine.ids.data());
  vo_heap_heapify(K, ref.val.data(), ref.ids.data());
  if (!same(mine, 0, ref, 0, K, "heapify", c, 0)) return false;
  for (int row = 0; row < (int)keys.size(); row++) {
    const float dist = keys[(size_t)row];
    if (mine.val[0] > dist) {
      vaq::refheap::pop(k, mine.val.data(), mine.ids.data());
      vaq::refheap::push(k, mine.val.data(), mine.ids.data(), dist, row);
    }
    if (ref.val[0] > dist) {
      vo_heap_pop(K, ref.val.data(), ref.ids.data());
      vo_heap_push(K, ref.val.data(), ref.ids.data(), dist, row);
    }
    if (!same(mine, 0, ref, 0, K, "row", c, row)) return false;
  }
  const int kept = vaq::refheap::reorder(k, mine.val.data(), mine.ids.data());
  const size_t nel = vo_heap_reorder(K, ref.val.data(), ref.ids.data());
  const size_t want = keys.size() < K ? keys.size() : K;  // (every key is below FLT_MAX)
  if (kept < 0 || (size_t)kept != nel || nel != want) {
    std::fprintf(stderr, "refheap_test: sequence %d: reorder keeps %d, the oracle %zu, of min(n, k) = %zu\n", c, kept, nel,
                 want);
    return false;
  }
  if (!same(mine, K - nel, ref, 0, nel, "reorder", c, 0)) return false;
  for (size_t i = nel; i < K; i++) {
    if (ref.val[i] != FLT_MAX || ref.ids[i] != -1) {
      std::fprintf(stderr, "refheap_test: sequence %d: the oracle's tail is not neutral\n", c);
      return false;
    }
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: refheap_test IN\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) {
    std::fprintf(stderr, "refheap_test: cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t count;
  read_exact(&count, sizeof count, in);
  int bad = 0;
  for (int c = 0; c < count; c++) {
    int32_t nk[2];
    read_exact(nk, sizeof nk, in);
    if (nk[0] < 0 || nk[0] > 4096 || nk[1] < 1 || nk[1] > 4096) {
      std::fprintf(stderr, "refheap_test: sequence %d has n=%d k=%d\n", c, nk[0], nk[1]);
      return 2;
    }
    std::vector<float> keys((size_t)nk[0]);
    read_exact(keys.data(), keys.size() * sizeof(float), in);
    if (!one_sequence(c, keys, nk[1])) bad++;
  }
  std::fclose(in);
  if (bad) {
    std::fprintf(stderr, "refheap_test: %d of %d sequences differ\n", bad, count);
    return 1;
  }
  std::printf("refheap_test: ok (%d sequences)\n", count);
  return 0;
}
