// stdsort_test.cpp -- vaq::stdsort::sort (vaq_amd/csrc/vaq_fast.h) against the real libstdc++ std::sort
// on the host.  KNNFromDists sorts (idx, int16 dist) pairs with a distance-only comparator, so the
// permutation std::sort makes of equal keys is part of the FAST answer; the restatement sorts
// dist << 16 | idx and must leave the rows in the same order item for item.
//
//   stdsort_test IN OUT
// IN:  int32 count, then per sequence int32 n and n int32 keys (0 <= key < 32768, n <= 1024)
// OUT: per sequence the n int32 row indices in std::sort's output order
// Built by tests/test_fast_cpu.py with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vaq_fast.h"

struct IdxDist {  // the element of KNNFromDists<int16_t>
  int idx;
  int16_t dist;
};

static int32_t read_i32(FILE *f) {
  int32_t v;
  if (std::fread(&v, sizeof v, 1, f) != 1) {
    std::fprintf(stderr, "stdsort_test: short input\n");
    std::exit(2);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: stdsort_test IN OUT\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  FILE *out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "stdsort_test: cannot open files\n");
    return 2;
  }
  const int count = read_i32(in);
  int bad = 0;
  for (int c = 0; c < count; c++) {
    const int n = read_i32(in);
    if (n < 0 || n > 1024) {
      std::fprintf(stderr, "stdsort_test: sequence %d has n=%d\n", c, n);
      return 2;
    }
    std::vector<IdxDist> ref((size_t)n);
    std::vector<uint32_t> mine((size_t)n);
    for (int i = 0; i < n; i++) {
      const int32_t key = read_i32(in);
      if (key < 0 || key > 32767) {
        std::fprintf(stderr, "stdsort_test: sequence %d key %d out of range\n", c, key);
        return 2;
      }
      ref[(size_t)i] = IdxDist{i, (int16_t)key};
      mine[(size_t)i] = ((uint32_t)key << 16) | (uint32_t)i;
    }
    std::sort(ref.begin(), ref.end(), [](const IdxDist &a, const IdxDist &b) -> bool { return a.dist < b.dist; });
    vaq::stdsort::sort(mine.data(), n);
    for (int i = 0; i < n; i++) {
      const int32_t idx = ref[(size_t)i].idx;
      if ((int32_t)(mine[(size_t)i] & 0xffffu) != idx || (int)(mine[(size_t)i] >> 16) != (int)ref[(size_t)i].dist) {
        if (bad < 10)
          std::fprintf(stderr, "stdsort_test: sequence %d (n=%d) differs at position %d: std::sort row %d, restatement row %u\n",
                       c, n, i, idx, mine[(size_t)i] & 0xffffu);
        bad++;
        break;
      }
    }
    for (int i = 0; i < n; i++) {
      const int32_t idx = ref[(size_t)i].idx;
      std::fwrite(&idx, sizeof idx, 1, out);
    }
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  if (bad) {
    std::fprintf(stderr, "stdsort_test: %d of %d sequences differ\n", bad, count);
    return 1;
  }
  std::printf("stdsort_test: ok (%d sequences)\n", count);
  return 0;
}
