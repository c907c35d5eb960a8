// stdsort_generic_test.cpp -- vaq::stdsort::sort_by (vaq_amd/csrc/vaq_restated.h) under the two comparators of
// option "exact_ties" on TI indexes, against the real libstdc++ std::sort on the host, element for element:
//   mode 0  VAQ::clusterTI's member sort (VAQ.cpp:973-979): row numbers 0..n-1, comparator key[i] > key[j]
//   mode 1  the cluster order of VAQ::search's TI branch (VAQ.cpp:815-820): ints 0..n-1, comparator
//           key[i] < key[j]; the keys may hold NaNs (every comparison with one is false)
//
//   stdsort_generic_test IN OUT
// IN:  int32 count, then per sequence int32 mode, int32 n and n float32 keys
// OUT: per sequence the n int32 elements in std::sort's output order
// A comparator over NaN keys is no strict weak order, so the real std::sort is outside its contract in mode 1:
// its "unguarded" scans may leave the sequence where no element stops them.  The sequences of
// tests/ti_exact_ref.py:sort_sequences are fixed (one seed) and chosen so that the real function stays inside --
// both builds run it under the same inputs, one of them under AddressSanitizer, which would report a read
// outside -- and the restatement is run twice on them, with and without its guards at the ends of the range:
// the two walks must agree, i.e. the guards never acted.  The device code uses the guarded form, which is
// defined for every input.
// Built by tests/test_ti_exact_cpu.py with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include), once more
// with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vaq_restated.h"

static int32_t read_i32(FILE *f) {
  int32_t v;
  if (std::fread(&v, sizeof v, 1, f) != 1) {
    std::fprintf(stderr, "stdsort_generic_test: short input\n");
    std::exit(2);
  }
  return v;
}

struct Desc {  // this->mCodeToCCDist[i] > this->mCodeToCCDist[j]
  const float *key;
  bool operator()(uint32_t i, uint32_t j) const { return key[i] > key[j]; }
};
struct Asc {  // qToCCDist[i] < qToCCDist[j]
  const float *key;
  bool operator()(int i, int j) const { return key[i] < key[j]; }
};

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: stdsort_generic_test IN OUT\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  FILE *out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "stdsort_generic_test: cannot open files\n");
    return 2;
  }
  const int count = read_i32(in);
  int bad = 0;
  for (int c = 0; c < count; c++) {
    const int mode = read_i32(in);
    const int n = read_i32(in);
    if (n < 0 || n > (1 << 20) || (mode != 0 && mode != 1)) {
      std::fprintf(stderr, "stdsort_generic_test: sequence %d has mode=%d n=%d\n", c, mode, n);
      return 2;
    }
    std::vector<float> key((size_t)n);
    if (n > 0 && std::fread(key.data(), sizeof(float), (size_t)n, in) != (size_t)n) {
      std::fprintf(stderr, "stdsort_generic_test: short input\n");
      return 2;
    }
    std::vector<int32_t> got((size_t)n), want((size_t)n);
    if (mode == 0) {
      std::vector<int> ref((size_t)n);
      std::vector<uint32_t> mine((size_t)n);
      for (int i = 0; i < n; i++) ref[(size_t)i] = i, mine[(size_t)i] = (uint32_t)i;
      const float *k = key.data();
      std::sort(ref.begin(), ref.end(), [k](int i, int j) { return k[i] > k[j]; });
      vaq::stdsort::sort_by<31, true>(mine.data(), n, Desc{k});
      for (int i = 0; i < n; i++) want[(size_t)i] = ref[(size_t)i], got[(size_t)i] = (int32_t)mine[(size_t)i];
    } else {
      std::vector<int> ref((size_t)n), mine((size_t)n), open_((size_t)n);
      for (int i = 0; i < n; i++) ref[(size_t)i] = mine[(size_t)i] = open_[(size_t)i] = i;
      const float *k = key.data();
      std::sort(ref.data(), ref.data() + n, [k](int i, int j) -> bool { return k[i] < k[j]; });
      vaq::stdsort::sort_by<31, true>(mine.data(), n, Asc{k});
      vaq::stdsort::sort_by<31, false>(open_.data(), n, Asc{k});
      if (open_ != mine) {
        std::fprintf(stderr, "stdsort_generic_test: sequence %d (n=%d): the guarded and the unguarded walk differ\n", c, n);
        bad++;
      }
      for (int i = 0; i < n; i++) want[(size_t)i] = ref[(size_t)i], got[(size_t)i] = mine[(size_t)i];
    }
    for (int i = 0; i < n; i++)
      if (got[(size_t)i] != want[(size_t)i]) {
        if (bad < 10)
          std::fprintf(stderr, "stdsort_generic_test: sequence %d (mode %d, n=%d) differs at position %d: std::sort %d, restatement %d\n",
                       c, mode, n, i, want[(size_t)i], got[(size_t)i]);
        bad++;
        break;
      }
    if (n > 0) std::fwrite(want.data(), sizeof(int32_t), (size_t)n, out);
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  if (bad) {
    std::fprintf(stderr, "stdsort_generic_test: %d of %d sequences differ\n", bad, count);
    return 1;
  }
  std::printf("stdsort_generic_test: ok (%d sequences)\n", count);
  return 0;
}
