// cluster_sort_test.cpp -- the sort of the cluster plan's fallback on the host: vaq::stdsort::sort_by<12, true> over
// ClusterPair under ClusterLt (vaq_amd/csrc/vaq_bitvec_clusters.h), the very call cluster_plan_kernel makes, on the
// centre distances of tests/bitvec_clusters_cases.py: ties, +inf, and NaN.
//
//   cluster_sort_test IN OUT
// IN:  int32 count, then per sequence int32 n and n float32 distances (pair i is (dist[i], i))
// OUT: per sequence the n int32 centre indices in the guarded sort's output order
//
// tests/test_bitvec_clusters_cpu.py compares OUT with bitvec_ref.std_sort_perm_f32, the order the checker of the GPU
// tests uses.  Checked here, per sequence:
//   - without a NaN the comparator is a strict weak order (inf == inf): the real libstdc++ std::sort gives the same;
//   - with a NaN, std::sort is outside what C++ defines and is not called.  The restatement is run a second time
//     without its guards at the ends of the range, on a heap copy of exactly n pairs: the two walks must agree, i.e.
//     on these arrays every scan stopped on a false comparison inside the array (the Python restatement has no
//     guards either).  The build under AddressSanitizer would report a scan that left the array.
// Built with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include), once more with -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "vaq_bitvec_clusters.h"

static int32_t read_i32(FILE *f) {
  int32_t v;
  if (std::fread(&v, sizeof v, 1, f) != 1) {
    std::fprintf(stderr, "cluster_sort_test: short input\n");
    std::exit(2);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: cluster_sort_test IN OUT\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  FILE *out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cluster_sort_test: cannot open files\n");
    return 2;
  }
  const int count = read_i32(in);
  int bad = 0, with_nan = 0;
  for (int c = 0; c < count; c++) {
    const int n = read_i32(in);
    if (n < 1 || n > vaq::BITVEC_CLUSTERS_MAX) {
      std::fprintf(stderr, "cluster_sort_test: sequence %d has n=%d\n", c, n);
      return 2;
    }
    std::vector<float> dist((size_t)n);
    if (std::fread(dist.data(), sizeof(float), (size_t)n, in) != (size_t)n) {
      std::fprintf(stderr, "cluster_sort_test: short input\n");
      return 2;
    }
    bool nan = false;
    // (heap arrays of exactly n pairs: a read outside is AddressSanitizer's to report)
    std::unique_ptr<vaq::ClusterPair[]> guarded(new vaq::ClusterPair[(size_t)n]), open_(new vaq::ClusterPair[(size_t)n]);
    for (int i = 0; i < n; i++) {
      guarded[(size_t)i] = open_[(size_t)i] = vaq::ClusterPair{dist[(size_t)i], i};
      nan |= std::isnan(dist[(size_t)i]);
    }
    with_nan += nan ? 1 : 0;
    vaq::stdsort::sort_by<12, true>(guarded.get(), n, vaq::ClusterLt{});
    vaq::stdsort::sort_by<12, false>(open_.get(), n, vaq::ClusterLt{});
    for (int i = 0; i < n; i++)
      if (guarded[(size_t)i].idx != open_[(size_t)i].idx) {
        std::fprintf(stderr, "cluster_sort_test: sequence %d (n=%d): the guarded and the unguarded walk differ at %d\n", c, n, i);
        bad++;
        break;
      }
    if (!nan) {
      std::vector<vaq::ClusterPair> ref((size_t)n);
      for (int i = 0; i < n; i++) ref[(size_t)i] = vaq::ClusterPair{dist[(size_t)i], i};
      std::sort(ref.begin(), ref.end(), vaq::ClusterLt{});
      for (int i = 0; i < n; i++)
        if (ref[(size_t)i].idx != guarded[(size_t)i].idx) {
          std::fprintf(stderr, "cluster_sort_test: sequence %d (n=%d) differs at position %d: std::sort %d, restatement %d\n", c,
                       n, i, ref[(size_t)i].idx, guarded[(size_t)i].idx);
          bad++;
          break;
        }
    }
    for (int i = 0; i < n; i++) {
      const int32_t v = guarded[(size_t)i].idx;
      std::fwrite(&v, sizeof v, 1, out);
    }
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  if (bad) {
    std::fprintf(stderr, "cluster_sort_test: %d of %d sequences differ\n", bad, count);
    return 1;
  }
  std::printf("cluster_sort_test: ok (%d sequences, %d with a NaN)\n", count, with_nan);
  return 0;
}
