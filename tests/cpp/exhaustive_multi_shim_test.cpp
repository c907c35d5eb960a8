// VaqHip::searchExhaustive(XTest, k) after setDevices({0, 0}) + setRefineDataset (include/vaqhip.hpp: the rows are cut
// over a multi-device refiner, the call is vaqhip_multi_refiner_search) against the same call on a single-device
// VaqHip over the same rows, with refineExactTies off and on.  argv[1] holds the inputs, written by
// tests/test_exhaustive_multi_gpu.py::test_cpp_shim:  int32 N, D, nq, k; raw rows N x D float; queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[4];
  if (std::fread(h, 4, 4, f) != 4) return 2;
  const int N = h[0], D = h[1], nq = h[2], k = h[3];
  vaqhip::RowMatrixF base((size_t)N, (size_t)D), q((size_t)nq, (size_t)D);
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  try {
    vaqhip::VaqHip one, many;
    many.setDevices({0, 0});
    bool threw = false;
    try {
      many.searchExhaustive(q, k);
    } catch (const vaqhip::Error &) {
      threw = true;  // (no refine dataset yet)
    }
    if (!threw) {
      std::printf("searchExhaustive ran without setRefineDataset\n");
      return 1;
    }
    one.setRefineDataset(base);
    many.setRefineDataset(base);
    if (!many.multiRefinerHandle() || many.refinerHandle() || !one.refinerHandle() || one.multiRefinerHandle()) {
      std::printf("setRefineDataset built the wrong refiner\n");
      return 1;
    }
    for (const bool exact : {false, true}) {
      one.refineExactTies = many.refineExactTies = exact;
      const auto a = one.searchExhaustive(q, k), b = many.searchExhaustive(q, k);
      if (a.labels.size() != (size_t)nq * k || a.labels != b.labels ||
          std::memcmp(a.distances.data(), b.distances.data(), a.distances.size() * 4) != 0) {
        std::printf("exact_ties %d: the sharded answer differs from the single device's\n", (int)exact);
        return 1;
      }
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("exhaustive_multi_shim ok\n");
  return 0;
}
