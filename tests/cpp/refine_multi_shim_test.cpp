// VaqHip::search(XTest, k, refineNum) after setDevices({0, 0, 0}) (include/vaqhip.hpp: setRefineDataset builds a
// multi-device refiner over the same devices, the fused call is vaqhip_multi_search_refine) against the same call on
// a single-device VaqHip over the same rows, with refineExactTies off and on.  argv[1] holds the inputs, written by
// tests/test_refine_multi_gpu.py::test_cpp_shim:
//   int32 N, M, L, bits, nq; codes N x M uint16; M codebooks (1 << bits) x L float; raw rows N x D float;
//   queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[5];
  if (std::fread(h, 4, 5, f) != 5) return 2;
  const int N = h[0], M = h[1], L = h[2], bits = h[3], nq = h[4], D = M * L;
  vaqhip::VaqHip one, many;
  many.setDevices({0, 0, 0});
  vaqhip::CodebookType codes((size_t)N, (size_t)M);
  if (std::fread(codes.data(), 2, (size_t)N * M, f) != (size_t)N * M) return 2;
  std::vector<vaqhip::RowMatrixF> cents;
  for (int s = 0; s < M; s++) {
    cents.emplace_back((size_t)1 << bits, (size_t)L);
    if (std::fread(cents[s].data(), 4, ((size_t)L) << bits, f) != ((size_t)L) << bits) return 2;
  }
  vaqhip::RowMatrixF base((size_t)N, (size_t)D), q((size_t)nq, (size_t)D);
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,HEAP", bits * M, M, bits, bits);
  try {
    for (vaqhip::VaqHip *v : {&one, &many}) {
      v->parseMethodString(method);
      v->mBitsAlloc.assign(M, bits);
      v->mCodebook = codes;
      v->mCentroidsPerSubs = cents;
      v->setRefineDataset(base);
    }
    if (!many.multiRefinerHandle() || many.refinerHandle() || !one.refinerHandle() || one.multiRefinerHandle()) {
      std::printf("setRefineDataset built the wrong refiner\n");
      return 1;
    }
    for (const bool exact : {false, true}) {
      for (vaqhip::VaqHip *v : {&one, &many}) v->exactTies = v->refineExactTies = exact;
      const auto a = one.search(q, 10, 100), b = many.search(q, 10, 100);
      if (a.labels.size() != (size_t)nq * 10 || a.labels != b.labels ||
          std::memcmp(a.distances.data(), b.distances.data(), a.distances.size() * 4) != 0) {
        std::printf("exact_ties %d: the sharded answer differs from the single device's\n", (int)exact);
        return 1;
      }
    }
    if (!many.multiHandle() || many.handle()) {
      std::printf("the search did not run on the multi-device index\n");
      return 1;
    }
    vaqhip_multi_refiner_info info;
    if (vaqhip_multi_refiner_get_info(many.multiRefinerHandle(), &info) || info.n_devices != 3 || info.N != N ||
        info.shard_rows[0] + info.shard_rows[1] + info.shard_rows[2] != N) {
      std::printf("the multi refiner holds %lld rows on %d devices\n", (long long)info.N, info.n_devices);
      return 1;
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("refine_multi_shim ok\n");
  return 0;
}
