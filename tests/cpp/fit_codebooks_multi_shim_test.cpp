// VaqHip after setDevices({0, 0, 0}) (include/vaqhip.hpp: fitCodebooks routes to vaqhip_multi_fit_codebooks,
// fitCodebooksRefineDataset fits over the multi refiner's shards) against the same adapter on one device:
// mCentroidsPerSubs bit for bit, mCodebookIters and mCodebookNanRows.  argv[1] holds the inputs, written by
// tests/test_codebooks_multi_gpu.py::test_cpp_shim:
//   int32 N, D, M; bits M x int32; eigenvectors D x D float; raw rows N x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static bool same_fit(const vaqhip::VaqHip &a, const vaqhip::VaqHip &b, const char *what) {
  bool ok = a.mCentroidsPerSubs.size() == b.mCentroidsPerSubs.size() && a.mCodebookIters == b.mCodebookIters &&
            a.mCodebookNanRows == b.mCodebookNanRows;
  for (size_t s = 0; ok && s < a.mCentroidsPerSubs.size(); s++) {
    const auto &x = a.mCentroidsPerSubs[s], &y = b.mCentroidsPerSubs[s];
    ok = x.rows() == y.rows() && x.cols() == y.cols() && std::memcmp(x.data(), y.data(), x.rows() * x.cols() * 4) == 0;
  }
  if (!ok) std::printf("%s: the sharded fit differs from the single device's\n", what);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[3];
  if (std::fread(h, 4, 3, f) != 3) return 2;
  const int N = h[0], D = h[1], M = h[2];
  std::vector<int> bits((size_t)M);
  if (std::fread(bits.data(), 4, (size_t)M, f) != (size_t)M) return 2;
  vaqhip::RowMatrixF eig((size_t)D, (size_t)D), base((size_t)N, (size_t)D);
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  std::fclose(f);
  try {
    vaqhip::VaqHip one, many;
    many.setDevices({0, 0, 0});
    for (vaqhip::VaqHip *v : {&one, &many}) {
      v->mBitsAlloc = bits;
      v->mEigenVectors = eig;
    }
    one.fitCodebooks(base);
    many.fitCodebooks(base);
    if (one.mCentroidsPerSubs.size() != (size_t)M || !same_fit(one, many, "fitCodebooks")) return 1;
    vaqhip_multi_fit_codebooks_timing t;
    if (vaqhip_multi_last_fit_codebooks_timing(&t) || t.n_devices != 3 || t.subspaces != M || t.rows != N) {
      std::printf("fitCodebooks after setDevices did not take the sharded call\n");
      return 1;
    }
    many.mCentroidsPerSubs.clear();
    many.setRefineDataset(base);
    if (!many.multiRefinerHandle()) {
      std::printf("setDevices did not choose the multi refiner\n");
      return 1;
    }
    many.fitCodebooksRefineDataset();
    if (!same_fit(one, many, "fitCodebooksRefineDataset")) return 1;
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("fit_codebooks_multi_shim ok\n");
  return 0;
}
