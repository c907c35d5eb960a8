// learnQuantization's device forms through the C++ adapter (include/vaqhip.hpp) against the float overload over the
// same rows widened: VaqHipFast::learnQuantization(RowMatrix<uint8_t>, ratio) and learnQuantizationRefineDataset(ratio)
// over a byte and a float refiner, on one device and after setDevices({0, 0, 0}): mOffsets, mScale and the answers of a
// FAST search.  argv[1] holds the inputs, written by tests/test_learn_device_gpu.py::test_cpp_shim:
//   int32 N, M, L, bits, nq; M codebooks (1 << bits) x L float; eigenvectors D x D float; raw rows N x D uint8;
//   queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const vaqhip::LabelDistVecF &a, const vaqhip::LabelDistVecF &b) {
  return !a.labels.empty() && a.labels == b.labels && a.distances.size() == b.distances.size() &&
         std::memcmp(a.distances.data(), b.distances.data(), a.distances.size() * 4) == 0;
}
static bool same_floats(const std::vector<float> &a, const std::vector<float> &b) {
  return !a.empty() && a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[5];
  if (std::fread(h, 4, 5, f) != 5) return 2;
  const int N = h[0], M = h[1], L = h[2], bits = h[3], nq = h[4], D = M * L;
  std::vector<vaqhip::RowMatrixF> cents;
  for (int s = 0; s < M; s++) {
    cents.emplace_back((size_t)1 << bits, (size_t)L);
    if (std::fread(cents[s].data(), 4, ((size_t)L) << bits, f) != ((size_t)L) << bits) return 2;
  }
  vaqhip::RowMatrixF eig((size_t)D, (size_t)D), base((size_t)N, (size_t)D), q((size_t)nq, (size_t)D);
  vaqhip::RowMatrix<uint8_t> base8((size_t)N, (size_t)D);
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base8.data(), 1, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  for (size_t i = 0; i < (size_t)N * D; i++) base.data()[i] = (float)base8.data()[i];
  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,FAST", bits * M, M, bits, bits);
  const float ratio = 0.1f;
  const int k = 10;
  try {
    // host float, host bytes, byte refiner, float refiner; the last three again over three shards
    vaqhip::VaqHipFast one, one8, oneR8, oneRf, many8, manyR8, manyRf;
    for (vaqhip::VaqHipFast *v : {&many8, &manyR8, &manyRf}) v->setDevices({0, 0, 0});
    for (vaqhip::VaqHipFast *v : {&one, &one8, &oneR8, &oneRf, &many8, &manyR8, &manyRf}) {
      v->parseMethodString(method);
      v->mBitsAlloc.assign(M, bits);
      v->mCentroidsPerSubs = cents;
      v->mEigenVectors = eig;
      v->encode(base8, false);
    }
    try {
      one.learnQuantizationRefineDataset(ratio);
      std::printf("learnQuantizationRefineDataset without setRefineDataset did not throw\n");
      return 1;
    } catch (const vaqhip::Error &e) {
      if (e.code != VAQHIP_ESTATE) return std::printf("without rows: code %d\n", e.code), 1;
    }
    one.learnQuantization(base, ratio);
    one8.learnQuantization(base8, ratio);
    many8.learnQuantization(base8, ratio);
    for (vaqhip::VaqHipFast *v : {&oneR8, &manyR8}) v->setRefineDataset(base8);
    for (vaqhip::VaqHipFast *v : {&oneRf, &manyRf}) v->setRefineDataset(base);
    for (vaqhip::VaqHipFast *v : {&oneR8, &oneRf, &manyR8, &manyRf}) v->learnQuantizationRefineDataset(ratio);
    if (!manyR8.multiRefinerHandle() || !oneR8.refinerHandle() || oneR8.multiRefinerHandle()) {
      std::printf("the refiners are not where setDevices() puts them\n");
      return 1;
    }
    const auto want = one.search(q, k);
    if (want.labels.size() != (size_t)nq * k) return std::printf("no answer from the float form\n"), 1;
    const char *names[] = {"bytes", "byte refiner", "float refiner", "bytes, sharded", "byte refiner, sharded",
                           "float refiner, sharded"};
    int i = 0;
    for (vaqhip::VaqHipFast *v : {&one8, &oneR8, &oneRf, &many8, &manyR8, &manyRf}) {
      if (!same_floats(v->mOffsets, one.mOffsets) || !same_floats(v->mScale, one.mScale))
        return std::printf("%s: mOffsets / mScale differ from the float form's\n", names[i]), 1;
      if (!same(want, v->search(q, k))) return std::printf("%s: the FAST search differs\n", names[i]), 1;
      i++;
    }
    // a failed learn leaves mOffsets / mScale as they were
    const std::vector<float> keep = one8.mOffsets;
    try {
      one8.learnQuantization(base8, 1.5f);
      return std::printf("a ratio above 1 did not throw\n"), 1;
    } catch (const vaqhip::Error &e) {
      if (e.code != VAQHIP_EINVAL || !same_floats(one8.mOffsets, keep)) return std::printf("after a refused learn\n"), 1;
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("learn_shim ok\n");
  return 0;
}
