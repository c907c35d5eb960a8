// VaqHip::setRefineDataset(RowMatrix<uint8_t>) (include/vaqhip.hpp: the raw rows stay the bytes a bvecs file holds)
// against the float overload over the same rows widened: search(XTest, k, refineNum), searchExhaustive and, after
// setDevices({0, 0}), encodeRefineDataset(), on one device and across two logical shards, with refineExactTies off and
// on.  argv[1] holds the inputs, written by tests/test_refine_u8_multi_gpu.py::test_cpp_shim:
//   int32 N, M, L, bits, nq; codes N x M uint16; M codebooks (1 << bits) x L float; raw rows N x D uint8;
//   queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const vaqhip::LabelDistVecF &a, const vaqhip::LabelDistVecF &b) {
  return !a.labels.empty() && a.labels == b.labels && a.distances.size() == b.distances.size() &&
         std::memcmp(a.distances.data(), b.distances.data(), a.distances.size() * 4) == 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[5];
  if (std::fread(h, 4, 5, f) != 5) return 2;
  const int N = h[0], M = h[1], L = h[2], bits = h[3], nq = h[4], D = M * L;
  vaqhip::CodebookType codes((size_t)N, (size_t)M);
  if (std::fread(codes.data(), 2, (size_t)N * M, f) != (size_t)N * M) return 2;
  std::vector<vaqhip::RowMatrixF> cents;
  for (int s = 0; s < M; s++) {
    cents.emplace_back((size_t)1 << bits, (size_t)L);
    if (std::fread(cents[s].data(), 4, ((size_t)L) << bits, f) != ((size_t)L) << bits) return 2;
  }
  vaqhip::RowMatrix<uint8_t> base8((size_t)N, (size_t)D);
  vaqhip::RowMatrixF base((size_t)N, (size_t)D), q((size_t)nq, (size_t)D);
  if (std::fread(base8.data(), 1, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  for (size_t i = 0; i < (size_t)N * D; i++) base.data()[i] = (float)base8.data()[i];
  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,HEAP", bits * M, M, bits, bits);
  try {
    vaqhip::VaqHip one8, one, many8, many;
    many8.setDevices({0, 0});
    many.setDevices({0, 0});
    for (vaqhip::VaqHip *v : {&one8, &one, &many8, &many}) {
      v->parseMethodString(method);
      v->mBitsAlloc.assign(M, bits);
      v->mCodebook = codes;
      v->mCentroidsPerSubs = cents;
    }
    one8.setRefineDataset(base8);
    many8.setRefineDataset(base8);
    one.setRefineDataset(base);
    many.setRefineDataset(base);
    if (vaqhip_refiner_elem_size(one8.refinerHandle()) != 1 || vaqhip_refiner_elem_size(one.refinerHandle()) != 4 ||
        vaqhip_multi_refiner_elem_size(many8.multiRefinerHandle()) != 1 ||
        vaqhip_multi_refiner_elem_size(many.multiRefinerHandle()) != 4) {
      std::printf("setRefineDataset left rows of the wrong element type\n");
      return 1;
    }
    for (const bool exact : {false, true}) {
      for (vaqhip::VaqHip *v : {&one8, &one, &many8, &many}) v->exactTies = v->refineExactTies = exact;
      const auto a = one.search(q, 10, 100);
      if (a.labels.size() != (size_t)nq * 10 || !same(a, one8.search(q, 10, 100)) || !same(a, many8.search(q, 10, 100)) ||
          !same(a, many.search(q, 10, 100))) {
        std::printf("exact_ties %d: search + refine over byte rows differs from the float rows'\n", (int)exact);
        return 1;
      }
      for (const int k : {1, 10, 100}) {
        const auto e = one.searchExhaustive(q, k);
        if (e.labels.size() != (size_t)nq * k || !same(e, one8.searchExhaustive(q, k)) ||
            !same(e, many8.searchExhaustive(q, k))) {
          std::printf("exact_ties %d k %d: searchExhaustive over byte rows differs from the float rows'\n", (int)exact, k);
          return 1;
        }
      }
    }
    // the byte overload switches a refiner that held float rows, and back
    one.setRefineDataset(base8);
    if (vaqhip_refiner_elem_size(one.refinerHandle()) != 1 || !same(one.searchExhaustive(q, 10), one8.searchExhaustive(q, 10))) {
      std::printf("setRefineDataset(bytes) after setRefineDataset(floats) differs\n");
      return 1;
    }
    // encodeRefineDataset() after the byte overload: the codes of the float overload's rows, and the same answers
    many8.encodeRefineDataset();
    many.encodeRefineDataset();
    if ((int)many.mCodebook.rows() != N || many8.mCodebook.rows() != many.mCodebook.rows() ||
        std::memcmp(many8.mCodebook.data(), many.mCodebook.data(), (size_t)N * M * 2) != 0) {
      std::printf("encodeRefineDataset over byte rows: mCodebook differs from the float rows'\n");
      return 1;
    }
    if (!same(many.search(q, 10, 100), many8.search(q, 10, 100))) {
      std::printf("search + refine after encodeRefineDataset differs\n");
      return 1;
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("refine_u8_shim ok\n");
  return 0;
}
