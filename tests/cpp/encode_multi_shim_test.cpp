// VaqHip::encode(XTrain, projected) after setDevices({0, 0, 0}) (include/vaqhip.hpp: it goes through
// vaqhip_multi_encode_set_codes, every shard encoding the rows it will hold) and encodeRefineDataset() (the refiner
// form, over the rows setRefineDataset left on the devices) against encode() on a single-device VaqHip: mCodebook code
// for code, search() answers slot for slot, and the sharded index holds the rows without a second upload.  argv[1]
// holds the inputs, written by tests/test_encode_multi_gpu.py::test_cpp_shim:
//   int32 N, M, L, bits, nq; M codebooks (1 << bits) x L float; eigenvectors D x D float; raw rows N x D float;
//   queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const vaqhip::LabelDistVecF &a, const vaqhip::LabelDistVecF &b) {
  return a.labels == b.labels && a.distances.size() == b.distances.size() &&
         std::memcmp(a.distances.data(), b.distances.data(), a.distances.size() * 4) == 0;
}

static bool same_codes(const vaqhip::CodebookType &a, const vaqhip::CodebookType &b) {
  return a.rows() == b.rows() && a.cols() == b.cols() && std::memcmp(a.data(), b.data(), a.rows() * a.cols() * 2) == 0;
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
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,HEAP", bits * M, M, bits, bits);
  try {
    vaqhip::VaqHip one, many, resident;
    many.setDevices({0, 0, 0});
    resident.setDevices({0, 0, 0});
    for (vaqhip::VaqHip *v : {&one, &many, &resident}) {
      v->parseMethodString(method);
      v->mBitsAlloc.assign(M, bits);
      v->mCentroidsPerSubs = cents;
      v->mEigenVectors = eig;
      v->mIdBase = 1000;
    }
    try {
      one.encodeRefineDataset();
      std::printf("encodeRefineDataset on one device did not throw\n");
      return 1;
    } catch (const vaqhip::Error &e) {
      if (e.code != VAQHIP_EUNSUPPORTED) {
        std::printf("encodeRefineDataset on one device threw %d\n", e.code);
        return 1;
      }
    }
    one.encode(base, false);
    many.encode(base, false);
    resident.setRefineDataset(base);
    resident.encodeRefineDataset();
    if ((int)one.mCodebook.rows() != N || !same_codes(one.mCodebook, many.mCodebook) ||
        !same_codes(one.mCodebook, resident.mCodebook)) {
      std::printf("mCodebook differs from the single device's\n");
      return 1;
    }
    // the shards hold the rows already: the multi index exists and reports them before any search
    for (vaqhip::VaqHip *v : {&many, &resident}) {
      vaqhip_multi_info info;
      if (!v->multiHandle() || vaqhip_multi_get_info(v->multiHandle(), &info) || info.N != N || info.id_base != 1000 ||
          info.shard_rows[0] + info.shard_rows[1] + info.shard_rows[2] != N) {
        std::printf("the shards do not hold the encoded rows\n");
        return 1;
      }
    }
    for (const bool exact : {false, true}) {
      for (vaqhip::VaqHip *v : {&one, &many, &resident}) v->exactTies = exact;
      for (const int k : {1, 10, 100}) {
        const auto a = one.search(q, k);
        if (a.labels.size() != (size_t)nq * k || !same(a, many.search(q, k)) || !same(a, resident.search(q, k))) {
          std::printf("exact_ties %d k %d: the sharded answer differs from the single device's\n", (int)exact, k);
          return 1;
        }
      }
    }
    // projected rows through the same call; then the fused search + refine over the rows the codes came from
    vaqhip::RowMatrixF proj((size_t)N, (size_t)D);
    if (vaqhip_project(one.handle(), base.data(), N, proj.data())) return 1;
    one.encode(proj, true);
    many.encode(proj, true);
    if (!same_codes(one.mCodebook, many.mCodebook) || !same_codes(one.mCodebook, resident.mCodebook)) {
      std::printf("projected rows: mCodebook differs\n");
      return 1;
    }
    if (!same(one.search(q, 10), many.search(q, 10))) {
      std::printf("projected rows: the sharded answer differs\n");
      return 1;
    }
    one.setRefineDataset(base);
    if (!same(one.search(q, 10, 100), resident.search(q, 10, 100))) {
      std::printf("search + refine after encodeRefineDataset differs from the single device's\n");
      return 1;
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("encode_multi_shim ok\n");
  return 0;
}
