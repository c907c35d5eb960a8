// The byte-row overloads of the C++ adapter (include/vaqhip.hpp) against the float overloads over the same rows
// widened: VaqHip::encode(RowMatrix<uint8_t>, projected) on one device and after setDevices({0, 0, 0}), then the
// answers of search(); BitVecEngineHip::binaryEncodingLUT(RowMatrix<uint8_t>, codebookOut) on one device and after
// setDevices({0, 0}): centroidsMat, quantiles, codebookOut, and queryLUT's answers.  argv[1] holds the inputs, written
// by tests/test_build_u8_gpu.py::test_cpp_shim:
//   int32 N, M, L, bits, nq; M codebooks (1 << bits) x L float; eigenvectors D x D float; raw rows N x D uint8;
//   queries nq x D float; D bits of the engine's allocation (int32)
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
static bool same_codes(const vaqhip::CodebookType &a, const vaqhip::CodebookType &b) {
  return a.rows() > 0 && a.rows() == b.rows() && a.cols() == b.cols() &&
         std::memcmp(a.data(), b.data(), a.rows() * a.cols() * 2) == 0;
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
  std::vector<int> engine_bits((size_t)D);
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base8.data(), 1, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  if (std::fread(engine_bits.data(), 4, (size_t)D, f) != (size_t)D) return 2;
  std::fclose(f);
  bool high = false, zero = false, full = false;
  for (size_t i = 0; i < (size_t)N * D; i++) {
    const uint8_t b = base8.data()[i];
    base.data()[i] = (float)b;
    high = high || b >= 128, zero = zero || b == 0, full = full || b == 255;
  }
  if (!high || !zero || !full) {
    std::printf("the rows do not hold 0, 255 and a value >= 128\n");
    return 1;
  }
  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,HEAP", bits * M, M, bits, bits);
  try {
    vaqhip::VaqHip one8, one, many8, many;
    many8.setDevices({0, 0, 0});
    many.setDevices({0, 0, 0});
    for (vaqhip::VaqHip *v : {&one8, &one, &many8, &many}) {
      v->parseMethodString(method);
      v->mBitsAlloc.assign(M, bits);
      v->mCentroidsPerSubs = cents;
      v->mEigenVectors = eig;
    }
    for (const bool projected : {false, true}) {
      one.encode(base, projected);
      one8.encode(base8, projected);
      many.encode(base, projected);
      many8.encode(base8, projected);
      if ((int)one.mCodebook.rows() != N || !same_codes(one8.mCodebook, one.mCodebook) ||
          !same_codes(many8.mCodebook, one.mCodebook) || !same_codes(many.mCodebook, one.mCodebook)) {
        std::printf("projected %d: encode over byte rows differs from the float rows'\n", (int)projected);
        return 1;
      }
      for (const int k : {1, 10}) {
        const auto a = one.search(q, k);
        if (a.labels.size() != (size_t)nq * k || !same(a, one8.search(q, k)) || !same(a, many8.search(q, k)) ||
            !same(a, many.search(q, k))) {
          std::printf("projected %d k %d: search after encode over byte rows differs\n", (int)projected, k);
          return 1;
        }
      }
    }
    vaqhip::BitVecEngineHip e, e8, m, m8;
    m.setDevices({0, 0});
    m8.setDevices({0, 0});
    vaqhip::CodebookType cb, cb8, mcb, mcb8;
    for (vaqhip::BitVecEngineHip *x : {&e, &e8, &m, &m8}) {
      x->solutionX = engine_bits;
      x->eigenVectors = eig;
      x->exactTies = true;
    }
    e.binaryEncodingLUT(base, cb);
    e8.binaryEncodingLUT(base8, cb8);
    m.binaryEncodingLUT(base, mcb);
    m8.binaryEncodingLUT(base8, mcb8);
    for (vaqhip::BitVecEngineHip *x : {&e8, &m, &m8})
      if (!same_floats(x->centroidsMat, e.centroidsMat) || !same_floats(x->quantiles, e.quantiles)) {
        std::printf("binaryEncodingLUT: centroidsMat or quantiles differ from the float rows' on one device\n");
        return 1;
      }
    if ((int)cb.rows() != N || !same_codes(cb8, cb) || !same_codes(mcb, cb) || !same_codes(mcb8, cb)) {
      std::printf("binaryEncodingLUT: codebookOut over byte rows differs from the float rows'\n");
      return 1;
    }
    const auto want = e.queryLUT(q, 10, cb);
    for (vaqhip::BitVecEngineHip *x : {&e8, &m8}) {
      const auto got = x->queryLUT(q, 10, cb8);
      if (got.size() != want.size()) return 1;
      for (size_t i = 0; i < want.size(); i++) {
        if (got[i].size() != want[i].size() || want[i].empty()) return 1;
        for (size_t j = 0; j < want[i].size(); j++)
          if (got[i][j].idx != want[i][j].idx || std::memcmp(&got[i][j].dist, &want[i][j].dist, 4) != 0) {
            std::printf("queryLUT after the byte build differs at query %zu slot %zu\n", i, j);
            return 1;
          }
      }
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("build_u8_shim ok\n");
  return 0;
}
