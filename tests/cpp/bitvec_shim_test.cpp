// BitVecEngineHip::loadBitV / loadOriginal / query / queryRerank (include/vaqhip.hpp) compile and convert: the
// answers must be the ones tests/test_bitvec_gpu.py::test_cpp_shim wrote beside the inputs.  argv[1]:
//   int32 n, nq, W, D, k, factor; rows n x W uint64; queries nq x W uint64; raw rows n x D uint8; raw queries nq x D
//   float; query's labels nq x k int32 and distances nq x k uint32; queryRerank's labels nq x k int32 and distances
//   nq x k float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[6];
  if (std::fread(h, 4, 6, f) != 6) return 2;
  const int n = h[0], nq = h[1], W = h[2], D = h[3], k = h[4], factor = h[5];
  std::vector<uint64_t> rows, queries;
  std::vector<uint8_t> X;
  std::vector<float> XQ, rdist;
  std::vector<int32_t> ql, rl;
  std::vector<uint32_t> qd;
  if (!rd(f, rows, (size_t)n * W) || !rd(f, queries, (size_t)nq * W) || !rd(f, X, (size_t)n * D) ||
      !rd(f, XQ, (size_t)nq * D) || !rd(f, ql, (size_t)nq * k) || !rd(f, qd, (size_t)nq * k) || !rd(f, rl, (size_t)nq * k) ||
      !rd(f, rdist, (size_t)nq * k))
    return 2;
  std::fclose(f);
  vaqhip::bitvectors data((size_t)n, vaqhip::bitv((size_t)W)), qs((size_t)nq, vaqhip::bitv((size_t)W));
  for (int i = 0; i < n; i++) std::memcpy(data[i].data(), &rows[(size_t)i * W], (size_t)W * 8);
  for (int i = 0; i < nq; i++) std::memcpy(qs[i].data(), &queries[(size_t)i * W], (size_t)W * 8);
  vaqhip::RowMatrix<uint8_t> ori8((size_t)n, (size_t)D);
  vaqhip::RowMatrixF ori((size_t)n, (size_t)D), oq((size_t)nq, (size_t)D);
  std::memcpy(ori8.data(), X.data(), X.size());
  for (size_t i = 0; i < X.size(); i++) ori.data()[i] = (float)X[i];
  std::memcpy(oq.data(), XQ.data(), XQ.size() * 4);
  try {
    vaqhip::BitVecEngineHip e;
    e.loadBitV(data);
    const auto a = e.query(qs, k, vaqhip::BitVecEngineHip::QueryMethod::Sort);
    if ((int)a.size() != nq) return 1;
    for (int q = 0; q < nq; q++) {
      if ((int)a[q].size() != k) return 1;
      for (int i = 0; i < k; i++)
        if (a[q][i].idx != ql[(size_t)q * k + i] || a[q][i].dist != qd[(size_t)q * k + i]) {
          std::printf("query: query %d slot %d is (%d, %u)\n", q, i, a[q][i].idx, a[q][i].dist);
          return 1;
        }
    }
    for (const bool bytes : {true, false}) {
      if (bytes) e.loadOriginal(ori8);
      else e.loadOriginal(ori);
      const auto r = e.queryRerank(qs, oq, k, factor);
      for (int q = 0; q < nq; q++) {
        if ((int)r[q].size() != k) return 1;
        for (int i = 0; i < k; i++)
          if (r[q][i].idx != rl[(size_t)q * k + i] || r[q][i].dist != rdist[(size_t)q * k + i]) {
            std::printf("queryRerank (bytes %d): query %d slot %d is (%d, %g)\n", (int)bytes, q, i, r[q][i].idx, r[q][i].dist);
            return 1;
          }
      }
    }
    // a method that is not provided throws, as parseMethodString does for a token it does not serve
    bool threw = false;
    try {
      e.query(qs, k, vaqhip::BitVecEngineHip::QueryMethod::Heap);
    } catch (const vaqhip::Error &err) {
      threw = err.code == VAQHIP_EUNSUPPORTED;
    }
    if (!threw) {
      std::printf("QueryMethod::Heap did not throw EUNSUPPORTED\n");
      return 1;
    }
  } catch (const std::exception &ex) {
    std::printf("threw: %s\n", ex.what());
    return 1;
  }
  std::printf("bitvec_shim ok\n");
  return 0;
}
