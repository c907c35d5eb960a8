// BitVecEngineHip::computeClusterIndex and ::loadClusterInfoFromOriginal (include/vaqhip.hpp) compile and convert: the
// answers must be the ones tests/test_cluster_index_gpu.py::test_cpp_shim wrote beside the inputs.  argv[1]:
//   int32 n, nq, D, T, k, atleast; raw rows n x D uint8; raw queries nq x D float; centres T x D float; cluster of each
//   row n int32; labels nq x k int32 and squared distances nq x k float of queryNaiveWithClusterInfo over those clusters
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
  const int n = h[0], nq = h[1], D = h[2], T = h[3], k = h[4], atleast = h[5];
  std::vector<uint8_t> X;
  std::vector<float> XQ, cen, dist;
  std::vector<int32_t> idx, lab;
  if (!rd(f, X, (size_t)n * D) || !rd(f, XQ, (size_t)nq * D) || !rd(f, cen, (size_t)T * D) || !rd(f, idx, (size_t)n) ||
      !rd(f, lab, (size_t)nq * k) || !rd(f, dist, (size_t)nq * k))
    return 2;
  std::fclose(f);
  vaqhip::RowMatrix<uint8_t> ori8((size_t)n, (size_t)D);
  vaqhip::RowMatrixF oq((size_t)nq, (size_t)D);
  std::memcpy(ori8.data(), X.data(), X.size());
  std::memcpy(oq.data(), XQ.data(), XQ.size() * 4);
  vaqhip::Matrixf centres((size_t)T, std::vector<float>((size_t)D));
  for (int c = 0; c < T; c++) std::memcpy(centres[c].data(), &cen[(size_t)c * D], (size_t)D * 4);
  try {
    vaqhip::BitVecEngineHip e;
    e.loadBitV(vaqhip::bitvectors((size_t)n, vaqhip::bitv(1)));  // the bits are never read
    e.loadOriginal(ori8);
    e.loadCentroids(centres);
    std::vector<int> got;
    e.computeClusterIndex(got);
    if (got != std::vector<int>(idx.begin(), idx.end())) {
      std::printf("computeClusterIndex differs\n");
      return 1;
    }
    e.loadClusterInfoFromOriginal();
    const auto a = e.queryNaiveWithClusterInfo(oq, k, vaqhip::BitVecEngineHip::QueryMethod::Sort, atleast);
    if ((int)a.size() != nq) return 1;
    for (int q = 0; q < nq; q++)
      for (int i = 0; i < k; i++)
        if ((int)a[q].size() != k || a[q][i].idx != lab[(size_t)q * k + i] ||
            a[q][i].dist != dist[(size_t)q * k + i]) {
          std::printf("query %d slot %d differs\n", q, i);
          return 1;
        }
  } catch (const std::exception &ex) {
    std::printf("threw: %s\n", ex.what());
    return 1;
  }
  std::printf("cluster_index_shim ok\n");
  return 0;
}
