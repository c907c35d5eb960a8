// ti_exact_shim_test.cpp -- include/vaqhip.hpp's VaqHip with exactTies after clusterTI(): the reference's call
// order (codes, then clusterTI over given centres, then search) through the C++ adapter.
//
//   ti_exact_shim_test IN OUT
// IN:  int32 M, L, N, T, seg, nq, k, ea; float32 visit; int32 bits[M]; then float32 centroids (per subspace
//      (1 << bits) x L), uint16 codes N x M, float32 clusters T x seg * L, float32 queries nq x M * L
// OUT: int32 labels nq x k, float32 distances nq x k
// Built and run by tests/test_ti_exact_gpu.py, which compares OUT with the recorded fixture.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vaqhip.hpp"

using namespace vaqhip;

template <class T> static void rd(FILE *f, T *p, size_t n) {
  if (n > 0 && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "ti_exact_shim_test: short input\n");
    std::exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t h[8];
  float visit;
  rd(in, h, 8);
  rd(in, &visit, 1);
  const int M = h[0], L = h[1], N = h[2], T = h[3], seg = h[4], nq = h[5], k = h[6], ea = h[7];
  try {
    VaqHip v;
    v.mBitsAlloc.resize((size_t)M);
    rd(in, v.mBitsAlloc.data(), (size_t)M);
    for (int s = 0; s < M; s++) {
      RowMatrixF c((size_t)1 << v.mBitsAlloc[(size_t)s], (size_t)L);
      rd(in, c.data(), c.rows() * c.cols());
      v.mCentroidsPerSubs.push_back(c);
    }
    v.mCodebook = CodebookType((size_t)N, (size_t)M);
    rd(in, v.mCodebook.data(), (size_t)N * M);
    v.mTIClusterNum = T;
    v.mTISegmentNum = seg;
    v.mTIClusters = RowMatrixF((size_t)T, (size_t)seg * L);
    rd(in, v.mTIClusters.data(), (size_t)T * seg * L);
    RowMatrixF q((size_t)nq, (size_t)M * L);
    rd(in, q.data(), (size_t)nq * M * L);
    std::fclose(in);
    v.mMethods = ea ? VaqHip::NNMethod::EA : VaqHip::NNMethod::Heap;
    v.mVisit = visit;
    v.search(q, 1);   // the codes are on the device in the exhaustive order, as after encode()
    if (!ea) v.mMethods = 0;
    v.clusterTI();    // the centres are given: sets TI, the rows are regrouped at the next search
    v.exactTies = true;
    LabelDistVecF r = v.search(q, k);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(r.labels.data(), sizeof(int), r.labels.size(), out);
    std::fwrite(r.distances.data(), sizeof(float), r.distances.size(), out);
    if (std::fclose(out) != 0) return 2;
  } catch (const Error &e) {
    std::fprintf(stderr, "ti_exact_shim_test: %s\n", e.what());
    return 1;
  }
  std::printf("ti_exact_shim ok\n");
  return 0;
}
