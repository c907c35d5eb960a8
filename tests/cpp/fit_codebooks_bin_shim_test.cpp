// VaqHip with mBinaryKmeans (include/vaqhip.hpp): fitCodebooks and fitCodebooksRefineDataset return
// vaqhip_fit_codebooks_bin's centres bit for bit; with mHierarchicalKmeans set as well the result is the hierarchical
// one (the reference's if / else if); after setDevices() the flag is refused.  argv[1] holds the inputs, written by
// tests/test_codebooks_bin_gpu.py::test_cpp_shim:
//   int32 N, D, M; bits M x int32; eigenvectors D x D float; raw rows N x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const vaqhip::VaqHip &v, const std::vector<float> &cent, const std::vector<int> &iters,
                 const std::vector<int> &nan, const char *what) {
  bool ok = v.mCodebookIters == iters && v.mCodebookNanRows == nan;
  size_t off = 0;
  for (size_t s = 0; ok && s < v.mCentroidsPerSubs.size(); s++) {
    const auto &x = v.mCentroidsPerSubs[s];
    const size_t floats = x.rows() * x.cols();
    ok = off + floats <= cent.size() && std::memcmp(x.data(), cent.data() + off, floats * 4) == 0;
    off += floats;
  }
  ok = ok && off == cent.size();
  if (!ok) std::printf("%s: the adapter's centres differ from the C call's\n", what);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[3];
  if (std::fread(h, 4, 3, f) != 3) return 2;
  const int N = h[0], D = h[1], M = h[2], L = D / M;
  std::vector<int> bits((size_t)M);
  if (std::fread(bits.data(), 4, (size_t)M, f) != (size_t)M) return 2;
  vaqhip::RowMatrixF eig((size_t)D, (size_t)D), base((size_t)N, (size_t)D);
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  std::fclose(f);
  size_t floats = 0;
  for (int b : bits) floats += ((size_t)1 << b) * L;
  std::vector<float> bin(floats), hier(floats);
  std::vector<int> bi((size_t)M), bn((size_t)M), hi((size_t)M), hn((size_t)M);
  if (vaqhip_fit_codebooks_bin(0, base.data(), N, D, M, bits.data(), eig.data(), 25, bin.data(), bi.data(), bn.data()) ||
      vaqhip_fit_codebooks_hier(0, base.data(), N, D, M, bits.data(), eig.data(), 25, hier.data(), hi.data(), hn.data())) {
    std::printf("the C calls failed: %s\n", vaqhip_last_error());
    return 1;
  }
  if (bin == hier) {
    std::printf("the case holds no subspace above 8 bits\n");
    return 1;
  }
  try {
    vaqhip::VaqHip v;
    v.mBitsAlloc = bits;
    v.mEigenVectors = eig;
    v.mBinaryKmeans = true;
    v.fitCodebooks(base);
    if (!same(v, bin, bi, bn, "fitCodebooks, mBinaryKmeans")) return 1;
    v.mCentroidsPerSubs.clear();
    v.setRefineDataset(base);
    v.fitCodebooksRefineDataset();
    if (!same(v, bin, bi, bn, "fitCodebooksRefineDataset, mBinaryKmeans")) return 1;
    v.mHierarchicalKmeans = true;  // both: the hierarchical fit wins
    v.fitCodebooksRefineDataset();
    if (!same(v, hier, hi, hn, "fitCodebooksRefineDataset, both flags")) return 1;
    vaqhip::VaqHip both;
    both.mBitsAlloc = bits;
    both.mEigenVectors = eig;
    both.mBinaryKmeans = both.mHierarchicalKmeans = true;
    both.fitCodebooks(base);
    if (!same(both, hier, hi, hn, "fitCodebooks, both flags")) return 1;
    vaqhip::VaqHip many;
    many.mBitsAlloc = bits;
    many.mEigenVectors = eig;
    many.mBinaryKmeans = true;
    many.setDevices({0, 0});
    bool refused = false;
    try {
      many.fitCodebooks(base);
    } catch (const vaqhip::Error &e) {
      refused = e.code == VAQHIP_EUNSUPPORTED;
    }
    if (!refused) {
      std::printf("mBinaryKmeans after setDevices() was not refused as unsupported\n");
      return 1;
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("fit_codebooks_bin_shim ok\n");
  return 0;
}
