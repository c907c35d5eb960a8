// BitVecEngineHip after setDevices({0, 0}) (include/vaqhip.hpp: binaryEncodingLUT fits over the devices, builds a
// sequential-sum multi index, gives it Q and encodes across the shards; queryLUT answers from the multi index) against
// the same engine on one device: centroidsMat, quantiles, codebookOut bit for bit and the queryLUT answers slot for
// slot.  argv[1] holds the inputs, written by tests/test_lutfit_multi_gpu.py::test_cpp_shim:
//   int32 N, D, nq; bits D x int32; eigenvectors D x D float; raw rows N x D float; queries nq x D float
#include "vaqhip.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

template <class T> static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[3];
  if (std::fread(h, 4, 3, f) != 3) return 2;
  const int N = h[0], D = h[1], nq = h[2];
  std::vector<int> bits((size_t)D);
  if (std::fread(bits.data(), 4, (size_t)D, f) != (size_t)D) return 2;
  vaqhip::RowMatrixF eig((size_t)D, (size_t)D), base((size_t)N, (size_t)D), q((size_t)nq, (size_t)D);
  if (std::fread(eig.data(), 4, (size_t)D * D, f) != (size_t)D * D) return 2;
  if (std::fread(base.data(), 4, (size_t)N * D, f) != (size_t)N * D) return 2;
  if (std::fread(q.data(), 4, (size_t)nq * D, f) != (size_t)nq * D) return 2;
  std::fclose(f);
  try {
    vaqhip::BitVecEngineHip one, many;
    many.setDevices({0, 0});
    vaqhip::CodebookType cb_one, cb_many;
    for (vaqhip::BitVecEngineHip *e : {&one, &many}) {
      e->solutionX = bits;
      e->eigenVectors = eig;
    }
    one.binaryEncodingLUT(base, cb_one);
    many.binaryEncodingLUT(base, cb_many);
    if (one.multiHandle() || !many.multiHandle()) {
      std::printf("setDevices did not choose the multi index\n");
      return 1;
    }
    if (!same_bytes(one.centroidsMat, many.centroidsMat) || !same_bytes(one.quantiles, many.quantiles)) {
      std::printf("centroidsMat / quantiles differ from the single device's\n");
      return 1;
    }
    if ((int)cb_one.rows() != N || cb_one.rows() != cb_many.rows() || cb_one.cols() != cb_many.cols() ||
        std::memcmp(cb_one.data(), cb_many.data(), cb_one.rows() * cb_one.cols() * 2) != 0) {
      std::printf("codebookOut differs from the single device's\n");
      return 1;
    }
    vaqhip_multi_info info;
    if (vaqhip_multi_get_info(many.multiHandle(), &info) || info.N != N || info.n_devices != 2 ||
        info.shard_rows[0] + info.shard_rows[1] != N) {
      std::printf("the shards do not hold the encoded rows\n");
      return 1;
    }
    for (const bool exact : {false, true}) {
      one.exactTies = many.exactTies = exact;
      for (const int k : {1, 10}) {
        const auto a = one.queryLUT(q, k, cb_one), b = many.queryLUT(q, k, cb_many);
        if ((int)a.size() != nq || a.size() != b.size()) return 1;
        for (int i = 0; i < nq; i++) {
          if (a[i].size() != b[i].size() || a[i].size() != (size_t)k ||
              std::memcmp(a[i].data(), b[i].data(), a[i].size() * sizeof(vaqhip::IdxDistPairFloat)) != 0) {
            std::printf("exact_ties %d k %d query %d: the sharded answer differs from the single device's\n", (int)exact, k, i);
            return 1;
          }
        }
      }
    }
  } catch (const std::exception &e) {
    std::printf("threw: %s\n", e.what());
    return 1;
  }
  std::printf("lutfit_multi_shim ok\n");
  return 0;
}
