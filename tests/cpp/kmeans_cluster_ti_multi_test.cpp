// VaqHip::clusterTI(true) after setDevices({0, 0, 0}) (include/vaqhip.hpp: the k-means over the shards of a
// multi-device index, vaqhip_multi_cluster_ti_kmeans) against a fixture recorded from the reference's
// KMeans::staticFitCodebook: argv[1] holds the inputs and the expected centres, written by
// tests/test_kmeans_multi_gpu.py::test_cpp_adapter_cluster_ti_multi.
//   int32 N, M, L, bits, T, seg, iterations, nan_rows; codes N x M uint16; M codebooks (1 << bits) x L float;
//   centres T x (seg * L) float
#include "vaqhip.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int h[8];
  if (std::fread(h, 4, 8, f) != 8) return 2;
  const int N = h[0], M = h[1], L = h[2], bits = h[3], T = h[4], seg = h[5];
  vaqhip::VaqHip vaq;
  vaq.setDevices({0, 0, 0});
  vaq.mBitsAlloc.assign(M, bits);
  vaq.mCodebook = vaqhip::CodebookType((size_t)N, (size_t)M);
  if (std::fread(vaq.mCodebook.data(), 2, (size_t)N * M, f) != (size_t)N * M) return 2;
  for (int s = 0; s < M; s++) {
    vaq.mCentroidsPerSubs.emplace_back((size_t)1 << bits, (size_t)L);
    if (std::fread(vaq.mCentroidsPerSubs[s].data(), 4, ((size_t)L) << bits, f) != ((size_t)L) << bits) return 2;
  }
  std::vector<float> want((size_t)T * seg * L);
  if (std::fread(want.data(), 4, want.size(), f) != want.size()) return 2;
  std::fclose(f);

  char method[64];
  std::snprintf(method, sizeof method, "VAQ%dm%dmin%dmax%dvar1,EA_TI%dm%d", bits * M, M, bits, bits, T, seg);
  try {
    vaq.parseMethodString(method);
    vaq.clusterTI(true, false);
  } catch (const std::exception &e) {
    std::printf("clusterTI(true) threw: %s\n", e.what());
    return 1;
  }
  if ((int)vaq.mTIClusters.rows() != T || (int)vaq.mTIClusters.cols() != seg * L) {
    std::printf("mTIClusters is %zu x %zu\n", (size_t)vaq.mTIClusters.rows(), (size_t)vaq.mTIClusters.cols());
    return 1;
  }
  int bad = 0;
  for (size_t i = 0; i < want.size(); i++) {
    const float g = vaq.mTIClusters.data()[i];
    if (std::isnan(want[i]) ? !std::isnan(g) : std::memcmp(&g, &want[i], 4) != 0) bad++;
  }
  if (bad || vaq.mKMeansIterations != h[6] || vaq.mKMeansNanRows != h[7]) {
    std::printf("%d values differ; iterations %d (want %d), NaN centres %d (want %d)\n", bad, vaq.mKMeansIterations,
                h[6], vaq.mKMeansNanRows, h[7]);
    return 1;
  }
  if (!vaq.multiHandle() || vaq.handle()) {
    std::printf("clusterTI(true) did not run on the multi-device index\n");
    return 1;
  }
  vaqhip_multi_info info;
  if (vaqhip_multi_get_info(vaq.multiHandle(), &info) || info.n_devices != 3 || info.N != N) {
    std::printf("the multi index holds %lld rows on %d devices\n", (long long)info.N, info.n_devices);
    return 1;
  }
  // the shards are grouped already: a search answers without another clusterTI
  vaqhip::RowMatrixF q(2, (size_t)M * L);
  for (size_t i = 0; i < q.rows() * q.cols(); i++) q.data()[i] = 0.25f * (float)(i % 7) - 0.5f;
  auto ans = vaq.search(q, 5);
  for (int i = 0; i < 10; i++)
    if (ans.labels[i] < 0 || ans.labels[i] >= N) {
      std::printf("label %d out of range\n", ans.labels[i]);
      return 1;
    }
  std::printf("kmeans_cluster_ti_multi ok\n");
  return 0;
}
