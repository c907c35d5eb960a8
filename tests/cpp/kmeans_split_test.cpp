// The host arithmetic of the k-means over the shards of a multi-device index (vaq_amd/csrc/kmeans_sample.h): the
// sample of KMeans::staticFitCodebook split over contiguous shards, and the slices of the assign step.  No HIP:
// built with plain g++ by tests/test_kmeans_multi_cpu.py.
//   kmeans_split_test N T G [appended]
// shards as vaqhip_multi_set_codes_u16 cuts N - appended rows over G devices, the appended rows then joining the
// last shard (vaqhip_multi_add_codes_u16).  Prints one line per sample position, "pos row shard local", then
// "slice g begin end" per device, and ends with "kmeans_split ok" when every sample position lies in exactly one
// shard at the right local row and the slices tile the sample.
#include "kmeans_sample.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const int64_t N = std::atoll(argv[1]);
  const int T = std::atoi(argv[2]), G = std::atoi(argv[3]);
  const int64_t appended = argc > 4 ? std::atoll(argv[4]) : 0;
  if (G < 1 || G > 16 || appended > N) return 2;
  int64_t lo[16], n[16];
  const int64_t first = N - appended, per = (first + G - 1) / G;
  for (int g = 0; g < G; g++) {
    lo[g] = std::min<int64_t>(first, (int64_t)g * per);
    n[g] = std::min<int64_t>(first, (int64_t)(g + 1) * per) - lo[g];
  }
  n[G - 1] += appended;

  const int rows = vaq::kmeans_sample_rows(N, T);
  std::vector<int> sample;
  if (N > rows) sample = vaq::permutation_head(N, rows);
  const std::vector<vaq::KmeansShardSample> split = vaq::kmeans_split_sample(sample, lo, n, G);
  std::vector<int> owner((size_t)rows, -1), local((size_t)rows, -1);
  int bad = 0;
  for (int g = 0; g < G; g++) {
    const vaq::KmeansShardSample &s = split[(size_t)g];
    if (s.local.size() != s.pos.size()) bad++;
    if (sample.empty()) {  // all rows: the shard's rows are the sample positions [lo, lo + n)
      if (!s.pos.empty()) bad++;
      for (int64_t i = 0; i < n[g]; i++) {
        if (owner[(size_t)(lo[g] + i)] != -1) bad++;
        owner[(size_t)(lo[g] + i)] = g;
        local[(size_t)(lo[g] + i)] = (int)i;
      }
      continue;
    }
    for (size_t i = 0; i < s.pos.size(); i++) {
      if (i > 0 && s.pos[i] <= s.pos[i - 1]) bad++;  // sample order
      if (s.pos[i] < 0 || s.pos[i] >= rows || owner[(size_t)s.pos[i]] != -1) {
        bad++;
        continue;
      }
      owner[(size_t)s.pos[i]] = g;
      local[(size_t)s.pos[i]] = s.local[i];
    }
  }
  for (int i = 0; i < rows; i++) {
    const int64_t row = sample.empty() ? i : sample[(size_t)i];
    const int g = owner[(size_t)i];
    if (g < 0 || local[(size_t)i] < 0 || local[(size_t)i] >= n[g] || lo[g] + local[(size_t)i] != row) bad++;
    std::printf("%d %lld %d %d\n", i, (long long)row, g, local[(size_t)i]);
  }
  int next = 0;
  for (int g = 0; g < G; g++) {
    int b = -1, e = -1;
    vaq::kmeans_assign_slice(rows, G, g, &b, &e);
    if (b != next || e < b || e - b > (rows + G - 1) / G) bad++;
    next = e;
    std::printf("slice %d %d %d\n", g, b, e);
  }
  if (next != rows) bad++;
  if (bad) {
    std::printf("%d checks failed\n", bad);
    return 1;
  }
  std::printf("kmeans_split ok\n");
  return 0;
}
