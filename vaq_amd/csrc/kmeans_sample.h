// kmeans_sample.h -- the host arithmetic of the k-means of clusterTI (vaq_kmeans.hip) that both hosts share:
// which rows KMeans::staticFitCodebook samples, which shard of a multi-device index holds each of them, and
// which slice of the sample every device assigns; and what every k-means here reports of its centres (nan_rows).
// No HIP in here: tests/cpp/kmeans_split_test.cpp and tests/cpp/nan_rows_test.cpp run it on the CPU.
#ifndef VAQ_KMEANS_SAMPLE_H_
#define VAQ_KMEANS_SAMPLE_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <random>
#include <unordered_map>
#include <vector>

namespace vaq {

// KMeans::staticFitCodebook's sample: more than 256 rows per centre are cut to the first 256 * T of a permutation
constexpr int64_t KMEANS_ROWS_PER_CENTRE = 256;

// The first r entries of randomPermutation(n) (utils/Random.hpp:18-28, mt19937(13517106), i2 = i + mt() % (n - i)):
// entry i is final after step i, so r steps over a sparse map of the positions touched so far suffice.
inline std::vector<int> permutation_head(int64_t n, int64_t r) {
  r = std::min(r, n);
  std::vector<int> out((size_t)r);
  std::unordered_map<int, int> moved;
  std::mt19937 mt(13517106u);
  auto at = [&](int i) {
    auto it = moved.find(i);
    return it == moved.end() ? i : it->second;
  };
  for (int64_t i = 0; i < r; i++) {
    if (i + 1 < n) {
      const int i2 = (int)i + (int)(mt() % (unsigned)(int)(n - i));
      const int vi = at((int)i);
      out[i] = at(i2);
      moved[i2] = vi;
    } else {
      out[i] = at((int)i);
    }
  }
  return out;
}

// rows of the sample over N rows and T centres
inline int kmeans_sample_rows(int64_t N, int T) { return (int)std::min<int64_t>(N, KMEANS_ROWS_PER_CENTRE * T); }

// The sample's rows that one shard (rows [lo, lo + n) of the database) holds, in sample order: `local` their
// rows within the shard, `pos` their positions in the sample.  Both stay empty when the sample is all rows:
// the shard then holds positions [lo, lo + n), local row i at position lo + i.
struct KmeansShardSample {
  std::vector<int> local, pos;
};

// sample: the sampled rows in sample order, or empty = all rows.  Shards are contiguous and ascending (an
// empty one has n == 0); a row outside every shard is dropped, which the caller's N rules out.
inline std::vector<KmeansShardSample> kmeans_split_sample(const std::vector<int> &sample, const int64_t *lo,
                                                          const int64_t *n, int G) {
  std::vector<KmeansShardSample> out((size_t)G);
  for (size_t i = 0; i < sample.size(); i++) {
    const int64_t row = sample[i];
    for (int g = 0; g < G; g++)
      if (row >= lo[g] && row < lo[g] + n[g]) {
        out[(size_t)g].local.push_back((int)(row - lo[g]));
        out[(size_t)g].pos.push_back((int)i);
        break;
      }
  }
  return out;
}

// sample rows [begin, end) that device g of G assigns: contiguous slices of ceil(rows / G), the last ones short
// or empty
inline void kmeans_assign_slice(int rows, int G, int g, int *begin, int *end) {
  const int64_t per = ((int64_t)rows + G - 1) / G;
  *begin = (int)std::min<int64_t>(rows, (int64_t)g * per);
  *end = (int)std::min<int64_t>(rows, (int64_t)(g + 1) * per);
}

// rows of the centre matrix m [rows][width] that hold a NaN (a centre no row was assigned to: 0 / 0), each counted once
inline int nan_rows(const float *m, int rows, int width) {
  int n = 0;
  for (int c = 0; c < rows; c++) {
    bool nan = false;
    for (int j = 0; j < width; j++) nan |= std::isnan(m[(size_t)c * width + j]);
    n += nan;
  }
  return n;
}

} // namespace vaq
#endif
