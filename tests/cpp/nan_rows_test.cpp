// vaq::nan_rows (vaq_amd/csrc/kmeans_sample.h): the rows of a centre matrix that hold a NaN, what the k-means of
// clusterTI and the codebook fits report as nan_rows_out.  No HIP: built with plain g++ by
// tests/test_kmeans_multi_cpu.py, once more under AddressSanitizer + UBSan.  Every matrix is a heap block of exactly
// rows x width floats, so a read past it is caught there.
#include "kmeans_sample.h"

#include <cstdio>
#include <limits>
#include <vector>

namespace {

int bad = 0;

void expect(const char *what, const std::vector<float> &m, int rows, int width, int want) {
  const int got = vaq::nan_rows(m.data(), rows, width);
  if (got != want) {
    std::printf("%s: %d rows, %d expected\n", what, got, want);
    bad++;
  }
}

}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  expect("zero rows", {}, 0, 5, 0);
  if (vaq::nan_rows(nullptr, 0, 3) != 0) bad++;
  expect("width 1", {1.0f, nan, -2.0f, nan, nan}, 5, 1, 3);
  expect("width 1, none", {1.0f, 2.0f}, 2, 1, 0);
  expect("first column", {nan, 1.0f, 2.0f, 3.0f, 4.0f, 5.0f}, 2, 3, 1);
  expect("last column", {0.0f, 1.0f, 2.0f, 3.0f, 4.0f, nan}, 2, 3, 1);
  expect("first and last row", {nan, 1.0f, 2.0f, 3.0f, 4.0f, nan}, 3, 2, 2);
  expect("two in one row, counted once", {nan, 1.0f, nan, 3.0f, 4.0f, 5.0f}, 2, 3, 1);
  expect("every value", {nan, nan, nan, nan}, 2, 2, 2);
  expect("an infinity is not a NaN", {inf, -inf, 1.0f, 2.0f}, 2, 2, 0);
  expect("an infinity next to a NaN", {inf, 1.0f, -inf, nan}, 2, 2, 1);
  expect("a negative NaN", {1.0f, -nan}, 1, 2, 1);
  if (bad) {
    std::printf("%d checks failed\n", bad);
    return 1;
  }
  std::printf("nan_rows_test: ok\n");
  return 0;
}
