// The single-thread host forms of vaq_amd/csrc/vaq_bitvec_encode.h against the answers of tests/bitvec_encode_ref.py.
// argv[1]: int32 ncases, then per case int32 {n, D, quantile, n_train}, bits[D], rows [n][D] (projected); for the
// quantile form the projected training rows [n_train][D] and the expected thresholds [D][256]; the expected words.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vaq_bitvec_encode.h"

template <class T> static std::vector<T> take(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2);
  return v;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return 2;
  const int ncases = take<int>(f, 1)[0];
  for (int c = 0; c < ncases; c++) {
    const std::vector<int> h = take<int>(f, 4);
    const int n = h[0], D = h[1], quant = h[2], nt = h[3];
    const std::vector<int> bits = take<int>(f, D);
    const std::vector<float> rows = take<float>(f, (size_t)n * D);
    int total = 0;
    for (int b : bits) total += b;
    const int W = ((quant ? total : D) + 63) / 64;
    std::vector<uint64_t> got((size_t)n * W);
    if (quant) {
      const std::vector<float> train = take<float>(f, (size_t)nt * D), want_t = take<float>(f, (size_t)D * 256);
      std::vector<float> thr((size_t)D * 256, 0.0f);
      std::vector<uint32_t> Z(nt);
      for (int d = 0; d < D; d++) {
        if (!bits[d]) continue;
        for (int i = 0; i < nt; i++) Z[i] = vaq::lutfit::float_to_key(train[(size_t)i * D + d]);
        std::sort(Z.begin(), Z.end());
        vaq::bvenc::thresholds_host(Z.data(), nt, bits[d], &thr[(size_t)d * 256]);
        if (memcmp(&thr[(size_t)d * 256], &want_t[(size_t)d * 256], sizeof(float) << bits[d]))
          return printf("case %d: thresholds of dimension %d differ\n", c, d), 1;
      }
      vaq::bvenc::quantile_encode_host(rows.data(), n, D, bits.data(), thr.data(), got.data());
    } else {
      vaq::bvenc::sign_encode_host(rows.data(), n, D, got.data());
    }
    const std::vector<uint64_t> want = take<uint64_t>(f, (size_t)n * W);
    for (size_t i = 0; i < want.size(); i++)
      if (got[i] != want[i]) return printf("case %d: word %zu of row %zu differs\n", c, i % W, i / W), 1;
  }
  printf("bitvec_encode_test: ok (%d cases)\n", ncases);
  return 0;
}
