// lutfit_test.cpp -- the host build of vaq_amd/csrc/vaq_lutfit.h (what the kernels of vaq_lutfit.hip run)
// against tests/lutfit_ref.py, bit for bit.  Stand-alone: reads the cases and the restatement's answers from a
// file written by tests/test_lutfit_cpu.py, which also runs it under AddressSanitizer + UBSan.
//   file: int32 ncases; per case: int32 n, D, m; int32 bits[D]; float X[n][D]; float P[m][D];
//         float cent[D][256]; float Q[D][257]; uint16 codes[m][D]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vaq_lutfit.h"

namespace lf = vaq::lutfit;

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int ncases = 0;
  if (!rd(f, &ncases, 1)) return 2;
  for (int t = 0; t < ncases; t++) {
    int hdr[3];
    if (!rd(f, hdr, 3)) return 2;
    const int n = hdr[0], D = hdr[1], m = hdr[2];
    std::vector<int> bits(D);
    std::vector<float> X((size_t)n * D), P((size_t)m * D), cent((size_t)D * lf::MAX_CENT), Q((size_t)D * lf::MAX_Q);
    std::vector<uint16_t> codes((size_t)m * D);
    if (!rd(f, bits.data(), bits.size()) || !rd(f, X.data(), X.size()) || !rd(f, P.data(), P.size()) ||
        !rd(f, cent.data(), cent.size()) || !rd(f, Q.data(), Q.size()) || !rd(f, codes.data(), codes.size()))
      return 2;
    for (int d = 0; d < D; d++) {
      const int N = 1 << bits[d];
      std::vector<uint32_t> Z((size_t)n);
      for (int r = 0; r < n; r++) {
        const float x = X[(size_t)r * D + d];
        if (!lf::is_finite(x)) { printf("case %d: non-finite training value\n", t); return 1; }
        Z[(size_t)r] = lf::float_to_key(x);
        if (lf::float_to_key(lf::key_to_float(Z[(size_t)r])) != Z[(size_t)r]) { printf("case %d: key round trip\n", t); return 1; }
      }
      std::sort(Z.begin(), Z.end());
      float q[lf::MAX_Q] = {0}, c[lf::MAX_CENT], pm[lf::MAX_Q];
      lf::fit_column_host(Z.data(), n, bits[d], q, c);
      if (memcmp(q, &Q[(size_t)d * lf::MAX_Q], sizeof q) != 0) {
        for (int i = 0; i <= N; i++)
          if (memcmp(&q[i], &Q[(size_t)d * lf::MAX_Q + i], 4) != 0)
            printf("case %d dim %d: Q[%d] = %.9g, restatement %.9g\n", t, d, i, q[i], Q[(size_t)d * lf::MAX_Q + i]);
        return 1;
      }
      if (memcmp(c, &cent[(size_t)d * lf::MAX_CENT], sizeof c) != 0) {
        for (int i = 0; i < N; i++)
          if (memcmp(&c[i], &cent[(size_t)d * lf::MAX_CENT + i], 4) != 0)
            printf("case %d dim %d: centre %d = %.9g, restatement %.9g\n", t, d, i, c[i], cent[(size_t)d * lf::MAX_CENT + i]);
        return 1;
      }
      lf::prefix_max_host(q, N, pm);
      for (int r = 0; r < m; r++) {
        const float x = P[(size_t)r * D + d];
        const uint16_t got = lf::encode_value(x, N, pm, c);
        // the scan as the reference writes it (:896-897), against the lower bound over the prefix maxima
        int first = N + 1;
        for (int j = 0; j <= N; j++)
          if (x <= q[j]) { first = j; break; }
        if (first != lf::first_boundary(x, pm, N)) { printf("case %d dim %d: boundary of %.9g\n", t, d, x); return 1; }
        if (got != codes[(size_t)r * D + d]) {
          printf("case %d dim %d probe %d (%.9g): code %d, restatement %d\n", t, d, r, x, (int)got, (int)codes[(size_t)r * D + d]);
          return 1;
        }
      }
    }
  }
  fclose(f);
  printf("lutfit_test: ok (%d cases)\n", ncases);
  return 0;
}
