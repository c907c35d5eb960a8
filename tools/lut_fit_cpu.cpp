// lut_fit_cpu.cpp -- BitVecEngine::binaryEncodingLUT from the bit allocation on, on ONE CPU thread through the
// header the kernels run (vaq_amd/csrc/vaq_lutfit.h): the reference's shape of the work (a std::sort per column,
// a sequential walk, one row and dimension after another).  tools/bench_lut_fit.py builds it as a shared object
// (g++ -O2 -ffp-contract=off), times it next to the GPU and compares the outputs.
#include <algorithm>
#include <vector>

#include "vaq_lutfit.h"

namespace lf = vaq::lutfit;

extern "C" {
// X n x D row-major in PCA space; cent [D][256], Q [D][257]
void lut_fit_cpu(const float *X, int64_t n, int D, const int *bits, float *cent, float *Q) {
  std::vector<uint32_t> Z((size_t)n);
  for (int d = 0; d < D; d++) {
    for (int64_t r = 0; r < n; r++) Z[(size_t)r] = lf::float_to_key(X[r * D + d]);
    std::sort(Z.begin(), Z.end());
    float *q = Q + (size_t)d * lf::MAX_Q;
    for (int j = 0; j < lf::MAX_Q; j++) q[j] = 0.0f;
    lf::fit_column_host(Z.data(), n, bits[d], q, cent + (size_t)d * lf::MAX_CENT);
  }
}

void lut_encode_cpu(const float *X, int64_t n, int D, const int *bits, const float *cent, const float *Q, uint16_t *codes) {
  std::vector<float> pm((size_t)D * lf::MAX_Q);
  for (int d = 0; d < D; d++) lf::prefix_max_host(Q + (size_t)d * lf::MAX_Q, 1 << bits[d], pm.data() + (size_t)d * lf::MAX_Q);
  for (int64_t r = 0; r < n; r++)
    for (int d = 0; d < D; d++)
      codes[r * D + d] = lf::encode_value(X[r * D + d], 1 << bits[d], pm.data() + (size_t)d * lf::MAX_Q, cent + (size_t)d * lf::MAX_CENT);
}
}
