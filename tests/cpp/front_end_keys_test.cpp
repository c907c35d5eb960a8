// front_end_keys_test <in.bin>: the cost keys that the table build makes (launch_lut_build with
// CostKeys) against launch_cost_order over the same tables, through the library's own launchers.
// in.bin: int32 M, L, n_nq, n_shift; int32 bits[M]; int32 nq[n_nq]; int32 shift[n_shift];
//         float cent_t (per subspace dimension-major: [L][ncent]); float queries [max nq][M * L] (already projected).
// For every nq x shift: tables bit-equal with and without keys; keys bit-equal; both orders are permutations of
// 0..nq-1 whose key classes (key >> 51) ascend.  Prints "front_end_keys ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vaq_front.h"

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      std::printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));    \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

static bool check_order(const std::vector<int> &order, const std::vector<unsigned long long> &keys, int nq, const char *what) {
  std::vector<char> seen(nq, 0);
  unsigned prev = 0;
  for (int i = 0; i < nq; i++) {
    const int q = order[i];
    if (q < 0 || q >= nq || seen[q]) {
      std::printf("%s: order[%d] = %d is %s\n", what, i, q, (q < 0 || q >= nq) ? "out of range" : "there twice");
      return false;
    }
    seen[q] = 1;
    if ((unsigned)(keys[q] & 0xffffffffu) != (unsigned)q) {
      std::printf("%s: key of query %d names query %u\n", what, q, (unsigned)(keys[q] & 0xffffffffu));
      return false;
    }
    const unsigned cls = (unsigned)(keys[q] >> 51);
    if (cls < prev) {
      std::printf("%s: class %u after class %u at place %d\n", what, cls, prev, i);
      return false;
    }
    prev = cls;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  if (std::fread(hdr, 4, 4, f) != 4) return 2;
  const int M = hdr[0], L = hdr[1], n_nq = hdr[2], n_shift = hdr[3], D = M * L;
  std::vector<int32_t> bits(M), nqs(n_nq), shifts(n_shift);
  if (std::fread(bits.data(), 4, M, f) != (size_t)M || std::fread(nqs.data(), 4, n_nq, f) != (size_t)n_nq ||
      std::fread(shifts.data(), 4, n_shift, f) != (size_t)n_shift)
    return 2;
  std::vector<vaq::SubDesc> sub(M);
  int lut_floats = 0, cent_floats = 0, max_nc = 0, min_nc = 1 << 30, max_nq = 0;
  for (int s = 0; s < M; s++) {
    std::memset(&sub[s], 0, sizeof sub[s]);
    sub[s].ncent = 1 << bits[s];
    sub[s].bits = bits[s];
    sub[s].lut_off = lut_floats;
    sub[s].cent_off = cent_floats;
    lut_floats += sub[s].ncent;
    cent_floats += sub[s].ncent * L;
    max_nc = sub[s].ncent > max_nc ? sub[s].ncent : max_nc;
    min_nc = sub[s].ncent < min_nc ? sub[s].ncent : min_nc;
  }
  for (int n : nqs) max_nq = n > max_nq ? n : max_nq;
  std::vector<float> cent((size_t)cent_floats), X((size_t)max_nq * D);
  if (std::fread(cent.data(), 4, cent.size(), f) != cent.size() || std::fread(X.data(), 4, X.size(), f) != X.size()) return 2;
  std::fclose(f);

  vaq::SubDesc *d_sub;
  float *d_cent, *d_x, *d_lut_a, *d_lut_b;
  unsigned long long *d_keys_a, *d_keys_b;
  int *d_order_a, *d_order_b;
  const size_t lut_bytes = (size_t)max_nq * lut_floats * sizeof(float);
  HIP_OK(hipMalloc(&d_sub, M * sizeof(vaq::SubDesc)));
  HIP_OK(hipMalloc(&d_cent, cent.size() * 4));
  HIP_OK(hipMalloc(&d_x, X.size() * 4));
  HIP_OK(hipMalloc(&d_lut_a, lut_bytes));
  HIP_OK(hipMalloc(&d_lut_b, lut_bytes));
  HIP_OK(hipMalloc(&d_keys_a, (size_t)max_nq * 8));
  HIP_OK(hipMalloc(&d_keys_b, (size_t)max_nq * 8));
  HIP_OK(hipMalloc(&d_order_a, (size_t)max_nq * 4));
  HIP_OK(hipMalloc(&d_order_b, (size_t)max_nq * 4));
  HIP_OK(hipMemcpy(d_sub, sub.data(), M * sizeof(vaq::SubDesc), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_cent, cent.data(), cent.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_x, X.data(), X.size() * 4, hipMemcpyHostToDevice));

  int cases = 0;
  for (int nq : nqs) {
    std::vector<float> lut_a((size_t)nq * lut_floats), lut_b(lut_a.size());
    std::vector<unsigned long long> keys_a(nq), keys_b(nq);
    std::vector<int> order_a(nq), order_b(nq);
    for (int shift : shifts) {
      // sentinels: a key or a place that nobody writes shows
      HIP_OK(hipMemset(d_lut_a, 0xff, lut_a.size() * 4));
      HIP_OK(hipMemset(d_lut_b, 0xff, lut_a.size() * 4));
      HIP_OK(hipMemset(d_keys_a, 0xff, (size_t)nq * 8));
      HIP_OK(hipMemset(d_keys_b, 0xff, (size_t)nq * 8));
      HIP_OK(hipMemset(d_order_a, 0xff, (size_t)nq * 4));
      HIP_OK(hipMemset(d_order_b, 0xff, (size_t)nq * 4));
      HIP_OK(vaq::launch_lut_build(d_x, nq, D, M, L, d_sub, d_cent, lut_floats, max_nc, d_lut_a, nullptr, min_nc));
      HIP_OK(vaq::launch_cost_order(d_lut_a, lut_floats, nq, sub[0].ncent, shift, d_keys_a, d_order_a, nullptr));
      const vaq::CostKeys ck = {d_keys_b, sub[0].ncent, shift};
      HIP_OK(vaq::launch_lut_build(d_x, nq, D, M, L, d_sub, d_cent, lut_floats, max_nc, d_lut_b, nullptr, min_nc, &ck));
      HIP_OK(vaq::launch_cost_scatter(d_keys_b, nq, d_order_b, nullptr));
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipMemcpy(lut_a.data(), d_lut_a, lut_a.size() * 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(lut_b.data(), d_lut_b, lut_b.size() * 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(keys_a.data(), d_keys_a, (size_t)nq * 8, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(keys_b.data(), d_keys_b, (size_t)nq * 8, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(order_a.data(), d_order_a, (size_t)nq * 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(order_b.data(), d_order_b, (size_t)nq * 4, hipMemcpyDeviceToHost));
      if (std::memcmp(lut_a.data(), lut_b.data(), lut_a.size() * 4) != 0) {
        std::printf("nq %d shift %d: the tables differ with keys asked for\n", nq, shift);
        return 1;
      }
      for (int q = 0; q < nq; q++)
        if (keys_a[q] != keys_b[q]) {
          std::printf("nq %d shift %d: key of query %d is %016llx from the table build, %016llx from the tables\n", nq,
                      shift, q, keys_b[q], keys_a[q]);
          return 1;
        }
      char what[96];
      std::snprintf(what, sizeof what, "nq %d shift %d, launch_cost_order", nq, shift);
      if (!check_order(order_a, keys_a, nq, what)) return 1;
      std::snprintf(what, sizeof what, "nq %d shift %d, table build + launch_cost_scatter", nq, shift);
      if (!check_order(order_b, keys_b, nq, what)) return 1;
      cases++;
    }
  }
  std::printf("front_end_keys ok %d\n", cases);
  return 0;
}
