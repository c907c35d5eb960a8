// wave_primitives_test.hip -- the two wave-wide register primitives of vaq_scan.h against the host:
//   wave_sort64       lane r holds the (r + 1)-th smallest of the wave's 64 values, for every r
//   wave_prefix_incl  inclusive prefix sum over the lanes
// Input: 64-vectors of float bits >= +0 (random, all equal, strictly descending, strictly ascending, one
// finite among +inf, all +inf, two values with 32 or more lanes tying, denormals and zeros) and of ints.
// One wave per vector.  Prints "wave primitives ok: <vectors>" and exits 0, or the first mismatch and 1.
// Built and run by tests/test_bf_serial_phases.py (hipcc --offload-arch=gfx950 -I vaq_amd/csrc -I include).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vaq_scan.h"

__global__ void wave_primitives_kernel(const unsigned *in, unsigned *sorted, const int *iin, int *prefix) {
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * 64 + lane;
  sorted[i] = vaq::wave_sort64(in[i], lane);
  prefix[i] = vaq::wave_prefix_incl(iin[i]);
}

static unsigned fbits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

#define CHECK(x)                                                               \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));                      \
      return 2;                                                                \
    }                                                                          \
  } while (0)

int main() {
  std::mt19937 rng(20240611);
  std::vector<std::vector<unsigned>> vs;
  std::vector<std::vector<int>> is;
  const float inf = INFINITY;
  auto push = [&](const std::vector<float> &f) {
    std::vector<unsigned> u(64);
    for (int i = 0; i < 64; i++) u[i] = fbits(f[i]);
    vs.push_back(u);
  };
  std::vector<float> f(64);
  for (int i = 0; i < 64; i++) f[i] = 7.25f;
  push(f);  // all equal
  for (int i = 0; i < 64; i++) f[i] = 1000.0f - (float)i;
  push(f);  // strictly descending
  for (int i = 0; i < 64; i++) f[i] = (float)i * 0.5f;
  push(f);  // strictly ascending
  for (int i = 0; i < 64; i++) f[i] = inf;
  push(f);  // all +inf
  for (int p : {0, 1, 15, 16, 31, 32, 47, 63}) {  // one finite among +inf, in every row and at the edges
    for (int i = 0; i < 64; i++) f[i] = i == p ? 3.5f : inf;
    push(f);
  }
  for (int ties : {32, 33, 48, 63}) {  // `ties` lanes share one value, the rest are spread around it
    for (int rep = 0; rep < 8; rep++) {
      for (int i = 0; i < 64; i++) f[i] = i < ties ? 10.0f : (float)(rng() % 20);
      std::shuffle(f.begin(), f.end(), rng);
      push(f);
    }
  }
  for (int rep = 0; rep < 8; rep++) {  // zeros, denormals, the largest finite value, +inf
    const float pool[6] = {0.0f, 1e-45f, 1e-39f, 1.17549435e-38f, 3.4028235e38f, inf};
    for (int i = 0; i < 64; i++) f[i] = pool[rng() % 6];
    push(f);
  }
  for (int have : {1, 2, 31, 33, 62, 63}) {  // `have` finite lanes, the others +inf (lanes that sampled no row)
    for (int i = 0; i < 64; i++) f[i] = i < have ? std::ldexp((float)(rng() % 4096), -4) : inf;
    std::shuffle(f.begin(), f.end(), rng);
    push(f);
  }
  while (vs.size() < 400) {  // random: few distinct values (many ties) up to all distinct
    const unsigned span = 1u << (1 + rng() % 30);
    std::vector<unsigned> u(64);
    for (int i = 0; i < 64; i++) u[i] = rng() % span;  // (any bits below 0x7f800000 are floats >= +0)
    vs.push_back(u);
  }
  for (size_t v = 0; v < vs.size(); v++) {
    std::vector<int> x(64);
    const int mode = (int)(v % 4);
    for (int i = 0; i < 64; i++)
      x[i] = mode == 0 ? 1 : mode == 1 ? (int)(rng() % 200) : mode == 2 ? (i == (int)(v % 64) ? 1 << 20 : 0) : (int)(rng() % (1 << 24));
    is.push_back(x);
  }
  const size_t n = vs.size() * 64;
  std::vector<unsigned> h_in(n), h_sorted(n);
  std::vector<int> h_iin(n), h_prefix(n);
  for (size_t v = 0; v < vs.size(); v++)
    for (int i = 0; i < 64; i++) {
      h_in[v * 64 + i] = vs[v][i];
      h_iin[v * 64 + i] = is[v][i];
    }
  unsigned *d_in, *d_sorted;
  int *d_iin, *d_prefix;
  CHECK(hipMalloc(&d_in, n * 4));
  CHECK(hipMalloc(&d_sorted, n * 4));
  CHECK(hipMalloc(&d_iin, n * 4));
  CHECK(hipMalloc(&d_prefix, n * 4));
  CHECK(hipMemcpy(d_in, h_in.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_iin, h_iin.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(wave_primitives_kernel, dim3((unsigned)vs.size()), dim3(64), 0, 0, d_in, d_sorted, d_iin, d_prefix);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h_sorted.data(), d_sorted, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(h_prefix.data(), d_prefix, n * 4, hipMemcpyDeviceToHost));
  for (size_t v = 0; v < vs.size(); v++) {
    std::vector<unsigned> want = vs[v];
    std::sort(want.begin(), want.end());
    int run = 0;
    for (int r = 0; r < 64; r++) {  // every rank 1..64: the r-th smallest is lane r - 1
      if (h_sorted[v * 64 + r] != want[r]) {
        std::printf("vector %zu: rank %d is %08x, host sort says %08x\n", v, r + 1, h_sorted[v * 64 + r], want[r]);
        return 1;
      }
      run += is[v][r];
      if (h_prefix[v * 64 + r] != run) {
        std::printf("vector %zu: prefix at lane %d is %d, host scan says %d\n", v, r, h_prefix[v * 64 + r], run);
        return 1;
      }
    }
  }
  std::printf("wave primitives ok: %zu\n", vs.size());
  return 0;
}
