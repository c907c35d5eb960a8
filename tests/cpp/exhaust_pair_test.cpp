// exhaust_pair_test.cpp -- xs_pair_sq_norm (vaq_amd/csrc/vaq_exhaust.h), the per-pair distance of the exhaustive
// form, against vaq::sq_norm_eigen (vaq_restated.h), the specification: bit for bit on random floats and on rows
// holding NaN and inf, for every path of Eigen's reduction.  Stand-alone host program, no input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vaq_exhaust.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t next_u32() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 32);
}
static float next_float(int kind) {
  const float u = (float)(next_u32() >> 8) / (float)(1 << 24);
  if (kind == 0) return u * 255.0f;                            // SIFT-like magnitudes
  if (kind == 1) return (u - 0.5f) * 2e-3f + (float)(next_u32() % 7);  // near-duplicates: sums a few ulps apart
  return std::ldexp(u - 0.5f, (int)(next_u32() % 60) - 30);    // wide exponent range
}

template <int NP>
static float pair_of(const float *q, const float *y, int D) {
  if (D % 16 == 0 && NP > 0) return vaq::xs_pair_sq_norm<NP, false>(q, y, D);
  return vaq::xs_pair_sq_norm<NP, true>(q, y, D);
}

static float pair_any(const float *q, const float *y, int D) {
  switch (D / 16) {
    case 0: return pair_of<0>(q, y, D);
    case 1: return pair_of<1>(q, y, D);
    case 2: return pair_of<2>(q, y, D);
    case 6: return pair_of<6>(q, y, D);
    case 8: return pair_of<8>(q, y, D);
    case 60: return pair_of<60>(q, y, D);
  }
  std::printf("no instantiation for D=%d\n", D);
  std::exit(2);
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  const int dims[] = {1, 7, 8, 12, 15, 16, 17, 24, 40, 100, 128, 129, 960};
  long pairs = 0;
  for (const int D : dims) {
    // the row buffer is as long as the widest template's slot count: slots at or past D are never read
    std::vector<float> q(D), y((size_t)D + 15, std::numeric_limits<float>::quiet_NaN());
    for (int rep = 0; rep < 400; rep++) {
      const int kind = rep % 3;
      for (int e = 0; e < D; e++) {
        q[e] = next_float(kind);
        y[e] = next_float(kind);
      }
      if (rep >= 300) {  // NaN, +-inf, and a difference whose square overflows, at a random place
        const int e = (int)(next_u32() % (uint32_t)D);
        const int what = rep % 4;
        y[e] = what == 0 ? std::numeric_limits<float>::quiet_NaN()
               : what == 1 ? std::numeric_limits<float>::infinity()
               : what == 2 ? -std::numeric_limits<float>::infinity() : 3e38f;
        if (what == 3) q[e] = -3e38f;
      }
      const float want = vaq::sq_norm_eigen<true>(q.data(), 1, y.data(), D);
      const float got = pair_any(q.data(), y.data(), D);
      const bool same = bits(want) == bits(got) || (std::isnan(want) && std::isnan(got));
      if (!same) {
        std::printf("D=%d rep=%d: sq_norm_eigen %a, xs_pair_sq_norm %a\n", D, rep, want, got);
        return 1;
      }
      pairs++;
    }
  }
  std::printf("exhaust_pair_test: ok (%ld pairs)\n", pairs);
  return 0;
}
