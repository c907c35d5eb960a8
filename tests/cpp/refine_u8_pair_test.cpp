// refine_u8_pair_test.cpp -- the byte-row forms of vaq_amd/csrc/vaq_exhaust.h against vaq::sq_norm_eigen
// (vaq_restated.h) over the WIDENED row, bit for bit: xs_pair_sq_norm<NP, REST, uint8_t>, which widens each element
// where it reads it, and xs_widen_row<NP, REST> followed by the float instantiation, which is what xs_tile_kernel
// runs.  Rows lie as the refiner holds them, row r at byte r * D of one allocation, so that D = 1, 7 puts row bases
// at odd addresses and D = 12, 40, 100 at multiples of 4 only; the allocation is exactly n * D bytes, so a load past
// a row's end is AddressSanitizer's to find and a misaligned wide load UBSan's.  Stand-alone host program, no input.
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
  if (kind == 0) return u * 255.0f;                                    // SIFT-like magnitudes, not integers
  if (kind == 1) return (u - 0.5f) * 2e-3f + (float)(next_u32() % 256);  // a hair off a byte value
  return std::ldexp(u - 0.5f, (int)(next_u32() % 60) - 30);            // wide exponent range
}

template <int NP, bool REST>
static void pair_forms(const float *q, const uint8_t *y, int D, float *direct, float *widened) {
  *direct = vaq::xs_pair_sq_norm<NP, REST, uint8_t>(q, y, D);
  float slots[vaq::XsRow<NP, REST>::SLOTS];
  vaq::xs_widen_row<NP, REST>(slots, y, D);
  *widened = vaq::xs_pair_sq_norm<NP, REST>(q, slots, D);
}

// the instantiation xs_tile_kernel takes for this width: REST only below the widest form
static void pair_any(const float *q, const uint8_t *y, int D, float *direct, float *widened) {
  switch (D / 16) {
    case 0: return pair_forms<0, true>(q, y, D, direct, widened);
    case 1: return pair_forms<1, true>(q, y, D, direct, widened);
    case 2: return pair_forms<2, true>(q, y, D, direct, widened);
    case 6: return pair_forms<6, true>(q, y, D, direct, widened);
    case 8: return pair_forms<8, false>(q, y, D, direct, widened);
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
  const int dims[] = {1, 7, 8, 12, 16, 40, 100, 128};
  const int ROWS = 5;
  long pairs = 0;
  for (const int D : dims) {
    std::vector<float> q(D), wide(D);
    for (int rep = 0; rep < 300; rep++) {
      std::vector<uint8_t> rows((size_t)ROWS * D);  // (a fresh allocation of exactly ROWS * D bytes, 16-byte aligned)
      if (reinterpret_cast<uintptr_t>(rows.data()) % 16 != 0) {
        std::printf("the allocation is not 16-byte aligned\n");
        return 2;
      }
      for (uint8_t &b : rows) b = (uint8_t)(next_u32() >> 24);
      for (int r = 0; r < ROWS; r++) {  // 0 and 255 in every row (one of them where D == 1)
        uint8_t *y = rows.data() + (size_t)r * D;
        y[next_u32() % (uint32_t)D] = (rep + r) % 2 ? 0 : 255;
        if (D > 1) {
          const uint32_t a = next_u32() % (uint32_t)D;
          y[a] = 0;
          y[(a + 1 + next_u32() % (uint32_t)(D - 1)) % (uint32_t)D] = 255;
        }
      }
      for (int e = 0; e < D; e++) q[e] = next_float(rep % 3);
      for (int r = 0; r < ROWS; r++) {
        const uint8_t *y = rows.data() + (size_t)r * D;
        for (int e = 0; e < D; e++) wide[e] = (float)y[e];
        const float want = vaq::sq_norm_eigen<true>(q.data(), 1, wide.data(), D);
        float direct, widened;
        pair_any(q.data(), y, D, &direct, &widened);
        if (bits(want) != bits(direct) || bits(want) != bits(widened)) {
          std::printf("D=%d rep=%d row=%d: sq_norm_eigen %a, byte rows %a, widened once %a\n", D, rep, r, want, direct, widened);
          return 1;
        }
        pairs++;
      }
    }
  }
  std::printf("refine_u8_pair_test: ok (%ld pairs)\n", pairs);
  return 0;
}
