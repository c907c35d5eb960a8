// refine_owner.h -- the cut of the multi-device refiner's rows and the way from a label to the shard that holds
// its row.  Compiled by the host (vaqhip_multi_refiner.cpp: the cut and the refine form's select; through
// vaqhip_multi_refiner.h also vaqhip_multi_refiner_search.cpp), by the select kernel (vaq_refine.hip) and, with a plain
// C++ compiler, by tests/cpp/refine_owner_test.cpp: one function, so that the host and the device cannot disagree
// about who owns a label.  Nothing of HIP in here.
#ifndef VAQ_REFINE_OWNER_H_
#define VAQ_REFINE_OWNER_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define VAQ_RF_HD __host__ __device__
#else
#define VAQ_RF_HD
#endif

namespace vaq {

constexpr int RF_MAX_SHARDS = 16;  // (= VAQHIP_MAX_DEVICES)

// Labels [b[g], b[g + 1]) belong to shard g: b[0] = id_base, b[G] = id_base + N, ascending, equal neighbours where a
// shard is empty.  Passed to the kernel by value.
struct RefineBounds {
  int G;
  int64_t b[RF_MAX_SHARDS + 1];
};

// The multi index's cut (vaqhip_multi_set_codes_u16): shard g holds rows [g * ceil(N / G), (g + 1) * ceil(N / G)),
// clipped to N; shards past the rows are empty.
inline RefineBounds refine_cut(int64_t N, int G, int64_t id_base) {
  RefineBounds r;
  r.G = G;
  const int64_t per = (N + G - 1) / G;
  for (int g = 0; g <= RF_MAX_SHARDS; g++) {
    const int64_t lo = (int64_t)g * per;
    r.b[g] = id_base + (g >= G || lo > N ? N : lo);
  }
  return r;
}

// Appended rows continue the numbering: they extend the last shard.
inline void refine_grow_last(RefineBounds &r, int64_t n_new) {
  for (int g = r.G; g <= RF_MAX_SHARDS; g++) r.b[g] += n_new;
}

// The shard whose range holds `label`, or -1 when none does (a negative label, one below id_base or past the last
// row).  The owner is the LAST g with b[g] <= label: its range is not empty (b[g + 1] > label, or g + 1 would be
// later), so a label on a cut goes to the shard that starts there and empty shards are never named.
// b: the G + 1 bounds (the kernel keeps them in LDS).
VAQ_RF_HD inline int refine_owner(const int64_t *b, int G, int64_t label) {
  if (label < 0 || label < b[0] || label >= b[G]) return -1;
  int lo = 0, hi = G;  // b[lo] <= label < b[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] <= label) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace vaq
#endif
