// refine_owner_test.cpp -- the multi-device refiner's cut and its way from a label to the owning shard
// (vaq_amd/csrc/refine_owner.h: the one function the host and the select kernel both compile) against a linear scan
// over the shards' ranges.  Stand-alone: plain C++, no HIP; tests/test_refine_multi_cpu.py builds it with -O2 and
// under AddressSanitizer + UBSan.
#include "refine_owner.h"

#include <cstdio>
#include <initializer_list>

namespace {

int checked = 0;

// the first non-empty range that holds the label, shard after shard
int scan(const vaq::RefineBounds &r, int64_t label) {
  if (label < 0) return -1;
  for (int g = 0; g < r.G; g++)
    if (r.b[g] <= label && label < r.b[g + 1]) return g;
  return -1;
}

bool check_all(const vaq::RefineBounds &r, int64_t id_base, int64_t N, const char *what) {
  for (int g = 0; g < r.G; g++)
    if (r.b[g] > r.b[g + 1]) {
      std::printf("%s: bounds descend at shard %d\n", what, g);
      return false;
    }
  if (r.b[0] != id_base || r.b[r.G] != id_base + N) {
    std::printf("%s: bounds [%lld, %lld) do not span the rows\n", what, (long long)r.b[0], (long long)r.b[r.G]);
    return false;
  }
  for (int64_t l = id_base - 2; l < id_base + N + 2; l++) {
    const int got = vaq::refine_owner(r.b, r.G, l), want = scan(r, l);
    checked++;
    if (got != want) {
      std::printf("%s: label %lld owner %d, the scan says %d\n", what, (long long)l, got, want);
      return false;
    }
    if ((l >= id_base && l < id_base + N && l >= 0) != (got >= 0)) {
      std::printf("%s: label %lld: owner %d\n", what, (long long)l, got);
      return false;
    }
  }
  return true;
}

}  // namespace

int main() {
  char what[128];
  for (int64_t N : {0LL, 1LL, 5LL, 300LL, 3000LL})
    for (int G : {1, 2, 3, 8, 16})
      for (int64_t id_base : {0LL, 1LL, 1000LL, 0x7fffffffLL - 3000}) {
        vaq::RefineBounds r = vaq::refine_cut(N, G, id_base);
        const int64_t per = (N + G - 1) / G;
        for (int g = 0; g < G; g++) {  // the cut is the multi index's
          const int64_t lo = (int64_t)g * per < N ? (int64_t)g * per : N, hi = (int64_t)(g + 1) * per < N ? (int64_t)(g + 1) * per : N;
          if (r.b[g] != id_base + lo || r.b[g + 1] != id_base + hi) {
            std::printf("N=%lld G=%d: shard %d is [%lld, %lld)\n", (long long)N, G, g, (long long)r.b[g], (long long)r.b[g + 1]);
            return 1;
          }
        }
        std::snprintf(what, sizeof what, "N=%lld G=%d id_base=%lld", (long long)N, G, (long long)id_base);
        if (!check_all(r, id_base, N, what)) return 1;
        if (id_base + N + 12 > 0x7fffffffLL) continue;
        // the last shard grown by two appends (also from nothing, and past empty shards)
        vaq::refine_grow_last(r, 7);
        vaq::refine_grow_last(r, 5);
        std::snprintf(what, sizeof what, "N=%lld+12 G=%d id_base=%lld", (long long)N, G, (long long)id_base);
        if (!check_all(r, id_base, N + 12, what)) return 1;
        if (vaq::refine_owner(r.b, r.G, id_base + N + 11) != G - 1 || vaq::refine_owner(r.b, r.G, id_base + N) != G - 1) {
          std::printf("%s: the appended rows are not the last shard's\n", what);
          return 1;
        }
      }
  // labels up to the largest int32
  vaq::RefineBounds r = vaq::refine_cut(10, 4, 0x7fffffffLL - 10);
  if (vaq::refine_owner(r.b, r.G, 0x7fffffffLL - 1) != 3 || vaq::refine_owner(r.b, r.G, 0x7fffffffLL) != -1 ||
      vaq::refine_owner(r.b, r.G, 0x7fffffffLL - 10) != 0 || vaq::refine_owner(r.b, r.G, 0x7fffffffLL - 11) != -1) {
    std::printf("id_base near 2^31: wrong owner\n");
    return 1;
  }
  std::printf("refine_owner_test: ok (%d labels)\n", checked);
  return 0;
}
