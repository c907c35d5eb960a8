// lutfit_multi_plan_test.cpp -- the host-only planning of the sharded quantile fit (vaq_amd/csrc/lutfit_multi_plan.h):
// every dimension is owned exactly once, the rounds cover 0..D-1 in order with a partial last round, the slices of a
// column tile [0, n) without gap or overlap, empty shards contribute zero words.  Host code with its own main: built
// plain and under AddressSanitizer + UBSan by tests/test_lutfit_multi_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lutfit_multi_plan.h"

namespace lp = vaq::lutfit_plan;

static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static void check_dims(int G, int D) {
  std::vector<int> seen((size_t)D, 0), per_owner((size_t)G, 0);
  const int R = lp::rounds(D, G);
  CHECK(R == (D + G - 1) / G);
  int next = 0;
  for (int t = 0; t < R; t++) {
    const int d0 = lp::round_first(t, G), W = lp::round_width(t, D, G);
    CHECK(d0 == next);
    CHECK(W >= 1 && W <= G && W <= lp::MAX_SHARDS);
    CHECK(t == R - 1 ? d0 + W == D : W == G);  // only the last round may be partial
    for (int w = 0; w < W; w++) {
      const int d = d0 + w;
      CHECK(d < D);
      CHECK(lp::owner_of(d, G) == w);   // a round gives every owner at most one column: slot w goes to owner w
      CHECK(lp::slot_of(d, G) == t);    // and the owner keeps it in the round's slot
      seen[(size_t)d]++;
      per_owner[(size_t)w]++;
    }
    next = d0 + W;
  }
  CHECK(next == D);
  CHECK(lp::round_width(R, D, G) == 0);
  for (int d = 0; d < D; d++) CHECK(seen[(size_t)d] == 1);
  int total = 0;
  for (int w = 0; w < G; w++) {
    CHECK(lp::owned_dims(w, D, G) == per_owner[(size_t)w]);  // (D < G: owners from D on stay idle)
    if (w >= D) CHECK(per_owner[(size_t)w] == 0);
    total += per_owner[(size_t)w];
  }
  CHECK(total == D);
}

static void check_tiling(const lp::Plan &p, int64_t n) {
  CHECK(p.n == n);
  int64_t at = 0, words = 0;
  for (int g = 0; g < p.G; g++) {
    CHECK(p.cnt[g] >= 0);
    CHECK(lp::slice_dst_word(p, g) == at);  // no gap, no overlap
    at += p.cnt[g];
    CHECK(lp::shard_scratch_words(p, g) == (int64_t)p.G * p.cnt[g]);
    if (p.cnt[g] == 0) CHECK(lp::shard_scratch_words(p, g) == 0);  // an empty shard contributes no word
    for (int w = 0; w < p.G; w++) {
      CHECK(lp::slice_src_word(p, g, w) == (int64_t)w * p.cnt[g]);
      CHECK(lp::slice_src_word(p, g, w) + p.cnt[g] <= lp::shard_scratch_words(p, g));
    }
    words += p.cnt[g];
  }
  CHECK(at == n && words == lp::owner_key_words(p));
}

int main() {
  const int Ds[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                    28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 4096};
  const int64_t ns[] = {1, 2, 3, 5, 15, 16, 17, 255, 256, 257, 4099, 1000003, ((int64_t)1 << 31) - 1, (int64_t)1 << 31,
                        ((int64_t)1 << 31) + 12345, (int64_t)1000000000 * 7};
  for (int G = 1; G <= 16; G++) {
    for (int D : Ds) check_dims(G, D);
    for (int64_t n : ns) {
      lp::Plan p;
      CHECK(lp::plan_host(G, 5, n, &p));
      check_tiling(p, n);
      // the host cut is vaqhip_multi_set_codes_u16's: shard g = rows [g * ceil(n / G), (g + 1) * ceil(n / G))
      const int64_t per = (n + G - 1) / G;
      for (int g = 0; g < G; g++) {
        const int64_t lo = (int64_t)g * per < n ? (int64_t)g * per : n;
        const int64_t hi = (int64_t)(g + 1) * per < n ? (int64_t)(g + 1) * per : n;
        CHECK(p.lo[g] == lo && p.cnt[g] == hi - lo);
      }
      // the refiner's cut: set_rows' cut, the last shard grown by add_rows, empty shards in the middle
      int64_t cnt[lp::MAX_SHARDS];
      int64_t total = 0;
      for (int g = 0; g < G; g++) {
        cnt[g] = (g % 3 == 1) ? 0 : p.cnt[g];
        if (g == G - 1) cnt[g] += 77;
        total += cnt[g];
      }
      lp::Plan r;
      CHECK(lp::plan_from_counts(G, 40, cnt, &r));
      check_tiling(r, total);
    }
  }
  lp::Plan p;
  CHECK(!lp::plan_host(0, 4, 10, &p) && !lp::plan_host(17, 4, 10, &p) && !lp::plan_host(2, 0, 10, &p));
  CHECK(!lp::plan_host(2, 4, -1, &p));
  int64_t neg[2] = {3, -1};
  CHECK(!lp::plan_from_counts(2, 4, neg, &p));
  std::printf("lutfit_multi_plan_test: ok (%ld checks)\n", g_checks);
  return 0;
}
