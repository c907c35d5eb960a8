// fit_codebooks_multi_plan_test.cpp -- the host-only planning of the sharded codebook fit
// (vaq_amd/csrc/fit_codebooks_multi_plan.h): the owners partition the subspaces, every owner's sub-plan is make_plan
// restricted to its subspaces, every shard's sample positions partition the permutation head and map to local rows in
// range, cuts with empty shards and a grown last shard behave, M < G leaves owners idle, and the owner rule is
// deterministic (s % G, pinned here).  Host code with its own main: built plain and under AddressSanitizer + UBSan by
// tests/test_codebooks_multi_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fit_codebooks_multi_plan.h"

namespace cm = vaq::cbfit_multi;
namespace cb = vaq::cbfit;

static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

struct Shape {
  const char *name;
  int64_t n;
  int D, M;
  std::vector<int> bits;
};

static void check_plan(const Shape &sh, int G, const int64_t *cnt, const cm::Plan &p) {
  const int M = sh.M, L = sh.D / sh.M;
  CHECK(p.G == G && p.M == M && p.L == L && p.n == sh.n);
  CHECK((int)p.owner.size() == G && (int)p.shard.size() == G);
  const cb::Plan whole = cb::make_plan(sh.n, M, sh.bits.data());
  CHECK(p.whole.n_pairs == whole.n_pairs && p.whole.gathered == whole.gathered && p.whole.sampled == whole.sampled);

  // ---- owners partition the subspaces; the rule is s % G ----
  std::vector<int> seen((size_t)M, 0);
  int widths = 0;
  for (int w = 0; w < G; w++) {
    const cm::Owner &o = p.owner[(size_t)w];
    CHECK(o.idle() == (w >= M));  // (M < G: the owners from M on have nothing)
    CHECK(o.D_w == (int)o.subs.size() * L);
    widths += o.D_w;
    for (size_t i = 0; i < o.subs.size(); i++) {
      const int s = o.subs[i];
      CHECK(s >= 0 && s < M);
      CHECK(cm::owner_of(s, G) == w && s == w + (int)i * G);
      seen[(size_t)s]++;
    }
    if (o.idle()) {
      CHECK(!o.full() && o.staged() == 0);
      continue;
    }
    // ---- the sub-plan is make_plan restricted to its subspaces, with offsets of its own ----
    std::vector<int> b;
    for (int s : o.subs) b.push_back(sh.bits[(size_t)s]);
    const cb::Plan mine = cb::make_plan(sh.n, (int)b.size(), b.data());
    CHECK(o.plan.sub.size() == o.subs.size());
    int runs = 0, cents = 0, n_full = 0;
    int64_t pairs = 0, gathered = 0;
    for (size_t i = 0; i < o.subs.size(); i++) {
      const cb::Sub &a = o.plan.sub[i], &g = whole.sub[(size_t)o.subs[i]], &m = mine.sub[i];
      CHECK(a.k == g.k && a.rows == g.rows && a.half == g.half && a.full == g.full);
      CHECK(a.run_off == runs && a.cent_off == cents && a.pair_off == pairs);
      CHECK(a.run_off == m.run_off && a.cent_off == m.cent_off && a.pair_off == m.pair_off);
      runs += 2 * a.k;
      cents += a.k;
      pairs += a.rows;
      n_full += a.full;
      if (!a.full) gathered = std::max<int64_t>(gathered, a.rows);
    }
    CHECK(o.plan.n_runs == runs && o.plan.n_cent == cents && o.plan.n_pairs == pairs && o.plan.n_full == n_full);
    CHECK(o.plan.gathered == gathered && gathered <= whole.gathered);
    CHECK(((uint64_t)1 << o.plan.key_bits) >= (uint64_t)runs);  // the key width from its own runs
    CHECK(o.plan.key_bits == 1 || ((uint64_t)1 << (o.plan.key_bits - 1)) < (uint64_t)runs);
    CHECK(o.plan.key_bits <= whole.key_bits);
    CHECK(o.full() == (n_full > 0));
    CHECK(o.staged() == (o.full() ? 0 : gathered));
  }
  for (int s = 0; s < M; s++) CHECK(seen[(size_t)s] == 1);
  CHECK(widths == sh.D);

  // ---- the shards tile the rows; their sample positions partition the head and map to local rows in range ----
  int64_t S = 0;
  for (const cm::Owner &o : p.owner) S = std::max(S, o.staged());
  const std::vector<int> head = vaq::permutation_head(sh.n, S);
  std::vector<int> hit((size_t)S, 0);
  int64_t at = 0;
  for (int g = 0; g < G; g++) {
    const cm::ShardPart &sp = p.shard[(size_t)g];
    CHECK(sp.lo == at && sp.cnt == cnt[g]);
    at += sp.cnt;
    CHECK(sp.pos.size() == sp.local.size());
    if (sp.cnt == 0) CHECK(sp.pos.empty());  // an empty shard holds no row of the sample
    for (size_t i = 0; i < sp.pos.size(); i++) {
      CHECK(sp.pos[i] >= 0 && sp.pos[i] < S);
      if (i) CHECK(sp.pos[i - 1] < sp.pos[i]);  // ascending: an owner's share is a prefix
      CHECK(sp.local[i] >= 0 && sp.local[i] < sp.cnt);
      CHECK(sp.lo + sp.local[i] == head[(size_t)sp.pos[i]]);
      hit[(size_t)sp.pos[i]]++;
    }
  }
  CHECK(at == sh.n);
  for (int64_t i = 0; i < S; i++) CHECK(hit[(size_t)i] == 1);

  // ---- blocks: per owner the shards' blocks cover what it needs, once; per shard they tile its scratch ----
  for (int w = 0; w < G; w++) {
    const cm::Owner &o = p.owner[(size_t)w];
    int64_t rows = 0;
    for (int g = 0; g < G; g++) {
      const int64_t r = cm::block_rows(p, g, w);
      if (o.idle()) CHECK(r == 0);
      else if (o.full()) CHECK(r == p.shard[(size_t)g].cnt);
      else {
        CHECK(r == cm::sample_count(p, g, w) && cm::stage_row(p, g, w) == rows);
        const std::vector<int> &pos = p.shard[(size_t)g].pos;
        for (int64_t i = 0; i < (int64_t)pos.size(); i++) CHECK((pos[(size_t)i] < o.staged()) == (i < r));
      }
      rows += r;
    }
    CHECK(rows == (o.idle() ? 0 : o.full() ? sh.n : o.staged()));
  }
  for (int g = 0; g < G; g++) {
    int64_t fl = 0;
    for (int w = 0; w < G; w++) {
      CHECK(cm::block_at(p, g, w) == fl);
      fl += cm::block_rows(p, g, w) * p.owner[(size_t)w].D_w;
    }
    CHECK(cm::scratch_floats(p, g) == fl);
    if (p.shard[(size_t)g].cnt == 0) CHECK(fl == 0);
  }
}

int main() {
  const Shape shapes[] = {
      {"tiny", 300, 8, 4, {1, 2, 3, 4}},        {"odd", 4001, 24, 2, {5, 3}},      {"sampled", 70000, 16, 2, {8, 5}},
      {"prefix", 140000, 8, 2, {9, 3}},         {"bytes", 5000, 8, 4, {5, 5, 2, 2}}, {"rotated", 3000, 16, 4, {4, 4, 4, 4}},
      {"mixed", 66000, 6, 3, {3, 9, 5}},        {"staged", 5000, 24, 2, {9, 3}},   {"len1", 600, 2, 2, {2, 3}},
      {"rot_sampled", 70000, 16, 4, {8, 5, 4, 3}},
      {"fast", 1000000, 128, 64, std::vector<int>(64, 4)},
      {"one", 1, 3, 3, {1, 1, 1}},  // (never accepted by the call: 2 centres from 1 row; the plan still holds)
  };
  for (const Shape &sh : shapes) {
    for (int G = 1; G <= cm::MAX_SHARDS; G++) {
      // the host cut: vaqhip_multi_set_codes_u16's
      int64_t cnt[cm::MAX_SHARDS];
      const int64_t per = (sh.n + G - 1) / G;
      for (int g = 0; g < G; g++) {
        int64_t lo;
        cm::host_cut(sh.n, G, g, &lo, &cnt[g]);
        CHECK(lo == std::min<int64_t>(sh.n, (int64_t)g * per) && lo + cnt[g] == std::min<int64_t>(sh.n, (int64_t)(g + 1) * per));
      }
      cm::Plan p, again;
      CHECK(cm::plan_host(G, sh.n, sh.D, sh.M, sh.bits.data(), &p));
      check_plan(sh, G, cnt, p);
      // deterministic: the same call gives the same owners and lists
      CHECK(cm::plan_host(G, sh.n, sh.D, sh.M, sh.bits.data(), &again));
      for (int g = 0; g < G; g++) {
        CHECK(p.owner[(size_t)g].subs == again.owner[(size_t)g].subs);
        CHECK(p.shard[(size_t)g].pos == again.shard[(size_t)g].pos && p.shard[(size_t)g].local == again.shard[(size_t)g].local);
      }
      // the refiner's cut: empty shards in the middle, the last shard grown by add_rows
      if (G >= 2 && sh.n >= 4) {
        int64_t odd[cm::MAX_SHARDS], left = sh.n - sh.n / 4;  // (the last quarter arrived by add_rows)
        const int64_t per2 = (left + G - 1) / G;
        for (int g = 0; g < G; g++) {
          odd[g] = (g % 3 == 1 && g != G - 1) ? 0 : std::min(per2, left);
          left -= odd[g];
        }
        odd[G - 1] += left + sh.n / 4;
        cm::Plan q;
        CHECK(cm::plan_from_counts(G, odd, sh.D, sh.M, sh.bits.data(), &q));
        check_plan(sh, G, odd, q);
      }
    }
  }
  // `mixed` at G = 16: thirteen idle owners, one owner of all rows beside two that take the sample
  {
    const int bits[3] = {3, 9, 5};
    cm::Plan p;
    CHECK(cm::plan_host(16, 66000, 6, 3, bits, &p));
    int idle = 0;
    for (const cm::Owner &o : p.owner) idle += o.idle();
    CHECK(idle == 13);
    CHECK(!p.owner[0].full() && p.owner[1].full() && !p.owner[2].full());
    CHECK(p.owner[0].staged() == 65536 && p.owner[1].staged() == 0 && p.owner[2].staged() == 65536);
    CHECK(cm::block_rows(p, 0, 1) == p.shard[0].cnt);
  }
  // `prefix` at G = 2: two owners take different prefixes of one sample
  {
    const int bits[2] = {9, 3};
    cm::Plan p;
    CHECK(cm::plan_host(2, 140000, 8, 2, bits, &p));
    CHECK(p.owner[0].staged() == 131072 && p.owner[1].staged() == 65536);
    CHECK(cm::sample_count(p, 0, 0) + cm::sample_count(p, 1, 0) == 131072);
    CHECK(cm::sample_count(p, 0, 1) + cm::sample_count(p, 1, 1) == 65536);
    CHECK(cm::sample_count(p, 0, 1) < cm::sample_count(p, 0, 0));
  }
  // refusals of the planner itself
  {
    const int bits[2] = {2, 2};
    cm::Plan p;
    int64_t neg[2] = {3, -1}, none[2] = {0, 0};
    CHECK(!cm::plan_host(0, 10, 4, 2, bits, &p) && !cm::plan_host(17, 10, 4, 2, bits, &p));
    CHECK(!cm::plan_host(2, 0, 4, 2, bits, &p) && !cm::plan_host(2, 10, 5, 2, bits, &p) && !cm::plan_host(2, 10, 4, 0, bits, &p));
    CHECK(!cm::plan_from_counts(2, neg, 4, 2, bits, &p) && !cm::plan_from_counts(2, none, 4, 2, bits, &p));
  }
  std::printf("fit_codebooks_multi_plan_test: ok (%ld checks)\n", g_checks);
  return 0;
}
