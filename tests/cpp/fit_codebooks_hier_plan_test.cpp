// fit_codebooks_hier_plan_test.cpp -- fit_codebooks_hier_plan.h on the CPU (tests/test_codebooks_hier_cpu.py builds and
// runs it as a stand-alone program, once more under AddressSanitizer / UBSan):
//   self                        -> internal checks, prints "fit_codebooks_hier_plan_test: ok"
//   rows <n> <M> <bits,...>     -> per hierarchical subspace: "s k K2 rows stage1_rows resampled c1_off pair_off"
#include "fit_codebooks_hier_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>

namespace cb = vaq::cbfit;
namespace ch = vaq::cbhier;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static std::vector<int> parse_bits(const char *s) {
  std::vector<int> v;
  for (const char *p = s; *p;) {
    v.push_back(std::atoi(p));
    while (*p && *p != ',') p++;
    if (*p) p++;
  }
  return v;
}

static void check_rows() {
  // 256 * k_s wins, cut by n; then uncut
  CHECK(ch::rows_for(1000000, 12, 64, 8) == 1000000);
  CHECK(ch::rows_for(10000000, 12, 64, 8) == 1048576);
  // 256 << (B / M) wins: B / M = 10 over a 9-bit subspace; integer division (87 / 8 = 10)
  CHECK(ch::rows_for(10000000, 9, 80, 8) == 262144);
  CHECK(ch::rows_for(10000000, 9, 87, 8) == 262144);
  CHECK(ch::rows_for(10000000, 9, 88, 8) == 524288);
  CHECK(ch::rows_for(20000, 9, 20, 2) == 20000);
  CHECK(!ch::hierarchical(8) && ch::hierarchical(9));
  CHECK(ch::group_limit(4) == 65536 && ch::group_limit(256) == 65536);
  const int b9[] = {9};
  CHECK(ch::first_short_subspace(300, 1, b9) == 0);   // 512 centres from 300 rows
  CHECK(ch::first_short_subspace(512, 1, b9) == -1);
  const int b38[] = {3, 8};
  CHECK(ch::first_short_subspace(10, 2, b38) == -1);  // (no hierarchical subspace: the flat rule decides)
}

static void check_plans() {
  {  // a flat subspace beside a hierarchical one, all rows each: the flat one reads them in place, R_s is permuted
    const int bits[] = {9, 3};
    const ch::Plan p = ch::make_plan(3000, 4, 2, bits);
    CHECK(p.hsub.size() == 1 && p.n_cent == 520 && p.n_full == 1 && p.gathered == 3000 && p.rows_max == 3000);
    const ch::HSub &h = p.hsub[0];
    CHECK(h.s == 0 && h.k == 512 && h.K2 == 4 && h.rows == 3000 && h.stage1_rows == 3000 && !h.resampled && h.c1_off == 520);
    CHECK(p.stage1.fit.size() == 2 && p.stage1.n_cent == 648 && p.stage1.n_runs == 2 * 128 + 16 && p.stage1.n_pairs == 6000);
    const cb::Fit &f0 = p.stage1.fit[0], &f1 = p.stage1.fit[1];
    CHECK(f0.k == 128 && f0.rows == 3000 && f0.half == 1500 && f0.src == cb::SRC_SAMPLE && f0.stride == 4 && f0.col == 0 &&
          f0.cent_off == 520 && f0.run_off == 0 && f0.pair_off == 0);
    CHECK(f1.k == 8 && f1.rows == 3000 && f1.src == cb::SRC_FULL && f1.stride == 4 && f1.col == 2 && f1.cent_off == 512 &&
          f1.run_off == 256 && f1.pair_off == 3000);
    CHECK(p.member.fit.size() == 1 && p.member.n_runs == 128 && p.member.key_bits == 7 && p.member.fit[0].rows == 3000 &&
          p.member.fit[0].cent_off == 520 && p.member.fit[0].run_off == 0 && p.member.k_max == 128);
  }
  {  // more than 65536 rows: stage 1 samples for itself, the membership takes all rows
    const int bits[] = {9};
    const ch::Plan p = ch::make_plan(70000, 2, 1, bits);
    const ch::HSub &h = p.hsub[0];
    CHECK(h.rows == 70000 && h.stage1_rows == 65536 && h.resampled && h.resample_off == 0 && p.resample_rows == 65536);
    const cb::Fit &f = p.stage1.fit[0];
    CHECK(f.src == cb::SRC_EXTRA && f.stride == 2 && f.col == 0 && f.rows == 65536 && f.half == 32768 && f.row0 == 0);
    CHECK(p.member.fit[0].rows == 70000 && p.member.fit[0].src == cb::SRC_SAMPLE && p.member.fit[0].stride == 2);
    CHECK(p.n_full == 0 && p.gathered == 70000);
  }
  {  // two hierarchical subspaces and two flat ones; a sampling flat subspace shares the gathered head
    const int bits[] = {10, 9, 8, 5};
    const ch::Plan p = ch::make_plan(6000, 16, 4, bits);
    CHECK(p.hsub.size() == 2 && p.n_cent == 1024 + 512 + 256 + 32 && p.n_pairs == 12000 && p.n_full == 2);
    CHECK(p.hsub[0].K2 == 8 && p.hsub[1].K2 == 4 && p.hsub[0].c1_off == p.n_cent && p.hsub[1].c1_off == p.n_cent + 128);
    CHECK(p.hsub[0].pair_off == 0 && p.hsub[1].pair_off == 6000);
    CHECK(p.stage1.fit.size() == 4 && p.stage1.fit[1].col == 4 && p.stage1.fit[2].cent_off == 1536 && p.stage1.fit[3].col == 12);
    CHECK(p.member.fit[1].run_off == 128 && p.member.fit[1].pair_off == 6000 && p.member.fit[1].col == 4 && p.member.key_bits == 8);
    const int big[] = {9, 8};
    const ch::Plan q = ch::make_plan(200000, 4, 2, big);  // B / M = 8: rows 131072; the flat subspace samples 65536
    CHECK(q.hsub[0].rows == 131072 && q.hsub[0].resampled && q.gathered == 131072 && q.n_full == 0);
    CHECK(q.stage1.fit[1].rows == 65536 && q.stage1.fit[1].src == cb::SRC_SAMPLE && q.stage1.rows_max == 65536);
  }
}

static void check_stage2_and_refusals() {
  const int bits[] = {3, 9};
  const int n = 5000, L = 2, R = 256;
  const ch::Plan p = ch::make_plan(n, 4, 2, bits);
  std::vector<int> counts(128, 0);
  counts[0] = R;      // exactly one tile
  counts[1] = R + 1;  // a tile and one row
  counts[2] = 4;      // K2 rows
  int rest = n - (R + R + 1 + 4);
  for (int g = 3; g < 128; g++) {
    counts[g] = g < 127 ? rest / 125 : rest - (rest / 125) * 124;
  }
  CHECK(std::accumulate(counts.begin(), counts.end(), 0) == n);
  CHECK(ch::check_groups(p, counts.data()).kind == ch::OK);
  const cb::Batch b = ch::make_stage2(p, counts.data(), L, R);
  CHECK(b.fit.size() == 128 && b.n_pairs == n && b.n_runs == 2 * 512 && b.k_max == 4 && b.key_bits == 10);
  CHECK(b.n_cent == 8 + 512);  // (the 9-bit subspace's block lies behind the 3-bit one's)
  int64_t row0 = 0;
  int run = 0;
  size_t t = 0;
  for (int g = 0; g < 128; g++) {
    const cb::Fit &f = b.fit[(size_t)g];
    CHECK(f.k == 4 && f.rows == counts[g] && f.half == (counts[g] + 1) / 2 && f.row0 == row0 && f.pair_off == row0);
    CHECK(f.run_off == run && f.cent_off == 8 + g * 4 && f.src == cb::SRC_SAMPLE && f.stride == L && f.col == 0);
    for (int r = 0; r < counts[g]; r += R, t++) CHECK(t < b.tile.size() && b.tile[t].fit == g && b.tile[t].row0 == r);
    row0 += counts[g];
    run += 8;
  }
  CHECK(t == b.tile.size());
  CHECK(b.tile[0].fit == 0 && b.tile[1].fit == 1 && b.tile[2].fit == 1 && b.tile[2].row0 == R && b.tile[3].fit == 2);

  // the refusals, each at the first group it concerns
  std::vector<int> c = counts;
  c[5] = 0;
  ch::Refusal r = ch::check_groups(p, c.data());
  CHECK(r.kind == ch::EMPTY_GROUP && r.s == 1 && r.group == 5 && !r.unsupported());
  c = counts;
  c[7] = 3;
  r = ch::check_groups(p, c.data());
  CHECK(r.kind == ch::SHORT_GROUP && r.s == 1 && r.group == 7 && r.rows == 3 && r.K2 == 4 && !r.unsupported());
  c = counts;
  c[9] = 65537;  // above max(256 * 4, 65536): the reference would sample the group
  r = ch::check_groups(p, c.data());
  CHECK(r.kind == ch::SAMPLED_GROUP && r.group == 9 && r.rows == 65537 && r.unsupported());
  c[9] = 65536;
  CHECK(ch::check_groups(p, c.data()).kind == ch::OK);
  c[9] = 65537;
  c[3] = 0;  // the first in group order is reported
  CHECK(ch::check_groups(p, c.data()).kind == ch::EMPTY_GROUP);
}

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "self")) {
    check_rows();
    check_plans();
    check_stage2_and_refusals();
    std::printf("fit_codebooks_hier_plan_test: ok\n");
    return 0;
  }
  if (argc == 5 && !std::strcmp(argv[1], "rows")) {
    const std::vector<int> bits = parse_bits(argv[4]);
    const int M = std::atoi(argv[3]);
    if ((int)bits.size() != M) return 2;
    const ch::Plan p = ch::make_plan(std::atoll(argv[2]), M, M, bits.data());
    for (const ch::HSub &h : p.hsub)
      std::printf("%d %d %d %d %d %d %d %lld\n", h.s, h.k, h.K2, h.rows, h.stage1_rows, h.resampled, h.c1_off, (long long)h.pair_off);
    return 0;
  }
  std::fprintf(stderr, "usage: fit_codebooks_hier_plan_test self | rows <n> <M> <bits,...>\n");
  return 2;
}
