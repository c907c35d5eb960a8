// fit_codebooks_plan_test.cpp -- fit_codebooks_plan.h on the CPU (tests/test_codebooks_cpu.py builds and runs it as a
// plain executable, once more with -fsanitize=address,undefined).  Commands on argv:
//   plan <n> <bits,...>   -> "sample n_pairs n_runs n_cent k_max key_bits sampled" (sample: the most rows a subspace
//                            works on; sampled: n > sample, every subspace samples),
//                            then per subspace "k rows half run_off cent_off pair_off", then "gathered n_full gather"
//                            and the subspaces' full flags on one line
//   head <n> <r>          -> the first r entries of randomPermutation(n), one line
//   self                  -> internal checks, prints "fit_codebooks_plan_test: ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "fit_codebooks_plan.h"
#include "kmeans_sample.h"

namespace cb = vaq::cbfit;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      return 1;                                                            \
    }                                                                      \
  } while (0)

// utils/Random.hpp:18-28 in full
static std::vector<int> full_permutation(int n) {
  std::vector<int> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::mt19937 mt(13517106u);
  for (int i = 0; i + 1 < n; i++) {
    const int i2 = i + (int)(mt() % (unsigned)(n - i));
    std::swap(perm[(size_t)i], perm[(size_t)i2]);
  }
  return perm;
}

static std::vector<int> int_list(const char *csv) {
  std::vector<int> v;
  std::stringstream ss(csv);
  std::string t;
  while (std::getline(ss, t, ',')) v.push_back(std::atoi(t.c_str()));
  return v;
}

static int self_test() {
  // KMeans.hpp:489: max(256 * k, 65536), never more than the rows there are
  CHECK(cb::sample_rows(300, 16) == 300);
  CHECK(cb::sample_rows(65536, 2) == 65536);
  CHECK(cb::sample_rows(65537, 2) == 65536);
  CHECK(cb::sample_rows(70000, 256) == 65536);
  CHECK(cb::sample_rows(140000, 512) == 131072);
  CHECK(cb::sample_rows(140000, 1024) == 140000);
  CHECK(cb::sample_rows(((int64_t)1 << 31) - 1, 1 << 15) == (int64_t)256 << 15);
  // the halves of schedule(static) over two threads
  CHECK(cb::half_rows(1) == 1 && cb::half_rows(2) == 1 && cb::half_rows(4001) == 2001 && cb::half_rows(4000) == 2000);
  CHECK(cb::half_rows(0x7fffffff) == 0x40000000);

  // mixed bits: offsets are running sums, the key is as wide as the runs need
  {
    const int bits[] = {9, 3, 1, 8};
    const cb::Plan p = cb::make_plan(140000, 4, bits);
    CHECK(p.sample == 131072 && p.sampled);
    CHECK(p.gathered == 131072 && p.gather && p.n_full == 0);
    CHECK(p.n_cent == 512 + 8 + 2 + 256 && p.n_runs == 2 * p.n_cent && p.k_max == 512);
    CHECK(p.n_pairs == 131072 + 3 * 65536);
    CHECK(((uint64_t)1 << p.key_bits) >= (uint64_t)p.n_runs && ((uint64_t)1 << (p.key_bits - 1)) < (uint64_t)p.n_runs);
    int runs = 0, cent = 0;
    int64_t pairs = 0;
    for (int s = 0; s < 4; s++) {
      const cb::Sub &d = p.sub[(size_t)s];
      CHECK(d.k == 1 << bits[s] && d.rows == (int)cb::sample_rows(140000, d.k) && d.half == cb::half_rows(d.rows));
      CHECK(d.run_off == runs && d.cent_off == cent && d.pair_off == pairs && !d.full);
      // the largest key of the subspace stays below the next one's first
      CHECK(d.run_off + d.k + (d.k - 1) < d.run_off + 2 * d.k);
      runs += 2 * d.k;
      cent += d.k;
      pairs += d.rows;
    }
  }
  {
    const int bits[] = {1};
    const cb::Plan p = cb::make_plan(2, 1, bits);
    CHECK(p.n_runs == 4 && p.key_bits == 2 && !p.sampled && p.sample == 2 && p.sub[0].half == 1);
    CHECK(!p.gather && p.gathered == 0 && p.n_full == 1 && p.sub[0].full == 1);
    const int one[] = {1, 1};
    const cb::Plan q = cb::make_plan(5, 2, one);
    CHECK(q.n_runs == 8 && q.key_bits == 3 && q.sub[1].pair_off == 5 && q.sub[1].run_off == 4);
  }
  {  // the widest the library accepts: 128 subspaces of 15 bits
    std::vector<int> bits(128, 15);
    const cb::Plan p = cb::make_plan(((int64_t)1 << 31) - 1, 128, bits.data());
    CHECK(p.n_runs == 128 * 65536 && p.key_bits == 23 && p.n_pairs == (int64_t)128 * 256 * 32768);
  }

  // every subspace decides for itself (KMeans.hpp:493): full[s] is n <= max(256 k_s, 65536), the gathered sample is
  // the largest prefix of those that sample, and the offsets stay running sums over both kinds
  {
    struct Want {
      int64_t n;
      std::vector<int> bits;
      std::vector<int> full;
      int64_t gathered, sample;
    };
    const std::vector<int> c3 = {12, 10, 9, 8, 8, 7, 6, 4};
    const std::vector<Want> wants = {
        {66000, {3, 9, 5}, {0, 1, 0}, 65536, 66000},                         // a sampling subspace on either side
        {1000000, c3, {1, 0, 0, 0, 0, 0, 0, 0}, 262144, 1000000},            // 256 * 4096 >= n: only the largest is full
        {1048576, c3, {1, 0, 0, 0, 0, 0, 0, 0}, 262144, 1048576},            // n == 256 k: still all rows
        {1048577, c3, {0, 0, 0, 0, 0, 0, 0, 0}, 1048576, 1048576},           // one row more: every subspace samples
        {65536, c3, {1, 1, 1, 1, 1, 1, 1, 1}, 0, 65536},                     // n == 65536: none does
        {65537, {3, 9, 5}, {0, 1, 0}, 65536, 65537},
        {131073, {9, 3, 10}, {0, 0, 1}, 131072, 131073},
    };
    for (const Want &w : wants) {
      const int M = (int)w.bits.size();
      const cb::Plan p = cb::make_plan(w.n, M, w.bits.data());
      CHECK(p.gathered == w.gathered && p.sample == w.sample && p.gather == (w.gathered > 0));
      CHECK(p.sampled == (w.n > w.sample));
      int n_full = 0, runs = 0, cent = 0;
      int64_t pairs = 0;
      for (int s = 0; s < M; s++) {
        const cb::Sub &d = p.sub[(size_t)s];
        const int64_t size = std::max<int64_t>((int64_t)256 << w.bits[s], 65536);
        CHECK(d.full == w.full[(size_t)s] && d.full == (w.n <= size));
        CHECK(d.rows == (d.full ? w.n : size) && d.half == cb::half_rows(d.rows));
        CHECK(d.full || d.rows <= p.gathered);  // a sampling subspace's rows are a prefix of the gathered sample
        CHECK(d.run_off == runs && d.cent_off == cent && d.pair_off == pairs);
        n_full += d.full;
        runs += 2 * d.k;
        cent += d.k;
        pairs += d.rows;
      }
      CHECK(p.n_full == n_full && p.n_pairs == pairs && p.n_runs == runs && p.n_cent == cent);
    }
    // C3 at 1M rows: the pairs of one iteration
    const cb::Plan p = cb::make_plan(1000000, 8, c3.data());
    CHECK(p.n_pairs == 1000000 + 262144 + 131072 + 5 * 65536 && p.k_max == 4096);
  }

  // the prefix property: the sample of a smaller subspace is the head of the larger one's, and both are heads of the
  // whole permutation
  for (int n : {1, 2, 37, 1000, 70001}) {
    const std::vector<int> full = full_permutation(n);
    for (int r : {1, n / 3 + 1, n}) {
      const std::vector<int> head = vaq::permutation_head(n, r);
      CHECK((int)head.size() == r);
      for (int i = 0; i < r; i++) CHECK(head[(size_t)i] == full[(size_t)i]);
    }
  }
  {
    const int n = 140000;
    const std::vector<int> big = vaq::permutation_head(n, cb::sample_rows(n, 512));
    const std::vector<int> small = vaq::permutation_head(n, cb::sample_rows(n, 8));
    CHECK(big.size() == 131072 && small.size() == 65536);
    CHECK(std::memcmp(big.data(), small.data(), small.size() * sizeof(int)) == 0);
    std::vector<char> seen((size_t)n, 0);
    for (int r : big) {
      CHECK(r >= 0 && r < n && !seen[(size_t)r]);
      seen[(size_t)r] = 1;
    }
  }
  std::printf("fit_codebooks_plan_test: ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "self") == 0) return self_test();
  if (argc == 4 && std::strcmp(argv[1], "plan") == 0) {
    const std::vector<int> bits = int_list(argv[3]);
    const cb::Plan p = cb::make_plan(std::atoll(argv[2]), (int)bits.size(), bits.data());
    std::printf("%" PRId64 " %" PRId64 " %d %d %d %u %d\n", p.sample, p.n_pairs, p.n_runs, p.n_cent, p.k_max, p.key_bits,
                (int)p.sampled);
    for (const cb::Sub &d : p.sub)
      std::printf("%d %d %d %d %d %" PRId64 "\n", d.k, d.rows, d.half, d.run_off, d.cent_off, d.pair_off);
    std::printf("%" PRId64 " %d %d\n", p.gathered, p.n_full, (int)p.gather);
    for (const cb::Sub &d : p.sub) std::printf("%d ", d.full);
    std::printf("\n");
    return 0;
  }
  if (argc == 4 && std::strcmp(argv[1], "head") == 0) {
    for (int r : vaq::permutation_head(std::atoll(argv[2]), std::atoll(argv[3]))) std::printf("%d ", r);
    std::printf("\n");
    return 0;
  }
  std::fprintf(stderr, "usage: fit_codebooks_plan_test self | plan <n> <bits,...> | head <n> <r>\n");
  return 2;
}
