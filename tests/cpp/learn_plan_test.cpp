// learn_plan_test.cpp -- learn_plan.h on the CPU (tests/test_learn_device_cpu.py builds and runs it, once more under
// -fsanitize=address,undefined).  Commands on argv:
//   plan <workspace> <sample> <M> <ksub>      -> "Mc groups" then one "s0 m" line per group
//   percentile <file> <rows> <percent>...     -> per percent: the percentile of the float32 column in <file> (rows
//                                                values, ascending) as its bit pattern, through the fetched statistics'
//                                                path where the percent is one of the alphas' (both ways must agree)
//   percentile_ramp <rows> <percent>          -> the same over the column v[i] = (float)i, never materialised
//   loss <file> <rows> <fl> <sc>              -> the sequential double sum of the column's terms, as its bit pattern
//   self                                      -> internal checks, prints "learn_plan_test: ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "learn_plan.h"

namespace ln = vaq::learn;

static std::vector<float> read_floats(const char *path, size_t n) {
  std::vector<float> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
    std::fprintf(stderr, "cannot read %zu floats from %s\n", n, path);
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

static uint32_t bits_of(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

static int self_test() {
  // every subspace exactly once, whatever the budget
  for (int M : {1, 6, 8, 64})
    for (int64_t sample : {1, 2, 4000})
      for (int Mc_want : {1, 3, 5, M}) {
        const int64_t ws = ln::group_bytes(sample, 16, Mc_want);
        const int Mc = ln::group_columns(ws, sample, M, 16);
        if (Mc != std::min(Mc_want, M)) return std::printf("Mc=%d for a budget of %d columns (M=%d)\n", Mc, Mc_want, M), 1;
        std::vector<int> seen((size_t)M, 0);
        for (int g = 0; g < ln::group_count(M, Mc); g++) {
          int s0, m;
          ln::group_range(M, Mc, g, &s0, &m);
          if (m < 1 || m > Mc) return std::printf("group of %d columns\n", m), 1;
          for (int s = s0; s < s0 + m; s++) seen[(size_t)s]++;
        }
        for (int s = 0; s < M; s++)
          if (seen[(size_t)s] != 1) return std::printf("subspace %d covered %d times\n", s, seen[(size_t)s]), 1;
      }
  if (ln::group_columns(1, 1000, 8, 16) != 1) return std::printf("a budget below one column must give Mc = 1\n"), 1;
  if (ln::group_columns(0, 1000, 8, 16) != 8) return std::printf("the default budget holds 8 columns of 16000 values\n"), 1;
  // the fetched statistics give the array's percentiles: floor and scale of every alpha on a column with ties and zeros
  for (int64_t rows : {16, 17, 32, 640, 5000}) {
    std::vector<float> v((size_t)rows);
    for (int64_t i = 0; i < rows; i++) v[(size_t)i] = i < rows / 3 ? 0.0f : (float)((i * 7919) % 1000) * 0.37f;
    std::sort(v.begin(), v.end());
    int64_t idx[ln::STATS_PER_COLUMN];
    ln::stat_indices(rows, idx);
    float stats[ln::STATS_PER_COLUMN];
    for (int j = 0; j < ln::STATS_PER_COLUMN; j++) {
      if (idx[j] < 0 || idx[j] >= rows) return std::printf("statistic %d reads element %" PRId64 " of %" PRId64 "\n", j, idx[j], rows), 1;
      stats[j] = v[(size_t)idx[j]];
    }
    for (int a = 0; a < ln::N_ALPHA; a++) {
      float fl, sc;
      ln::floor_scale_from_stats(stats, rows, a, &fl, &sc);
      const float fl2 = ln::percentile_at([&](int64_t i) { return v[(size_t)i]; }, rows, ln::ALPHAS[a]);
      std::vector<float> offc((size_t)rows);
      for (int64_t i = 0; i < rows; i++) offc[(size_t)i] = std::max(v[(size_t)i] - fl2, 0.0f);
      const float ceil = ln::percentile_at([&](int64_t i) { return offc[(size_t)i]; }, rows, 1.0f - ln::ALPHAS[a]);
      const float sc2 = 255.0f / ceil;
      if (bits_of(fl) != bits_of(fl2) || bits_of(sc) != bits_of(sc2))
        return std::printf("rows=%" PRId64 " alpha %d: (%g, %g) from statistics, (%g, %g) from the array\n", rows, a, fl, sc, fl2, sc2), 1;
    }
  }
  // ties go to the later alpha; nothing finite: -1
  {
    std::vector<double> loss((size_t)ln::N_ALPHA * 2, 1.0);
    double tot[ln::N_ALPHA];
    if (ln::best_alpha(loss.data(), 2, tot) != ln::N_ALPHA - 1 || tot[0] != 2.0) return std::printf("tie rule\n"), 1;
    loss[2 * 3] = 0.25;
    if (ln::best_alpha(loss.data(), 2, nullptr) != 3) return std::printf("argmin\n"), 1;
    for (auto &l : loss) l = std::numeric_limits<double>::infinity();
    if (ln::best_alpha(loss.data(), 2, nullptr) != -1) return std::printf("no finite loss\n"), 1;
  }
  std::printf("learn_plan_test: ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "self") return self_test();
  if (cmd == "plan" && argc == 6) {
    const int64_t ws = std::atoll(argv[2]), sample = std::atoll(argv[3]);
    const int M = std::atoi(argv[4]), ksub = std::atoi(argv[5]);
    const int Mc = ln::group_columns(ws, sample, M, ksub), G = ln::group_count(M, Mc);
    std::printf("%d %d\n", Mc, G);
    for (int g = 0; g < G; g++) {
      int s0, m;
      ln::group_range(M, Mc, g, &s0, &m);
      std::printf("%d %d\n", s0, m);
    }
    return 0;
  }
  if (cmd == "percentile" && argc >= 5) {
    const int64_t rows = std::atoll(argv[3]);
    const std::vector<float> v = read_floats(argv[2], (size_t)rows);
    for (int i = 4; i < argc; i++) {
      const float pct = std::strtof(argv[i], nullptr);
      std::printf("%08x\n", bits_of(ln::percentile_at([&](int64_t j) { return v[(size_t)j]; }, rows, pct)));
    }
    return 0;
  }
  if (cmd == "percentile_ramp" && argc == 4) {
    const int64_t rows = std::atoll(argv[2]);
    const float pct = std::strtof(argv[3], nullptr);
    int64_t idx[2] = {-1, -1};
    const int n = ln::percentile_reads(rows, pct, idx);
    std::printf("%08x %d %" PRId64 " %" PRId64 "\n", bits_of(ln::percentile_at([](int64_t j) { return (float)j; }, rows, pct)), n,
                idx[0], n > 1 ? idx[1] : idx[0]);
    return 0;
  }
  if (cmd == "loss" && argc == 6) {
    const int64_t rows = std::atoll(argv[3]);
    const std::vector<float> v = read_floats(argv[2], (size_t)rows);
    const float fl = std::strtof(argv[4], nullptr), sc = std::strtof(argv[5], nullptr);
    const double l = ln::loss_sequential([&](int64_t j) { return v[(size_t)j]; }, rows, fl, sc);
    uint64_t u;
    std::memcpy(&u, &l, 8);
    std::printf("%016" PRIx64 "\n", u);
    return 0;
  }
  return 2;
}
