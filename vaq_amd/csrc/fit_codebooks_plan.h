// fit_codebooks_plan.h -- the host arithmetic of the subspace codebook fit (vaq_codebooks.hip, vaqhip_codebooks.cpp):
// how many rows KMeans::staticFitSampling (KMeans.hpp:487-503) works on per subspace and which -- every call of the
// reference decides for itself: all n rows in their own order when n <= max(256 k_s, 65536), else the head of
// randomPermutation(n) --, where each subspace's (key, row) pairs, runs and centres lie in the batched buffers, how
// wide the sort key is, and where the reference's two OpenMP threads cut the rows.
// No HIP in here: tests/cpp/fit_codebooks_plan_test.cpp runs it on the CPU.
#ifndef VAQ_FIT_CODEBOOKS_PLAN_H_
#define VAQ_FIT_CODEBOOKS_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <vector>

namespace vaq {
namespace cbfit {

// KMeans.hpp:489: sampleSize = max(k * 256, 256 * 256)
constexpr int64_t ROWS_PER_CENTRE = 256;
constexpr int64_t MIN_SAMPLE = 256 * 256;

// rows the fit of k centres works on out of n: all of them, or the first sample_rows() of randomPermutation(n)
inline int64_t sample_rows(int64_t n, int k) { return std::min<int64_t>(n, std::max<int64_t>(ROWS_PER_CENTRE * k, MIN_SAMPLE)); }
// rows [0, half_rows) are the first OpenMP thread's (schedule(static), two threads), the rest the second's
inline int half_rows(int rows) { return (int)(((int64_t)rows + 1) / 2); }

// One subspace of the batch (the kernels read it as it is).  Centre c of half h owns run run_off + h * k + c; row r
// of the subspace's rows emits pair pair_off + r.
struct Sub {
  int k;             // centres: 1 << bits
  int rows;          // rows it works on: sample_rows(n, k)
  int half;          // half_rows(rows)
  int run_off;       // first of its 2 * k runs (= sort keys)
  int cent_off;      // its centres in the output, in centres (floats: cent_off * L)
  int full;          // 1: rows == n, it reads all rows in their own order; 0: its prefix of the gathered sample
  int64_t pair_off;  // first of its rows (key, row) pairs
};

struct Plan {
  std::vector<Sub> sub;
  int64_t sample = 0;    // the most rows a subspace works on (n when one reads all rows)
  int64_t gathered = 0;  // rows of the gathered sample permutation_head(n, gathered): the largest prefix a subspace
                         // that samples (full == 0) takes; 0 when none does
  int64_t n_pairs = 0;   // sum of rows
  int n_runs = 0;        // sum of 2 * k
  int n_cent = 0;        // sum of k
  int n_full = 0;        // subspaces that read all n rows
  int k_max = 0;
  unsigned key_bits = 1;  // radix-sort key width: the smallest with 1 << key_bits >= n_runs
  bool sampled = false;   // n > sample: every subspace samples (n_full == 0, gathered == sample)
  bool gather = false;    // gathered > 0 and the fit is handed all n rows: it gathers the sample itself.  A caller that
                          // hands over just the sample's rows, in the sample's order, clears it (only when n_full == 0)
};

// bits[s] in 1..30 (the caller's limit is tighter), n >= 1
inline Plan make_plan(int64_t n, int M, const int *bits) {
  Plan p;
  p.sub.resize((size_t)M);
  for (int s = 0; s < M; s++) {
    Sub &d = p.sub[(size_t)s];
    d.k = 1 << bits[s];
    d.rows = (int)sample_rows(n, d.k);
    d.half = half_rows(d.rows);
    d.run_off = p.n_runs;
    d.cent_off = p.n_cent;
    d.full = d.rows == n;
    d.pair_off = p.n_pairs;
    p.n_runs += 2 * d.k;
    p.n_cent += d.k;
    p.n_pairs += d.rows;
    p.k_max = std::max(p.k_max, d.k);
    p.sample = std::max<int64_t>(p.sample, d.rows);
    if (d.full)
      p.n_full++;
    else
      p.gathered = std::max<int64_t>(p.gathered, d.rows);
  }
  while (p.key_bits < 32 && ((uint64_t)1 << p.key_bits) < (uint64_t)p.n_runs) p.key_bits++;
  p.sampled = n > p.sample;
  p.gather = p.gathered > 0;
  return p;
}

}  // namespace cbfit
}  // namespace vaq
#endif
