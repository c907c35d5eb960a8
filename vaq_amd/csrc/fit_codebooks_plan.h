// fit_codebooks_plan.h -- the host arithmetic of the subspace codebook fit (vaq_codebooks.hip, vaqhip_codebooks.cpp):
// how many rows KMeans::staticFitSampling (KMeans.hpp:487-503) works on per subspace and which -- every call of the
// reference decides for itself: all n rows in their own order when n <= max(256 k_s, 65536), else the head of
// randomPermutation(n) --, where each subspace's (key, row) pairs, runs and centres lie in the batched buffers, how
// wide the sort key is, where the reference's two OpenMP threads cut the rows, and the head that the plans of the two
// forms for subspaces above 8 bits share.
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
// radix-sort key width: the smallest with 1 << key_bits >= n_runs, at least 1
inline unsigned key_bits_for(int n_runs) {
  unsigned b = 1;
  while (b < 32 && ((uint64_t)1 << b) < (uint64_t)n_runs) b++;
  return b;
}

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
  unsigned key_bits = 1;  // key_bits_for(n_runs)
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
  p.key_bits = key_bits_for(p.n_runs);
  p.sampled = n > p.sample;
  p.gather = p.gathered > 0;
  return p;
}

// ---- the batch as the kernels address it ----
// One fit of a batch: a subspace of the flat fit, or one of the 129 fits of a hierarchical subspace
// (fit_codebooks_hier_plan.h).  Its rows are rows [row0, row0 + rows) of source matrix `src`, `stride` floats apart,
// its slice the L floats from column `col` on.  Centre c of half h owns run run_off + h * k + c; its row r emits pair
// pair_off + r with value r.
struct Fit {
  int k;             // centres
  int rows;          // rows it works on
  int half;          // half_rows(rows)
  int run_off;       // first of its 2 * k runs (= sort keys)
  int cent_off;      // its centres in the centre table, in centres
  int src;           // which of the batch's source matrices it reads
  int stride;        // floats between two rows of that matrix
  int col;           // first column of its slice
  int64_t row0;      // its first row in that matrix
  int64_t pair_off;  // first of its (key, row) pairs
};
// rows [row0, row0 + tile rows) of fit `fit`: what one workgroup of the assign kernel takes where the fits differ
// widely in size (a grid of (largest fit's tiles, fits) would be mostly empty)
struct Tile {
  int fit;
  int row0;
};
constexpr int SRC_SAMPLE = 0, SRC_FULL = 1, SRC_EXTRA = 2, N_SOURCES = 3;

struct Batch {
  std::vector<Fit> fit;
  std::vector<Tile> tile;  // empty: the assign grid is (tiles of the largest fit, fits)
  int64_t n_pairs = 0;     // sum of rows
  int64_t rows_max = 0;
  int n_runs = 0;          // sum of 2 * k
  int n_cent = 0;          // centres the centre table spans: the largest cent_off + k
  int k_max = 0;
  unsigned key_bits = 1;   // key_bits_for(n_runs)
};

// bytes of LDS the assign kernel's tile of slices may take; wider slices are read from global memory
constexpr int TILE_BYTES = 40 * 1024;
// rows a workgroup of the assign kernel takes: the widest workgroup whose tile of slices fits, at least a wavefront
inline int assign_tile_rows(int L) {
  int R = 256;
  while (R > 64 && (size_t)R * L * sizeof(float) > (size_t)TILE_BYTES) R >>= 1;
  return R;
}

inline void batch_add(Batch &b, int k, int rows, int cent_off, int src, int stride, int col, int64_t row0) {
  Fit f;
  f.k = k;
  f.rows = rows;
  f.half = half_rows(rows);
  f.run_off = b.n_runs;
  f.cent_off = cent_off;
  f.src = src;
  f.stride = stride;
  f.col = col;
  f.row0 = row0;
  f.pair_off = b.n_pairs;
  b.fit.push_back(f);
  b.n_runs += 2 * k;
  b.n_pairs += rows;
  b.n_cent = std::max(b.n_cent, cent_off + k);
  b.k_max = std::max(b.k_max, k);
  b.rows_max = std::max<int64_t>(b.rows_max, rows);
  b.key_bits = key_bits_for(b.n_runs);
}
// the tile table's entries of fit `fit`: its rows in pieces of tile_rows, none across a fit
inline void batch_add_tiles(Batch &b, int fit, int rows, int tile_rows) {
  for (int r = 0; r < rows; r += tile_rows) b.tile.push_back(Tile{fit, r});
}

// the flat fit's batch: subspace s reads columns [s * L, (s + 1) * L) of the full matrix or of the sample, D wide
inline Batch make_batch(const Plan &p, int D, int L) {
  Batch b;
  for (size_t s = 0; s < p.sub.size(); s++) {
    const Sub &d = p.sub[s];
    batch_add(b, d.k, d.rows, d.cent_off, d.full ? SRC_FULL : SRC_SAMPLE, D, (int)s * L, 0);
  }
  return b;
}

// ---- what the two forms for wide subspaces share (fit_codebooks_hier_plan.h, fit_codebooks_bin_plan.h) ----
constexpr int FLAT_MAX_BITS = 8;  // a subspace with more bits is wide: hierarchical or binary (VAQ.cpp:546)
inline bool wide(int bits) { return bits > FLAT_MAX_BITS; }
// rows R_s of a wide subspace, VAQ.cpp:535-536: min(n, max(256 * k_s, 256 << (B / M))), B the bit budget, integer division
inline int64_t rows_for(int64_t n, int bits_s, int B, int M) {
  return std::min<int64_t>(n, std::max<int64_t>(ROWS_PER_CENTRE << bits_s, (int64_t)256 << (B / M)));
}
inline int bit_budget(int M, const int *bits) {
  int B = 0;
  for (int s = 0; s < M; s++) B += bits[s];
  return B;
}
// -1 when the shape can be planned, else the first wide subspace with rows_s < k_s (refused: seeds out of bounds)
inline int first_short_subspace(int64_t n, int M, const int *bits) {
  const int B = bit_budget(M, bits);
  for (int s = 0; s < M; s++)
    if (wide(bits[s]) && rows_for(n, bits[s], B, M) < ((int64_t)1 << bits[s])) return s;
  return -1;
}

// The head of a wide form's plan.  R_s = rows randomPermutation(n)[0 .. rows[s]) of the projected matrix.
// (hidden, as the host's own types are: the library exports nothing for it)
struct __attribute__((visibility("hidden"))) WideHead {
  Plan flat;              // make_plan over ALL subspaces: cent_off of every subspace, rows / full of the flat ones
  std::vector<int> rows;  // rows of R_s per subspace; 0 for a flat one
  int64_t rows_max = 0;   // the largest R_s
  int64_t gathered = 0;   // rows of the ONE gathered head of randomPermutation(n): the largest R_s or sampling flat
                          // subspace's prefix; every such reader takes a prefix of it
  int64_t n_pairs = 0;    // sum of rows over the wide subspaces
  int n_full = 0;         // flat subspaces that read all n rows in their own order
  int n_cent = 0;         // final centres: sum of k_s
};

// bits[s] in 1..15, n in 1..2^31-1
__attribute__((visibility("hidden"))) inline WideHead wide_head(int64_t n, int M, const int *bits) {
  WideHead p;
  p.flat = make_plan(n, M, bits);
  p.n_cent = p.flat.n_cent;
  p.rows.assign((size_t)M, 0);
  const int B = bit_budget(M, bits);
  for (int s = 0; s < M; s++) {
    const Sub &d = p.flat.sub[(size_t)s];
    if (wide(bits[s])) {
      p.rows[(size_t)s] = (int)rows_for(n, bits[s], B, M);
      p.n_pairs += p.rows[(size_t)s];
      p.rows_max = std::max<int64_t>(p.rows_max, p.rows[(size_t)s]);
    } else if (d.full) {
      p.n_full++;
    } else {
      p.gathered = std::max<int64_t>(p.gathered, d.rows);
    }
  }
  p.gathered = std::max(p.gathered, p.rows_max);
  return p;
}

}  // namespace cbfit

// the names these had while the hierarchical form alone owned them (the plan tests of both wide forms spell them so)
namespace cbhier {
using cbfit::first_short_subspace;
using cbfit::rows_for;
inline bool hierarchical(int bits) { return cbfit::wide(bits); }
}  // namespace cbhier
}  // namespace vaq
#endif
