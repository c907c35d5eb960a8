// fit_codebooks_hier_plan.h -- the host arithmetic of the hierarchical codebook fit (vaqhip_fit_codebooks_hier*,
// VAQ::train with mHierarchicalKmeans, VAQ.cpp:535-594): which subspaces are fitted in two stages (more than 8 bits:
// 128 centres, then 1 << (bits - 7) centres inside each of the 128 groups), how many rows R_s such a subspace works
// on, the stage-1 batch (the flat subspaces and the 128-centre fits in ONE run of the Lloyd phases), and -- from the
// group counts read back after the membership pass -- the refusals, the stage-2 batch and its table of row tiles.
// No HIP in here: tests/cpp/fit_codebooks_hier_plan_test.cpp runs it on the CPU.
#ifndef VAQ_FIT_CODEBOOKS_HIER_PLAN_H_
#define VAQ_FIT_CODEBOOKS_HIER_PLAN_H_

#include "fit_codebooks_plan.h"

namespace vaq {
namespace cbhier {

constexpr int K1 = 128;           // centres of stage 1 (VAQ.cpp:548)
constexpr int K1_BITS = 7;
// (which subspaces: cbfit::wide; the rows R_s of one: cbfit::rows_for)
// the most rows a stage-2 fit takes without sampling (KMeans.hpp:489 with k = K2); larger groups are not built
inline int64_t group_limit(int K2) { return std::max<int64_t>(cbfit::ROWS_PER_CENTRE * K2, cbfit::MIN_SAMPLE); }

// One hierarchical subspace.  R_s = rows randomPermutation(n)[0 .. rows) of the projected matrix.
struct HSub {
  int s;               // the subspace
  int k;               // 1 << bits
  int K2;              // centres per group: k / 128
  int rows;            // rows of R_s
  int stage1_rows;     // rows staticFitSampling works on when handed R_s: min(rows, 65536)
  int resampled;       // 1: stage 1 reads rows randomPermutation(rows)[0 .. 65536) of R_s, gathered compactly
  int c1_off;          // its 128 stage-1 centres in the centre table, in centres (behind the final centres)
  int64_t resample_off;  // first row of its compact stage-1 matrix ([65536][L], back to back); resampled only
  int64_t pair_off;    // first of its membership pairs = first row of its compact regrouped matrix
};

struct Plan : cbfit::WideHead {
  std::vector<HSub> hsub;     // the hierarchical subspaces, ascending
  int64_t resample_rows = 0;  // rows of the compact stage-1 matrices
  cbfit::Batch stage1;        // flat subspaces, then the 128-centre fits, in subspace order (fit index = subspace)
  cbfit::Batch member;        // fit h: 128 centres over all rows of R_s, keys h * 128 + group
};

// bits[s] in 1..15, n in 1..2^31-1, D % M == 0; rows_s >= k_s has been checked (cbfit::first_short_subspace)
inline Plan make_plan(int64_t n, int D, int M, const int *bits) {
  Plan p;
  static_cast<cbfit::WideHead &>(p) = cbfit::wide_head(n, M, bits);
  const int L = D / M;
  for (int s = 0; s < M; s++) {
    const cbfit::Sub &d = p.flat.sub[(size_t)s];
    if (!cbfit::wide(bits[s])) {
      cbfit::batch_add(p.stage1, d.k, d.rows, d.cent_off, d.full ? cbfit::SRC_FULL : cbfit::SRC_SAMPLE, D, s * L, 0);
      continue;
    }
    HSub h;
    h.s = s;
    h.k = 1 << bits[s];
    h.K2 = h.k / K1;
    h.rows = p.rows[(size_t)s];
    h.stage1_rows = (int)cbfit::sample_rows(h.rows, K1);
    h.resampled = h.stage1_rows < h.rows;
    h.c1_off = p.n_cent + (int)p.hsub.size() * K1;
    h.resample_off = p.resample_rows;
    h.pair_off = p.member.n_pairs;
    if (h.resampled) {
      p.resample_rows += h.stage1_rows;
      cbfit::batch_add(p.stage1, K1, h.stage1_rows, h.c1_off, cbfit::SRC_EXTRA, L, 0, h.resample_off);
    } else {
      cbfit::batch_add(p.stage1, K1, h.stage1_rows, h.c1_off, cbfit::SRC_SAMPLE, D, s * L, 0);
    }
    cbfit::batch_add(p.member, K1, h.rows, h.c1_off, cbfit::SRC_SAMPLE, D, s * L, 0);
    // (the membership keys carry no half: group g of subspace h is key h * 128 + g)
    p.member.fit.back().run_off = (int)p.hsub.size() * K1;
    p.hsub.push_back(h);
  }
  p.member.n_runs = (int)p.hsub.size() * K1;
  p.member.key_bits = cbfit::key_bits_for(p.member.n_runs);
  return p;
}

// What the group counts refuse, in the order the header lists them.
enum RefusalKind { OK = 0, NAN_CENTRE, EMPTY_GROUP, SHORT_GROUP, NO_CENTRE, SAMPLED_GROUP };
struct Refusal {
  RefusalKind kind = OK;
  int s = -1, group = -1;  // the subspace and the group (-1 where no single group is to blame)
  int64_t rows = 0;        // the group's rows
  int K2 = 0;
  bool unsupported() const { return kind == SAMPLED_GROUP; }  // the others: the input cannot be fitted at all
};

// counts[h * 128 + g]: rows of group g of hierarchical subspace h.  The first refusal in (subspace, group) order;
// within a group: empty, fewer rows than centres, more rows than a stage-2 fit takes unsampled.
inline Refusal check_groups(const Plan &p, const int *counts) {
  Refusal r;
  for (size_t h = 0; h < p.hsub.size(); h++)
    for (int g = 0; g < K1; g++) {
      const int64_t m = counts[h * K1 + g];
      const HSub &hs = p.hsub[h];
      const RefusalKind kind = m == 0 ? EMPTY_GROUP : m < hs.K2 ? SHORT_GROUP : m > group_limit(hs.K2) ? SAMPLED_GROUP : OK;
      if (kind == OK) continue;
      r.kind = kind;
      r.s = hs.s;
      r.group = g;
      r.rows = m;
      r.K2 = hs.K2;
      return r;
    }
  return r;
}

// The stage-2 batch: fit h * 128 + g has K2 centres over the rows of group g, which are rows
// [pair_off_h + sum of the groups before, ...) of the compact regrouped matrix (row stride L, column 0); its centres
// are rows g * K2 .. of the subspace's block of the output (VAQ.cpp:593).  The tiles cut every group into pieces of
// tile_rows rows, none across a group.  counts must have passed check_groups.
inline cbfit::Batch make_stage2(const Plan &p, const int *counts, int L, int tile_rows) {
  cbfit::Batch b;
  for (size_t h = 0; h < p.hsub.size(); h++) {
    const HSub &hs = p.hsub[h];
    int64_t row0 = hs.pair_off;
    for (int g = 0; g < K1; g++) {
      const int m = counts[h * K1 + g];
      cbfit::batch_add(b, hs.K2, m, p.flat.sub[(size_t)hs.s].cent_off + g * hs.K2, cbfit::SRC_SAMPLE, L, 0, row0);
      cbfit::batch_add_tiles(b, (int)b.fit.size() - 1, m, tile_rows);
      row0 += m;
    }
  }
  return b;
}

}  // namespace cbhier
}  // namespace vaq
#endif
