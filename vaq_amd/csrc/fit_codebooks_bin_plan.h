// fit_codebooks_bin_plan.h -- the host arithmetic of the binary-tree codebook fit (vaqhip_fit_codebooks_bin*, VAQ::train
// with mBinaryKmeans: hierarchicalBinKmeans, VAQ.cpp:1293-1371): which subspaces are fitted as a tree (more than 8
// bits), which block of the output node (depth, index) owns, what becomes of a node once the sizes of its two sides
// are read back (leaf / cut / split), the batches of a level -- the 2-centre fits of all live nodes, the split of all
// their rows, the flat fits of the nodes that are cut --, each cut into chunks of at most 65535 fits with a table of
// row tiles, which fits sample for themselves, and the next level's nodes in the regrouped compact matrix.
// No HIP in here: tests/cpp/fit_codebooks_bin_plan_test.cpp runs it on the CPU.
#ifndef VAQ_FIT_CODEBOOKS_BIN_PLAN_H_
#define VAQ_FIT_CODEBOOKS_BIN_PLAN_H_

#include "fit_codebooks_plan.h"

namespace vaq {
namespace cbbin {

constexpr int MAX_BATCH_FITS = 65535;  // fits one run of the Lloyd phases takes (a grid dimension)

// (which subspaces: cbfit::wide, the hierarchical form's)
// centres node (depth d of maxdepth, any index) stands for: 1 << (maxdepth - d + 1) (VAQ.cpp:1318)
inline int temp_k(int maxdepth, int d) { return 1 << (maxdepth - d + 1); }

// One binary subspace.  R_s = rows randomPermutation(n)[0 .. rows) of the projected matrix (cbfit::rows_for).
struct BSub {
  int s;         // the subspace
  int bits;      // = maxdepth
  int k;         // 1 << bits
  int rows;      // rows of R_s
  int cent_off;  // its block of the output, in centres
};

struct Plan : cbfit::WideHead {  // (n_pairs: rows of a level's compact matrix at most)
  std::vector<BSub> bsub;  // the binary subspaces, ascending
  int max_bits = 0;        // the deepest tree
};

// bits[s] in 1..15, n in 1..2^31-1, D % M == 0; rows_s >= k_s has been checked (cbfit::first_short_subspace)
inline Plan make_plan(int64_t n, int M, const int *bits) {
  Plan p;
  static_cast<cbfit::WideHead &>(p) = cbfit::wide_head(n, M, bits);
  for (int s = 0; s < M; s++) {
    if (!cbfit::wide(bits[s])) continue;
    p.bsub.push_back(BSub{s, bits[s], 1 << bits[s], p.rows[(size_t)s], p.flat.sub[(size_t)s].cent_off});
    p.max_bits = std::max(p.max_bits, bits[s]);
  }
  return p;
}

// Node (depth, index) of binary subspace bsub[b]: `rows` rows of source matrix `src` from row0 on, `stride` floats
// apart, its slice the L floats from column `col`.  The root reads its prefix of the gathered sample in place; every
// later level lives in a compact [rows][L] matrix, the nodes back to back in (subspace, index) order.
struct Node {
  int b, depth, index, rows;
  int src, stride, col;
  int64_t row0;
};
// first centre of the node's block [index * tempK, (index + 1) * tempK) of the subspace's output (VAQ.cpp:1361-1367)
inline int node_cent_off(const BSub &bs, const Node &nd) { return bs.cent_off + nd.index * temp_k(bs.bits, nd.depth); }

inline std::vector<Node> root_level(const Plan &p, int D, int L) {
  std::vector<Node> level;
  for (size_t b = 0; b < p.bsub.size(); b++)
    level.push_back(Node{(int)b, 1, 0, p.bsub[b].rows, cbfit::SRC_SAMPLE, D, p.bsub[b].s * L, 0});
  return level;
}

enum Kind { LEAF = 0, CUT, SPLIT };
// what becomes of a node after its 2-centre fit: at depth maxdepth the two centres are its output; a side with fewer
// rows than the tempK / 2 centres it would have to yield ends the recursion in a flat fit of tempK centres
// (VAQ.cpp:1353); else two children.  left / right are not looked at for a leaf (its rows are not split).
inline Kind decide(const BSub &bs, const Node &nd, int left, int right) {
  if (nd.depth == bs.bits) return LEAF;
  const int half = temp_k(bs.bits, nd.depth) / 2;
  return left < half || right < half ? CUT : SPLIT;
}

// One fit of a level that samples for itself (KMeans.hpp:489-503 over the node's rows): rows
// randomPermutation(node rows)[0 .. rows) of the node, gathered at row `off` of the level's extra matrix ([.][L])
struct Resample {
  int node, rows;
  int64_t off;
};
// The fits of one kind of a level (2-centre fits, or the flat fits of the cut nodes), in chunks the Lloyd phases take.
// owner[c][f]: the node of fit f of chunk c, or -1 - s for flat subspace s (first level only).
struct Fits {
  std::vector<cbfit::Batch> chunk;
  std::vector<std::vector<int>> owner;
  std::vector<Resample> resample;
  int64_t extra_rows = 0;
};

inline void add_fit(Fits &f, int owner, int k, int rows, int cent_off, int src, int stride, int col, int64_t row0, int tile_rows) {
  if (f.chunk.empty() || (int)f.chunk.back().fit.size() == MAX_BATCH_FITS) {
    f.chunk.emplace_back();
    f.owner.emplace_back();
  }
  cbfit::Batch &b = f.chunk.back();
  cbfit::batch_add(b, k, rows, cent_off, src, stride, col, row0);
  cbfit::batch_add_tiles(b, (int)b.fit.size() - 1, rows, tile_rows);
  f.owner.back().push_back(owner);
}

// which[i]: the nodes of `level` to fit, ascending; k = 2, or the node's tempK when `cut`.  with_flat: the call's flat
// subspaces ride in front (the first level's 2-centre batch), reading the sample or all rows, D wide.
inline Fits make_fits(const Plan &p, const std::vector<Node> &level, const std::vector<int> &which, bool cut, bool with_flat,
                      int D, int L, int tile_rows) {
  Fits f;
  if (with_flat) {
    size_t bi = 0;
    for (size_t s = 0; s < p.flat.sub.size(); s++) {
      if (bi < p.bsub.size() && p.bsub[bi].s == (int)s) {
        bi++;
        continue;
      }
      const cbfit::Sub &d = p.flat.sub[s];
      add_fit(f, -1 - (int)s, d.k, d.rows, d.cent_off, d.full ? cbfit::SRC_FULL : cbfit::SRC_SAMPLE, D, (int)s * L, 0, tile_rows);
    }
  }
  for (int i : which) {
    const Node &nd = level[(size_t)i];
    const BSub &bs = p.bsub[(size_t)nd.b];
    const int k = cut ? temp_k(bs.bits, nd.depth) : 2;
    const int rows = (int)cbfit::sample_rows(nd.rows, k);
    if (rows < nd.rows) {
      f.resample.push_back(Resample{i, rows, f.extra_rows});
      add_fit(f, i, k, rows, node_cent_off(bs, nd), cbfit::SRC_EXTRA, L, 0, f.extra_rows, tile_rows);
      f.extra_rows += rows;
    } else {
      add_fit(f, i, k, rows, node_cent_off(bs, nd), nd.src, nd.stride, nd.col, nd.row0, tile_rows);
    }
  }
  return f;
}

// The split of ALL rows of the nodes which[i] (getBelongsToBinaryCluster, VAQ.cpp:1293-1310): fit i = node which[i]
// with its two centres, row r of it emits pair pair_off + r with key 2 * i + side (0 left, 1 right).  A stable sort by
// key leaves every node's rows where they were as a block, its left rows first, each side in ascending position.
inline cbfit::Batch make_split(const Plan &p, const std::vector<Node> &level, const std::vector<int> &which, int tile_rows) {
  cbfit::Batch b;
  for (size_t i = 0; i < which.size(); i++) {
    const Node &nd = level[(size_t)which[i]];
    cbfit::batch_add(b, 2, nd.rows, node_cent_off(p.bsub[(size_t)nd.b], nd), nd.src, nd.stride, nd.col, nd.row0);
    b.fit.back().run_off = 2 * (int)i;
    cbfit::batch_add_tiles(b, (int)i, nd.rows, tile_rows);
  }
  b.n_runs = 2 * (int)which.size();
  b.key_bits = cbfit::key_bits_for(b.n_runs);
  return b;
}

// The next level from the kinds of the split batch's nodes: the children of every SPLIT node which[i], left then
// right, back to back in a compact [.][L] matrix.  dest[i]: the first row there of node which[i]'s sorted block (-1:
// the node has no children, its rows are dropped); *rows: rows of the new matrix.
inline std::vector<Node> next_level(const std::vector<Node> &level, const std::vector<int> &which, const std::vector<Kind> &kind,
                                    const int *left, const int *right, int L, std::vector<int64_t> *dest, int64_t *rows) {
  std::vector<Node> next;
  dest->assign(which.size(), -1);
  int64_t row0 = 0;
  for (size_t i = 0; i < which.size(); i++) {
    if (kind[i] != SPLIT) continue;
    const Node &nd = level[(size_t)which[i]];
    (*dest)[i] = row0;
    next.push_back(Node{nd.b, nd.depth + 1, 2 * nd.index, left[i], cbfit::SRC_SAMPLE, L, 0, row0});
    next.push_back(Node{nd.b, nd.depth + 1, 2 * nd.index + 1, right[i], cbfit::SRC_SAMPLE, L, 0, row0 + left[i]});
    row0 += nd.rows;
  }
  *rows = row0;
  return next;
}

}  // namespace cbbin
}  // namespace vaq
#endif
