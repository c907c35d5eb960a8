// fit_codebooks_bin_plan_test.cpp -- the host arithmetic of the binary-tree codebook fit
// (vaq_amd/csrc/fit_codebooks_bin_plan.h) on the CPU: the plan of a mixed call, the decision per node, node offsets
// that tile the subspace's block for EVERY cut pattern of a 4-level tree, the chunks of a level above 65535 fits,
// tiles that never span a node, and which fits sample for themselves.
//   fit_codebooks_bin_plan_test self
//   fit_codebooks_bin_plan_test rows n M b0,b1,...   -> one line per binary subspace: s bits k rows cent_off
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fit_codebooks_bin_plan.h"

using namespace vaq;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static std::vector<int> all_of(const std::vector<cbbin::Node> &level) {
  std::vector<int> w(level.size());
  for (size_t i = 0; i < w.size(); i++) w[i] = (int)i;
  return w;
}

// every tile lies inside its fit, starts on a multiple of tile_rows, and the tiles of a fit cover its rows once
static void check_tiles(const cbfit::Batch &b, int tile_rows) {
  std::vector<int64_t> covered(b.fit.size(), 0);
  for (const cbfit::Tile &t : b.tile) {
    CHECK(t.fit >= 0 && t.fit < (int)b.fit.size());
    CHECK(t.row0 % tile_rows == 0 && t.row0 < b.fit[(size_t)t.fit].rows);
    covered[(size_t)t.fit] += std::min(tile_rows, b.fit[(size_t)t.fit].rows - t.row0);
  }
  for (size_t f = 0; f < b.fit.size(); f++) CHECK(covered[f] == b.fit[f].rows);
}

// a 4-level tree under every pattern of cuts: bit i of `pattern` cuts the i-th inner node met in level order
static void check_tree(int pattern) {
  cbbin::Plan p;
  p.bsub.push_back(cbbin::BSub{0, 4, 16, 1600, 5});
  std::vector<int> covered(5 + 16 + 3, 0);
  std::vector<cbbin::Node> level = {cbbin::Node{0, 1, 0, 1600, cbfit::SRC_SAMPLE, 2, 0, 0}};
  int met = 0;
  for (int depth = 1; !level.empty(); depth++) {
    CHECK(depth <= 4);
    std::vector<int> inner;
    for (size_t i = 0; i < level.size(); i++) {
      const cbbin::Node &nd = level[i];
      CHECK(nd.depth == depth && nd.rows >= cbbin::temp_k(4, depth));
      if (cbbin::decide(p.bsub[0], nd, 0, 0) == cbbin::LEAF) {
        CHECK(depth == 4);
        for (int c = 0; c < 2; c++) covered[(size_t)cbbin::node_cent_off(p.bsub[0], nd) + c]++;
      } else {
        inner.push_back((int)i);
      }
    }
    if (inner.empty()) break;
    const cbfit::Batch split = cbbin::make_split(p, level, inner, 64);
    check_tiles(split, 64);
    std::vector<int> left(inner.size()), right(inner.size());
    std::vector<cbbin::Kind> kind(inner.size());
    int64_t pair = 0;
    for (size_t i = 0; i < inner.size(); i++) {
      const cbbin::Node &nd = level[(size_t)inner[i]];
      const int half = cbbin::temp_k(4, depth) / 2;
      const bool cut = (pattern >> met++) & 1;
      left[i] = cut ? half - 1 : nd.rows / 2 + 1;  // (uneven on purpose)
      right[i] = nd.rows - left[i];
      kind[i] = cbbin::decide(p.bsub[0], nd, left[i], right[i]);
      CHECK(kind[i] == (cut ? cbbin::CUT : cbbin::SPLIT));
      CHECK(split.fit[i].run_off == 2 * (int)i && split.fit[i].pair_off == pair && split.fit[i].rows == nd.rows);
      pair += nd.rows;
      if (cut)
        for (int c = 0; c < cbbin::temp_k(4, depth); c++) covered[(size_t)cbbin::node_cent_off(p.bsub[0], nd) + c]++;
    }
    std::vector<int64_t> dest;
    int64_t rows = 0;
    std::vector<cbbin::Node> next = cbbin::next_level(level, inner, kind, left.data(), right.data(), 2, &dest, &rows);
    int64_t at = 0;
    size_t ni = 0;
    for (size_t i = 0; i < inner.size(); i++) {
      if (kind[i] != cbbin::SPLIT) {
        CHECK(dest[i] == -1);
        continue;
      }
      const cbbin::Node &nd = level[(size_t)inner[i]];
      CHECK(dest[i] == at);
      CHECK(next[ni].index == 2 * nd.index && next[ni].row0 == at && next[ni].rows == left[i]);
      CHECK(next[ni + 1].index == 2 * nd.index + 1 && next[ni + 1].row0 == at + left[i] && next[ni + 1].rows == right[i]);
      CHECK(next[ni].stride == 2 && next[ni].col == 0 && next[ni].src == cbfit::SRC_SAMPLE);
      at += nd.rows;
      ni += 2;
    }
    CHECK(ni == next.size() && rows == at);
    level.swap(next);
  }
  for (size_t c = 0; c < covered.size(); c++) CHECK(covered[c] == (c >= 5 && c < 21 ? 1 : 0));  // the block, exactly once
}

static int self() {
  // ---- the plan of a mixed call: `two`'s shape, and the budget term of rows_s ----
  {
    const int bits[4] = {10, 9, 8, 5};
    const cbbin::Plan p = cbbin::make_plan(6000, 4, bits);
    CHECK(p.bsub.size() == 2 && p.bsub[0].s == 0 && p.bsub[1].s == 1);
    CHECK(p.bsub[0].k == 1024 && p.bsub[0].rows == 6000 && p.bsub[0].cent_off == 0);
    CHECK(p.bsub[1].k == 512 && p.bsub[1].rows == 6000 && p.bsub[1].cent_off == 1024);
    CHECK(p.n_cent == 1024 + 512 + 256 + 32 && p.n_pairs == 12000 && p.max_bits == 10 && p.gathered == 6000 && p.n_full == 2);
    const int wide[2] = {9, 11};
    const cbbin::Plan q = cbbin::make_plan(1000000, 2, wide);
    CHECK(q.bsub[0].rows == (256 << 10) && q.bsub[1].rows == (256 << 11) && q.gathered == (256 << 11));
    CHECK(cbhier::first_short_subspace(300, 2, wide) == 0 && cbhier::first_short_subspace(3000, 2, wide) == -1);
    const std::vector<cbbin::Node> root = cbbin::root_level(q, 4, 2);
    CHECK(root.size() == 2 && root[1].stride == 4 && root[1].col == 2 && root[1].row0 == 0 && root[1].rows == (256 << 11));
  }
  // ---- the decision ----
  {
    const cbbin::BSub bs{0, 9, 512, 3000, 0};
    const cbbin::Node mid{0, 3, 1, 900, 0, 2, 0, 0};  // tempK = 128: a side needs 64 rows
    CHECK(cbbin::temp_k(9, 3) == 128 && cbbin::temp_k(9, 9) == 2 && cbbin::temp_k(9, 1) == 512);
    CHECK(cbbin::decide(bs, mid, 64, 836) == cbbin::SPLIT && cbbin::decide(bs, mid, 63, 837) == cbbin::CUT);
    CHECK(cbbin::decide(bs, mid, 836, 63) == cbbin::CUT && cbbin::decide(bs, mid, 0, 900) == cbbin::CUT);
    const cbbin::Node leaf{0, 9, 7, 3, 0, 2, 0, 0};
    CHECK(cbbin::decide(bs, leaf, 0, 0) == cbbin::LEAF && cbbin::node_cent_off(bs, leaf) == 14);
    CHECK(cbbin::node_cent_off(bs, mid) == 128);
  }
  // ---- every cut pattern of a 4-level tree tiles the block ----
  for (int pattern = 0; pattern < 128; pattern++) check_tree(pattern);
  // ---- a level of more fits than one run of the phases takes; tiles; flat subspaces in front ----
  {
    const int bits[3] = {3, 15, 15};
    cbbin::Plan p = cbbin::make_plan(5000000, 3, bits);
    std::vector<cbbin::Node> level;
    int64_t row0 = 0;
    for (int b = 0; b < 2; b++)
      for (int j = 0; j < 35000; j++) {
        const int rows = 2 + (j % 300);
        level.push_back(cbbin::Node{b, 15, j % 16384, rows, cbfit::SRC_SAMPLE, 2, 0, row0});
        row0 += rows;
      }
    const cbbin::Fits f = cbbin::make_fits(p, level, all_of(level), false, true, 6, 2, 256);
    CHECK(f.chunk.size() == 2 && f.chunk[0].fit.size() == 65535 && f.chunk[1].fit.size() == 70001 - 65535);
    CHECK(f.owner[0][0] == -1 && f.owner[0][1] == 0 && f.owner[1][0] == 65534 && f.resample.empty());
    CHECK(f.chunk[0].fit[0].k == 8 && f.chunk[0].fit[0].stride == 6 && f.chunk[0].fit[0].col == 0);
    CHECK(f.chunk[1].fit[0].run_off == 0 && f.chunk[1].fit[0].pair_off == 0);  // (a chunk is a batch of its own)
    for (size_t c = 0; c < 2; c++) {
      check_tiles(f.chunk[c], 256);
      for (size_t i = 0; i < f.chunk[c].fit.size(); i++) {
        const int o = f.owner[c][i];
        if (o < 0) continue;
        const cbfit::Fit &fd = f.chunk[c].fit[i];
        CHECK(fd.k == 2 && fd.rows == level[(size_t)o].rows && fd.row0 == level[(size_t)o].row0 && fd.stride == 2);
        CHECK(fd.cent_off == p.bsub[(size_t)level[(size_t)o].b].cent_off + 2 * level[(size_t)o].index);
      }
    }
  }
  // ---- which fits sample for themselves ----
  {
    const int bits[1] = {9};
    const cbbin::Plan p = cbbin::make_plan(140000, 1, bits);
    CHECK(p.bsub[0].rows == 131072);
    std::vector<cbbin::Node> level = {cbbin::Node{0, 2, 0, 98304, cbfit::SRC_SAMPLE, 2, 0, 0},
                                      cbbin::Node{0, 2, 1, 32768, cbfit::SRC_SAMPLE, 2, 0, 98304}};
    const cbbin::Fits two = cbbin::make_fits(p, level, all_of(level), false, false, 2, 2, 256);
    CHECK(two.resample.size() == 1 && two.resample[0].node == 0 && two.resample[0].rows == 65536 && two.extra_rows == 65536);
    CHECK(two.chunk[0].fit[0].src == cbfit::SRC_EXTRA && two.chunk[0].fit[0].rows == 65536 && two.chunk[0].fit[0].row0 == 0);
    CHECK(two.chunk[0].fit[1].src == cbfit::SRC_SAMPLE && two.chunk[0].fit[1].rows == 32768 && two.chunk[0].fit[1].row0 == 98304);
    const cbbin::Fits cut = cbbin::make_fits(p, level, {0}, true, false, 2, 2, 256);  // tempK = 256: above 65536 rows it samples
    CHECK(cut.chunk[0].fit[0].k == 256 && cut.resample.size() == 1 && cut.chunk[0].fit[0].rows == 65536);
    CHECK(cut.chunk[0].fit[0].cent_off == 0);
    std::vector<cbbin::Node> root = cbbin::root_level(p, 2, 2);
    const cbbin::Fits rootcut = cbbin::make_fits(p, root, {0}, true, false, 2, 2, 256);  // 131072 = 256 * 512: all rows
    CHECK(rootcut.resample.empty() && rootcut.chunk[0].fit[0].k == 512 && rootcut.chunk[0].fit[0].rows == 131072);
    check_tiles(rootcut.chunk[0], 256);
  }
  std::printf("fit_codebooks_bin_plan_test: ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "self") == 0) return self();
  if (argc == 5 && std::strcmp(argv[1], "rows") == 0) {
    const int64_t n = std::atoll(argv[2]);
    const int M = std::atoi(argv[3]);
    std::vector<int> bits;
    for (char *tok = std::strtok(argv[4], ","); tok; tok = std::strtok(nullptr, ",")) bits.push_back(std::atoi(tok));
    if ((int)bits.size() != M) return 2;
    const cbbin::Plan p = cbbin::make_plan(n, M, bits.data());
    for (const cbbin::BSub &b : p.bsub) std::printf("%d %d %d %d %d\n", b.s, b.bits, b.k, b.rows, b.cent_off);
    return 0;
  }
  std::printf("usage: fit_codebooks_bin_plan_test self | rows n M bits\n");
  return 2;
}
