// fit_codebooks_multi_plan.h -- the host-only planning of the sharded codebook fit (vaqhip_multi_codebooks.cpp,
// DESIGN.md section 4f "Across shards"): who owns a subspace, every owner's compact columns and sub-plan, which rows of
// the sample each shard holds, and where a shard's block lands at its owner.  No HIP in here:
// tests/cpp/fit_codebooks_multi_plan_test.cpp runs it on the CPU, plain and under AddressSanitizer / UBSan.
//
// Subspace s is owned by device s % G; owner w holds its subspaces w, w + G, ... in that order as the columns
// [i * L, (i + 1) * L) of a compact matrix D_w = |subs_w| * L wide, and its sub-plan is cbfit::make_plan over just
// their bits: the Sub entries the kernels read, with offsets of the owner's own.  M < G leaves owners idle.
// An owner whose sub-plan has a subspace with full == 1 receives ALL n rows of its columns (shard g's block at row
// lo_g of its n x D_w matrix) and gathers the sample of its other subspaces from them itself, as the single fit does.
// Every other owner receives the sample only: shard g holds the positions `pos` of permutation_head(n, gathered) whose
// row lies in [lo_g, lo_g + n_g), ascending, at the local rows `local`; owner w takes those below its own
// plan.gathered -- a prefix of the shard's list, since a smaller sample is a prefix of a larger one -- and the
// shards' blocks lie back to back in shard order in its staging area, each row to be placed at its position.
#ifndef VAQ_FIT_CODEBOOKS_MULTI_PLAN_H_
#define VAQ_FIT_CODEBOOKS_MULTI_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <vector>

#include "fit_codebooks_plan.h"
#include "kmeans_sample.h"

namespace vaq {
namespace cbfit_multi {

constexpr int MAX_SHARDS = 16;  // VAQHIP_MAX_DEVICES

inline int owner_of(int s, int G) { return s % G; }

// the cut of n rows over G shards in the host form: vaqhip_multi_set_codes_u16's (shard_cut)
inline void host_cut(int64_t n, int G, int g, int64_t *lo, int64_t *cnt) {
  const int64_t per = (n + G - 1) / G;
  const int64_t a = std::min<int64_t>(n, (int64_t)g * per), b = std::min<int64_t>(n, (int64_t)(g + 1) * per);
  *lo = a;
  *cnt = b - a;
}

struct Owner {
  std::vector<int> subs;  // its subspaces, ascending: compact column i * L + j is column subs[i] * L + j of the rows
  int D_w = 0;            // |subs| * L
  cbfit::Plan plan;       // make_plan(n, |subs|, their bits); unused when subs is empty
  bool idle() const { return subs.empty(); }
  bool full() const { return !subs.empty() && plan.n_full > 0; }  // it receives all n rows
  int64_t staged() const { return idle() || full() ? 0 : plan.gathered; }  // sample rows it receives through staging
};

struct ShardPart {
  int64_t lo = 0, cnt = 0;     // rows [lo, lo + cnt) of the training rows
  std::vector<int> pos, local;  // the sample positions it holds, ascending, and the local row of each
};

struct Plan {
  int G = 0, M = 0, L = 0;
  int64_t n = 0;
  cbfit::Plan whole;  // make_plan(n, M, bits): what the single fit works from
  std::vector<Owner> owner;
  std::vector<ShardPart> shard;
};

// rows of shard g's sample block for owner w: its positions below the owner's own sample length
inline int64_t sample_count(const Plan &p, int g, int w) {
  const std::vector<int> &pos = p.shard[(size_t)g].pos;
  const int64_t S = p.owner[(size_t)w].staged();
  return std::lower_bound(pos.begin(), pos.end(), S, [](int a, int64_t b) { return (int64_t)a < b; }) - pos.begin();
}
// the staging row at owner w where shard g's sample block starts: the blocks of the shards before it
inline int64_t stage_row(const Plan &p, int g, int w) {
  int64_t at = 0;
  for (int h = 0; h < g; h++) at += sample_count(p, h, w);
  return at;
}
// rows of shard g's block for owner w, either kind
inline int64_t block_rows(const Plan &p, int g, int w) {
  const Owner &o = p.owner[(size_t)w];
  return o.idle() ? 0 : o.full() ? p.shard[(size_t)g].cnt : sample_count(p, g, w);
}
// floats of shard g's packed blocks over all owners (its scratch), and where owner w's starts
inline int64_t block_at(const Plan &p, int g, int w) {
  int64_t at = 0;
  for (int v = 0; v < w; v++) at += block_rows(p, g, v) * p.owner[(size_t)v].D_w;
  return at;
}
inline int64_t scratch_floats(const Plan &p, int g) { return block_at(p, g, p.G); }

// cnt[G]: the shards' row counts in shard order (the refiner's own cut: empty shards, a grown last shard); bits[M] in
// 1..30, D % M == 0.  false when G, a count or the sum is out of range.
inline bool plan_from_counts(int G, const int64_t *cnt, int D, int M, const int *bits, Plan *p) {
  if (G < 1 || G > MAX_SHARDS || M < 1 || D < 1 || D % M != 0) return false;
  int64_t n = 0;
  for (int g = 0; g < G; g++) {
    if (cnt[g] < 0) return false;
    n += cnt[g];
  }
  if (n < 1 || n >= ((int64_t)1 << 31)) return false;
  p->G = G;
  p->M = M;
  p->L = D / M;
  p->n = n;
  p->whole = cbfit::make_plan(n, M, bits);
  p->owner.assign((size_t)G, Owner{});
  for (int s = 0; s < M; s++) p->owner[(size_t)owner_of(s, G)].subs.push_back(s);
  for (Owner &o : p->owner) {
    if (o.subs.empty()) continue;
    std::vector<int> b;
    for (int s : o.subs) b.push_back(bits[s]);
    o.D_w = (int)o.subs.size() * p->L;
    o.plan = cbfit::make_plan(n, (int)b.size(), b.data());
  }
  // the longest sample an owner receives through staging (an owner of a full subspace gathers for itself)
  int64_t S = 0;
  for (const Owner &o : p->owner) S = std::max(S, o.staged());
  int64_t lo[MAX_SHARDS], at = 0;
  for (int g = 0; g < G; g++) {
    lo[g] = at;
    at += cnt[g];
  }
  std::vector<KmeansShardSample> split((size_t)G);
  if (S > 0) split = kmeans_split_sample(permutation_head(n, S), lo, cnt, G);
  p->shard.assign((size_t)G, ShardPart{});
  for (int g = 0; g < G; g++) {
    ShardPart &sp = p->shard[(size_t)g];
    sp.lo = lo[g];
    sp.cnt = cnt[g];
    sp.pos.swap(split[(size_t)g].pos);
    sp.local.swap(split[(size_t)g].local);
  }
  return true;
}

inline bool plan_host(int G, int64_t n, int D, int M, const int *bits, Plan *p) {
  if (G < 1 || G > MAX_SHARDS || n < 1) return false;
  int64_t cnt[MAX_SHARDS];
  for (int g = 0; g < G; g++) {
    int64_t lo;
    host_cut(n, G, g, &lo, &cnt[g]);
  }
  return plan_from_counts(G, cnt, D, M, bits, p);
}

}  // namespace cbfit_multi
}  // namespace vaq
#endif
