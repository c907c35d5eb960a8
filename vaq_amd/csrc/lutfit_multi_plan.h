// lutfit_multi_plan.h -- the host-only planning of the sharded quantile fit (vaqhip_multi_lutfit.cpp, DESIGN.md
// section 4d "Across shards"): who owns a dimension, the rounds, where a shard's slice of a column lies in its owner's
// key buffer, and how many words each side needs.  No HIP in here: tests/cpp/lutfit_multi_plan_test.cpp runs it on the
// CPU, plain and under AddressSanitizer / UBSan.
//
// Dimension d is owned by device d % G.  Round t covers the dimensions [t * G, min(D, (t + 1) * G)): slot w of the
// round is dimension t * G + w and its owner is w, so a round gives every owner at most one column, the last round
// may be partial and D < G leaves owners idle.  Owner w keeps the results of its dimensions w, w + G, ... in
// consecutive slots (slot t = round t).  A column of n keys is tiled by the shards' slices in shard order: shard g's
// n_g keys lie at words [lo_g, lo_g + n_g), lo_g the rows before it.  All counts are int64_t.
#ifndef VAQ_LUTFIT_MULTI_PLAN_H_
#define VAQ_LUTFIT_MULTI_PLAN_H_

#include <stdint.h>

namespace vaq {
namespace lutfit_plan {

constexpr int MAX_SHARDS = 16;  // VAQHIP_MAX_DEVICES; also the most columns the column kernel takes at once

inline int owner_of(int d, int G) { return d % G; }
inline int slot_of(int d, int G) { return d / G; }  // where the owner keeps dimension d
inline int rounds(int D, int G) { return (D + G - 1) / G; }
inline int round_first(int t, int G) { return t * G; }
inline int round_width(int t, int D, int G) {
  const int left = D - t * G;
  return left < G ? (left < 0 ? 0 : left) : G;
}
// dimensions owner w fits in all: the slots it holds
inline int owned_dims(int w, int D, int G) { return w < D ? (D - w + G - 1) / G : 0; }

// the cut of n rows over G shards in the host form: vaqhip_multi_set_codes_u16's (shard_cut)
inline void host_cut(int64_t n, int G, int g, int64_t *lo, int64_t *cnt) {
  const int64_t per = (n + G - 1) / G;
  const int64_t a = (int64_t)g * per < n ? (int64_t)g * per : n;
  const int64_t b = (int64_t)(g + 1) * per < n ? (int64_t)(g + 1) * per : n;
  *lo = a;
  *cnt = b - a;
}

struct Plan {
  int G = 0, D = 0;
  int64_t n = 0;
  int64_t lo[MAX_SHARDS] = {}, cnt[MAX_SHARDS] = {};
};

// From the shards' row counts in shard order (the refiner form: whatever set_rows and add_rows left).  false when G,
// D or a count is out of range.
inline bool plan_from_counts(int G, int D, const int64_t *cnt, Plan *p) {
  if (G < 1 || G > MAX_SHARDS || D < 1) return false;
  p->G = G;
  p->D = D;
  int64_t at = 0;
  for (int g = 0; g < G; g++) {
    if (cnt[g] < 0) return false;
    p->lo[g] = at;
    p->cnt[g] = cnt[g];
    at += cnt[g];
  }
  p->n = at;
  return true;
}

inline bool plan_host(int G, int D, int64_t n, Plan *p) {
  if (G < 1 || G > MAX_SHARDS || D < 1 || n < 0) return false;
  int64_t cnt[MAX_SHARDS];
  for (int g = 0; g < G; g++) {
    int64_t lo;
    host_cut(n, G, g, &lo, &cnt[g]);
  }
  return plan_from_counts(G, D, cnt, p);
}

// words of shard g's column scratch (G slices of n_g keys) and of one of an owner's two key buffers
inline int64_t shard_scratch_words(const Plan &p, int g) { return (int64_t)p.G * p.cnt[g]; }
inline int64_t owner_key_words(const Plan &p) { return p.n; }
// where slice w of shard g's scratch starts, and where it goes in owner w's key buffer
inline int64_t slice_src_word(const Plan &p, int g, int w) { return (int64_t)w * p.cnt[g]; }
inline int64_t slice_dst_word(const Plan &p, int g) { return p.lo[g]; }

}  // namespace lutfit_plan
}  // namespace vaq
#endif
