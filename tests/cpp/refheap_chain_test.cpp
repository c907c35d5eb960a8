// The hand-over of the exhaustive form's "exact_ties" chain (vaq_exhaust.hip, xs_replay_kernel as one link of a chain
// over shards): vaq::refheap (vaq_amd/csrc/vaq_restated.h) driven over a distance sequence in one go, and again with
// the RAW heap arrays copied to fresh arrays at every cut of 2, 3 and 8 parts of ceil(n / G) rows (empty parts
// included, as on a multi-device refiner whose last shards hold no rows).  The raw arrays after the last part and the
// reordered result must be identical bit for bit -- the statements applied to the heap are the same ones in the same
// order, whatever memory holds it in between.  Stand-alone: no device, its own main.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vaq_restated.h"

namespace {

struct Heap {
  std::vector<float> v;
  std::vector<int> id;
};

// VAQ.cpp:863-872 over rows [lo, hi) of the sequence, as the link's lane 0 applies it
void walk(Heap &h, int k, const std::vector<float> &d, int lo, int hi, int id_base) {
  for (int i = lo; i < hi; i++)
    if (h.v[0] > d[i]) {
      vaq::refheap::pop(k, h.v.data(), h.id.data());
      vaq::refheap::push(k, h.v.data(), h.id.data(), d[i], id_base + i);
    }
}

Heap fresh(int k) {
  Heap h{std::vector<float>((size_t)k), std::vector<int>((size_t)k)};
  vaq::refheap::heapify(k, h.v.data(), h.id.data());
  return h;
}

bool same(const Heap &a, const Heap &b) {
  return std::memcmp(a.v.data(), b.v.data(), a.v.size() * 4) == 0 && a.id == b.id;
}

// the k slots a finishing link writes
Heap finish(Heap h, int k) {
  const int kept = vaq::refheap::reorder(k, h.v.data(), h.id.data());
  Heap out{std::vector<float>((size_t)k, FLT_MAX), std::vector<int>((size_t)k, -1)};
  for (int i = 0; i < kept; i++) {
    out.v[(size_t)i] = h.v[(size_t)(k - kept + i)];
    out.id[(size_t)i] = h.id[(size_t)(k - kept + i)];
  }
  return out;
}

int check(const char *what, const std::vector<float> &d, int k, int id_base) {
  const int n = (int)d.size();
  Heap whole = fresh(k);
  walk(whole, k, d, 0, n, id_base);
  const Heap want = finish(whole, k);
  int bad = 0;
  for (const int G : {2, 3, 8}) {
    const int per = n > 0 ? (n + G - 1) / G : 0;
    Heap carried = fresh(k);
    for (int g = 0; g < G; g++) {
      const int lo = std::min(n, g * per), hi = std::min(n, lo + per);
      if (lo == hi) continue;  // (a shard without rows is skipped by the chain)
      Heap mine{carried.v, carried.id};  // the hand-over: a copy of the raw arrays, nothing else
      walk(mine, k, d, lo, hi, id_base);
      carried = mine;
    }
    if (!same(carried, whole) || !same(finish(carried, k), want)) {
      std::printf("%s: k=%d n=%d G=%d differs\n", what, k, n, G);
      bad++;
    }
  }
  return bad;
}

uint32_t rng_state = 12345u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (const int k : {1, 2, 10, 100}) {
    for (const int n : {0, 1, 2, 7, 8, 9, 50, 99, 100, 101, 300, 1000}) {
      std::vector<float> ints((size_t)n), cont((size_t)n), odd((size_t)n);
      for (int i = 0; i < n; i++) {
        ints[(size_t)i] = (float)(rnd() % 12);  // integer-valued, many ties
        cont[(size_t)i] = (float)rnd() / 1024.0f;
        const uint32_t r = rnd() % 10;
        odd[(size_t)i] = r == 0   ? std::numeric_limits<float>::infinity()
                         : r == 1 ? std::numeric_limits<float>::quiet_NaN()
                         : r == 2 ? FLT_MAX
                                  : (float)(rnd() % 6);
      }
      bad += check("integers", ints, k, 0);
      bad += check("continuous", cont, k, 1000000);
      bad += check("inf/NaN", odd, k, 7);
      cases += 3;
    }
  }
  if (bad) return 1;
  std::printf("refheap_chain_test: ok (%d sequences x 3 cuts)\n", cases);
  return 0;
}
