// train_plan.h -- the host arithmetic of VAQ::train's front half between the eigenvalues and the bits (no HIP):
//   sample_rows    which rows the second moment reads (VAQ.cpp:17-24)
//   make_plan      VAQ.cpp:80-96, 243-280, 301-336, 374-412 restated in float, bit for bit: the descending order, the
//                  partial balance, varExplainedPerSubs in Eigen's sum() / segment().sum() order, the sequential
//                  cumSum (Math.hpp:173), mHighestSubs, the lower bounds and the k_i = nextPow2 (Math.hpp:183) of the ILP
//   allocate_bits  the ILP itself, solved exactly by dynamic programming (glpk is not reproduced)
// Pinned by tests/golden/train against the compiled statements of the reference (tests/test_train_cpu.py).
#ifndef VAQ_TRAIN_PLAN_H_
#define VAQ_TRAIN_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

namespace vaq {
namespace train {

constexpr int64_t MOMENT_ROWS_PER_DIM = 1000;  // covmatsamplesize = 1000 * XTrain.cols()
constexpr int MOMENT_TILE = 1024;              // sample positions whose products are added into one partial

// rows the second moment sums, and whether they are the head of randomPermutation(n) (else all rows in order)
inline int64_t sample_rows(int64_t n, int D, bool *sampled) {
  const int64_t s = MOMENT_ROWS_PER_DIM * D;
  *sampled = s < n;
  return *sampled ? s : n;
}

// Eigen's sum() over the `size` floats at v + off, v the data of a VectorXf (32-byte aligned): Redux.h's
// LinearVectorizedTraversal with 8-float packets.  A segment starts its packets at the first aligned element, adds
// the elements before it and after the last packet one by one AFTER the packets' predux.
inline float eigen_sum(const float *v, int off, int size) {
  const float *x = v + off;
  const int start = std::min((8 - (off & 7)) & 7, size);
  const int n1 = ((size - start) / 8) * 8, n2 = ((size - start) / 16) * 16;
  const int end1 = start + n1, end2 = start + n2;
  if (!n1) {
    float res = x[0];
    for (int j = 1; j < size; j++) res += x[j];
    return res;
  }
  float a0[8], a1[8];
  for (int l = 0; l < 8; l++) a0[l] = x[start + l];
  if (n1 > 8) {
    for (int l = 0; l < 8; l++) a1[l] = x[start + 8 + l];
    for (int i = start + 16; i < end2; i += 16)
      for (int l = 0; l < 8; l++) {
        a0[l] += x[i + l];
        a1[l] += x[i + 8 + l];
      }
    for (int l = 0; l < 8; l++) a0[l] += a1[l];
    if (end1 > end2)
      for (int l = 0; l < 8; l++) a0[l] += x[end2 + l];
  }
  float res = ((a0[0] + a0[4]) + (a0[2] + a0[6])) + ((a0[1] + a0[5]) + (a0[3] + a0[7]));
  for (int j = 0; j < start; j++) res += x[j];
  for (int j = end1; j < size; j++) res += x[j];
  return res;
}

// Math.hpp:183 on the float ratio widened to double, then VAQ.cpp:409-411; the power is clamped to 2^30 (the
// reference's (int) cast of a larger one is undefined, and any k >= max_bits constrains nothing)
inline int next_pow2_k(double x) {
  if (x == 0) return 0;
  const double p = std::pow(2, std::floor(std::log2(std::fabs(x))));
  if (!(p > 0)) return 0;  // (NaN too)
  if (p >= 1073741824.0) return 1 << 30;
  return (int)p;
}

struct Plan {
  std::vector<int> sorted, order;  // columns by descending eigenvalue; the same after the partial balance
  std::vector<float> var, cum;     // varExplainedPerSubs[M], mCumSumVarExplainedPerSubs[M]
  std::vector<int> lb, k;          // lb[highest], k[highest - 1]
  int highest = 0, swaps_kept = 0;
};

// 0, or 1: a non-finite eigenvalue, 2: their sum is not positive.  D % M == 0, M >= 1 are the caller's.
inline int make_plan(const float *eig, int D, int M, float percent_var, int min_bits, Plan *out) {
  for (int i = 0; i < D; i++)
    if (!std::isfinite(eig[i])) return 1;
  const int L = D / M;
  Plan &pl = *out;
  pl.sorted.resize((size_t)D);
  std::iota(pl.sorted.begin(), pl.sorted.end(), 0);
  std::stable_sort(pl.sorted.begin(), pl.sorted.end(), [&](int a, int b) { return eig[a] > eig[b]; });
  pl.order = pl.sorted;
  std::vector<float> ev((size_t)D), subs((size_t)M);
  for (int i = 0; i < D; i++) ev[(size_t)i] = eig[pl.order[(size_t)i]];
  // the partial balance: dimension i of subspace 0 against the last of subspace i, while the sums stay sorted
  const int maxsubswap = std::min(L, M);
  pl.swaps_kept = 0;
  for (int i = 1; i < maxsubswap; i++) {
    const int j = i * L + (L - 1);
    std::swap(ev[(size_t)i], ev[(size_t)j]);
    for (int s = 0; s < M; s++) subs[(size_t)s] = eigen_sum(ev.data(), s * L, L);
    bool ordered = true;  // std::is_sorted by lhs > rhs: no element above the one before it
    for (int s = 1; s < M; s++) ordered &= !(subs[(size_t)s] > subs[(size_t)s - 1]);
    if (!ordered) {
      std::swap(ev[(size_t)i], ev[(size_t)j]);
      break;
    }
    std::swap(pl.order[(size_t)i], pl.order[(size_t)j]);
    pl.swaps_kept++;
  }
  const float total = eigen_sum(ev.data(), 0, D);
  if (!(total > 0.0f) || !std::isfinite(total)) return 2;
  for (int i = 0; i < D; i++) {
    ev[(size_t)i] /= total;
    if (ev[(size_t)i] < 0.000000000001) ev[(size_t)i] = 0.000000000001;  // (compared in double, stored as float)
  }
  pl.var.resize((size_t)M);
  pl.cum.resize((size_t)M);
  for (int s = 0; s < M; s++) pl.var[(size_t)s] = eigen_sum(ev.data(), s * L, L);
  pl.cum[0] = pl.var[0];
  for (int s = 1; s < M; s++) pl.cum[(size_t)s] = pl.var[(size_t)s] + pl.cum[(size_t)s - 1];
  pl.highest = M;
  if (percent_var < 1) {
    pl.highest = 0;
    for (int s = 0; s < M; s++)
      if (pl.cum[(size_t)s] <= percent_var) pl.highest = s;
    pl.highest += 1;
  }
  pl.lb.assign((size_t)pl.highest, 0);
  pl.k.assign((size_t)pl.highest - 1, 0);
  for (int s = 0; s < pl.highest; s++)
    if (pl.cum[(size_t)s] <= percent_var) pl.lb[(size_t)s] = min_bits;
  for (int s = 0; s + 1 < pl.highest; s++) pl.k[(size_t)s] = next_pow2_k((double)(pl.var[(size_t)s] / pl.var[(size_t)s + 1]));
  return 0;
}

// The ILP of VAQ.cpp:342-452: maximise sum c_i x_i subject to sum x_i = budget, lb_i <= x_i <= max_bits and
// x_i - x_(i+1) <= k_i.  The objective of an allocation is its sum in double in ascending i (c_i widened, as glpk
// receives it).  Rounded addition is monotone, so the best value over all allocations is the best value of a forward
// pass over (subspace, its bits, bits spent) that keeps the largest prefix sum per state.  Among the allocations that
// reach it the lexicographically greatest is returned: subspace by subspace the most bits from which the optimum is
// still reached, each candidate checked by the same forward pass from the prefix's own sum.
struct BitsDp {
  int H, maxb, B;
  const float *c;
  const int *lb, *k;
  std::vector<double> cur, nxt;
  static double none() { return -std::numeric_limits<double>::infinity(); }
  size_t at(int x, int sp) const { return (size_t)x * (size_t)(B + 1) + (size_t)sp; }

  // best final objective from subspace i holding x bits with `spent` bits used and the prefix sum v
  double best_from(int i, int x, int spent, double v) {
    cur.assign((size_t)(maxb + 1) * (size_t)(B + 1), none());
    cur[at(x, spent)] = v;
    for (int j = i + 1; j < H; j++) {
      nxt.assign(cur.size(), none());
      const double cj = (double)c[j];
      for (int xp = 0; xp <= maxb; xp++)
        for (int sp = 0; sp <= B; sp++) {
          const double pv = cur[at(xp, sp)];
          if (pv == none()) continue;
          // (and at least what the subspaces behind j cannot take any more)
          const int lo = std::max(std::max(lb[j], xp - std::min(k[j - 1], maxb)), B - sp - (H - 1 - j) * maxb);
          for (int xn = lo; xn <= maxb && sp + xn <= B; xn++) {
            const double nv = pv + cj * (double)xn;
            double &slot = nxt[at(xn, sp + xn)];
            if (nv > slot) slot = nv;
          }
        }
      cur.swap(nxt);
    }
    double best = none();
    for (int xl = 0; xl <= maxb; xl++) best = std::max(best, cur[at(xl, B)]);
    return best;
  }
};

// 0 and bits[H], *objective; 1 when no allocation satisfies the constraints.  Arguments checked by the caller:
// H >= 1, 0 <= lb_i <= max_bits, k_i >= 0, budget >= 0; every c_i finite.
inline int allocate_bits(const float *c, int H, const int *lb, int max_bits, const int *k, int budget, int *bits,
                         double *objective) {
  if (budget > (int64_t)H * max_bits) return 1;
  BitsDp dp{H, max_bits, budget, c, lb, k, {}, {}};
  // the optimum: over every first allocation
  double best = BitsDp::none();
  for (int x0 = lb[0]; x0 <= max_bits && x0 <= budget; x0++)
    best = std::max(best, dp.best_from(0, x0, x0, (double)c[0] * (double)x0));
  if (best == BitsDp::none()) return 1;
  int spent = 0, prev = 0;
  double v = 0.0;
  for (int i = 0; i < H; i++) {
    const int lo = i ? std::max(lb[i], prev - std::min(k[i - 1], max_bits)) : lb[0];
    int x = std::min(max_bits, budget - spent);
    for (; x >= lo; x--) {
      const double pv = i ? v + (double)c[i] * (double)x : (double)c[0] * (double)x;
      if (dp.best_from(i, x, spent + x, pv) == best) {
        v = pv;
        break;
      }
    }
    if (x < lo) return 1;  // (cannot happen: `best` was reached through this prefix)
    bits[i] = x;
    spent += x;
    prev = x;
  }
  if (objective) *objective = v;
  return 0;
}

}  // namespace train
}  // namespace vaq
#endif  // VAQ_TRAIN_PLAN_H_
