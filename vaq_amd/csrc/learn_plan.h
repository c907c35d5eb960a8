// learn_plan.h -- the host arithmetic of VAQ::learnQuantization (VAQ.cpp:1118-1187) that the host form
// (vaqhip_fast.cpp) and the device forms (vaqhip_learn.cpp, kernels in vaq_learn.hip) share: the percentile of
// utils/Math.hpp over an accessor, which order statistics it reads, the seven alphas, the floor / scale of one
// (alpha, column), the argmin over alphas, and how many subspaces' tables the device forms hold at a time.
// No HIP in here: tests/cpp/learn_plan_test.cpp runs it on the CPU.
// Everything is compiled with -ffp-contract=off: no expression below may fuse.
#ifndef VAQ_LEARN_PLAN_H_
#define VAQ_LEARN_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

// (loss_term is the one function the loss kernel runs too: under hipcc it is compiled for both sides)
#ifdef __HIPCC__
#define VAQ_LEARN_HD __host__ __device__
#else
#define VAQ_LEARN_HD
#endif

namespace vaq {
namespace learn {

constexpr int N_ALPHA = 7;
constexpr float ALPHAS[N_ALPHA] = {.001f, .002f, .005f, .01f, .02f, .05f, .1f};  // VAQ.cpp:1141

// utils/Math.hpp:190-213 on an ascending column: the value at rank percent * (rows - 1), as written (its `fraction`
// is taken against round(), not floor(), and may be negative).  v(i): element i of the sorted column.  Which elements
// are read depends on rows and percent only, never on a value.
template <class At> inline float percentile_at(At &&v, int64_t rows, float percent) {
  const float nthF = percent * static_cast<float>(rows - 1);
  if (std::fabs(std::round(nthF) - nthF) <= 0.00001f) return v(static_cast<int64_t>(nthF));
  const float f = v(static_cast<int64_t>(std::floor(nthF))), c = v(static_cast<int64_t>(std::ceil(nthF)));
  const float fraction = nthF - std::round(nthF);
  return f + (c - f) * fraction;
}

// the elements percentile_at reads for (rows, percent): idx[0 .. returned count), count 1 or 2, in reading order
inline int percentile_reads(int64_t rows, float percent, int64_t idx[2]) {
  int n = 0;
  (void)percentile_at([&](int64_t i) { if (n < 2) idx[n] = i; n++; return 0.0f; }, rows, percent);
  return std::min(n, 2);
}

// The order statistics one column's seven (floor, ceil) pairs need: per alpha two reads for percentile(alpha) and two
// for percentile(1 - alpha) (a percentile that reads one element repeats it).  Slots of one column:
// [alpha][floor 0, floor 1, ceil 0, ceil 1].
constexpr int STATS_PER_ALPHA = 4, STATS_PER_COLUMN = N_ALPHA * STATS_PER_ALPHA;
inline void stat_indices(int64_t rows, int64_t idx[STATS_PER_COLUMN]) {
  for (int a = 0; a < N_ALPHA; a++) {
    int64_t *p = idx + a * STATS_PER_ALPHA;
    if (percentile_reads(rows, ALPHAS[a], p) == 1) p[1] = p[0];
    if (percentile_reads(rows, 1.0f - ALPHAS[a], p + 2) == 1) p[3] = p[2];
  }
}

// fl = percentile(alpha) of the sorted column, ceil = percentile(1 - alpha) of max(sorted - fl, 0) -- monotone, so
// that column's order statistics are the sorted column's, shifted -- and sc = 255 / ceil (VAQ.cpp:1146-1160), from
// the fetched statistics of stat_indices (stats: this column's STATS_PER_COLUMN values).
inline void floor_scale_from_stats(const float *stats, int64_t rows, int a, float *fl_out, float *sc_out) {
  const float *s = stats + a * STATS_PER_ALPHA;
  int64_t fi[2] = {0, 0}, ci[2] = {0, 0};
  percentile_reads(rows, ALPHAS[a], fi);
  percentile_reads(rows, 1.0f - ALPHAS[a], ci);
  const float fl = percentile_at([&](int64_t i) { return i == fi[0] ? s[0] : s[1]; }, rows, ALPHAS[a]);
  const float ceil = percentile_at([&](int64_t i) { return std::max((i == ci[0] ? s[2] : s[3]) - fl, 0.0f); }, rows,
                                   1.0f - ALPHAS[a]);
  *fl_out = fl;
  *sc_out = 255.0f / ceil;
}

// One table value's share of the loss of (fl, sc), VAQ.cpp:1171-1176 as the host form (vaqhip_fast.cpp) evaluates it.
// Two things are spelt out so that host and device give the same bits where the host form leans on its platform:
//  - std::max(a, 0.0f) and std::min(a, 255.0f) are written as the ternaries <algorithm> defines them by, (a < b) ? b : a
//    and (b < a) ? b : a: a NaN first operand (0 * inf, when ceil = 0) comes through, which fmaxf / fminf would drop;
//  - (uint8_t)qv is undefined for a negative or NaN qv (a percentile may interpolate below zero and give a negative
//    scale).  The host form's x86 code truncates to an int and keeps the low byte (cvttss2si); that is written here as
//    (uint8_t)(int32_t)qv -- which the GPU's conversion, clamping to 0, would not give -- with NaN and values below
//    INT_MIN sent to the 0 that instruction's INT_MIN leaves.  tests/test_learn_device_gpu.py compares the two forms on
//    such columns (one sampled row, mixed code widths).
VAQ_LEARN_HD inline double loss_term(float x, float fl, float sc) {
  const float d = x - fl;
  const float off = (d < 0.0f) ? 0.0f : d;
  const float fq = std::floor(off * sc);
  const float qv = (255.0f < fq) ? 255.0f : fq;
  const int32_t qi = (qv >= -2147483648.0f) ? (int32_t)qv : 0;  // (false for NaN too)
  const float quant = (float)(uint8_t)qi;
  const float ideal = ((x - off) * sc) - quant;
  return (double)(ideal * ideal);
}

// the loss of one (alpha, column): the terms added one after another in table order (sample major, centroid minor)
template <class At> inline double loss_sequential(At &&x, int64_t rows, float fl, float sc) {
  double l = 0.0;
  for (int64_t i = 0; i < rows; i++) l += loss_term(x(i), fl, sc);
  return l;
}

// The alpha of least total loss: per alpha the columns' losses added for s = 0 .. M - 1 in order; `<=`, so a later
// alpha wins ties; -1 when no total is at most FLT_MAX.  loss: [N_ALPHA][M]; totals (optional): [N_ALPHA]
inline int best_alpha(const double *loss, int M, double *totals) {
  double best = (double)std::numeric_limits<float>::max();
  int best_a = -1;
  for (int a = 0; a < N_ALPHA; a++) {
    double l = 0.0;
    for (int s = 0; s < M; s++) l += loss[(size_t)a * M + s];
    if (totals) totals[a] = l;
    if (l <= best) {
      best = l;
      best_a = a;
    }
  }
  return best_a;
}

// ---- column groups ----
// The device forms hold the tables of Mc subspaces at a time, [sample][Mc][ksub] floats, beside one column's keys and
// sorted keys (2 * rows words, rows = sample * ksub) and the radix sort's scratch (taken as another 2 * rows words).
constexpr int64_t DEFAULT_WORKSPACE = (int64_t)1 << 30;

inline int64_t group_bytes(int64_t sample, int ksub, int Mc) { return sample * ksub * 4 * ((int64_t)Mc + 4); }

// the largest Mc in 1 .. M whose group fits `workspace` bytes (<= 0: the default); 1 when not even one does
inline int group_columns(int64_t workspace, int64_t sample, int M, int ksub) {
  if (workspace <= 0) workspace = DEFAULT_WORKSPACE;
  const int64_t col = sample * ksub * 4;
  const int64_t fit = workspace / col - 4;
  return (int)std::max<int64_t>(1, std::min<int64_t>(M, fit));
}

inline int group_count(int M, int Mc) { return (M + Mc - 1) / Mc; }
// group g holds subspaces [*s0, *s0 + *m)
inline void group_range(int M, int Mc, int g, int *s0, int *m) {
  *s0 = g * Mc;
  *m = std::min(Mc, M - *s0);
}

}  // namespace learn
}  // namespace vaq
#endif
