// vaq_train_rot.h -- the symmetric eigen-solver of the training front half (vaqhip_sym_eigen_device /
// vaqhip_sym_eigen_host): a cyclic two-sided Jacobi in double.  What the device kernels (vaq_train.hip) and the host
// function share lives here: the rotation of one pair, the round-robin ordering, and the ordering and signs of the
// result.  The host solver below is the same algorithm step for step, so the CPU tests exercise all of it.
//   step      the pairs of one round of a chess tournament over D (odd D: D + 1, one bye) players: disjoint.  Every
//             pair's rotation is taken from ITS OWN a_pp, a_qq, a_pq as the step finds them; then every pair updates its
//             two columns of A and V (rows ascending), then every pair updates its two rows of A, and a_pq = a_qp = 0.
//   sweep     D - 1 (odd D: D) steps: every pair once.  Stop after the first sweep without a rotation, or at 60.
//   result    every vector normalised, its eigenvalue its Rayleigh quotient on the matrix as it came (jacobi_finish, on
//             the host in both forms); eigenvalues descending, equal ones by ascending column; each vector's largest
//             |component| positive (the first such on ties).
// Plain double multiply, add, divide and sqrt, no fused operation (-ffp-contract=off everywhere it is compiled).
#ifndef VAQ_TRAIN_ROT_H_
#define VAQ_TRAIN_ROT_H_

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vaq {
namespace train {

constexpr int JACOBI_MAX_SWEEPS = 60;

struct Rot {
  double c, s;
  int apply;  // 0: the pair is left alone (c = 1, s = 0)
};

// A pair is rotated when |a_pq| > 2^-52 * sqrt(|a_pp * a_qq|) (a zero product: when a_pq != 0).  theta = (a_qq - a_pp) /
// (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t * c.
__host__ __device__ inline Rot jacobi_rot(double app, double aqq, double apq) {
  Rot r{1.0, 0.0, 0};
  const double prod = fabs(app * aqq);
  const bool rotate = prod == 0.0 ? apq != 0.0 : fabs(apq) > 0x1p-52 * sqrt(prod);
  if (!rotate) return r;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  r.c = 1.0 / sqrt(t * t + 1.0);
  r.s = t * r.c;
  r.apply = 1;
  return r;
}

// players of the tournament, steps of a sweep, pairs of a step (a pair with the bye is no pair)
__host__ __device__ inline int jacobi_players(int D) { return D + (D & 1); }
__host__ __device__ inline int jacobi_steps(int D) { return D < 2 ? 0 : jacobi_players(D) - 1; }
__host__ __device__ inline int jacobi_slots(int D) { return jacobi_players(D) / 2; }

// slot i of step r: the last player stays, the others turn.  Returns 0 for the bye's slot, else p < q.
__host__ __device__ inline int jacobi_pair(int D, int r, int i, int *p, int *q) {
  const int n = jacobi_players(D), m = n - 1;
  int a, b;
  if (i == 0) {
    a = m;
    b = r % m;
  } else {
    a = (r + i) % m;
    b = (r - i + m) % m;
  }
  if (a >= D || b >= D) return 0;
  *p = a < b ? a : b;
  *q = a < b ? b : a;
  return 1;
}

// the two halves of a pair's update on one element pair: (x, y) -> (c x - s y, s x + c y)
__host__ __device__ inline void jacobi_apply(const Rot &r, double *x, double *y) {
  const double a = *x, b = *y;
  *x = r.c * a - r.s * b;
  *y = r.s * a + r.c * b;
}

// A0 (the matrix as it came, D x D row-major) and V (vectors in columns) as the sweeps left them -> values[D]
// descending, vectors[D x D].  A column of V is a product of some hundreds of rotations whose c^2 + s^2 is 1 only up to
// rounding, so its norm drifts, and the diagonal the sweeps leave has taken a rounding per rotation: each vector is
// divided by its norm (squares added in ascending row from +0), and its eigenvalue is its Rayleigh quotient on A0,
// v^T (A0 v), both sums in ascending index from +0.
inline void jacobi_finish(const double *A0, const double *V, int D, double *values, double *vectors) {
  const size_t nn = (size_t)D * D;
  std::vector<double> Vn(nn), W(nn, 0.0), nrm((size_t)D, 0.0), lam((size_t)D, 0.0);
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) nrm[(size_t)j] = nrm[(size_t)j] + V[(size_t)i * D + j] * V[(size_t)i * D + j];
  for (int j = 0; j < D; j++) nrm[(size_t)j] = nrm[(size_t)j] > 0.0 ? sqrt(nrm[(size_t)j]) : 1.0;
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) Vn[(size_t)i * D + j] = V[(size_t)i * D + j] / nrm[(size_t)j];
  for (int i = 0; i < D; i++)
    for (int k = 0; k < D; k++) {
      const double a = A0[(size_t)i * D + k];
      for (int j = 0; j < D; j++) W[(size_t)i * D + j] = W[(size_t)i * D + j] + a * Vn[(size_t)k * D + j];
    }
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) lam[(size_t)j] = lam[(size_t)j] + Vn[(size_t)i * D + j] * W[(size_t)i * D + j];
  std::vector<int> order((size_t)D);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lam[(size_t)a] > lam[(size_t)b]; });
  for (int j = 0; j < D; j++) {
    const int src = order[(size_t)j];
    values[j] = lam[(size_t)src];
    int big = 0;
    for (int i = 1; i < D; i++)
      if (fabs(Vn[(size_t)i * D + src]) > fabs(Vn[(size_t)big * D + src])) big = i;
    const bool flip = Vn[(size_t)big * D + src] < 0.0;
    for (int i = 0; i < D; i++) vectors[(size_t)i * D + j] = flip ? -Vn[(size_t)i * D + src] : Vn[(size_t)i * D + src];
  }
}

inline bool all_finite(const double *A, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(A[i])) return false;
  return true;
}

// The solver on the host.  A (D x D row-major) is destroyed.  Returns 0, 1 when a value of A is not finite (nothing
// done), 2 when sweep 60 still rotated (the outputs hold what it reached).
inline int sym_eigen_host(double *A, int D, double *values, double *vectors, int *sweeps_out) {
  if (sweeps_out) *sweeps_out = 0;
  if (!all_finite(A, (size_t)D * D)) return 1;
  std::vector<double> V((size_t)D * D, 0.0);
  const std::vector<double> A0(A, A + (size_t)D * D);
  for (int i = 0; i < D; i++) V[(size_t)i * D + i] = 1.0;
  const int steps = jacobi_steps(D), slots = jacobi_slots(D);
  std::vector<Rot> rot((size_t)std::max(slots, 1));
  int sweeps = 0, status = 0;
  for (;;) {
    if (sweeps == JACOBI_MAX_SWEEPS) {
      status = 2;
      break;
    }
    long rotated = 0;
    for (int r = 0; r < steps; r++) {
      int p, q;
      for (int i = 0; i < slots; i++) {
        rot[(size_t)i] = Rot{1.0, 0.0, 0};
        if (jacobi_pair(D, r, i, &p, &q)) rot[(size_t)i] = jacobi_rot(A[(size_t)p * D + p], A[(size_t)q * D + q], A[(size_t)p * D + q]);
        rotated += rot[(size_t)i].apply;
      }
      for (int i = 0; i < slots; i++) {
        if (!rot[(size_t)i].apply || !jacobi_pair(D, r, i, &p, &q)) continue;
        for (int k = 0; k < D; k++) {
          jacobi_apply(rot[(size_t)i], &A[(size_t)k * D + p], &A[(size_t)k * D + q]);
          jacobi_apply(rot[(size_t)i], &V[(size_t)k * D + p], &V[(size_t)k * D + q]);
        }
      }
      for (int i = 0; i < slots; i++) {
        if (!rot[(size_t)i].apply || !jacobi_pair(D, r, i, &p, &q)) continue;
        for (int k = 0; k < D; k++) jacobi_apply(rot[(size_t)i], &A[(size_t)p * D + k], &A[(size_t)q * D + k]);
        A[(size_t)p * D + q] = 0.0;
        A[(size_t)q * D + p] = 0.0;
      }
    }
    if (!rotated) break;  // (a sweep without a rotation is not counted: `sweeps` are those that rotated)
    sweeps++;
  }
  jacobi_finish(A0.data(), V.data(), D, values, vectors);
  if (sweeps_out) *sweeps_out = sweeps;
  return status;
}

}  // namespace train
}  // namespace vaq
#endif  // VAQ_TRAIN_ROT_H_
