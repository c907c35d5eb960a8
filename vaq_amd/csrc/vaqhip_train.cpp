// vaqhip_train.cpp -- host side of the training front half of include/vaqhip.h: the second moment of the sampled rows
// (vaqhip_train_moment*), the symmetric eigen-solver (vaqhip_sym_eigen_device / _host), the plan and the exact bit
// allocation (vaqhip_train_plan, vaqhip_allocate_bits; train_plan.h) and their composite (vaqhip_train_rotation*).
// No index handle: eigvec and bits are what vaqhip_fit_codebooks and vaqhip_index_create take.
#include "vaqhip_index.h"

#include <chrono>
#include <cstring>
#include <vector>

#include "kmeans_sample.h"
#include "train_plan.h"
#include "vaq_train.h"

using namespace vaqhost;
namespace tr = vaq::train;

namespace {
thread_local vaqhip_train_timing g_tr_last = {};
thread_local float g_finish_ms = 0.0f;  // the host finish of the calling thread's last solve
constexpr size_t MOMENT_SCRATCH_BYTES = (size_t)256 << 20;

float ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// every refusal of the moment that needs no device
int check_moment(const void *X, int64_t n, int D, const void *out) {
  if (!X || !out) return fail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return fail(VAQHIP_EINVAL, "n=%lld: no row to sum", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(VAQHIP_EINVAL, "n=%lld: randomPermutation counts rows in an int", (long long)n);
  if (D < 1 || D > 4096) return fail(VAQHIP_EINVAL, "D=%d outside 1..4096", D);
  return VAQHIP_OK;
}

// ... and of the plan behind it
int check_plan(int D, int M, int bit_budget, int min_bits, int max_bits, float percent_var) {
  if (M < 1 || D % M != 0) return fail(VAQHIP_EINVAL, "D=%d is not M=%d subspaces of equal length", D, M);
  if (M > VAQHIP_MAX_SUBSPACES) return fail(VAQHIP_EINVAL, "M=%d > %d", M, VAQHIP_MAX_SUBSPACES);
  if (min_bits < 0 || min_bits > max_bits) return fail(VAQHIP_EINVAL, "min_bits=%d, max_bits=%d", min_bits, max_bits);
  if (max_bits > VAQHIP_MAX_BITS) return fail(VAQHIP_EINVAL, "max_bits=%d > %d", max_bits, VAQHIP_MAX_BITS);
  if (bit_budget < 0) return fail(VAQHIP_EINVAL, "bit_budget=%d", bit_budget);
  if (!(percent_var > 0.0f)) return fail(VAQHIP_EINVAL, "percent_var=%g is not positive", (double)percent_var);
  return VAQHIP_OK;
}

// d_X: the n rows on the current device (complete on st), or -- `compact` -- the sample itself in sample order.
// Enqueues; d_out / d_out_f are device pointers.  *s_out: the rows summed.
int moment_core(vaq::RowsRef d_X, int64_t n, int D, bool compact, double *d_out, float *d_out_f, DevBuf *b_part,
                DevBuf *b_rows, int64_t *s_out, hipStream_t st) {
  bool sampled;
  const int64_t s = tr::sample_rows(n, D, &sampled);
  const int *d_rows = nullptr;
  if (sampled && !compact) {
    const std::vector<int> rows = vaq::permutation_head(n, s);
    HIP_TRY(b_rows->ensure((size_t)s * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(b_rows->p, rows.data(), (size_t)s * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (`rows` leaves scope)
    d_rows = b_rows->as<int>();
  }
  const int64_t tiles = (s + tr::MOMENT_TILE - 1) / tr::MOMENT_TILE;
  const int chunk = vaq::moment_chunk_tiles(D, tiles, MOMENT_SCRATCH_BYTES);
  HIP_TRY(b_part->ensure((size_t)chunk * D * D * sizeof(double)));
  HIP_TRY(vaq::launch_train_moment(d_X, d_rows, s, D, b_part->as<double>(), chunk, d_out, d_out_f, st));
  *s_out = s;
  return VAQHIP_OK;
}

// the rows of a host form on the current device: the sample alone, in sample order, where the moment samples
int upload_rows(vaq::RowsRef X, int64_t n, int D, DevBuf *d_x) {
  bool sampled;
  const int64_t s = tr::sample_rows(n, D, &sampled);
  const size_t row_bytes = (size_t)D * (size_t)X.elem, bytes = (size_t)s * row_bytes;
  HIP_TRY(d_x->ensure(bytes));
  if (!sampled) {
    HIP_TRY(hipMemcpy(d_x->p, X.p, bytes, hipMemcpyHostToDevice));
    return VAQHIP_OK;
  }
  const std::vector<int> rows = vaq::permutation_head(n, s);
  std::vector<char> picked(bytes);
  for (int64_t i = 0; i < s; i++)
    std::memcpy(picked.data() + (size_t)i * row_bytes, static_cast<const char *>(X.p) + (size_t)rows[(size_t)i] * row_bytes, row_bytes);
  HIP_TRY(hipMemcpy(d_x->p, picked.data(), bytes, hipMemcpyHostToDevice));
  return VAQHIP_OK;
}

// the solver on the current device; d_A is destroyed.  The outputs are device pointers; hv / hvec (may be null)
// receive the same on the host.
int eigen_core(double *d_A, int D, double *d_values, double *d_vectors, int *sweeps_out, double *hv, double *hvec,
               hipStream_t st) {
  const size_t nn = (size_t)D * D;
  const int steps = tr::jacobi_steps(D), slots = tr::jacobi_slots(D);
  DevBuf b_V, b_rot, b_small;
  HIP_TRY(b_V.ensure(nn * sizeof(double)));
  HIP_TRY(b_rot.ensure((size_t)slots * sizeof(tr::Rot)));
  HIP_TRY(b_small.ensure((size_t)(tr::JACOBI_MAX_SWEEPS + 1) * sizeof(int)));
  int *d_bad = b_small.as<int>(), *d_count = d_bad + 1;
  HIP_TRY(hipMemsetAsync(b_small.p, 0, (size_t)(tr::JACOBI_MAX_SWEEPS + 1) * sizeof(int), st));
  HIP_TRY(vaq::launch_train_finite(d_A, (int64_t)nn, d_bad, st));
  HIP_TRY(vaq::launch_train_identity(b_V.as<double>(), D, st));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (sweeps_out) *sweeps_out = 0;
  if (bad) return fail(VAQHIP_EINVAL, "the matrix holds a NaN or an infinite value");
  std::vector<double> A0(nn);  // the matrix as it came: jacobi_finish takes the eigenvalues from it
  HIP_TRY(hipMemcpyAsync(A0.data(), d_A, nn * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int sweeps = 0, status = VAQHIP_OK;
  for (;;) {
    if (sweeps == tr::JACOBI_MAX_SWEEPS) {
      status = VAQHIP_ENOCONV;
      break;
    }
    for (int r = 0; r < steps; r++)
      HIP_TRY(vaq::launch_train_jacobi_step(d_A, b_V.as<double>(), D, r, b_rot.as<tr::Rot>(), d_count + sweeps, st));
    int rotated = 0;
    if (steps) {
      HIP_TRY(hipMemcpyAsync(&rotated, d_count + sweeps, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (!rotated) break;
    sweeps++;
  }
  std::vector<double> V(nn), values((size_t)D), vectors(nn);
  HIP_TRY(hipMemcpyAsync(V.data(), b_V.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const auto tf = std::chrono::steady_clock::now();
  tr::jacobi_finish(A0.data(), V.data(), D, values.data(), vectors.data());
  g_finish_ms = ms_since(tf);
  if (d_values) HIP_TRY(hipMemcpyAsync(d_values, values.data(), (size_t)D * sizeof(double), hipMemcpyHostToDevice, st));
  if (d_vectors) HIP_TRY(hipMemcpyAsync(d_vectors, vectors.data(), nn * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (hv) std::memcpy(hv, values.data(), (size_t)D * sizeof(double));
  if (hvec) std::memcpy(hvec, vectors.data(), nn * sizeof(double));
  if (sweeps_out) *sweeps_out = sweeps;
  if (status) return fail(status, "the Jacobi sweeps still rotated after %d sweeps", tr::JACOBI_MAX_SWEEPS);
  return VAQHIP_OK;
}

// the plan's refusals in words
int plan_or_fail(const float *eig, int D, int M, float percent_var, int min_bits, tr::Plan *pl) {
  const int rc = tr::make_plan(eig, D, M, percent_var, min_bits, pl);
  if (rc == 1) return fail(VAQHIP_EINVAL, "an eigenvalue is not finite");
  if (rc == 2) return fail(VAQHIP_EINVAL, "the eigenvalues do not sum to a positive value");
  return VAQHIP_OK;
}

int allocate_or_fail(const float *c, int H, const int *lb, int max_bits, const int *k, int budget, int *bits, double *obj) {
  if (tr::allocate_bits(c, H, lb, max_bits, k, budget, bits, obj))
    return fail(VAQHIP_EINVAL, "no allocation of %d bits over %d subspaces satisfies the constraints (the reference asserts)",
                budget, H);
  return VAQHIP_OK;
}

struct RotationOut {
  float *eigvec;       // D x D, host, or a device pointer with eigvec_device
  bool eigvec_device;
  float *eigenvalues;  // host [D]
  int *bits, *highest;  // host [M], host
};

// moment -> eigen -> plan -> allocation over rows on the current device
int rotation_core(vaq::RowsRef d_X, int64_t n, int D, bool compact, int M, int budget, int min_bits, int max_bits,
                  float percent_var, const RotationOut &o, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nn = (size_t)D * D;
  DevBuf b_cov, b_part, b_rows;
  HIP_TRY(b_cov.ensure(nn * sizeof(double)));
  int64_t s = 0;
  if (int rc = moment_core(d_X, n, D, compact, b_cov.as<double>(), nullptr, &b_part, &b_rows, &s, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  const float moment_ms = ms_since(t0);
  b_part.release();
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<double> values((size_t)D), vectors(nn);
  int sweeps = 0;
  if (int rc = eigen_core(b_cov.as<double>(), D, nullptr, nullptr, &sweeps, values.data(), vectors.data(), st)) return rc;
  const float eigen_ms = ms_since(t1);
  const auto t2 = std::chrono::steady_clock::now();
  std::vector<float> eig((size_t)D);
  for (int i = 0; i < D; i++) eig[(size_t)i] = (float)values[(size_t)i];
  tr::Plan pl;
  if (int rc = plan_or_fail(eig.data(), D, M, percent_var, min_bits, &pl)) return rc;
  std::vector<int> bits((size_t)pl.highest);
  if (int rc = allocate_or_fail(pl.var.data(), pl.highest, pl.lb.data(), max_bits, pl.k.data(), budget, bits.data(), nullptr))
    return rc;
  std::vector<float> ev(nn);
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) ev[(size_t)i * D + j] = (float)vectors[(size_t)i * D + pl.order[(size_t)j]];
  if (o.eigvec_device) {
    HIP_TRY(hipMemcpyAsync(o.eigvec, ev.data(), nn * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  } else {
    std::memcpy(o.eigvec, ev.data(), nn * sizeof(float));
  }
  if (o.eigenvalues)
    for (int j = 0; j < D; j++) o.eigenvalues[j] = eig[(size_t)pl.order[(size_t)j]];
  for (int i = 0; i < M; i++) o.bits[i] = i < pl.highest ? bits[(size_t)i] : 0;
  *o.highest = pl.highest;
  g_tr_last = vaqhip_train_timing{};
  g_tr_last.moment_ms = moment_ms;
  g_tr_last.eigen_ms = eigen_ms;
  g_tr_last.finish_ms = g_finish_ms;
  g_tr_last.plan_ms = ms_since(t2);
  g_tr_last.total_ms = ms_since(t0);
  g_tr_last.sweeps = sweeps;
  g_tr_last.subspaces = M;
  g_tr_last.dims = D;
  g_tr_last.sample_rows = s;
  g_tr_last.rows = n;
  return VAQHIP_OK;
}

int check_rotation(const void *X, int64_t n, int D, int M, int budget, int min_bits, int max_bits, float percent_var,
                   const RotationOut &o) {
  if (!o.bits || !o.highest) return fail(VAQHIP_EINVAL, "null pointer");
  if (int rc = check_moment(X, n, D, o.eigvec)) return rc;
  return check_plan(D, M, budget, min_bits, max_bits, percent_var);
}

int moment_host_entry(int device, vaq::RowsRef X, int64_t n, int D, double *cov_out, float *cov_f_out) {
  if (int rc = check_moment(X.p, n, D, cov_out)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  const size_t nn = (size_t)D * D;
  DevBuf d_x, b_cov, b_cov_f, b_part, b_rows;
  if (int rc = upload_rows(X, n, D, &d_x)) return rc;
  HIP_TRY(b_cov.ensure(nn * sizeof(double)));
  if (cov_f_out) HIP_TRY(b_cov_f.ensure(nn * sizeof(float)));
  CallStream st;
  HIP_TRY(st.open());
  int64_t s = 0;
  if (int rc = moment_core(vaq::RowsRef{d_x.p, X.elem}, n, D, true, b_cov.as<double>(), cov_f_out ? b_cov_f.as<float>() : nullptr,
                           &b_part, &b_rows, &s, st.s))
    return rc;
  HIP_TRY(hipMemcpyAsync(cov_out, b_cov.p, nn * sizeof(double), hipMemcpyDeviceToHost, st.s));
  if (cov_f_out) HIP_TRY(hipMemcpyAsync(cov_f_out, b_cov_f.p, nn * sizeof(float), hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipStreamSynchronize(st.s));
  return VAQHIP_OK;
}

int moment_device_entry(int device, vaq::RowsRef d_X, int64_t n, int D, double *d_cov_out, float *d_cov_f_out, void *stream) {
  if (int rc = check_moment(d_X.p, n, D, d_cov_out)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DevBuf b_part, b_rows;
  int64_t s = 0;
  if (int rc = moment_core(d_X, n, D, false, d_cov_out, d_cov_f_out, &b_part, &b_rows, &s, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // (the scratch leaves scope)
  return VAQHIP_OK;
}

int rotation_host_entry(int device, vaq::RowsRef X, int64_t n, int D, int M, int budget, int min_bits, int max_bits,
                        float percent_var, const RotationOut &o) {
  if (int rc = check_rotation(X.p, n, D, M, budget, min_bits, max_bits, percent_var, o)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  DevBuf d_x;
  if (int rc = upload_rows(X, n, D, &d_x)) return rc;
  CallStream st;
  HIP_TRY(st.open());
  return rotation_core(vaq::RowsRef{d_x.p, X.elem}, n, D, true, M, budget, min_bits, max_bits, percent_var, o, st.s);
}

int rotation_device_entry(int device, vaq::RowsRef d_X, int64_t n, int D, int M, int budget, int min_bits, int max_bits,
                          float percent_var, const RotationOut &o, void *stream) {
  if (int rc = check_rotation(d_X.p, n, D, M, budget, min_bits, max_bits, percent_var, o)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  return rotation_core(d_X, n, D, false, M, budget, min_bits, max_bits, percent_var, o, static_cast<hipStream_t>(stream));
}
}  // namespace

// vaqhip_refiner.cpp calls these over its resident rows (n x D on `device`, complete), its lock held
int vaqhost::train_moment_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, double *cov_out, float *cov_f_out) {
  if (int rc = check_moment(d_X.p, n, D, cov_out)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  const size_t nn = (size_t)D * D;
  DevBuf b_cov, b_cov_f, b_part, b_rows;
  HIP_TRY(b_cov.ensure(nn * sizeof(double)));
  if (cov_f_out) HIP_TRY(b_cov_f.ensure(nn * sizeof(float)));
  CallStream st;
  HIP_TRY(st.open());
  int64_t s = 0;
  if (int rc = moment_core(d_X, n, D, false, b_cov.as<double>(), cov_f_out ? b_cov_f.as<float>() : nullptr, &b_part, &b_rows,
                           &s, st.s))
    return rc;
  HIP_TRY(hipMemcpyAsync(cov_out, b_cov.p, nn * sizeof(double), hipMemcpyDeviceToHost, st.s));
  if (cov_f_out) HIP_TRY(hipMemcpyAsync(cov_f_out, b_cov_f.p, nn * sizeof(float), hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipStreamSynchronize(st.s));
  return VAQHIP_OK;
}

int vaqhost::train_rotation_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, int bit_budget, int min_bits,
                                        int max_bits, float percent_var, float *eigvec_out, float *eigenvalues_out,
                                        int *bits_out, int *highest_subs_out) {
  const RotationOut o{eigvec_out, false, eigenvalues_out, bits_out, highest_subs_out};
  if (int rc = check_rotation(d_X.p, n, D, M, bit_budget, min_bits, max_bits, percent_var, o)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  CallStream st;
  HIP_TRY(st.open());
  return rotation_core(d_X, n, D, false, M, bit_budget, min_bits, max_bits, percent_var, o, st.s);
}

extern "C" {

int vaqhip_train_moment(int device_id, const float *X, int64_t n, int D, double *cov_out, float *cov_f_out) {
  return moment_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, cov_out, cov_f_out);
}
int vaqhip_train_moment_u8(int device_id, const uint8_t *X, int64_t n, int D, double *cov_out, float *cov_f_out) {
  return moment_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, cov_out, cov_f_out);
}
int vaqhip_train_moment_device(int device_id, const float *d_X, int64_t n, int D, double *d_cov_out, float *d_cov_f_out,
                               void *stream) {
  return moment_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, d_cov_out, d_cov_f_out, stream);
}
int vaqhip_train_moment_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, double *d_cov_out,
                                  float *d_cov_f_out, void *stream) {
  return moment_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, d_cov_out, d_cov_f_out, stream);
}

int vaqhip_sym_eigen_device(int device_id, double *d_A, int D, double *d_values, double *d_vectors, int *sweeps_out,
                            void *stream) {
  if (!d_A || !d_values || !d_vectors) return fail(VAQHIP_EINVAL, "null pointer");
  if (D < 1 || D > 4096) return fail(VAQHIP_EINVAL, "D=%d outside 1..4096", D);
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return eigen_core(d_A, D, d_values, d_vectors, sweeps_out, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int vaqhip_sym_eigen_host(double *A, int D, double *values, double *vectors, int *sweeps_out) {
  if (!A || !values || !vectors) return fail(VAQHIP_EINVAL, "null pointer");
  if (D < 1 || D > 4096) return fail(VAQHIP_EINVAL, "D=%d outside 1..4096", D);
  const int rc = tr::sym_eigen_host(A, D, values, vectors, sweeps_out);
  if (rc == 1) return fail(VAQHIP_EINVAL, "the matrix holds a NaN or an infinite value");
  if (rc == 2) return fail(VAQHIP_ENOCONV, "the Jacobi sweeps still rotated after %d sweeps", tr::JACOBI_MAX_SWEEPS);
  return VAQHIP_OK;
}

int vaqhip_train_plan(const float *eigenvalues, int D, int M, float percent_var, int min_bits, int max_bits,
                      int *sorted_out, int *order_out, float *var_out, float *cum_out, int *highest_subs_out, int *lb_out,
                      int *k_out, int *swaps_kept_out) {
  if (!eigenvalues || !order_out || !var_out || !cum_out || !highest_subs_out || !lb_out || !k_out)
    return fail(VAQHIP_EINVAL, "null pointer");
  if (D < 1 || D > 4096) return fail(VAQHIP_EINVAL, "D=%d outside 1..4096", D);
  if (int rc = check_plan(D, M, 0, min_bits, max_bits, percent_var)) return rc;
  tr::Plan pl;
  if (int rc = plan_or_fail(eigenvalues, D, M, percent_var, min_bits, &pl)) return rc;
  if (sorted_out) std::copy(pl.sorted.begin(), pl.sorted.end(), sorted_out);
  std::copy(pl.order.begin(), pl.order.end(), order_out);
  std::copy(pl.var.begin(), pl.var.end(), var_out);
  std::copy(pl.cum.begin(), pl.cum.end(), cum_out);
  *highest_subs_out = pl.highest;
  std::copy(pl.lb.begin(), pl.lb.end(), lb_out);
  std::copy(pl.k.begin(), pl.k.end(), k_out);
  if (swaps_kept_out) *swaps_kept_out = pl.swaps_kept;
  return VAQHIP_OK;
}

int vaqhip_allocate_bits(const float *c, int H, const int *lb, int max_bits, const int *k, int budget, int *bits_out,
                         double *objective_out) {
  if (!c || !lb || !bits_out || (H > 1 && !k)) return fail(VAQHIP_EINVAL, "null pointer");
  if (H < 1 || H > VAQHIP_MAX_SUBSPACES) return fail(VAQHIP_EINVAL, "H=%d outside 1..%d", H, VAQHIP_MAX_SUBSPACES);
  if (max_bits < 0 || max_bits > VAQHIP_MAX_BITS) return fail(VAQHIP_EINVAL, "max_bits=%d outside 0..%d", max_bits, VAQHIP_MAX_BITS);
  if (budget < 0) return fail(VAQHIP_EINVAL, "budget=%d", budget);
  for (int i = 0; i < H; i++) {
    if (!std::isfinite(c[i])) return fail(VAQHIP_EINVAL, "c[%d] is not finite", i);
    if (lb[i] < 0 || lb[i] > max_bits) return fail(VAQHIP_EINVAL, "lb[%d]=%d outside 0..max_bits=%d", i, lb[i], max_bits);
    if (i + 1 < H && k[i] < 0) return fail(VAQHIP_EINVAL, "k[%d]=%d", i, k[i]);
  }
  return allocate_or_fail(c, H, lb, max_bits, k, budget, bits_out, objective_out);
}

int vaqhip_train_rotation(int device_id, const float *X, int64_t n, int D, int M, int bit_budget, int min_bits, int max_bits,
                          float percent_var, float *eigvec_out, float *eigenvalues_out, int *bits_out,
                          int *highest_subs_out) {
  return rotation_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, M, bit_budget, min_bits, max_bits, percent_var,
                             RotationOut{eigvec_out, false, eigenvalues_out, bits_out, highest_subs_out});
}
int vaqhip_train_rotation_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, int bit_budget, int min_bits,
                             int max_bits, float percent_var, float *eigvec_out, float *eigenvalues_out, int *bits_out,
                             int *highest_subs_out) {
  return rotation_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, M, bit_budget, min_bits, max_bits, percent_var,
                             RotationOut{eigvec_out, false, eigenvalues_out, bits_out, highest_subs_out});
}
int vaqhip_train_rotation_device(int device_id, const float *d_X, int64_t n, int D, int M, int bit_budget, int min_bits,
                                 int max_bits, float percent_var, float *d_eigvec_out, float *eigenvalues_out,
                                 int *bits_out, int *highest_subs_out, void *stream) {
  return rotation_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, M, bit_budget, min_bits, max_bits, percent_var,
                               RotationOut{d_eigvec_out, true, eigenvalues_out, bits_out, highest_subs_out}, stream);
}
int vaqhip_train_rotation_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, int bit_budget,
                                    int min_bits, int max_bits, float percent_var, float *d_eigvec_out,
                                    float *eigenvalues_out, int *bits_out, int *highest_subs_out, void *stream) {
  return rotation_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, M, bit_budget, min_bits, max_bits, percent_var,
                               RotationOut{d_eigvec_out, true, eigenvalues_out, bits_out, highest_subs_out}, stream);
}

int vaqhip_last_train_timing(vaqhip_train_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_tr_last;
  return VAQHIP_OK;
}

}  // extern "C"
