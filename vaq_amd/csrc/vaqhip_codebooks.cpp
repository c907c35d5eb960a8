// vaqhip_codebooks.cpp -- host side of the subspace codebook fit of include/vaqhip.h (vaqhip_fit_codebooks*): the
// argument checks, the copies around vaq::codebooks_fit (vaq_codebooks.hip) and the calling thread's timing.  No
// index handle: the centres are what vaqhip_index_create takes.  The plan is fit_codebooks_plan.h's.
#include "vaqhip_index.h"

#include <chrono>
#include <cstring>
#include <vector>

#include "fit_codebooks_plan.h"
#include "kmeans_sample.h"

using namespace vaqhost;
namespace cb = vaq::cbfit;

namespace {
thread_local int g_cb_timing = 0;
thread_local vaqhip_fit_codebooks_timing g_cb_last = {};

// every refusal that needs no device, in the order the header lists them; fills the plan when there is none
int check_args(const void *X, int64_t n, int D, int M, const int *bits, int max_iter, const void *cent, cb::Plan *plan) {
  if (!X || !bits || !cent) return fail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return fail(VAQHIP_EINVAL, "n=%lld: no row to seed a centre from", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(VAQHIP_EINVAL, "n=%lld: randomPermutation counts rows in an int", (long long)n);
  if (D < 1 || M < 1 || D % M != 0) return fail(VAQHIP_EINVAL, "D=%d is not M=%d subspaces of equal length", D, M);
  if (max_iter < 1) return fail(VAQHIP_EINVAL, "max_iter=%d", max_iter);
  if (M > VAQHIP_MAX_SUBSPACES) return fail(VAQHIP_EUNSUPPORTED, "M=%d > %d", M, VAQHIP_MAX_SUBSPACES);
  if (D > 4096) return fail(VAQHIP_EUNSUPPORTED, "D=%d > 4096", D);
  for (int s = 0; s < M; s++) {
    if (bits[s] < 1 || bits[s] > VAQHIP_MAX_BITS)
      return fail(VAQHIP_EINVAL, "bits[%d]=%d outside 1..%d", s, bits[s], VAQHIP_MAX_BITS);
    if (((int64_t)1 << bits[s]) > cb::sample_rows(n, 1 << bits[s]))
      return fail(VAQHIP_EINVAL, "bits[%d]=%d: %d centres from %lld rows (the reference seeds from rows out of bounds)", s,
                  bits[s], 1 << bits[s], (long long)n);
  }
  // (at most VAQHIP_MAX_SUBSPACES * 256 << VAQHIP_MAX_BITS = 2^30 sampled rows over all subspaces: the runs fit an int)
  *plan = cb::make_plan(n, M, bits);
  return VAQHIP_OK;
}

// device pointers throughout (bits, iters_out, nan_rows_out: host), the device current; the outputs are written only
// when the fit succeeds
int fit_core(vaq::RowsRef d_X, int64_t n, int D, const cb::Plan &plan, const float *d_eig, int max_iter,
             float *d_cent_out, int *iters_out, int *nan_rows_out, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const int M = (int)plan.sub.size(), L = D / M;
  const size_t cent_floats = (size_t)plan.n_cent * L;
  DevBuf b_means;
  HIP_TRY(b_means.ensure(cent_floats * sizeof(float)));
  std::vector<int> iters((size_t)M, 0);
  int no_centre = 0;
  vaq::CodebookPhases ph;
  HIP_TRY(vaq::codebooks_fit(d_X, n, D, L, plan, d_eig, max_iter, b_means.as<float>(), iters.data(), &no_centre,
                             g_cb_timing ? &ph : nullptr, st));  // synchronises
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  std::vector<float> means(cent_floats);
  HIP_TRY(hipMemcpyAsync(means.data(), b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  int max_iters = 0;
  for (int s = 0; s < M; s++) {
    const cb::Sub &sd = plan.sub[(size_t)s];
    if (iters_out) iters_out[s] = iters[(size_t)s];
    if (nan_rows_out) nan_rows_out[s] = vaq::nan_rows(means.data() + (size_t)sd.cent_off * L, sd.k, L);
    max_iters = std::max(max_iters, iters[(size_t)s]);
  }
  g_cb_last = vaqhip_fit_codebooks_timing{};
  g_cb_last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_cb_last.gather_ms = (float)ph.gather_ms;
  g_cb_last.assign_ms = (float)ph.assign_ms;
  g_cb_last.accumulate_ms = (float)ph.accumulate_ms;
  g_cb_last.update_ms = (float)ph.update_ms;
  g_cb_last.iterations = max_iters;
  g_cb_last.sample_rows = plan.sample;
  g_cb_last.rows = n;
  g_cb_last.dims = D;
  g_cb_last.subspaces = M;
  return VAQHIP_OK;
}

int fit_device_entry(int device_id, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits, const float *d_eigvec,
                     int max_iter, float *d_centroids_out, int *iters_out, int *nan_rows_out, void *stream) {
  cb::Plan plan;
  if (int rc = check_args(d_X.p, n, D, M, bits, max_iter, d_centroids_out, &plan)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return fit_core(d_X, n, D, plan, d_eigvec, max_iter, d_centroids_out, iters_out, nan_rows_out,
                  static_cast<hipStream_t>(stream));
}

// the rest of a host-output call once the rows are on the device (current): eigvec up, fit, centres down
int fit_to_host(vaq::RowsRef d_X, int64_t n, int D, const cb::Plan &plan, const float *eigvec, int max_iter,
                float *centroids_out, int *iters_out, int *nan_rows_out) {
  DevBuf d_eig, d_cent;
  const size_t cent_bytes = (size_t)plan.n_cent * (D / (int)plan.sub.size()) * sizeof(float);
  HIP_TRY(d_cent.ensure(cent_bytes));
  if (eigvec) {
    HIP_TRY(d_eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(d_eig.p, eigvec, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
  }
  CallStream st;
  HIP_TRY(st.open());
  if (int rc = fit_core(d_X, n, D, plan, eigvec ? d_eig.as<float>() : nullptr, max_iter, d_cent.as<float>(), iters_out,
                        nan_rows_out, st.s))
    return rc;
  HIP_TRY(hipMemcpy(centroids_out, d_cent.p, cent_bytes, hipMemcpyDeviceToHost));
  return VAQHIP_OK;
}

// X: host rows of X.elem bytes per element, uploaded as they are.  Where every subspace samples, only the sample goes
// up: its rows are copied out in the sample's order here, and the device is handed the sample itself.  Where one
// subspace reads all rows, all rows go up, and the device gathers the sample of the others.
int fit_host_entry(int device_id, vaq::RowsRef X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                   int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  cb::Plan plan;
  if (int rc = check_args(X.p, n, D, M, bits, max_iter, centroids_out, &plan)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  DevBuf d_x;
  const size_t row_bytes = (size_t)D * (size_t)X.elem, x_bytes = (size_t)(plan.sampled ? plan.sample : n) * row_bytes;
  HIP_TRY(d_x.ensure(x_bytes));
  if (plan.sampled) {
    const std::vector<int> rows = vaq::permutation_head(n, plan.sample);
    std::vector<char> picked(x_bytes);
    for (int64_t i = 0; i < plan.sample; i++)
      std::memcpy(picked.data() + (size_t)i * row_bytes, static_cast<const char *>(X.p) + (size_t)rows[(size_t)i] * row_bytes, row_bytes);
    HIP_TRY(hipMemcpy(d_x.p, picked.data(), x_bytes, hipMemcpyHostToDevice));
    plan.gather = false;
  } else {
    HIP_TRY(hipMemcpy(d_x.p, X.p, x_bytes, hipMemcpyHostToDevice));
  }
  return fit_to_host(vaq::RowsRef{d_x.p, X.elem}, n, D, plan, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
}  // namespace

// vaqhip_refiner.cpp calls this over its resident rows (n x D on `device`, complete), its lock held
int vaqhost::fit_codebooks_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                                       const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                       int *nan_rows_out) {
  cb::Plan plan;
  if (int rc = check_args(d_X.p, n, D, M, bits, max_iter, centroids_out, &plan)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  return fit_to_host(d_X, n, D, plan, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

extern "C" {

int vaqhip_fit_codebooks(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                         int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                            int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_fit_codebooks_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                   const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                   int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}

// ---- vaqhip_internal.h: what the sharded fit takes from here ----
int vaqhip_internal_fit_codebooks_check(const void *X, int64_t n, int D, int M, const int *bits, int max_iter,
                                        const void *centroids_out) {
  cb::Plan plan;
  return check_args(X, n, D, M, bits, max_iter, centroids_out, &plan);
}
int vaqhip_internal_fit_codebooks_rows_device(int device, const void *d_X, int elem, int64_t n, int D, int M,
                                              const int *bits, const float *eigvec, int max_iter, float *centroids_out,
                                              int *iters_out, int *nan_rows_out) {
  return fit_codebooks_rows_device(device, vaq::RowsRef{d_X, elem}, n, D, M, bits, eigvec, max_iter, centroids_out,
                                   iters_out, nan_rows_out);
}
int vaqhip_internal_fit_codebooks_timing_on(void) { return g_cb_timing; }

int vaqhip_fit_codebooks_set_timing(int on) {
  g_cb_timing = on != 0;
  return VAQHIP_OK;
}

int vaqhip_last_fit_codebooks_timing(vaqhip_fit_codebooks_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_cb_last;
  return VAQHIP_OK;
}

}  // extern "C"
