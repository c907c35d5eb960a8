// vaqhip_lutfit.cpp -- host side of building a queryLUT index (BitVecEngine::binaryEncodingLUT from the bit
// allocation on): vaqhip_lut_fit_quantiles*, vaqhip_index_set_lut_quantiles, and the vaqhip_encode_lut* entries, which
// run vaqhip_api.cpp's encode driver under encode_rule_lut().  Kernels in vaq_lutfit.hip, arithmetic in vaq_lutfit.h.
#include "vaqhip_index.h"

#include <chrono>
#include <cmath>

#include "vaq_front.h"
#include "vaq_lutfit.h"
#include "vaq_lutfit_dev.h"

using namespace vaqhost;
namespace lf = vaq::lutfit;

namespace {
thread_local int g_fit_timing = 0;
thread_local vaqhip_lut_fit_timing g_fit_last = {};

int check_fit_args(int64_t n, int D, const int *bits, const void *X, const void *cent, const void *q) {
  if (!X || !bits || !cent || !q) return fail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return fail(VAQHIP_EINVAL, "n=%lld: centroidsQuantile reads Z.front() of an empty column", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(VAQHIP_EINVAL, "n=%lld: the reference counts a bucket in an int", (long long)n);
  if (D < 1) return fail(VAQHIP_EINVAL, "D=%d", D);
  if (D > 4096) return fail(VAQHIP_EUNSUPPORTED, "D=%d > 4096", D);
  for (int d = 0; d < D; d++)
    if (bits[d] < 1 || bits[d] > 8) return fail(VAQHIP_EINVAL, "bits[%d]=%d outside 1..8 (centroidsMat has 256 rows)", d, bits[d]);
  return VAQHIP_OK;
}

// device pointers throughout, the device current; the outputs are written only when the fit succeeds
int fit_core(vaq::RowsRef d_X, int64_t n, int D, const int *bits, const float *d_eig, float *d_cent_out, float *d_q_out,
             hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf b_proj, b_cent, b_q, b_bad;
  float project_ms = 0.0f;
  vaq::RowsRef xp = d_X;  // (byte rows without a rotation: the extract widens them, no float copy)
  if (d_eig) {  // unchecked, as :620 projects the training rows
    HIP_TRY(b_proj.ensure((size_t)n * D * sizeof(float)));
    HIP_TRY(vaq::launch_project(d_X, n, D, d_eig, b_proj.as<float>(), st, 0));
    xp = vaq::RowsRef{b_proj.p, 4};
    if (g_fit_timing) {
      HIP_TRY(hipStreamSynchronize(st));
      project_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  HIP_TRY(b_cent.ensure((size_t)D * lf::MAX_CENT * sizeof(float)));
  HIP_TRY(b_q.ensure((size_t)D * lf::MAX_Q * sizeof(float)));
  HIP_TRY(b_bad.ensure(sizeof(int)));
  float phase[4] = {0, 0, 0, 0};
  HIP_TRY(vaq::lut_fit_columns(xp, n, D, bits, b_cent.as<float>(), b_q.as<float>(), b_bad.as<int>(),
                               g_fit_timing ? phase : nullptr, st));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, b_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) return fail(VAQHIP_EINVAL, "a training value is NaN or infinite%s: std::sort has no defined result on it",
                       d_eig ? " after the projection" : "");
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_cent.p, (size_t)D * lf::MAX_CENT * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_q_out, b_q.p, (size_t)D * lf::MAX_Q * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  g_fit_last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_fit_last.project_ms = project_ms;
  g_fit_last.extract_ms = phase[0];
  g_fit_last.sort_ms = phase[1];
  g_fit_last.quantile_ms = phase[2];
  g_fit_last.means_ms = phase[3];
  g_fit_last.rows = n;
  g_fit_last.dims = D;
  return VAQHIP_OK;
}

int fit_device_entry(int device_id, vaq::RowsRef d_X, int64_t n, int D, const int *bits, const float *d_eigvec,
                     float *d_centroids_out, float *d_quantiles_out, void *stream) {
  if (int rc = check_fit_args(n, D, bits, d_X.p, d_centroids_out, d_quantiles_out)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return fit_core(d_X, n, D, bits, d_eigvec, d_centroids_out, d_quantiles_out, static_cast<hipStream_t>(stream));
}

// X: host rows of X.elem bytes per element, uploaded as they are
int fit_host_entry(int device_id, vaq::RowsRef X, int64_t n, int D, const int *bits, const float *eigvec,
                   float *centroids_out, float *quantiles_out) {
  if (int rc = check_fit_args(n, D, bits, X.p, centroids_out, quantiles_out)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  DevBuf d_x, d_eig, d_cent, d_q;
  const size_t cent_bytes = (size_t)D * lf::MAX_CENT * sizeof(float), q_bytes = (size_t)D * lf::MAX_Q * sizeof(float);
  const size_t x_bytes = (size_t)n * D * (size_t)X.elem;
  HIP_TRY(d_x.ensure(x_bytes));
  HIP_TRY(d_cent.ensure(cent_bytes));
  HIP_TRY(d_q.ensure(q_bytes));
  HIP_TRY(hipMemcpy(d_x.p, X.p, x_bytes, hipMemcpyHostToDevice));
  if (eigvec) {
    HIP_TRY(d_eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(d_eig.p, eigvec, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
  }
  CallStream st;
  HIP_TRY(st.open());
  if (int rc = fit_core(vaq::RowsRef{d_x.p, X.elem}, n, D, bits, eigvec ? d_eig.as<float>() : nullptr, d_cent.as<float>(),
                        d_q.as<float>(), st.s))
    return rc;
  HIP_TRY(hipMemcpy(centroids_out, d_cent.p, cent_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(quantiles_out, d_q.p, q_bytes, hipMemcpyDeviceToHost));
  return VAQHIP_OK;
}
}  // namespace

extern "C" {

int vaqhip_lut_fit_quantiles_device(int device_id, const float *d_X, int64_t n, int D, const int *bits,
                                    const float *d_eigvec, float *d_centroids_out, float *d_quantiles_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, bits, d_eigvec, d_centroids_out, d_quantiles_out, stream);
}
int vaqhip_lut_fit_quantiles_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, const int *bits,
                                       const float *d_eigvec, float *d_centroids_out, float *d_quantiles_out,
                                       void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, bits, d_eigvec, d_centroids_out, d_quantiles_out, stream);
}
int vaqhip_lut_fit_quantiles(int device_id, const float *X, int64_t n, int D, const int *bits, const float *eigvec,
                             float *centroids_out, float *quantiles_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, bits, eigvec, centroids_out, quantiles_out);
}
int vaqhip_lut_fit_quantiles_u8(int device_id, const uint8_t *X, int64_t n, int D, const int *bits, const float *eigvec,
                                float *centroids_out, float *quantiles_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, bits, eigvec, centroids_out, quantiles_out);
}

// ---- vaqhip_internal.h: what the sharded fit takes from here ----
int vaqhip_internal_lut_fit_check(const void *X, int64_t n, int D, const int *bits, const void *centroids_out,
                                  const void *quantiles_out) {
  return check_fit_args(n, D, bits, X, centroids_out, quantiles_out);
}

int vaqhip_lut_fit_set_timing(int on) {
  g_fit_timing = on != 0;
  return VAQHIP_OK;
}

int vaqhip_last_lut_fit_timing(vaqhip_lut_fit_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_fit_last;
  return VAQHIP_OK;
}

int vaqhip_index_set_lut_quantiles(vaqhip_index *ix, const float *quantiles) {
  if (!ix || !quantiles) return fail(VAQHIP_EINVAL, "null pointer");
  if (!ix->seq) return fail(VAQHIP_EINVAL, "quantiles belong to a VAQHIP_SUM_SEQUENTIAL index (BitVecEngine's scalar quantisers)");
  if (ix->L != 1) return fail(VAQHIP_EINVAL, "D=%d != M=%d: the engine has one quantiser per dimension", ix->D, ix->M);
  int cent_total = 0;
  for (int s = 0; s < ix->M; s++) {
    if (ix->bits[s] > 8) return fail(VAQHIP_EINVAL, "bits[%d]=%d > 8: Q has at most 257 entries", s, ix->bits[s]);
    for (int j = 0; j <= ix->sub[s].ncent; j++)
      if (std::isnan(quantiles[(size_t)s * lf::MAX_Q + j])) return fail(VAQHIP_EINVAL, "quantiles[%d][%d] is NaN", s, j);
    cent_total += ix->sub[s].ncent;
  }
  std::vector<float> pm((size_t)cent_total + ix->M);
  for (int s = 0; s < ix->M; s++)
    lf::prefix_max_host(quantiles + (size_t)s * lf::MAX_Q, ix->sub[s].ncent, pm.data() + ix->sub[s].cent_off + s);
  ENTRY(ix);
  HIP_TRY(ix->d_lut_pm.ensure(pm.size() * sizeof(float)));
  WS_SCOPE(ws, ix, ix->stream);  // (an encode on another stream may still read the old boundaries)
  HIP_TRY(hipMemcpyAsync(ix->d_lut_pm.p, pm.data(), pm.size() * sizeof(float), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->lut_q.assign(quantiles, quantiles + (size_t)ix->M * lf::MAX_Q);
  return ws.finish();
}

int vaqhip_encode_lut_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected, uint16_t *d_codes,
                             void *stream) {
  return encode_device_entry(ix, encode_rule_lut(), vaq::RowsRef{d_X, 4}, n, projected, d_codes, stream);
}
int vaqhip_encode_lut_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected, uint16_t *d_codes,
                                void *stream) {
  return encode_device_entry(ix, encode_rule_lut(), vaq::RowsRef{d_X, 1}, n, projected, d_codes, stream);
}
int vaqhip_encode_lut(vaqhip_index *ix, const float *X, int64_t n, int projected, uint16_t *codes) {
  return encode_host_entry(ix, encode_rule_lut(), vaq::RowsRef{X, 4}, n, projected, codes);
}
int vaqhip_encode_lut_u8(vaqhip_index *ix, const uint8_t *X, int64_t n, int projected, uint16_t *codes) {
  return encode_host_entry(ix, encode_rule_lut(), vaq::RowsRef{X, 1}, n, projected, codes);
}

}  // extern "C"
