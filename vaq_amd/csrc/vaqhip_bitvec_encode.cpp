// vaqhip_bitvec_encode.cpp -- the Hamming engine makes its own bits: vaqhip_bitvec_fit_thresholds*, vaqhip_bitvec_set_encoder
// and the vaqhip_bitvec_encode* entries of include/vaqhip.h (BitVecEngine::binaryEncodingSimple and ::binaryEncoding
// from the eigenvectors and the bit allocation on).  Kernels in vaq_bitvec_encode.hip, statements in vaq_bitvec_encode.h.
#include "vaqhip_bitvec.h"

#include <cmath>

#include "vaq_fast.h"

using namespace vaqhost;
namespace be = vaq::bvenc;

namespace {

constexpr int64_t HOST_CHUNK_ROWS = (int64_t)1 << 20;  // rows per staged piece of the host forms

int check_dims(int D) {
  if (D < 1) return fail(VAQHIP_EINVAL, "D=%d", D);
  if (D > be::MAX_DIM) return fail(VAQHIP_EUNSUPPORTED, "D=%d > %d: a row must fit the encoder's LDS tile", D, be::MAX_DIM);
  return VAQHIP_OK;
}

int check_bits(int D, const int *bits) {
  for (int d = 0; d < D; d++)
    if (bits[d] < 0 || bits[d] > be::MAX_BITS) return fail(VAQHIP_EINVAL, "bits[%d]=%d outside 0..8 (Q has 256 rows)", d, bits[d]);
  return VAQHIP_OK;
}

// the LUT fit's refusals, with 0 bits allowed (the dimension is skipped)
int check_fit(const void *X, int64_t n, int D, const int *bits, const void *out) {
  if (!X || !bits || !out) return fail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return fail(VAQHIP_EINVAL, "n=%lld: the quantile reads Z[0] of an empty column", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(VAQHIP_EINVAL, "n=%lld: at most 2^31 - 1 rows, as the LUT fit", (long long)n);
  if (int rc = check_dims(D)) return rc;
  return check_bits(D, bits);
}

// device pointers, the device current; d_thr is written only when the fit succeeds
int fit_core(vaq::RowsRef d_X, int64_t n, int D, const int *bits, const float *d_eig, float *d_thr, hipStream_t st) {
  int bad = 0;
  HIP_TRY(vaq::bitvec_fit_thresholds(d_X, n, D, bits, d_eig, d_thr, &bad, st));
  if (bad) return fail(VAQHIP_EINVAL, "a training value is NaN or infinite%s: std::sort has no defined result on it",
                       d_eig ? " after the projection" : "");
  return VAQHIP_OK;
}

int fit_device_entry(int device_id, vaq::RowsRef d_X, int64_t n, int D, const int *bits, const float *d_eig, float *d_thr,
                     void *stream) {
  if (int rc = check_fit(d_X.p, n, D, bits, d_thr)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return fit_core(d_X, n, D, bits, d_eig, d_thr, static_cast<hipStream_t>(stream));
}

int fit_host_entry(int device_id, vaq::RowsRef X, int64_t n, int D, const int *bits, const float *eigvec, float *thr_out) {
  if (int rc = check_fit(X.p, n, D, bits, thr_out)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  DevBuf d_x, d_eig, d_thr;
  const size_t x_bytes = (size_t)n * D * (size_t)X.elem, thr_floats = (size_t)D * be::THR_STRIDE;
  HIP_TRY(d_x.ensure(x_bytes));
  HIP_TRY(d_thr.ensure(thr_floats * sizeof(float)));
  HIP_TRY(hipMemcpy(d_x.p, X.p, x_bytes, hipMemcpyHostToDevice));
  if (eigvec) {
    HIP_TRY(d_eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(d_eig.p, eigvec, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
  }
  CallStream st;
  HIP_TRY(st.open());
  if (int rc = fit_core(vaq::RowsRef{d_x.p, X.elem}, n, D, bits, eigvec ? d_eig.as<float>() : nullptr, d_thr.as<float>(), st.s))
    return rc;
  std::vector<float> h(thr_floats);
  HIP_TRY(hipMemcpy(h.data(), d_thr.p, thr_floats * sizeof(float), hipMemcpyDeviceToHost));
  for (int d = 0; d < D; d++)  // (only what the fit wrote: the rest of the caller's table is left as it is)
    std::copy_n(h.data() + (size_t)d * be::THR_STRIDE, bits[d] ? 1 << bits[d] : 0, thr_out + (size_t)d * be::THR_STRIDE);
  return VAQHIP_OK;
}

int check_rows(const vaqhip_bitvec *bv, const void *X, int64_t n) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (n < 0 || (n > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  return VAQHIP_OK;
}
int check_encoder(const vaqhip_bitvec *bv) {
  return bv->enc.set ? VAQHIP_OK : fail(VAQHIP_ESTATE, "no encoder: call vaqhip_bitvec_set_encoder first");
}
int check_labels(int64_t n, int64_t id_base) {
  if (id_base < 0) return fail(VAQHIP_EINVAL, "id_base < 0");
  if (n > 0x7fffffffLL - 1 || id_base + n > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints: id_base+n = %lld", (long long)(id_base + n));
  return VAQHIP_OK;
}

// n host rows in staged pieces through w.oq on the engine's stream, encoded to d_out (the device's) or, staged through
// w.q, to h_out (the host's).  Caller holds bv->mu.
int encode_host_rows(vaqhip_bitvec *bv, vaq::RowsRef X, int64_t n, uint64_t *d_out, uint64_t *h_out) {
  const int64_t chunk = std::min(n, HOST_CHUNK_ROWS);
  const size_t row_bytes = (size_t)bv->enc.D * X.elem, word_bytes = (size_t)bv->W * sizeof(uint64_t);
  HIP_TRY(bv->w.oq.ensure((size_t)chunk * row_bytes));
  if (h_out) HIP_TRY(bv->w.q.ensure((size_t)chunk * word_bytes));
  WS_SCOPE(ws, bv, bv->stream);
  const vaq::BitvecEncodePlan plan = bv->enc.plan(bv->W);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t m = std::min(chunk, n - r0);
    HIP_TRY(hipMemcpyAsync(bv->w.oq.p, static_cast<const char *>(X.p) + (size_t)r0 * row_bytes, (size_t)m * row_bytes,
                           hipMemcpyHostToDevice, bv->stream));
    uint64_t *dst = h_out ? bv->w.q.as<uint64_t>() : d_out + (size_t)r0 * bv->W;
    HIP_TRY(vaq::launch_bitvec_encode(vaq::RowsRef{bv->w.oq.p, X.elem}, m, plan, dst, bv->stream));
    if (h_out)
      HIP_TRY(hipMemcpyAsync(h_out + (size_t)r0 * bv->W, dst, (size_t)m * word_bytes, hipMemcpyDeviceToHost, bv->stream));
    HIP_TRY(hipStreamSynchronize(bv->stream));  // (the next piece overwrites the staging)
  }
  return ws.finish();
}

int encode_entry(vaqhip_bitvec *bv, vaq::RowsRef X, int64_t n, uint64_t *out, bool on_device, void *stream) {
  if (int rc = check_rows(bv, X.p, n)) return rc;
  if (n > 0 && !out) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(bv);
  if (int rc = check_encoder(bv)) return rc;
  if (n == 0) return VAQHIP_OK;
  if (!on_device) return encode_host_rows(bv, X, n, nullptr, out);
  HIP_TRY(vaq::launch_bitvec_encode(X, n, bv->enc.plan(bv->W), out, static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}

// the padding behind row `end` of the store zeroed, and everything enqueued on the engine's stream waited for
int finish_store(vaqhip_bitvec *bv, int64_t end) {
  const size_t rb = bv->rows.row_bytes(bv->W);
  const int64_t pad = vaq::fast_pad_rows(end) - end;
  if (pad > 0) HIP_TRY(hipMemsetAsync(bv->rows.buf.as<char>() + (size_t)end * rb, 0, (size_t)pad * rb, bv->stream));
  HIP_TRY(hipStreamSynchronize(bv->stream));
  return VAQHIP_OK;
}

// replaces the engine's rows by the encoded X (host rows, or the rows of a device on the engine's GPU)
int set_encoded(vaqhip_bitvec *bv, vaq::RowsRef X, bool on_device, int64_t n, int64_t id_base) {
  bv->N = 0;  // (a failure below leaves no rows, not rows half replaced)
  bv->drop_clusters();
  HIP_TRY(bv->rows.reserve(vaq::fast_pad_rows(n), RowStore::DROP, bv->W));
  HIP_TRY(hipDeviceSynchronize());  // (a query enqueued on any stream may still read the old rows)
  if (n > 0 && on_device)
    HIP_TRY(vaq::launch_bitvec_encode(X, n, bv->enc.plan(bv->W), bv->rows.buf.as<uint64_t>(), bv->stream));
  if (n > 0 && !on_device)
    if (int rc = encode_host_rows(bv, X, n, bv->rows.buf.as<uint64_t>(), nullptr)) return rc;
  if (int rc = finish_store(bv, n)) return rc;
  bv->N = n;
  bv->id_base = id_base;
  return VAQHIP_OK;
}

int set_rows_entry(vaqhip_bitvec *bv, vaq::RowsRef X, int64_t n, int64_t id_base) {
  if (int rc = check_rows(bv, X.p, n)) return rc;
  if (int rc = check_labels(n, id_base)) return rc;
  ENTRY(bv);
  if (int rc = check_encoder(bv)) return rc;
  return set_encoded(bv, X, false, n, id_base);
}

int add_rows_entry(vaqhip_bitvec *bv, vaq::RowsRef X, int64_t n_new) {
  if (int rc = check_rows(bv, X.p, n_new)) return rc;
  ENTRY(bv);
  if (int rc = check_encoder(bv)) return rc;
  if (n_new == 0) return VAQHIP_OK;
  if (int rc = check_labels(bv->N + n_new, bv->id_base)) return rc;
  bv->drop_clusters();  // (the cluster state describes the rows as they were)
  HIP_TRY(bv->rows.reserve(vaq::fast_pad_rows(bv->N + n_new), bv->N, bv->W));
  // (rows past N are the padding: a query in flight may read them, but no answer depends on what they hold)
  if (int rc = encode_host_rows(bv, X, n_new, bv->rows.buf.as<uint64_t>() + (size_t)bv->N * bv->W, nullptr)) return rc;
  if (int rc = finish_store(bv, bv->N + n_new)) return rc;
  bv->N += n_new;
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_bitvec_fit_thresholds(int device_id, const float *X, int64_t n, int D, const int *bits, const float *eigvec,
                                 float *thresholds_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, bits, eigvec, thresholds_out);
}
int vaqhip_bitvec_fit_thresholds_u8(int device_id, const uint8_t *X, int64_t n, int D, const int *bits, const float *eigvec,
                                    float *thresholds_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, bits, eigvec, thresholds_out);
}
int vaqhip_bitvec_fit_thresholds_device(int device_id, const float *d_X, int64_t n, int D, const int *bits,
                                        const float *d_eigvec, float *d_thresholds_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, bits, d_eigvec, d_thresholds_out, stream);
}
int vaqhip_bitvec_fit_thresholds_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, const int *bits,
                                           const float *d_eigvec, float *d_thresholds_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, bits, d_eigvec, d_thresholds_out, stream);
}

int vaqhip_bitvec_set_encoder(vaqhip_bitvec *bv, int D, const float *eigvec, const int *bits, const float *thresholds) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (int rc = check_dims(D)) return rc;
  std::vector<vaq::BitvecLive> live;
  std::vector<float> pm;
  if (!bits) {  // the sign form
    if (bv->n_bits != D) return fail(VAQHIP_EINVAL, "the sign form gives D=%d bits a row, the engine has n_bits=%d", D, bv->n_bits);
    if (!be::sign_form_defined(D))
      return fail(VAQHIP_EUNSUPPORTED, "D=%d: with D %% 64 == 63 binaryEncodingSimple shifts by 64 and writes word (D + 1) / 64, "
                  "past the row's last word", D);
  } else {
    if (!thresholds) return fail(VAQHIP_EINVAL, "the quantile form needs its thresholds");
    if (int rc = check_bits(D, bits)) return rc;
    int pos = 0;
    for (int d = 0; d < D; pos += bits[d], d++) {
      if (bits[d] == 0) continue;
      const int N = 1 << bits[d];
      const float *T = thresholds + (size_t)d * be::THR_STRIDE;
      for (int q = 0; q < N; q++)
        if (std::isnan(T[q])) return fail(VAQHIP_EINVAL, "thresholds[%d][%d] is NaN", d, q);
      live.push_back(vaq::BitvecLive{d, bits[d], pos, (int)pm.size()});
      pm.resize(pm.size() + N);
      vaq::lutfit::prefix_max_host(T, N - 1, pm.data() + pm.size() - N);
    }
    if (pos != bv->n_bits) return fail(VAQHIP_EINVAL, "sum(bits)=%d, the engine has n_bits=%d", pos, bv->n_bits);
  }
  ENTRY(bv);
  BitvecEncoder &e = bv->enc;
  HIP_TRY(hipDeviceSynchronize());  // (an encode enqueued on any stream may still read the old tables)
  e.set = false;
  if (eigvec) {
    HIP_TRY(e.eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(e.eig.p, eigvec, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
  }
  if (bits) {
    HIP_TRY(e.live.ensure(live.size() * sizeof(vaq::BitvecLive)));
    HIP_TRY(e.pm.ensure(pm.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(e.live.p, live.data(), live.size() * sizeof(vaq::BitvecLive), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e.pm.p, pm.data(), pm.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  e.D = D;
  e.has_eig = eigvec != nullptr;
  e.quantile = bits != nullptr;
  e.n_live = bits ? (int)live.size() : D;
  e.pm_floats = (int)pm.size();
  e.set = true;
  return VAQHIP_OK;
}

int vaqhip_bitvec_encode(vaqhip_bitvec *bv, const float *X, int64_t n, uint64_t *rows_out) {
  return encode_entry(bv, vaq::RowsRef{X, 4}, n, rows_out, false, nullptr);
}
int vaqhip_bitvec_encode_u8(vaqhip_bitvec *bv, const uint8_t *X, int64_t n, uint64_t *rows_out) {
  return encode_entry(bv, vaq::RowsRef{X, 1}, n, rows_out, false, nullptr);
}
int vaqhip_bitvec_encode_device(vaqhip_bitvec *bv, const float *d_X, int64_t n, uint64_t *d_rows_out, void *stream) {
  return encode_entry(bv, vaq::RowsRef{d_X, 4}, n, d_rows_out, true, stream);
}
int vaqhip_bitvec_encode_u8_device(vaqhip_bitvec *bv, const uint8_t *d_X, int64_t n, uint64_t *d_rows_out, void *stream) {
  return encode_entry(bv, vaq::RowsRef{d_X, 1}, n, d_rows_out, true, stream);
}

int vaqhip_bitvec_encode_set_rows(vaqhip_bitvec *bv, const float *X, int64_t n, int64_t id_base) {
  return set_rows_entry(bv, vaq::RowsRef{X, 4}, n, id_base);
}
int vaqhip_bitvec_encode_set_rows_u8(vaqhip_bitvec *bv, const uint8_t *X, int64_t n, int64_t id_base) {
  return set_rows_entry(bv, vaq::RowsRef{X, 1}, n, id_base);
}
int vaqhip_bitvec_encode_add_rows(vaqhip_bitvec *bv, const float *X, int64_t n_new) {
  return add_rows_entry(bv, vaq::RowsRef{X, 4}, n_new);
}
int vaqhip_bitvec_encode_add_rows_u8(vaqhip_bitvec *bv, const uint8_t *X, int64_t n_new) {
  return add_rows_entry(bv, vaq::RowsRef{X, 1}, n_new);
}

int vaqhip_bitvec_encode_from_refiner(vaqhip_bitvec *bv, vaqhip_refiner *r, int64_t id_base) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  ENTRY(bv);
  if (int rc = check_encoder(bv)) return rc;
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (rv.device != bv->device)
    return fail(VAQHIP_EINVAL, "the bitvec engine is on device %d, the refiner on device %d", bv->device, rv.device);
  if (rv.D != bv->enc.D) return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the encoder D=%d", rv.D, bv->enc.D);
  if (int rc = check_labels(rv.N, id_base)) return rc;
  return set_encoded(bv, rv.rows, true, rv.N, id_base);
}

}  // extern "C"
