// vaqhip_api.cpp -- host side of the C ABI declared in include/vaqhip.h: errors, the index's life, its
// options and timing, and the entry points that need no scan (project, build_lut, encode, merge, refine).
// The scan is in vaqhip_search.cpp (planned by vaqhip_plan.cpp), the rows in vaqhip_codes.cpp, FAST in
// vaqhip_fast.cpp.  There is no CPU path here: every entry point needs a HIP
// device and fails with VAQHIP_ENODEVICE / VAQHIP_EHIP otherwise.
#include "vaqhip_index.h"
#include "vaq_codes.h"
#include "vaq_front.h"
#include "vaq_lutfit_dev.h"
#include "vaq_merge.h"
#include "vaq_refine.h"

#include <cstdarg>
#include <string>

using namespace vaqhost;

namespace {
thread_local std::string g_err;
}

int vaqhost::fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// ---- rows of either element type to codes: one driver, two rules (vaqhip_index.h) ----
namespace vaqhost {
// VAQ::encode.  (BitVecEngine::queryLUT projects with checking, BitVecEngine.hpp:1226: non-finite coordinates -> 0,
//  which needs a pass over the queries even without a rotation)
static bool vaq_projects(const vaqhip_index *ix) { return ix->has_eig || ix->seq; }
static hipError_t vaq_launch(const vaqhip_index *ix, const float *xp, int64_t m, uint16_t *d_codes, hipStream_t st) {
  return vaq::launch_encode(xp, m, ix->D, ix->M, ix->L, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent.as<float>(), d_codes, st);
}
// encodeToLUTCode.  The projection is unchecked (:620); without a rotation the rows are their own image
static bool lut_projects(const vaqhip_index *ix) { return ix->has_eig; }
static hipError_t lut_launch(const vaqhip_index *ix, const float *xp, int64_t m, uint16_t *d_codes, hipStream_t st) {
  return vaq::launch_lut_encode(xp, m, ix->D, ix->sub.data(), ix->d_sub.as<vaq::SubDesc>(), ix->d_lut_pm.as<float>(),
                                ix->d_cent.as<float>(), d_codes, ix->n_cu, st);
}
// (functions, not constants: this file is compiled as HIP, where a constant object is emitted for the device too)
EncodeRule encode_rule_vaq() { return {false, vaq_projects, vaq_launch}; }
EncodeRule encode_rule_lut() { return {true, lut_projects, lut_launch}; }

int check_encode_args(const vaqhip_index *ix, const EncodeRule &rule, const void *X, int64_t n, const void *codes) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (n < 0 || (n > 0 && (!X || !codes))) return fail(VAQHIP_EINVAL, "bad arguments");
  if (rule.lut && ix->lut_q.empty()) return fail(VAQHIP_ESTATE, "vaqhip_encode_lut needs vaqhip_index_set_lut_quantiles first");
  return VAQHIP_OK;
}

// core of vaqhip_encode*: caller holds ix->mu and has the device current.  d_X: float or byte rows.  Byte rows are
// widened by the projection's own load; where no projection runs, by launch_widen_rows_u8 into the buffer the
// projection would have written
int encode_rows_locked(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef d_X, int64_t n, int projected,
                       uint16_t *d_codes, hipStream_t st) {
  const bool do_project = !projected && rule.project(ix);
  const bool widen = !do_project && d_X.elem == 1;
  const int64_t chunk = std::min<int64_t>(n, 1 << 20);
  if (do_project || widen) HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  WS_SCOPE(ws, ix, st);
  for (int64_t r = 0; r < n; r += chunk) {
    const int64_t m = std::min(chunk, n - r);
    const vaq::RowsRef x = vaq::rows_at(d_X, (size_t)r * ix->D);
    const float *xp = static_cast<const float *>(x.p);
    if (do_project) {
      HIP_TRY(vaq::launch_project(x, m, ix->D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st, 0));
      xp = ix->w_qproj.as<float>();
    } else if (widen) {
      HIP_TRY(vaq::launch_widen_rows_u8(static_cast<const uint8_t *>(x.p), m * ix->D, ix->w_qproj.as<float>(), st));
      xp = ix->w_qproj.as<float>();
    }
    HIP_TRY(rule.launch(ix, xp, m, d_codes + r * ix->M, st));
  }
  return ws.finish();
}

int encode_device_entry(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef d_X, int64_t n, int projected,
                        uint16_t *d_codes, void *stream) {
  if (int rc = check_encode_args(ix, rule, d_X.p, n, d_codes)) return rc;
  if (n == 0) return VAQHIP_OK;
  ENTRY(ix);
  return encode_rows_locked(ix, rule, d_X, n, projected, d_codes, static_cast<hipStream_t>(stream));
}

// X: host rows of X.elem bytes per element; the staging buffer is sized in bytes
int encode_host_entry(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef X, int64_t n, int projected, uint16_t *codes) {
  if (int rc = check_encode_args(ix, rule, X.p, n, codes)) return rc;
  if (n == 0) return VAQHIP_OK;
  const int64_t chunk = std::min<int64_t>(n, 1 << 20);
  // the staging buffers (w_q, w_stage) are the index's: hold its lock across upload, encode and
  // download, as search_host does
  ENTRY(ix);
  HIP_TRY(ix->w_q.ensure((size_t)chunk * ix->D * (size_t)X.elem));
  HIP_TRY(ix->w_stage.ensure((size_t)chunk * ix->M * sizeof(uint16_t)));
  WS_SCOPE(ws, ix, ix->stream);  // (w_q may still be read by a search on another stream)
  for (int64_t r = 0; r < n; r += chunk) {
    const int64_t m = std::min(chunk, n - r);
    HIP_TRY(hipMemcpyAsync(ix->w_q.p, vaq::rows_at(X, (size_t)r * ix->D).p, (size_t)m * ix->D * (size_t)X.elem,
                           hipMemcpyHostToDevice, ix->stream));
    if (int rc = encode_rows_locked(ix, rule, vaq::RowsRef{ix->w_q.p, X.elem}, m, projected, ix->w_stage.as<uint16_t>(), ix->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(codes + r * ix->M, ix->w_stage.p, (size_t)m * ix->M * sizeof(uint16_t),
                           hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
  }
  return ws.finish();
}
}  // namespace vaqhost

extern "C" {
const char *vaqhip_last_error(void) { return g_err.c_str(); }
int vaqhip_version(void) { return VAQHIP_VERSION; }

int vaqhip_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(VAQHIP_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int vaqhip_index_create(vaqhip_index **out, int D, int M, const int *bits,
                        const float *const *centroids, const float *eig, int device_id) {
  return vaqhip_index_create_ex(out, D, M, bits, centroids, eig, device_id, 0u);
}

int vaqhip_index_create_ex(vaqhip_index **out, int D, int M, const int *bits,
                           const float *const *centroids, const float *eig, int device_id,
                           unsigned flags) {
  if (!out) return fail(VAQHIP_EINVAL, "out is null");
  const bool seq = (flags & VAQHIP_SUM_SEQUENTIAL) != 0;
  if (flags & ~(unsigned)VAQHIP_SUM_SEQUENTIAL) return fail(VAQHIP_EINVAL, "unknown flags 0x%x", flags);
  *out = nullptr;
  if (D <= 0 || M <= 0 || !bits || !centroids) return fail(VAQHIP_EINVAL, "bad D/M/bits/centroids");
  if (M > VAQHIP_MAX_SUBSPACES) return fail(VAQHIP_EUNSUPPORTED, "M=%d > %d", M, VAQHIP_MAX_SUBSPACES);
  if (M % 4 != 0 && !seq)
    return fail(VAQHIP_EINVAL, "M=%d: the reference scan reads 4 codes per step (VAQ.cpp:1741-1746)", M);
  if (D % M != 0) return fail(VAQHIP_EINVAL, "D=%d is not a multiple of M=%d", D, M);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VAQHIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
  if (device_id < 0 || device_id >= ndev) return fail(VAQHIP_EINVAL, "device_id=%d of %d", device_id, ndev);

  vaqhip_index *ix = new (std::nothrow) vaqhip_index();
  if (!ix) return fail(VAQHIP_ENOMEM, "host allocation");
  struct Cleanup {
    vaqhip_index *p;
    ~Cleanup() { if (p) vaqhip_index_destroy(p); }
  } cleanup{ix};
  ix->D = D;
  ix->M = M;
  ix->L = D / M;
  ix->device = device_id;
  ix->bits.assign(bits, bits + M);
  ix->sub.resize(M);
  int bit_off = 0, lut_off = 0, cent_off = 0, maxb = 0;
  bool all8 = true;
  for (int s = 0; s < M; s++) {
    const int b = bits[s];
    if (b < 1 || b > VAQHIP_MAX_BITS) return fail(VAQHIP_EINVAL, "bits[%d]=%d outside 1..%d", s, b, VAQHIP_MAX_BITS);
    if (!centroids[s]) return fail(VAQHIP_EINVAL, "centroids[%d] is null", s);
    vaq::SubDesc &sd = ix->sub[s];
    sd.ncent = 1 << b;
    sd.bits = b;
    sd.bit_off = bit_off;
    sd.lut_off = lut_off;
    sd.cent_off = cent_off;
    sd.word = bit_off / 32;
    sd.shift = bit_off % 32;
    sd.pad = 0;
    bit_off += b;
    lut_off += sd.ncent;
    cent_off += sd.ncent * ix->L;
    maxb = std::max(maxb, b);
    all8 = all8 && b == 8;
  }
  ix->max_bits = maxb;
  ix->min_bits = *std::min_element(bits, bits + M);
  ix->total_bits = bit_off;
  ix->lut_floats = lut_off;
  ix->W = (bit_off + 31) / 32;
  ix->seq = seq ? 1 : 0;
  ix->fast_ok = !seq && maxb <= 4;
  ix->layout =(!seq && all8 && (M == 8 || M == 16 || M == 32)) ? vaq::LAYOUT_BYTES : vaq::LAYOUT_BITS;
  if (ix->layout == vaq::LAYOUT_BITS && ix->W > 8)
    return fail(VAQHIP_EUNSUPPORTED, "%d code bits per row; this build packs at most 256", bit_off);
  std::vector<int> first_sub(ix->W + 1, M);
  first_sub[0] = 0;
  for (int w = 1; w <= ix->W; w++) {
    int f = M;
    for (int s = 0; s < M; s++)
      if (ix->sub[s].bit_off >= 32 * w) { f = s; break; }
    first_sub[w] = f;
  }

  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device_id);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
    ix->n_cu = prop.multiProcessorCount;
  HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
  HIP_TRY(ix->d_cent.ensure((size_t)cent_off * sizeof(float)));
  for (int s = 0; s < M; s++)
    HIP_TRY(hipMemcpy(ix->d_cent.as<float>() + ix->sub[s].cent_off, centroids[s],
                      (size_t)ix->sub[s].ncent * ix->L * sizeof(float), hipMemcpyHostToDevice));
  {
    // the same matrices dimension-major (the reference keeps mCentroidsPerSubsCMajor for its
    // AVX loads, VAQ.cpp:655-660): the LUT build reads them one centroid per lane, coalesced
    std::vector<float> t((size_t)cent_off);
    for (int s = 0; s < M; s++) {
      const int K = ix->sub[s].ncent;
      for (int c = 0; c < K; c++)
        for (int j = 0; j < ix->L; j++)
          t[(size_t)ix->sub[s].cent_off + (size_t)j * K + c] = centroids[s][(size_t)c * ix->L + j];
    }
    HIP_TRY(ix->d_cent_t.ensure((size_t)cent_off * sizeof(float)));
    HIP_TRY(hipMemcpy(ix->d_cent_t.p, t.data(), (size_t)cent_off * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(ix->d_sub.ensure(M * sizeof(vaq::SubDesc)));
  HIP_TRY(hipMemcpy(ix->d_sub.p, ix->sub.data(), M * sizeof(vaq::SubDesc), hipMemcpyHostToDevice));
  HIP_TRY(ix->d_first_sub.ensure(first_sub.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(ix->d_first_sub.p, first_sub.data(), first_sub.size() * sizeof(int),
                    hipMemcpyHostToDevice));
  if (eig) {
    HIP_TRY(ix->d_eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(ix->d_eig.p, eig, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
    ix->has_eig = true;
  }
  cleanup.p = nullptr;
  *out = ix;
  return VAQHIP_OK;
}

void vaqhip_index_destroy(vaqhip_index *ix) {
  if (!ix) return;
  DeviceGuard g(ix->device);
  if (ix->stream) {
    (void)hipStreamSynchronize(ix->stream);
    (void)hipStreamDestroy(ix->stream);
  }
  for (auto &e : ix->ev) (void)hipEventDestroy(e);
  if (ix->ws_event) (void)hipEventDestroy(ix->ws_event);
  delete ix;  // every DevBuf goes here: the index's device is current, its stream idle and gone
}

int vaqhip_project(vaqhip_index *ix, const float *X, int64_t n, float *out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (n < 0 || (n > 0 && (!X || !out))) return fail(VAQHIP_EINVAL, "bad arguments");
  if (n == 0) return VAQHIP_OK;
  ENTRY(ix);
  if (!ix->has_eig) {
    std::memcpy(out, X, (size_t)n * ix->D * sizeof(float));
    return VAQHIP_OK;
  }
  const int64_t chunk = std::min<int64_t>(n, 1 << 20);
  HIP_TRY(ix->w_q.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  WS_SCOPE(ws, ix, ix->stream);
  for (int64_t r = 0; r < n; r += chunk) {
    const int64_t m = std::min(chunk, n - r);
    const size_t bytes = (size_t)m * ix->D * sizeof(float);
    HIP_TRY(hipMemcpyAsync(ix->w_q.p, X + r * ix->D, bytes, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(vaq::launch_project(ix->w_q.as<float>(), m, ix->D, ix->d_eig.as<float>(),
                                ix->w_qproj.as<float>(), ix->stream));
    HIP_TRY(hipMemcpyAsync(out + r * ix->D, ix->w_qproj.p, bytes, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
  }
  return ws.finish();
}

int vaqhip_build_lut(vaqhip_index *ix, const float *queries, int nq, int projected, float *lut_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (nq < 0 || (nq > 0 && (!queries || !lut_out))) return fail(VAQHIP_EINVAL, "bad arguments");
  if (nq == 0) return VAQHIP_OK;
  ENTRY(ix);
  const int ksub = 1 << ix->max_bits;
  const size_t per_q = (size_t)ix->M * ksub;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, ((size_t)256 << 20) / (per_q * 4)));
  HIP_TRY(ix->w_q.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  HIP_TRY(ix->w_lutref.ensure((size_t)chunk * per_q * sizeof(float)));
  hipStream_t st = ix->stream;
  WS_SCOPE(ws, ix, st);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    HIP_TRY(hipMemcpyAsync(ix->w_q.p, queries + (size_t)q0 * ix->D, (size_t)n * ix->D * sizeof(float),
                           hipMemcpyHostToDevice, st));
    const float *qp = ix->w_q.as<float>();
    if (!projected && ix->has_eig) {
      HIP_TRY(vaq::launch_project(qp, n, ix->D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st));
      qp = ix->w_qproj.as<float>();
    }
    HIP_TRY(vaq::launch_lut_build(qp, n, ix->D, ix->M, ix->L, ix->d_sub.as<vaq::SubDesc>(),
                                  ix->d_cent_t.as<float>(), ix->lut_floats, 1 << ix->max_bits, ix->w_lut.as<float>(), st,
                                  1 << ix->min_bits));
    HIP_TRY(vaq::launch_lut_expand(ix->w_lut.as<float>(), n, ix->M, ix->d_sub.as<vaq::SubDesc>(),
                                   ix->lut_floats, ksub, ix->w_lutref.as<float>(), st));
    HIP_TRY(hipMemcpyAsync(lut_out + (size_t)q0 * per_q, ix->w_lutref.p, (size_t)n * per_q * sizeof(float),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return ws.finish();
}

int vaqhip_merge_topk_device(int device_id, const float *d_dist_lists, const int32_t *d_label_lists,
                             int n_lists, int nq, int k, int32_t *d_labels_out, float *d_dist_out,
                             void *stream) {
  return vaqhip_merge_topk_strided_device(device_id, d_dist_lists, d_label_lists, n_lists,
                                          (int64_t)nq * k, k, nq, k, d_labels_out, d_dist_out, stream);
}

int vaqhip_merge_topk_strided_device(int device_id, const float *d_dist_lists,
                                     const int32_t *d_label_lists, int n_lists, int64_t list_stride,
                                     int64_t query_stride, int nq, int k, int32_t *d_labels_out,
                                     float *d_dist_out, void *stream) {
  if (n_lists < 0 || nq < 0 || k <= 0) return fail(VAQHIP_EINVAL, "bad sizes");
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (nq == 0) return VAQHIP_OK;
  if ((n_lists > 0 && (!d_dist_lists || !d_label_lists)) || !d_labels_out || !d_dist_out)
    return fail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device_id);
  if (n_lists > 16) return fail(VAQHIP_EUNSUPPORTED, "at most 16 lists per merge");
  if (list_stride < 0 || query_stride < 0) return fail(VAQHIP_EINVAL, "negative stride");
  HIP_TRY(vaq::launch_merge(d_dist_lists, d_label_lists, nullptr, n_lists, list_stride, query_stride, nq, k, 0, 1,
                            d_labels_out, d_dist_out, nullptr, nullptr, nullptr,
                            static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}

int vaqhip_encode_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected,
                         uint16_t *d_codes, void *stream) {
  return encode_device_entry(ix, encode_rule_vaq(), vaq::RowsRef{d_X, 4}, n, projected, d_codes, stream);
}
int vaqhip_encode_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected,
                            uint16_t *d_codes, void *stream) {
  return encode_device_entry(ix, encode_rule_vaq(), vaq::RowsRef{d_X, 1}, n, projected, d_codes, stream);
}
int vaqhip_encode(vaqhip_index *ix, const float *X, int64_t n, int projected, uint16_t *codes) {
  return encode_host_entry(ix, encode_rule_vaq(), vaq::RowsRef{X, 4}, n, projected, codes);
}
int vaqhip_encode_u8(vaqhip_index *ix, const uint8_t *X, int64_t n, int projected, uint16_t *codes) {
  return encode_host_entry(ix, encode_rule_vaq(), vaq::RowsRef{X, 1}, n, projected, codes);
}

int vaqhip_refine_device(int device_id, const float *d_queries, int nq, int D, const float *d_dataset,
                         const int32_t *d_labels_in, int R, int k, int32_t *d_labels_out,
                         float *d_dist_out, void *stream) {
  if (nq < 0 || D <= 0 || R <= 0 || k <= 0) return fail(VAQHIP_EINVAL, "bad sizes");
  if (R > 2048 || k > R) return fail(VAQHIP_EUNSUPPORTED, "need k <= R <= 2048 (R=%d k=%d)", R, k);
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries || !d_dataset || !d_labels_in || !d_labels_out || !d_dist_out)
    return fail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device_id);
  HIP_TRY(vaq::launch_refine(d_queries, nq, D, d_dataset, nullptr, d_labels_in, R, k, d_labels_out,
                             d_dist_out, static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}

int vaqhip_refine(int device_id, const float *queries, int nq, int D, const float *dataset, int64_t N,
                  const int32_t *labels_in, int R, int k, int32_t *labels_out, float *dist_out) {
  if (nq < 0 || D <= 0 || R <= 0 || k <= 0 || N < 0) return fail(VAQHIP_EINVAL, "bad sizes");
  if (R > 2048 || k > R) return fail(VAQHIP_EUNSUPPORTED, "need k <= R <= 2048 (R=%d k=%d)", R, k);
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !dataset || !labels_in || !labels_out || !dist_out) return fail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  // gather the candidate rows on the host, re-rank on the GPU, in chunks of queries
  const size_t per_q = (size_t)R * D;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, ((size_t)256 << 20) / (per_q * 4)));
  DevBuf d_q, d_rows, d_lab, d_ol, d_od;
  HIP_TRY(d_q.ensure((size_t)chunk * D * 4));
  HIP_TRY(d_rows.ensure((size_t)chunk * per_q * 4));
  HIP_TRY(d_lab.ensure((size_t)chunk * R * 4));
  HIP_TRY(d_ol.ensure((size_t)chunk * k * 4));
  HIP_TRY(d_od.ensure((size_t)chunk * k * 4));
  std::vector<float> rows((size_t)chunk * per_q);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    for (int q = 0; q < n; q++)
      for (int i = 0; i < R; i++) {
        const int32_t lab = labels_in[(size_t)(q0 + q) * R + i];
        float *dst = rows.data() + ((size_t)q * R + i) * D;
        if (lab >= 0 && (int64_t)lab < N) std::memcpy(dst, dataset + (size_t)lab * D, (size_t)D * 4);
        else if (lab >= 0) return fail(VAQHIP_EINVAL, "label %d outside the dataset", lab);
        else std::memset(dst, 0, (size_t)D * 4);
      }
    HIP_TRY(hipMemcpy(d_q.p, queries + (size_t)q0 * D, (size_t)n * D * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rows.p, rows.data(), (size_t)n * per_q * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lab.p, labels_in + (size_t)q0 * R, (size_t)n * R * 4, hipMemcpyHostToDevice));
    HIP_TRY(vaq::launch_refine(d_q.as<float>(), n, D, nullptr, d_rows.as<float>(), d_lab.as<int32_t>(), R, k,
                               d_ol.as<int32_t>(), d_od.as<float>(), nullptr));
    HIP_TRY(hipMemcpy(labels_out + (size_t)q0 * k, d_ol.p, (size_t)n * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dist_out + (size_t)q0 * k, d_od.p, (size_t)n * k * 4, hipMemcpyDeviceToHost));
  }
  return VAQHIP_OK;
}

int vaqhip_index_set_method(vaqhip_index *ix, unsigned methods, float visit) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (methods & ~(VAQHIP_METHOD_EA | VAQHIP_METHOD_TI | VAQHIP_METHOD_HEAP | VAQHIP_METHOD_FAST))
    return fail(VAQHIP_EUNSUPPORTED, "method bits 0x%x: only HEAP, EA, TI and FAST are on this path", methods);
  if (!(methods & (VAQHIP_METHOD_EA | VAQHIP_METHOD_TI | VAQHIP_METHOD_HEAP | VAQHIP_METHOD_FAST)))
    return fail(VAQHIP_EUNSUPPORTED, "no search method selected (SORT is not provided)");
  if ((methods & VAQHIP_METHOD_FAST) && !ix->fast_ok)
    return fail(VAQHIP_EUNSUPPORTED, ix->seq ? "FAST is not defined for the sequential row sum"
                                             : "FAST needs max bits per subspace <= 4 (VAQ.cpp:1263-1266), this index has %d",
                ix->max_bits);
  if (!(visit > 0.0f)) return fail(VAQHIP_EINVAL, "visit must be > 0");
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->methods = methods;
  ix->ti_visit = visit;
  if (!fast_only(ix) && (ix->fast_rows >= 0 || ix->w_fast_dist.p)) {
    DeviceGuard g(ix->device);
    WS_SCOPE(ws, ix, ix->stream);  // (a FAST search may still read them)
    HIP_TRY(hipStreamSynchronize(ix->stream));
    fast_release(ix);
    return ws.finish();
  }
  return VAQHIP_OK;
}

int vaqhip_index_info(const vaqhip_index *ix, vaqhip_info *out) {
  if (!ix || !out) return fail(VAQHIP_EINVAL, "null pointer");
  out->D = ix->D;
  out->M = ix->M;
  out->L = ix->L;
  out->max_bits = ix->max_bits;
  out->total_bits = ix->total_bits;
  out->code_bytes = ix->layout == vaq::LAYOUT_BYTES ? ix->M : ix->W * 4;
  out->algo_code_bytes = (ix->total_bits + 7) / 8;
  out->lut_floats = ix->lut_floats;
  out->N = ix->N < 0 ? 0 : ix->N;
  out->id_base = ix->id_base;
  out->device_id = ix->device;
  out->layout = ix->layout;
  out->ti_clusters = ix->ti_T;
  out->ti_segments = ix->ti_seg;
  out->methods = ix->methods;
  out->visit = ix->ti_visit;
  return VAQHIP_OK;
}

int vaqhip_set_option(vaqhip_index *ix, const char *key, int64_t value) {
  if (!ix || !key) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::string k(key);
  if (k == "queries_per_pass") {
    if (value != 0 && value != 1 && value != 2 && value != 4)
      return fail(VAQHIP_EINVAL, "queries_per_pass must be 0, 1, 2 or 4");
    ix->opt_qb = (int)value;
  } else if (k == "slices") {
    if (value < 0 || value > (1 << 20)) return fail(VAQHIP_EINVAL, "slices out of range");
    ix->opt_slices = (int)value;
  } else if (k == "timing") {
    ix->opt_timing = value != 0;
    if (ix->opt_timing) {  // create the event ring now, not inside the first timed search
      DeviceGuard g(ix->device);
      if (int rc = ensure_events(ix)) return rc;
    }
  } else if (k == "early_abandon") {
    if (value < 0 || value > 3) return fail(VAQHIP_EINVAL, "early_abandon must be 0..3");
    ix->opt_ea = (int)value;
  } else if (k == "ordered_slices") {
    ix->opt_order = value != 0;
  } else if (k == "seed_fraction") {
    if (value < 2 || value > 65536) return fail(VAQHIP_EINVAL, "seed_fraction must be 2..65536");
    ix->opt_seed_frac = (int)value;
  } else if (k == "hot_buckets") {
    if (value < 0 || value > 32) return fail(VAQHIP_EINVAL, "hot_buckets must be 0..32");
    ix->opt_hot = (int)value;
  } else if (k == "bucket_skip") {
    ix->opt_no_skip = value == 0;
  } else if (k == "bucket_bits") {
    if (value < 0 || value > 12) return fail(VAQHIP_EINVAL, "bucket_bits must be 0..12");
    ix->opt_bucket_bits = (int)value;  // takes effect when the codes are (re)set
  } else if (k == "group_queries") {
    if (value < 0 || value > 2) return fail(VAQHIP_EINVAL, "group_queries must be 0, 1 or 2");
    ix->opt_group = (int)value;
  } else if (k == "best_first") {
    ix->opt_bf = value != 0;
  } else if (k == "cost_order") {
    ix->opt_cost_order = value != 0;
  } else if (k == "defer_units") {
    if (value < -1 || value > 1 << 20) return fail(VAQHIP_EINVAL, "defer_units must be -1 (automatic), 0 (off) or a number of work units");
    ix->opt_defer = (int)value;
  } else if (k == "exact_ties") {
    ix->opt_exact = value != 0;
  } else if (k == "bm_boot") {
    if (value < 0 || value > 2) return fail(VAQHIP_EINVAL, "bm_boot must be 0 (never), 1 (automatic) or 2 (always)");
    ix->opt_bm_boot = (int)value;
  } else if (k == "bm_round") {
    if (value < 0 || value > 1024) return fail(VAQHIP_EINVAL, "bm_round must be 0..1024 buckets");
    ix->opt_bm_round = (int)value;
  } else if (k == "bm_runs") {
    ix->opt_bm_sub = value != 0;  // 0: the bucket-major pass ignores the order inside the buckets (every row of a bucket read)
  } else if (k == "sub_order") {
    ix->opt_sub_order = value != 0;  // takes effect when the codes are (re)set
  } else if (k == "bucket_major") {
    if (value < 0 || value > 2) return fail(VAQHIP_EINVAL, "bucket_major must be 0 (off), 1 (automatic) or 2 (whenever a kernel exists)");
    ix->opt_bm = (int)value;
  } else if (k == "bm_candidates") {
    if (value < 0 || value > 7168) return fail(VAQHIP_EINVAL, "bm_candidates must be 0 (default) or 1..7168");
    ix->opt_bm_cap = (int)value;
  } else if (k == "bm_units") {
    if (value < 0 || value > (1 << 20)) return fail(VAQHIP_EINVAL, "bm_units must be 0 (automatic) or a number of work units");
    ix->opt_bm_units = (int)value;
  } else if (k == "bm_queries_per_group") {
    if (value != 0 && value != 2 && value != 4) return fail(VAQHIP_EINVAL, "bm_queries_per_group must be 0, 2 or 4");
    ix->opt_bm_qb = (int)value;
  } else if (k == "bm_waves") {
    if (value != 0 && value != 4 && value != 8 && value != 16) return fail(VAQHIP_EINVAL, "bm_waves must be 0, 4, 8 or 16");
    ix->opt_bm_nwaves = (int)value;
  } else if (k == "seed_thresholds") {
    ix->opt_seed = value != 0;
  } else if (k == "waves_per_workgroup") {
    if (value != 0 && value != 4 && value != 8 && value != 16)
      return fail(VAQHIP_EINVAL, "waves_per_workgroup must be 0, 4, 8 or 16");
    ix->opt_nwaves = (int)value;
  } else {
    return fail(VAQHIP_EINVAL, "unknown option '%s'", key);
  }
  return VAQHIP_OK;
}

int vaqhip_last_timing(vaqhip_index *ix, vaqhip_timing *out) {
  if (!ix || !out) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->ev_used > 0) {
    DeviceGuard g(ix->device);
    double acc[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ix->ev_used; i++) {
      hipEvent_t *ev = ix->ev.data() + (size_t)i * 6;
      HIP_TRY(hipEventSynchronize(ev[5]));
      for (int j = 0; j < 5; j++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[j], ev[j + 1]));
        acc[j] += ms;
      }
    }
    const double n = ix->ev_used;
    ix->last.project_ms = (float)(acc[0] / n);
    ix->last.lut_ms = (float)(acc[1] / n);
    ix->last.seed_ms = (float)(acc[2] / n);
    ix->last.scan_ms = (float)(acc[3] / n);
    ix->last.merge_ms = (float)(acc[4] / n);
    ix->last.n_searches = ix->ev_used;
    ix->ev_used = 0;
    if (ix->last.deferred_queries >= 0 && ix->w_defer.p) {  // (the events above are past: the counter is final)
      unsigned asked = 0;
      HIP_TRY(hipMemcpy(&asked, ix->w_defer.p, sizeof asked, hipMemcpyDeviceToHost));
      ix->last.deferred_queries = ix->last.bucket_major ? (int)asked : (int)std::min<unsigned>(asked, (unsigned)DEFER_CAP);
    }
  }
  *out = ix->last;
  return VAQHIP_OK;
}
} // extern "C"
