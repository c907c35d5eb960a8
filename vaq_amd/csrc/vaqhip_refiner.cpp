// vaqhip_refiner.cpp -- the resident refiner of include/vaqhip.h: the raw rows VAQ::refine reads (VAQ.cpp:849-876)
// kept on the device, the reference-exact re-rank over them (vaq_refine.hip), and the search fused with it.  It sees
// the index through the public ABI only (vaqhip_index_info, vaqhip_search_device): the candidates of a fused call go
// from the search's output buffer straight into the refine kernel and never to the host.  The exhaustive form
// (vaqhip_refiner_search: every resident row a candidate) runs the launches of vaq_exhaust.hip as
// vaqhip_exhaust_plan.h plans them -- the plan and the set of launches it shares with the multi-device refiner.
#include "vaqhip_index.h"

#include "vaqhip_exhaust_plan.h"

#include <string>

using namespace vaqhost;

struct vaqhip_refiner {
  int device = 0, D = 0;
  int64_t N = 0, id_base = 0;
  int64_t cap_rows = 0;  // rows the allocation holds (appends grow it geometrically)
  int opt_exact = 0;
  int opt_splits = 0;  // "exhaustive_splits": 0 = automatic
  int opt_timing = 0;  // "timing": events around the phases of the exhaustive form
  DevBuf d_rows;
  // workspaces of the host forms and of the fused call (grow-only)
  DevBuf w_q, w_lin, w_lout, w_dout, w_cand_l, w_cand_d;
  XsWork xs;  // the exhaustive form's
  vaqhip_refiner_search_timing x_timing = {};
  hipStream_t stream = nullptr;
  // the candidate buffers of the fused _device call are shared by its callers' streams: as on the index, the last
  // enqueue leaves an event and a call on another stream waits for it first
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  std::mutex mu;
};

namespace {

constexpr int REFINE_MAX_R = 2048;
constexpr int HOST_CHUNK = 65536;  // queries per launch of the host forms

struct REntry {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  int rc;
  explicit REntry(vaqhip_refiner *r)
      : lk(r->mu), g(r->device), rc(g.ok ? VAQHIP_OK : fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", r->device)) {}
};
#define RENTRY(r) REntry entry_(r); if (entry_.rc) return entry_.rc

int check_sizes(const vaqhip_refiner *r, int nq, int R, int k) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq < 0 || R <= 0 || k <= 0) return fail(VAQHIP_EINVAL, "bad sizes (nq=%d R=%d k=%d)", nq, R, k);
  if (R > REFINE_MAX_R || k > R) return fail(VAQHIP_EUNSUPPORTED, "need k <= R <= %d (R=%d k=%d)", REFINE_MAX_R, R, k);
  return VAQHIP_OK;
}

int check_labels_fit(int64_t N, int64_t id_base) {
  if (id_base < 0) return fail(VAQHIP_EINVAL, "id_base < 0");
  if (N > 0x7fffffffLL - 1 || id_base + N > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld", (long long)(id_base + N));
  return VAQHIP_OK;
}

// room for `rows` rows; keep != 0: the first r->N rows survive the move
int reserve_rows(vaqhip_refiner *r, int64_t rows, bool keep) {
  if (rows <= r->cap_rows) return VAQHIP_OK;
  const int64_t want = keep ? std::max(rows, r->cap_rows + r->cap_rows / 2) : rows;
  DevBuf nb;
  HIP_TRY(nb.ensure((size_t)want * r->D * sizeof(float)));
  HIP_TRY(hipDeviceSynchronize());  // (a refine enqueued on any stream may still read the old rows)
  if (keep && r->N > 0)
    HIP_TRY(hipMemcpy(nb.p, r->d_rows.p, (size_t)r->N * r->D * sizeof(float), hipMemcpyDeviceToDevice));
  std::swap(nb.p, r->d_rows.p);
  std::swap(nb.cap, r->d_rows.cap);
  r->cap_rows = want;
  return VAQHIP_OK;
}

int refine_locked(vaqhip_refiner *r, const float *d_q, int nq, const int32_t *d_lin, int R, int k, int32_t *d_lout,
                  float *d_dout, hipStream_t st) {
  HIP_TRY(vaq::launch_refine_rows(d_q, nq, r->D, r->d_rows.as<float>(), r->N, r->id_base, d_lin, R, k, r->opt_exact, d_lout,
                                  d_dout, st));
  return VAQHIP_OK;
}

// the index and the refiner of a fused call must describe the same rows on the same device
int check_pair(vaqhip_index *ix, const vaqhip_refiner *r, int R) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (R > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "R=%d > %d (the search returns the candidates)", R, VAQHIP_MAX_K);
  vaqhip_info inf;
  if (int rc = vaqhip_index_info(ix, &inf)) return rc;
  if (inf.device_id != r->device)
    return fail(VAQHIP_EINVAL, "the index is on device %d, the refiner on device %d", inf.device_id, r->device);
  if (inf.D != r->D) return fail(VAQHIP_EINVAL, "the index has D=%d, the refiner D=%d", inf.D, r->D);
  if (inf.N != r->N || inf.id_base != r->id_base)
    return fail(VAQHIP_ESTATE, "the index holds %lld rows from label %lld, the refiner %lld from %lld", (long long)inf.N,
                (long long)inf.id_base, (long long)r->N, (long long)r->id_base);
  return VAQHIP_OK;
}

// search with k = R into the refiner's candidate buffers, refine from there; caller holds r->mu, device current
int search_refine_locked(vaqhip_index *ix, vaqhip_refiner *r, const float *d_q, int nq, int R, int k, int32_t *d_lout,
                         float *d_dout, hipStream_t st) {
  HIP_TRY(r->w_cand_l.ensure((size_t)nq * R * sizeof(int32_t)));
  HIP_TRY(r->w_cand_d.ensure((size_t)nq * R * sizeof(float)));
  if (!r->ws_event) HIP_TRY(hipEventCreateWithFlags(&r->ws_event, hipEventDisableTiming));
  if (r->ws_used && st != r->ws_stream) HIP_TRY(hipStreamWaitEvent(st, r->ws_event, 0));
  int rc = vaqhip_search_device(ix, d_q, nq, R, 0, r->w_cand_l.as<int32_t>(), r->w_cand_d.as<float>(), st);
  if (!rc) rc = refine_locked(r, d_q, nq, r->w_cand_l.as<int32_t>(), R, k, d_lout, d_dout, st);
  if (hipEventRecord(r->ws_event, st) == hipSuccess) {  // (also after a failure: work may be enqueued already)
    r->ws_stream = st;
    r->ws_used = true;
  }
  return rc;
}

// ---- the exhaustive form ----
int check_search(const vaqhip_refiner *r, int nq, int k, const void *a, const void *b, const void *c) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq < 0 || k < 1) return fail(VAQHIP_EINVAL, "bad sizes (nq=%d k=%d)", nq, k);
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (nq > 0 && (!a || !b || !c)) return fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

// all sets of one call, enqueued on st; caller holds r->mu, device current
int search_locked(vaqhip_refiner *r, const float *d_q, int nq, int k, int32_t *d_lout, float *d_dout, hipStream_t st) {
  if (r->cap_rows == 0 && r->N == 0) return fail(VAQHIP_ESTATE, "no rows were set");
  HIP_TRY(r->xs.size_for(r->device, r->D));
  const bool exact = r->opt_exact != 0;
  const int k1 = exact ? k + 1 : k;
  const XsPlan pl = xs_plan(r->xs, r->N, r->opt_splits, nq, k1);
  HIP_TRY(r->xs.fit(pl, k1, exact, r->opt_timing != 0));
  if (!r->ws_event) HIP_TRY(hipEventCreateWithFlags(&r->ws_event, hipEventDisableTiming));
  if (r->ws_used && st != r->ws_stream) HIP_TRY(hipStreamWaitEvent(st, r->ws_event, 0));
  r->x_timing = {};
  r->x_timing.splits = pl.S;
  r->x_timing.register_form = r->D <= (int)vaq::exhaust_register_max_dim();
  const XsRows rows = {r->d_rows.as<float>(), r->N, r->id_base, r->D};
  hipError_t e = hipSuccess;
  for (int q0 = 0; q0 < nq && e == hipSuccess; q0 += pl.chunk)
    e = xs_search_set(r->xs, pl, rows, d_q + (size_t)q0 * r->D, std::min(pl.chunk, nq - q0), k, exact,
                      d_lout + (size_t)q0 * k, d_dout + (size_t)q0 * k, st, r->opt_timing ? &r->x_timing : nullptr);
  const int rc = e == hipSuccess ? VAQHIP_OK
                                 : fail(e == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP, "exhaustive search: %s",
                                        hipGetErrorString(e));
  if (hipEventRecord(r->ws_event, st) == hipSuccess) {  // (also after a failure: work may be enqueued already)
    r->ws_stream = st;
    r->ws_used = true;
  }
  return rc;
}

}  // namespace

extern "C" {

int vaqhip_refiner_create(vaqhip_refiner **out, int device_id, int D) {
  if (!out) return fail(VAQHIP_EINVAL, "out is null");
  *out = nullptr;
  if (D <= 0) return fail(VAQHIP_EINVAL, "D=%d", D);
  if ((size_t)D > vaq::refine_rows_max_dim())
    return fail(VAQHIP_EUNSUPPORTED, "D=%d: the query row must fit the workgroup's LDS (%zu floats)", D,
                vaq::refine_rows_max_dim());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VAQHIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
  if (device_id < 0 || device_id >= ndev) return fail(VAQHIP_EINVAL, "device_id=%d of %d", device_id, ndev);
  vaqhip_refiner *r = new (std::nothrow) vaqhip_refiner();
  if (!r) return fail(VAQHIP_ENOMEM, "host allocation");
  r->device = device_id;
  r->D = D;
  DeviceGuard g(device_id);
  hipError_t e = g.ok ? hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) : hipErrorInvalidDevice;
  if (e != hipSuccess) {
    delete r;
    return fail(VAQHIP_ENODEVICE, "device %d: %s", device_id, hipGetErrorString(e));
  }
  *out = r;
  return VAQHIP_OK;
}

void vaqhip_refiner_destroy(vaqhip_refiner *r) {
  if (!r) return;
  DeviceGuard g(r->device);
  (void)hipDeviceSynchronize();  // (refines enqueued on the callers' streams read the rows)
  if (r->stream) (void)hipStreamDestroy(r->stream);
  if (r->ws_event) (void)hipEventDestroy(r->ws_event);
  r->xs.release();
  delete r;  // every DevBuf goes here, with the refiner's device current
}

int vaqhip_refiner_set_rows_device(vaqhip_refiner *r, const float *d_X, int64_t N, int64_t id_base, void *stream) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (N < 0 || (N > 0 && !d_X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (int rc = check_labels_fit(N, id_base)) return rc;
  RENTRY(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = reserve_rows(r, N, false)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (N > 0) HIP_TRY(hipMemcpyAsync(r->d_rows.p, d_X, (size_t)N * r->D * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  r->N = N;
  r->id_base = id_base;
  return VAQHIP_OK;
}

int vaqhip_refiner_set_rows(vaqhip_refiner *r, const float *X, int64_t N, int64_t id_base) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (N < 0 || (N > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (int rc = check_labels_fit(N, id_base)) return rc;
  RENTRY(r);
  if (int rc = reserve_rows(r, N, false)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (N > 0) HIP_TRY(hipMemcpy(r->d_rows.p, X, (size_t)N * r->D * sizeof(float), hipMemcpyHostToDevice));
  r->N = N;
  r->id_base = id_base;
  return VAQHIP_OK;
}

int vaqhip_refiner_add_rows(vaqhip_refiner *r, const float *X, int64_t n_new) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (n_new < 0 || (n_new > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (n_new == 0) return VAQHIP_OK;
  RENTRY(r);
  if (int rc = check_labels_fit(r->N + n_new, r->id_base)) return rc;
  if (int rc = reserve_rows(r, r->N + n_new, true)) return rc;
  // (rows past N are read by no launch in flight: no wait is needed before they are written)
  HIP_TRY(hipMemcpy(r->d_rows.as<float>() + (size_t)r->N * r->D, X, (size_t)n_new * r->D * sizeof(float),
                    hipMemcpyHostToDevice));
  r->N += n_new;
  return VAQHIP_OK;
}

int vaqhip_refiner_set_option(vaqhip_refiner *r, const char *key, int64_t value) {
  if (!r || !key) return fail(VAQHIP_EINVAL, "null pointer");
  const std::string name(key);
  if (name != "exact_ties" && name != "exhaustive_splits" && name != "timing")
    return fail(VAQHIP_EINVAL, "unknown option '%s'", key);
  if (name == "exhaustive_splits" && (value < 0 || value > 64))  // (refused before the refiner is touched)
    return fail(VAQHIP_EINVAL, "exhaustive_splits=%lld: 0 (automatic) or 1..64", (long long)value);
  std::lock_guard<std::mutex> lk(r->mu);
  if (name == "exact_ties") r->opt_exact = value != 0;
  else if (name == "exhaustive_splits") r->opt_splits = (int)value;
  else r->opt_timing = value != 0;
  return VAQHIP_OK;
}

int vaqhip_refiner_search_device(vaqhip_refiner *r, const float *d_queries, int nq, int k, int32_t *d_labels_out,
                                 float *d_distances_out, void *stream) {
  if (int rc = check_search(r, nq, k, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  RENTRY(r);
  return search_locked(r, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_refiner_search(vaqhip_refiner *r, const float *queries, int nq, int k, int32_t *labels_out,
                          float *distances_out) {
  if (int rc = check_search(r, nq, k, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  RENTRY(r);
  HIP_TRY(r->w_q.ensure((size_t)nq * r->D * sizeof(float)));
  HIP_TRY(r->w_lout.ensure((size_t)nq * k * sizeof(int32_t)));
  HIP_TRY(r->w_dout.ensure((size_t)nq * k * sizeof(float)));
  hipStream_t st = r->stream;
  HIP_TRY(hipMemcpyAsync(r->w_q.p, queries, (size_t)nq * r->D * sizeof(float), hipMemcpyHostToDevice, st));
  if (int rc = search_locked(r, r->w_q.as<float>(), nq, k, r->w_lout.as<int32_t>(), r->w_dout.as<float>(), st)) return rc;
  HIP_TRY(hipMemcpyAsync(labels_out, r->w_lout.p, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(distances_out, r->w_dout.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VAQHIP_OK;
}

int vaqhip_refiner_last_search_timing(vaqhip_refiner *r, vaqhip_refiner_search_timing *out) {
  if (!r || !out) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  *out = r->x_timing;
  return VAQHIP_OK;
}

int vaqhip_refiner_refine_device(vaqhip_refiner *r, const float *d_queries, int nq, const int32_t *d_labels_in, int R,
                                 int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (int rc = check_sizes(r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries || !d_labels_in || !d_labels_out || !d_distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  RENTRY(r);
  return refine_locked(r, d_queries, nq, d_labels_in, R, k, d_labels_out, d_distances_out,
                       static_cast<hipStream_t>(stream));
}

int vaqhip_refiner_refine(vaqhip_refiner *r, const float *queries, int nq, const int32_t *labels_in, int R, int k,
                          int32_t *labels_out, float *distances_out) {
  if (int rc = check_sizes(r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !labels_in || !labels_out || !distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  RENTRY(r);
  const int chunk = std::min(nq, HOST_CHUNK);
  HIP_TRY(r->w_q.ensure((size_t)chunk * r->D * sizeof(float)));
  HIP_TRY(r->w_lin.ensure((size_t)chunk * R * sizeof(int32_t)));
  HIP_TRY(r->w_lout.ensure((size_t)chunk * k * sizeof(int32_t)));
  HIP_TRY(r->w_dout.ensure((size_t)chunk * k * sizeof(float)));
  hipStream_t st = r->stream;
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    HIP_TRY(hipMemcpyAsync(r->w_q.p, queries + (size_t)q0 * r->D, (size_t)n * r->D * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(r->w_lin.p, labels_in + (size_t)q0 * R, (size_t)n * R * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (int rc = refine_locked(r, r->w_q.as<float>(), n, r->w_lin.as<int32_t>(), R, k, r->w_lout.as<int32_t>(),
                               r->w_dout.as<float>(), st))
      return rc;
    HIP_TRY(hipMemcpyAsync(labels_out + (size_t)q0 * k, r->w_lout.p, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(distances_out + (size_t)q0 * k, r->w_dout.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return VAQHIP_OK;
}

int vaqhip_search_refine_device(vaqhip_index *ix, vaqhip_refiner *r, const float *d_queries_raw, int nq, int R, int k,
                                int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (int rc = check_sizes(r, nq, R, k)) return rc;
  RENTRY(r);
  if (int rc = check_pair(ix, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries_raw || !d_labels_out || !d_distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  return search_refine_locked(ix, r, d_queries_raw, nq, R, k, d_labels_out, d_distances_out,
                              static_cast<hipStream_t>(stream));
}

int vaqhip_search_refine(vaqhip_index *ix, vaqhip_refiner *r, const float *queries_raw, int nq, int R, int k,
                         int32_t *labels_out, float *distances_out) {
  if (int rc = check_sizes(r, nq, R, k)) return rc;
  RENTRY(r);
  if (int rc = check_pair(ix, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries_raw || !labels_out || !distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  const int chunk = std::min(nq, HOST_CHUNK);
  HIP_TRY(r->w_q.ensure((size_t)chunk * r->D * sizeof(float)));
  HIP_TRY(r->w_lout.ensure((size_t)chunk * k * sizeof(int32_t)));
  HIP_TRY(r->w_dout.ensure((size_t)chunk * k * sizeof(float)));
  hipStream_t st = r->stream;
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    HIP_TRY(hipMemcpyAsync(r->w_q.p, queries_raw + (size_t)q0 * r->D, (size_t)n * r->D * sizeof(float), hipMemcpyHostToDevice, st));
    if (int rc = search_refine_locked(ix, r, r->w_q.as<float>(), n, R, k, r->w_lout.as<int32_t>(), r->w_dout.as<float>(), st))
      return rc;
    HIP_TRY(hipMemcpyAsync(labels_out + (size_t)q0 * k, r->w_lout.p, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(distances_out + (size_t)q0 * k, r->w_dout.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return VAQHIP_OK;
}

}  // extern "C"
