// vaqhip_refiner.cpp -- the resident refiner of include/vaqhip.h: the raw rows VAQ::refine reads (VAQ.cpp:849-876)
// kept on the device, the reference-exact re-rank over them (vaq_refine.hip), and the search fused with it.  It sees
// the index through the public ABI only (vaqhip_index_info, vaqhip_search_device): the candidates of a fused call go
// from the search's output buffer straight into the refine kernel and never to the host.  The exhaustive form
// (vaqhip_refiner_search: every resident row a candidate) runs the launches of vaq_exhaust.hip as
// vaqhip_exhaust_plan.h plans them -- the plan and the set of launches it shares with the multi-device refiner.
#include "vaqhip_index.h"

#include "vaqhip_refine_common.h"
#include "vaq_exhaust_launch.h"
#include "vaq_refine.h"

using namespace vaqhost;

struct vaqhip_refiner {
  int device = 0, D = 0;
  int64_t N = 0, id_base = 0;
  RefineOptions opt;  // ("timing": around the phases of the exhaustive form)
  RowStore rows;
  StagingBufs w;  // of the host forms and of the fused call (grow-only)
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

namespace vaqhost {
std::mutex &refiner_mutex(vaqhip_refiner *r) { return r->mu; }
RefinerView refiner_view(const vaqhip_refiner *r) { return RefinerView{r->rows.rows(), r->N, r->id_base, r->device, r->D}; }
}  // namespace vaqhost

namespace {

constexpr RefineHost REFINER = {fail, "refiner"};
constexpr int HOST_CHUNK = 65536;  // queries per launch of the host forms

struct REntry {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  int rc;
  explicit REntry(vaqhip_refiner *r)
      : lk(r->mu), g(r->device), rc(g.ok ? VAQHIP_OK : fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", r->device)) {}
};
#define RENTRY(r) REntry entry_(r); if (entry_.rc) return entry_.rc

int refine_locked(vaqhip_refiner *r, const float *d_q, int nq, const int32_t *d_lin, int R, int k, int32_t *d_lout,
                  float *d_dout, hipStream_t st) {
  HIP_TRY(vaq::launch_refine_rows(d_q, nq, r->D, r->rows.rows(), r->N, r->id_base, d_lin, R, k, r->opt.exact, d_lout, d_dout, st));
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
  HIP_TRY(r->w.cand_l.ensure((size_t)nq * R * sizeof(int32_t)));
  HIP_TRY(r->w.cand_d.ensure((size_t)nq * R * sizeof(float)));
  if (!r->ws_event) HIP_TRY(hipEventCreateWithFlags(&r->ws_event, hipEventDisableTiming));
  if (r->ws_used && st != r->ws_stream) HIP_TRY(hipStreamWaitEvent(st, r->ws_event, 0));
  int rc = vaqhip_search_device(ix, d_q, nq, R, 0, r->w.cand_l.as<int32_t>(), r->w.cand_d.as<float>(), st);
  if (!rc) rc = refine_locked(r, d_q, nq, r->w.cand_l.as<int32_t>(), R, k, d_lout, d_dout, st);
  if (hipEventRecord(r->ws_event, st) == hipSuccess) {  // (also after a failure: work may be enqueued already)
    r->ws_stream = st;
    r->ws_used = true;
  }
  return rc;
}

// ---- the exhaustive form ----
// all sets of one call, enqueued on st; caller holds r->mu, device current
int search_locked(vaqhip_refiner *r, const float *d_q, int nq, int k, int32_t *d_lout, float *d_dout, hipStream_t st) {
  if (r->rows.cap_rows == 0 && r->N == 0) return fail(VAQHIP_ESTATE, "no rows were set");
  HIP_TRY(r->xs.size_for(r->device, r->D, r->rows.elem));
  const bool exact = r->opt.exact != 0;
  const int k1 = exact ? k + 1 : k;
  const XsPlan pl = xs_plan(r->xs, r->N, r->opt.splits, nq, k1);
  HIP_TRY(r->xs.fit(pl, k1, exact, r->opt.timing != 0));
  if (!r->ws_event) HIP_TRY(hipEventCreateWithFlags(&r->ws_event, hipEventDisableTiming));
  if (r->ws_used && st != r->ws_stream) HIP_TRY(hipStreamWaitEvent(st, r->ws_event, 0));
  r->x_timing = {};
  r->x_timing.splits = pl.S;
  r->x_timing.register_form = r->D <= (int)vaq::exhaust_register_max_dim();
  const XsRows rows = {r->rows.rows(), r->N, r->id_base, r->D};
  hipError_t e = hipSuccess;
  for (int q0 = 0; q0 < nq && e == hipSuccess; q0 += pl.chunk)
    e = xs_search_set(r->xs, pl, rows, d_q + (size_t)q0 * r->D, std::min(pl.chunk, nq - q0), k, exact,
                      d_lout + (size_t)q0 * k, d_dout + (size_t)q0 * k, st, r->opt.timing ? &r->x_timing : nullptr);
  const int rc = e == hipSuccess ? VAQHIP_OK
                                 : fail(e == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP, "exhaustive search: %s",
                                        hipGetErrorString(e));
  if (hipEventRecord(r->ws_event, st) == hipSuccess) {  // (also after a failure: work may be enqueued already)
    r->ws_stream = st;
    r->ws_used = true;
  }
  return rc;
}

// the host form of a device call on the refiner's stream (vaqhip_refine_common.h); caller holds r->mu
template <class Call> int through_staging(vaqhip_refiner *r, int chunk, const float *queries, int nq, const int32_t *labels_in,
                                          int R, int k, int32_t *labels_out, float *distances_out, Call &&call) {
  int rc = 0;
  HIP_TRY(through_staging(r->w, r->stream, r->D, chunk, queries, nq, labels_in, R, k, labels_out, distances_out, rc, call));
  return rc;
}

// The three row calls, for either element type (elem: 4 or 1).  A set replaces the rows and their type; an append
// keeps the type of the rows there are, and an empty refiner takes either.
int set_rows_any(vaqhip_refiner *r, const void *X, int elem, bool on_device, int64_t N, int64_t id_base, void *stream) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (N < 0 || (N > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (int rc = check_labels_fit(REFINER, N, id_base)) return rc;
  RENTRY(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r->rows.elem != elem) {  // (the rows there are go either way: a failure below leaves none, not rows misread)
    r->N = 0;
    r->rows.retype(elem, r->D);
  }
  HIP_TRY(r->rows.reserve(N, RowStore::DROP, r->D));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = (size_t)N * r->rows.row_bytes(r->D);
  if (N > 0 && on_device) HIP_TRY(hipMemcpyAsync(r->rows.buf.p, X, bytes, hipMemcpyDeviceToDevice, st));
  if (on_device) HIP_TRY(hipStreamSynchronize(st));
  if (N > 0 && !on_device) HIP_TRY(hipMemcpy(r->rows.buf.p, X, bytes, hipMemcpyHostToDevice));
  r->N = N;
  r->id_base = id_base;
  return VAQHIP_OK;
}

int add_rows_any(vaqhip_refiner *r, const void *X, int elem, int64_t n_new) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (n_new < 0 || (n_new > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (n_new == 0) return VAQHIP_OK;
  RENTRY(r);
  if (r->N > 0 && r->rows.elem != elem)
    return fail(VAQHIP_ESTATE, "the refiner holds %s rows: append rows of that type (nothing is converted)",
                r->rows.elem == 1 ? "uint8" : "float32");
  if (int rc = check_labels_fit(REFINER, r->N + n_new, r->id_base)) return rc;
  r->rows.retype(elem, r->D);
  HIP_TRY(r->rows.reserve(r->N + n_new, r->N, r->D));
  // (rows past N are read by no launch in flight: no wait is needed before they are written)
  const size_t rb = r->rows.row_bytes(r->D);
  HIP_TRY(hipMemcpy(r->rows.buf.as<char>() + (size_t)r->N * rb, X, (size_t)n_new * rb, hipMemcpyHostToDevice));
  r->N += n_new;
  return VAQHIP_OK;
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
  return set_rows_any(r, d_X, 4, true, N, id_base, stream);
}
int vaqhip_refiner_set_rows(vaqhip_refiner *r, const float *X, int64_t N, int64_t id_base) {
  return set_rows_any(r, X, 4, false, N, id_base, nullptr);
}
int vaqhip_refiner_add_rows(vaqhip_refiner *r, const float *X, int64_t n_new) { return add_rows_any(r, X, 4, n_new); }

int vaqhip_refiner_set_rows_u8_device(vaqhip_refiner *r, const uint8_t *d_X, int64_t N, int64_t id_base, void *stream) {
  return set_rows_any(r, d_X, 1, true, N, id_base, stream);
}
int vaqhip_refiner_set_rows_u8(vaqhip_refiner *r, const uint8_t *X, int64_t N, int64_t id_base) {
  return set_rows_any(r, X, 1, false, N, id_base, nullptr);
}
int vaqhip_refiner_add_rows_u8(vaqhip_refiner *r, const uint8_t *X, int64_t n_new) { return add_rows_any(r, X, 1, n_new); }

int vaqhip_refiner_elem_size(vaqhip_refiner *r) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  return r->rows.elem;
}

int vaqhip_refiner_set_option(vaqhip_refiner *r, const char *key, int64_t value) {
  return set_option(REFINER, r, key, value);
}

int vaqhip_refiner_search_device(vaqhip_refiner *r, const float *d_queries, int nq, int k, int32_t *d_labels_out,
                                 float *d_distances_out, void *stream) {
  if (int rc = check_search(REFINER, r, nq, k, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  RENTRY(r);
  return search_locked(r, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_refiner_search(vaqhip_refiner *r, const float *queries, int nq, int k, int32_t *labels_out,
                          float *distances_out) {
  if (int rc = check_search(REFINER, r, nq, k, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  RENTRY(r);
  return through_staging(r, nq, queries, nq, nullptr, 0, k, labels_out, distances_out, [&](int n) {
    return search_locked(r, r->w.q.as<float>(), n, k, r->w.lout.as<int32_t>(), r->w.dout.as<float>(), r->stream);
  });
}

int vaqhip_refiner_last_search_timing(vaqhip_refiner *r, vaqhip_refiner_search_timing *out) {
  if (!r || !out) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  *out = r->x_timing;
  return VAQHIP_OK;
}

int vaqhip_refiner_refine_device(vaqhip_refiner *r, const float *d_queries, int nq, const int32_t *d_labels_in, int R,
                                 int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (int rc = check_sizes(REFINER, r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries || !d_labels_in || !d_labels_out || !d_distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  RENTRY(r);
  return refine_locked(r, d_queries, nq, d_labels_in, R, k, d_labels_out, d_distances_out,
                       static_cast<hipStream_t>(stream));
}

int vaqhip_refiner_refine(vaqhip_refiner *r, const float *queries, int nq, const int32_t *labels_in, int R, int k,
                          int32_t *labels_out, float *distances_out) {
  if (int rc = check_sizes(REFINER, r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !labels_in || !labels_out || !distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  RENTRY(r);
  return through_staging(r, std::min(nq, HOST_CHUNK), queries, nq, labels_in, R, k, labels_out, distances_out, [&](int n) {
    return refine_locked(r, r->w.q.as<float>(), n, r->w.lin.as<int32_t>(), R, k, r->w.lout.as<int32_t>(), r->w.dout.as<float>(),
                         r->stream);
  });
}

int vaqhip_search_refine_device(vaqhip_index *ix, vaqhip_refiner *r, const float *d_queries_raw, int nq, int R, int k,
                                int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (int rc = check_sizes(REFINER, r, nq, R, k)) return rc;
  RENTRY(r);
  if (int rc = check_pair(ix, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries_raw || !d_labels_out || !d_distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  return search_refine_locked(ix, r, d_queries_raw, nq, R, k, d_labels_out, d_distances_out,
                              static_cast<hipStream_t>(stream));
}

int vaqhip_search_refine(vaqhip_index *ix, vaqhip_refiner *r, const float *queries_raw, int nq, int R, int k,
                         int32_t *labels_out, float *distances_out) {
  if (int rc = check_sizes(REFINER, r, nq, R, k)) return rc;
  RENTRY(r);
  if (int rc = check_pair(ix, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries_raw || !labels_out || !distances_out) return fail(VAQHIP_EINVAL, "null pointer");
  return through_staging(r, std::min(nq, HOST_CHUNK), queries_raw, nq, nullptr, R, k, labels_out, distances_out, [&](int n) {
    return search_refine_locked(ix, r, r->w.q.as<float>(), n, R, k, r->w.lout.as<int32_t>(), r->w.dout.as<float>(), r->stream);
  });
}

// learnQuantization over the resident rows, read in place as raw rows (vaqhip_learn.cpp does the rest, under the
// index's lock; the refiner's lock keeps the rows where they are meanwhile)
int vaqhip_learn_quantization_from_refiner(vaqhip_index *ix, vaqhip_refiner *r, float sample_ratio, float *offsets_out,
                                           float *scale_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return fail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_refiner_set_rows first");
  vaqhip_info inf;
  if (int rc = vaqhip_index_info(ix, &inf)) return rc;
  if (inf.D != r->D) return fail(VAQHIP_EINVAL, "the index has D=%d, the refiner D=%d", inf.D, r->D);
  if (inf.device_id != r->device)
    return fail(VAQHIP_EINVAL, "the index is on device %d, the refiner on device %d", inf.device_id, r->device);
  // (set_rows and add_rows copy synchronously: the rows are complete)
  return learn_rows_device(ix, r->rows.rows(), r->N, 0, sample_ratio, offsets_out, scale_out);
}

// the subspace codebooks over the resident rows, read in place, by any form of the fit (vaqhip_codebooks.cpp does the
// rest; the refiner's lock keeps the rows where they are meanwhile)
static int refiner_fit_codebooks(CodebookForm form, vaqhip_refiner *r, int M, const int *bits, const float *eigvec, int max_iter,
                                 float *centroids_out, int *iters_out, int *nan_rows_out) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return fail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_refiner_set_rows first");
  // (set_rows and add_rows copy synchronously: the rows are complete)
  return fit_codebooks_rows_device(form, r->device, r->rows.rows(), r->N, r->D, M, bits, eigvec, max_iter, centroids_out,
                                   iters_out, nan_rows_out);
}
int vaqhip_refiner_fit_codebooks(vaqhip_refiner *r, int M, const int *bits, const float *eigvec, int max_iter,
                                 float *centroids_out, int *iters_out, int *nan_rows_out) {
  return refiner_fit_codebooks(CodebookForm::FLAT, r, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
// the hierarchical form of the same (subspaces above 8 bits in two stages)
int vaqhip_refiner_fit_codebooks_hier(vaqhip_refiner *r, int M, const int *bits, const float *eigvec, int max_iter,
                                      float *centroids_out, int *iters_out, int *nan_rows_out) {
  return refiner_fit_codebooks(CodebookForm::HIER, r, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
// the binary-tree form of the same (subspaces above 8 bits as a tree of 2-centre fits)
int vaqhip_refiner_fit_codebooks_bin(vaqhip_refiner *r, int M, const int *bits, const float *eigvec, int max_iter,
                                     float *centroids_out, int *iters_out, int *nan_rows_out) {
  return refiner_fit_codebooks(CodebookForm::BIN, r, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

// the training front half over the resident rows, read in place (vaqhip_train.cpp does the rest)
int vaqhip_refiner_train_moment(vaqhip_refiner *r, double *cov_out, float *cov_f_out) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return fail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_refiner_set_rows first");
  return train_moment_rows_device(r->device, r->rows.rows(), r->N, r->D, cov_out, cov_f_out);
}

int vaqhip_refiner_train_rotation(vaqhip_refiner *r, int M, int bit_budget, int min_bits, int max_bits, float percent_var,
                                  float *eigvec_out, float *eigenvalues_out, int *bits_out, int *highest_subs_out) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return fail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_refiner_set_rows first");
  return train_rotation_rows_device(r->device, r->rows.rows(), r->N, r->D, M, bit_budget, min_bits, max_bits, percent_var,
                                    eigvec_out, eigenvalues_out, bits_out, highest_subs_out);
}

}  // extern "C"
