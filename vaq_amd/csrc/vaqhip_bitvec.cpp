// vaqhip_bitvec.cpp -- the Hamming engine of include/vaqhip.h: packed bit rows resident on the device,
// BitVecEngine::query with QueryMethod::Sort over them (vaq_bitvec.hip's scan, then FAST's selection: vaq_fast.hip)
// and BitVecEngine::queryRerank over a resident refiner's raw rows (the Hamming candidates stay on the device).
#include "vaqhip_index.h"

#include "vaq_bitvec.h"
#include "vaq_fast.h"
#include "vaqhip_refine_common.h"

using namespace vaqhost;

struct vaqhip_bitvec {
  int device = 0, n_bits = 0, W = 0;
  int64_t N = 0, id_base = 0;
  int64_t dist_chunk_bytes = (int64_t)1 << 30;  // option "dist_chunk_bytes": the distance matrix of a chunk of queries
  RowStore rows;  // uint64 words (elem 8, W a row), room for the rows padded to FAST_ROW_PAD
  // workspaces (grow-only): the distance matrix, FAST's head order and its scratch, the rerank's candidates, the
  // staging of the host forms
  DevBuf w_dist, w_order, w_scratch, w_cand_l, w_cand_d, w_q, w_oq, w_lout, w_dout;
  hipStream_t stream = nullptr;
  // the workspaces are shared by the callers' streams: WS_SCOPE's three members, as on the index
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  std::mutex mu;
};

namespace {

struct BEntry {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  int rc;
  explicit BEntry(vaqhip_bitvec *bv)
      : lk(bv->mu), g(bv->device), rc(g.ok ? VAQHIP_OK : fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", bv->device)) {}
};
#define BENTRY(bv) BEntry entry_(bv); if (entry_.rc) return entry_.rc

int64_t pad_rows(int64_t n) { return std::max<int64_t>(1, (n + vaq::FAST_ROW_PAD - 1) / vaq::FAST_ROW_PAD) * vaq::FAST_ROW_PAD; }

const char *method_name(int m) {
  static const char *names[4] = {"Heap", "Sort", "HeapEarlyAbandon", "SortEarlyAbandon"};
  return names[m];
}

// the refusals of both queries, before any device work; nq == 0 passes (no pointer is looked at)
int check_query(const vaqhip_bitvec *bv, int nq, int k, int method, const void *q, const void *l, const void *d) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (nq < 0 || k < 1) return fail(VAQHIP_EINVAL, "bad sizes (nq=%d k=%d)", nq, k);
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (method < VAQHIP_BITVEC_HEAP || method > VAQHIP_BITVEC_SORT_EARLY_ABANDON)
    return fail(VAQHIP_EINVAL, "method=%d is no QueryMethod", method);
  if (method != VAQHIP_BITVEC_SORT)
    return fail(VAQHIP_EUNSUPPORTED,
                "QueryMethod::%s: it returns the same distances as Sort but keeps other rows among equal ones (its "
                "answer follows from a sequential walk of all rows per query); only QueryMethod::Sort is provided",
                method_name(method));
  if (nq > 0 && (!q || !l || !d)) return fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

// rows [at, at + n) from X (host or device), the padding behind the last row zeroed; the caller has made room
int write_rows(vaqhip_bitvec *bv, const uint64_t *X, int64_t at, int64_t n, bool on_device, hipStream_t st) {
  const size_t rb = (size_t)bv->W * sizeof(uint64_t);
  char *base = bv->rows.buf.as<char>();
  if (n > 0 && on_device) HIP_TRY(hipMemcpyAsync(base + (size_t)at * rb, X, (size_t)n * rb, hipMemcpyDeviceToDevice, st));
  if (on_device) HIP_TRY(hipStreamSynchronize(st));
  if (n > 0 && !on_device) HIP_TRY(hipMemcpy(base + (size_t)at * rb, X, (size_t)n * rb, hipMemcpyHostToDevice));
  const int64_t end = at + n;
  HIP_TRY(hipMemset(base + (size_t)end * rb, 0, (size_t)(pad_rows(end) - end) * rb));
  return VAQHIP_OK;
}

int set_rows_any(vaqhip_bitvec *bv, const uint64_t *X, bool on_device, int64_t n, int64_t id_base, void *stream) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (n < 0 || (n > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (id_base < 0) return fail(VAQHIP_EINVAL, "id_base < 0");
  if (n > 0x7fffffffLL - 1 || id_base + n > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints: id_base+n = %lld", (long long)(id_base + n));
  BENTRY(bv);
  bv->N = 0;  // (a failure below leaves no rows, not rows half replaced)
  HIP_TRY(bv->rows.reserve(pad_rows(n), RowStore::DROP, bv->W));
  HIP_TRY(hipDeviceSynchronize());  // (a query enqueued on any stream may still read the old rows)
  if (int rc = write_rows(bv, X, 0, n, on_device, static_cast<hipStream_t>(stream))) return rc;
  bv->N = n;
  bv->id_base = id_base;
  return VAQHIP_OK;
}

// BitVecEngine::query(queries, k, Sort) for nq queries on the device, enqueued on st inside the caller's workspace
// scope: per chunk of queries the scan, KNNFromDists' std::sort of rows < k, the k best by (dist, seq)
int query_enqueue(vaqhip_bitvec *bv, const uint64_t *d_q, int nq, int k, int32_t *d_labels, float *d_dist, hipStream_t st) {
  const int64_t N = bv->N, n_pad = pad_rows(N);
  const int kk = (int)std::min<int64_t>(k, N);
  const int chunk = (int)std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nq, (int64_t)QUERY_CHUNK, bv->dist_chunk_bytes / (int64_t)sizeof(uint16_t) / n_pad}));
  HIP_TRY(bv->w_dist.ensure((size_t)chunk * n_pad * sizeof(uint16_t)));
  HIP_TRY(bv->w_order.ensure((size_t)chunk * std::max(kk, 1) * sizeof(uint16_t)));
  HIP_TRY(bv->w_scratch.ensure((size_t)chunk * std::max(kk, 1) * sizeof(uint32_t)));
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    if (N > 0) {
      HIP_TRY(vaq::launch_bitvec_scan(bv->rows.buf.as<uint64_t>(), n_pad, bv->W, d_q + (size_t)q0 * bv->W, n,
                                      bv->w_dist.as<uint16_t>(), st));
      HIP_TRY(vaq::launch_fast_head_sort(bv->w_dist.as<uint16_t>(), n_pad, n, kk, bv->w_scratch.as<uint32_t>(),
                                         bv->w_order.as<uint16_t>(), st));
    }
    HIP_TRY(vaq::launch_fast_select(bv->w_dist.as<uint16_t>(), n_pad, N, n, k, vaq::bitvec_select_m(bv->W),
                                    bv->w_order.as<uint16_t>(), bv->id_base, d_labels + (size_t)q0 * k,
                                    d_dist + (size_t)q0 * k, st));
  }
  return VAQHIP_OK;
}

int query_locked(vaqhip_bitvec *bv, const uint64_t *d_q, int nq, int k, int32_t *d_labels, float *d_dist, hipStream_t st) {
  WS_SCOPE(ws, bv, st);
  if (int rc = query_enqueue(bv, d_q, nq, k, d_labels, d_dist, st)) return rc;
  return ws.finish();
}

// what a rerank call must hold before any device work; rv is read under the refiner's lock
int check_rerank(const vaqhip_bitvec *bv, const RefinerView &rv, int k, int factor) {
  if (factor < 1) return fail(VAQHIP_EINVAL, "factor=%d < 1", factor);
  if ((int64_t)factor * k > VAQHIP_MAX_K)
    return fail(VAQHIP_EUNSUPPORTED, "factor * k = %lld > %d candidates per query", (long long)factor * k, VAQHIP_MAX_K);
  if (rv.device != bv->device)
    return fail(VAQHIP_EINVAL, "the bitvec engine is on device %d, the refiner on device %d", bv->device, rv.device);
  if (rv.N != bv->N || rv.id_base != bv->id_base)
    return fail(VAQHIP_ESTATE, "the bitvec engine holds %lld rows from label %lld, the refiner %lld from %lld",
                (long long)bv->N, (long long)bv->id_base, (long long)rv.N, (long long)rv.id_base);
  if ((size_t)rv.D > vaq::bitvec_rerank_max_dim())
    return fail(VAQHIP_EUNSUPPORTED, "D=%d: the query row must fit the workgroup's LDS (%zu floats)", rv.D,
                vaq::bitvec_rerank_max_dim());
  return VAQHIP_OK;
}

// BitVecEngine::queryRerank(..., Sort, earlyAbandonRank = false) on the device, enqueued on st
int rerank_locked(vaqhip_bitvec *bv, const RefinerView &rv, const uint64_t *d_bq, const float *d_oq, int nq, int k, int factor,
                  int32_t *d_labels, float *d_dist, hipStream_t st) {
  const int k_temp = (int)std::min<int64_t>((int64_t)factor * k, bv->N);
  if (k_temp == 0) return query_locked(bv, d_bq, nq, k, d_labels, d_dist, st);  // no rows: every slot -1 / FLT_MAX
  const int chunk = std::min(nq, QUERY_CHUNK);
  HIP_TRY(bv->w_cand_l.ensure((size_t)chunk * k_temp * sizeof(int32_t)));
  HIP_TRY(bv->w_cand_d.ensure((size_t)chunk * k_temp * sizeof(float)));
  WS_SCOPE(ws, bv, st);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    if (int rc = query_enqueue(bv, d_bq + (size_t)q0 * bv->W, n, k_temp, bv->w_cand_l.as<int32_t>(), bv->w_cand_d.as<float>(), st))
      return rc;
    HIP_TRY(vaq::launch_bitvec_rerank(d_oq + (size_t)q0 * rv.D, n, rv.D, rv.rows, rv.N, rv.id_base, bv->w_cand_l.as<int32_t>(),
                                      k_temp, k_temp, k, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return ws.finish();
}

}  // namespace

extern "C" {

int vaqhip_bitvec_create(vaqhip_bitvec **out, int device_id, int n_bits) {
  if (!out) return fail(VAQHIP_EINVAL, "out is null");
  *out = nullptr;
  if (n_bits < 1) return fail(VAQHIP_EINVAL, "n_bits=%d", n_bits);
  const int W = (int)(((int64_t)n_bits + 63) / 64);
  if (W > vaq::BITVEC_MAX_WORDS)
    return fail(VAQHIP_EUNSUPPORTED, "n_bits=%d: at most %d words of 64 bits a row (a distance must fit 16 bits)", n_bits,
                vaq::BITVEC_MAX_WORDS);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VAQHIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
  if (device_id < 0 || device_id >= ndev) return fail(VAQHIP_EINVAL, "device_id=%d of %d", device_id, ndev);
  vaqhip_bitvec *bv = new (std::nothrow) vaqhip_bitvec();
  if (!bv) return fail(VAQHIP_ENOMEM, "host allocation");
  bv->device = device_id;
  bv->n_bits = n_bits;
  bv->W = W;
  bv->rows.elem = (int)sizeof(uint64_t);
  DeviceGuard g(device_id);
  hipError_t e = g.ok ? hipStreamCreateWithFlags(&bv->stream, hipStreamNonBlocking) : hipErrorInvalidDevice;
  if (e != hipSuccess) {
    delete bv;
    return fail(VAQHIP_ENODEVICE, "device %d: %s", device_id, hipGetErrorString(e));
  }
  *out = bv;
  return VAQHIP_OK;
}

void vaqhip_bitvec_destroy(vaqhip_bitvec *bv) {
  if (!bv) return;
  DeviceGuard g(bv->device);
  (void)hipDeviceSynchronize();  // (queries enqueued on the callers' streams read the rows and the workspaces)
  if (bv->stream) (void)hipStreamDestroy(bv->stream);
  if (bv->ws_event) (void)hipEventDestroy(bv->ws_event);
  delete bv;  // every DevBuf goes here, with the engine's device current
}

int vaqhip_bitvec_set_rows(vaqhip_bitvec *bv, const uint64_t *rows, int64_t n, int64_t id_base) {
  return set_rows_any(bv, rows, false, n, id_base, nullptr);
}
int vaqhip_bitvec_set_rows_device(vaqhip_bitvec *bv, const uint64_t *d_rows, int64_t n, int64_t id_base, void *stream) {
  return set_rows_any(bv, d_rows, true, n, id_base, stream);
}

int vaqhip_bitvec_add_rows(vaqhip_bitvec *bv, const uint64_t *rows, int64_t n_new) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (n_new < 0 || (n_new > 0 && !rows)) return fail(VAQHIP_EINVAL, "bad rows");
  if (n_new == 0) return VAQHIP_OK;
  BENTRY(bv);
  if (bv->N + n_new > 0x7fffffffLL - 1 || bv->id_base + bv->N + n_new > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints: id_base+n = %lld", (long long)(bv->id_base + bv->N + n_new));
  HIP_TRY(bv->rows.reserve(pad_rows(bv->N + n_new), bv->N, bv->W));
  // (rows past N are the padding: a query in flight may read them, but no answer depends on what they hold)
  if (int rc = write_rows(bv, rows, bv->N, n_new, false, nullptr)) return rc;
  bv->N += n_new;
  return VAQHIP_OK;
}

int64_t vaqhip_bitvec_size(vaqhip_bitvec *bv) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  std::lock_guard<std::mutex> lk(bv->mu);
  return bv->N;
}

int vaqhip_bitvec_set_option(vaqhip_bitvec *bv, const char *key, int64_t value) {
  if (!bv || !key) return fail(VAQHIP_EINVAL, "null pointer");
  if (std::strcmp(key, "dist_chunk_bytes") != 0) return fail(VAQHIP_EINVAL, "unknown option '%s'", key);
  if (value < 1 || value > ((int64_t)1 << 40)) return fail(VAQHIP_EINVAL, "dist_chunk_bytes=%lld: 1 .. 2^40", (long long)value);
  std::lock_guard<std::mutex> lk(bv->mu);
  bv->dist_chunk_bytes = value;
  return VAQHIP_OK;
}

int vaqhip_bitvec_query_device(vaqhip_bitvec *bv, const uint64_t *d_queries, int nq, int k, int method, int32_t *d_labels_out,
                               float *d_distances_out, void *stream) {
  if (int rc = check_query(bv, nq, k, method, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  BENTRY(bv);
  return query_locked(bv, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_query(vaqhip_bitvec *bv, const uint64_t *queries, int nq, int k, int method, int32_t *labels_out,
                        float *distances_out) {
  if (int rc = check_query(bv, nq, k, method, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  BENTRY(bv);
  hipStream_t st = bv->stream;
  const size_t qb = (size_t)nq * bv->W * sizeof(uint64_t);
  HIP_TRY(bv->w_q.ensure(qb));
  HIP_TRY(bv->w_lout.ensure((size_t)nq * k * sizeof(int32_t)));
  HIP_TRY(bv->w_dout.ensure((size_t)nq * k * sizeof(float)));
  HIP_TRY(hipMemcpyAsync(bv->w_q.p, queries, qb, hipMemcpyHostToDevice, st));
  if (int rc = query_locked(bv, bv->w_q.as<uint64_t>(), nq, k, bv->w_lout.as<int32_t>(), bv->w_dout.as<float>(), st)) return rc;
  HIP_TRY(hipMemcpyAsync(labels_out, bv->w_lout.p, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(distances_out, bv->w_dout.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VAQHIP_OK;
}

int vaqhip_bitvec_query_rerank_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *d_bit_queries,
                                      const float *d_ori_queries, int nq, int k, int factor, int32_t *d_labels_out,
                                      float *d_distances_out, void *stream) {
  if (int rc = check_query(bv, nq, k, VAQHIP_BITVEC_SORT, d_bit_queries, d_labels_out, d_distances_out)) return rc;
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq > 0 && !d_ori_queries) return fail(VAQHIP_EINVAL, "null pointer");
  BENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_rerank(bv, rv, k, factor)) return rc;
  if (nq == 0) return VAQHIP_OK;
  return rerank_locked(bv, rv, d_bit_queries, d_ori_queries, nq, k, factor, d_labels_out, d_distances_out,
                       static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_query_rerank(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *bit_queries, const float *ori_queries,
                               int nq, int k, int factor, int32_t *labels_out, float *distances_out) {
  if (int rc = check_query(bv, nq, k, VAQHIP_BITVEC_SORT, bit_queries, labels_out, distances_out)) return rc;
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq > 0 && !ori_queries) return fail(VAQHIP_EINVAL, "null pointer");
  BENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_rerank(bv, rv, k, factor)) return rc;
  if (nq == 0) return VAQHIP_OK;
  hipStream_t st = bv->stream;
  const size_t qb = (size_t)nq * bv->W * sizeof(uint64_t), ob = (size_t)nq * rv.D * sizeof(float);
  HIP_TRY(bv->w_q.ensure(qb));
  HIP_TRY(bv->w_oq.ensure(ob));
  HIP_TRY(bv->w_lout.ensure((size_t)nq * k * sizeof(int32_t)));
  HIP_TRY(bv->w_dout.ensure((size_t)nq * k * sizeof(float)));
  HIP_TRY(hipMemcpyAsync(bv->w_q.p, bit_queries, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(bv->w_oq.p, ori_queries, ob, hipMemcpyHostToDevice, st));
  if (int rc = rerank_locked(bv, rv, bv->w_q.as<uint64_t>(), bv->w_oq.as<float>(), nq, k, factor, bv->w_lout.as<int32_t>(),
                             bv->w_dout.as<float>(), st))
    return rc;
  HIP_TRY(hipMemcpyAsync(labels_out, bv->w_lout.p, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(distances_out, bv->w_dout.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VAQHIP_OK;
}

}  // extern "C"
