// vaqhip_bitvec.cpp -- the Hamming engine of include/vaqhip.h: packed bit rows resident on the device,
// BitVecEngine::query with QueryMethod::Sort over them (vaq_bitvec.hip's scan, then FAST's selection: vaq_fast.hip)
// and BitVecEngine::queryRerank over a resident refiner's raw rows (the Hamming candidates stay on the device); the
// cluster forms of both (queryWithClusterInfo: vaq_bitvec_clusters.hip's plan and fused scan-and-select); the exact
// cluster form (queryNaiveWithClusterInfo: the same plan, then vaq_bitvec_naive.hip over the refiner's raw rows).
#include "vaqhip_index.h"

#include "vaq_bitvec.h"
#include "vaq_bitvec_naive.h"
#include "vaq_fast.h"
#include "vaqhip_bitvec.h"

using namespace vaqhost;

namespace {

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
  const size_t rb = bv->rows.row_bytes(bv->W);
  HIP_TRY(bv->rows.write(X, at, n, rb, on_device, st));
  const int64_t end = at + n;
  HIP_TRY(hipMemset(bv->rows.buf.as<char>() + (size_t)end * rb, 0, (size_t)(vaq::fast_pad_rows(end) - end) * rb));
  return VAQHIP_OK;
}

int set_rows_any(vaqhip_bitvec *bv, const uint64_t *X, bool on_device, int64_t n, int64_t id_base, void *stream) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (n < 0 || (n > 0 && !X)) return fail(VAQHIP_EINVAL, "bad rows");
  if (id_base < 0) return fail(VAQHIP_EINVAL, "id_base < 0");
  if (n > 0x7fffffffLL - 1 || id_base + n > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints: id_base+n = %lld", (long long)(id_base + n));
  ENTRY(bv);
  bv->N = 0;  // (a failure below leaves no rows, not rows half replaced)
  bv->drop_clusters();
  HIP_TRY(bv->rows.reserve(vaq::fast_pad_rows(n), RowStore::DROP, bv->W));
  HIP_TRY(hipDeviceSynchronize());  // (a query enqueued on any stream may still read the old rows)
  if (int rc = write_rows(bv, X, 0, n, on_device, static_cast<hipStream_t>(stream))) return rc;
  bv->N = n;
  bv->id_base = id_base;
  return VAQHIP_OK;
}

// BitVecEngine::query(queries, k, Sort) for nq queries on the device, enqueued on st inside the caller's workspace
// scope: per chunk of queries the scan, KNNFromDists' std::sort of rows < k, the k best by (dist, seq)
int query_enqueue(vaqhip_bitvec *bv, const uint64_t *d_q, int nq, int k, int32_t *d_labels, float *d_dist, hipStream_t st) {
  const int64_t N = bv->N, n_pad = vaq::fast_pad_rows(N);
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

}  // namespace

// the refiner describes the engine's rows, on the engine's device; rv is read under the refiner's lock
int vaqhost::check_refiner_rows(const vaqhip_bitvec *bv, const RefinerView &rv) {
  if (rv.device != bv->device)
    return fail(VAQHIP_EINVAL, "the bitvec engine is on device %d, the refiner on device %d", bv->device, rv.device);
  if (rv.N != bv->N || rv.id_base != bv->id_base)
    return fail(VAQHIP_ESTATE, "the bitvec engine holds %lld rows from label %lld, the refiner %lld from %lld",
                (long long)bv->N, (long long)bv->id_base, (long long)rv.N, (long long)rv.id_base);
  return VAQHIP_OK;
}

namespace {

// what a rerank call must hold before any device work
int check_rerank(const vaqhip_bitvec *bv, const RefinerView &rv, int k, int factor) {
  if (factor < 1) return fail(VAQHIP_EINVAL, "factor=%d < 1", factor);
  if ((int64_t)factor * k > VAQHIP_MAX_K)
    return fail(VAQHIP_EUNSUPPORTED, "factor * k = %lld > %d candidates per query", (long long)factor * k, VAQHIP_MAX_K);
  if (int rc = check_refiner_rows(bv, rv)) return rc;
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
  HIP_TRY(bv->w.cand_l.ensure((size_t)chunk * k_temp * sizeof(int32_t)));
  HIP_TRY(bv->w.cand_d.ensure((size_t)chunk * k_temp * sizeof(float)));
  WS_SCOPE(ws, bv, st);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    if (int rc = query_enqueue(bv, d_bq + (size_t)q0 * bv->W, n, k_temp, bv->w.cand_l.as<int32_t>(), bv->w.cand_d.as<float>(), st))
      return rc;
    HIP_TRY(vaq::launch_bitvec_rerank(d_oq + (size_t)q0 * rv.D, n, rv.D, rv.rows, rv.N, rv.id_base, bv->w.cand_l.as<int32_t>(),
                                      k_temp, k_temp, k, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return ws.finish();
}

// the host form of a device call: all nq queries at once through the staging on the engine's stream
// (vaqhip_refine_common.h); call() runs from the inputs' buffers into w.lout, w.dout.  Caller holds bv->mu
template <class Call> int through_staging(vaqhip_bitvec *bv, std::initializer_list<StagedInput> inputs, int nq, int k,
                                          int32_t *labels_out, float *distances_out, Call &&call) {
  int rc = 0;
  HIP_TRY(through_staging(bv->w, bv->stream, inputs, nq, nq, k, labels_out, distances_out, rc, [&](int) { return call(); }));
  return rc;
}

// both rerank entries: the queries, labels and distances are the device's and the work goes on st, or the host's
int rerank_entry(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *bit_queries, const float *ori_queries, int nq, int k,
                 int factor, int32_t *labels_out, float *distances_out, bool on_device, hipStream_t st) {
  if (int rc = check_query(bv, nq, k, VAQHIP_BITVEC_SORT, bit_queries, labels_out, distances_out)) return rc;
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq > 0 && !ori_queries) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_rerank(bv, rv, k, factor)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (on_device) return rerank_locked(bv, rv, bit_queries, ori_queries, nq, k, factor, labels_out, distances_out, st);
  StagingBufs &w = bv->w;
  return through_staging(bv, {{&w.q, bit_queries, bv->W * sizeof(uint64_t)}, {&w.oq, ori_queries, rv.D * sizeof(float)}}, nq, k,
                         labels_out, distances_out, [&] {
    return rerank_locked(bv, rv, w.q.as<uint64_t>(), w.oq.as<float>(), nq, k, factor, w.lout.as<int32_t>(), w.dout.as<float>(),
                         bv->stream);
  });
}

// what a cluster query must hold beside check_query's; under the engine's lock
int check_clusters(const vaqhip_bitvec *bv, int atleast) {
  if (!bv->cl.set)
    return fail(VAQHIP_ESTATE, "no cluster state: call vaqhip_bitvec_set_clusters once the rows are in place (a set or an "
                "append of rows drops it)");
  if (atleast < 1 || atleast > bv->cl.T)
    return fail(VAQHIP_EINVAL, "atleast_cluster=%d outside 1..%d (past the centres the reference reads outside its array)",
                atleast, bv->cl.T);
  return VAQHIP_OK;
}

// BitVecEngine::queryWithClusterInfo(queries, oriQueries, k, Sort, atleast) for nq queries on the device, enqueued on
// st inside the caller's workspace scope: per chunk of queries the visiting plan, then the scan and the selection in one
int clusters_enqueue(vaqhip_bitvec *bv, const uint64_t *d_bq, const float *d_oq, int nq, int k, int atleast, int32_t *d_labels,
                     float *d_dist, hipStream_t st) {
  const BitvecClusters &cl = bv->cl;
  const int64_t per_query = (int64_t)cl.T * sizeof(int32_t) + sizeof(vaq::BitvecClusterPlan);
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, (int64_t)QUERY_CHUNK, bv->dist_chunk_bytes / per_query}));
  HIP_TRY(bv->w_visit.ensure((size_t)chunk * cl.T * sizeof(int32_t)));
  HIP_TRY(bv->w_plan.ensure((size_t)chunk * sizeof(vaq::BitvecClusterPlan)));
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    HIP_TRY(vaq::launch_bitvec_cluster_plan(d_oq + (size_t)q0 * cl.D, n, cl.D, cl.centres_t.as<float>(), cl.T,
                                            cl.start.as<int32_t>(), k, atleast, bv->w_visit.as<int32_t>(),
                                            bv->w_plan.as<vaq::BitvecClusterPlan>(), st));
    HIP_TRY(vaq::launch_bitvec_cluster_select(cl.image.as<uint64_t>(), bv->W, cl.start.as<int32_t>(), cl.member.as<int32_t>(),
                                              cl.T, d_bq + (size_t)q0 * bv->W, n, bv->w_visit.as<int32_t>(),
                                              bv->w_plan.as<vaq::BitvecClusterPlan>(), k, bv->id_base,
                                              d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return VAQHIP_OK;
}

// the plain form (rv null) or queryRerankWithClusterInfo(..., Sort, atleast, earlyAbandonRank = false) on the device
int clusters_locked(vaqhip_bitvec *bv, const RefinerView *rv, const uint64_t *d_bq, const float *d_oq, int nq, int k, int factor,
                    int atleast, int32_t *d_labels, float *d_dist, hipStream_t st) {
  const int k_temp = rv ? (int)std::min<int64_t>((int64_t)factor * k, bv->N) : 0;
  if (k_temp == 0) {  // the plain form, or no rows: every slot -1 / FLT_MAX
    WS_SCOPE(ws, bv, st);
    if (int rc = clusters_enqueue(bv, d_bq, d_oq, nq, k, atleast, d_labels, d_dist, st)) return rc;
    return ws.finish();
  }
  const int chunk = std::min(nq, QUERY_CHUNK);
  HIP_TRY(bv->w.cand_l.ensure((size_t)chunk * k_temp * sizeof(int32_t)));
  HIP_TRY(bv->w.cand_d.ensure((size_t)chunk * k_temp * sizeof(float)));
  WS_SCOPE(ws, bv, st);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    if (int rc = clusters_enqueue(bv, d_bq + (size_t)q0 * bv->W, d_oq + (size_t)q0 * rv->D, n, k_temp, atleast,
                                  bv->w.cand_l.as<int32_t>(), bv->w.cand_d.as<float>(), st))
      return rc;
    HIP_TRY(vaq::launch_bitvec_rerank(d_oq + (size_t)q0 * rv->D, n, rv->D, rv->rows, rv->N, rv->id_base, bv->w.cand_l.as<int32_t>(),
                                      k_temp, k_temp, k, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return ws.finish();
}

// all four cluster entries: r null is the plain form; the queries and the answer are the device's, or the host's
int clusters_entry(vaqhip_bitvec *bv, vaqhip_refiner *r, bool rerank, const uint64_t *bit_queries, const float *ori_queries,
                   int nq, int k, int factor, int method, int atleast, int32_t *labels_out, float *distances_out,
                   bool on_device, hipStream_t st) {
  if (int rc = check_query(bv, nq, k, method, bit_queries, labels_out, distances_out)) return rc;
  if (rerank && !r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq > 0 && !ori_queries) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(bv);
  std::unique_lock<std::mutex> rlk;
  RefinerView rv{};
  if (rerank) {
    rlk = std::unique_lock<std::mutex>(refiner_mutex(r));
    rv = refiner_view(r);
    if (int rc = check_rerank(bv, rv, k, factor)) return rc;
  }
  if (int rc = check_clusters(bv, atleast)) return rc;
  if (rerank && rv.D != bv->cl.D)
    return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the centres D=%d", rv.D, bv->cl.D);
  if (nq == 0) return VAQHIP_OK;
  const RefinerView *rvp = rerank ? &rv : nullptr;
  if (on_device)
    return clusters_locked(bv, rvp, bit_queries, ori_queries, nq, k, factor, atleast, labels_out, distances_out, st);
  StagingBufs &w = bv->w;
  return through_staging(bv, {{&w.q, bit_queries, bv->W * sizeof(uint64_t)}, {&w.oq, ori_queries, bv->cl.D * sizeof(float)}}, nq,
                         k, labels_out, distances_out, [&] {
    return clusters_locked(bv, rvp, w.q.as<uint64_t>(), w.oq.as<float>(), nq, k, factor, atleast, w.lout.as<int32_t>(),
                           w.dout.as<float>(), bv->stream);
  });
}

// BitVecEngine::queryNaiveWithClusterInfo(oriQueries, k, Sort, atleast) for nq queries on the device, enqueued on st:
// per chunk of queries the visiting plan, then the exact distances to every member visited and the selection in one
int naive_locked(vaqhip_bitvec *bv, const RefinerView &rv, const float *d_oq, int nq, int k, int atleast, int32_t *d_labels,
                 float *d_dist, hipStream_t st) {
  const BitvecClusters &cl = bv->cl;
  const int64_t per_query = (int64_t)cl.T * sizeof(int32_t) + sizeof(vaq::BitvecClusterPlan);
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, (int64_t)QUERY_CHUNK, bv->dist_chunk_bytes / per_query}));
  WS_SCOPE(ws, bv, st);
  HIP_TRY(bv->w_visit.ensure((size_t)chunk * cl.T * sizeof(int32_t)));
  HIP_TRY(bv->w_plan.ensure((size_t)chunk * sizeof(vaq::BitvecClusterPlan)));
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    const float *oq = d_oq + (size_t)q0 * cl.D;
    HIP_TRY(vaq::launch_bitvec_cluster_plan(oq, n, cl.D, cl.centres_t.as<float>(), cl.T, cl.start.as<int32_t>(), k, atleast,
                                            bv->w_visit.as<int32_t>(), bv->w_plan.as<vaq::BitvecClusterPlan>(), st));
    HIP_TRY(vaq::launch_bitvec_cluster_exact_select(oq, n, cl.D, rv.rows, rv.N, cl.start.as<int32_t>(), cl.member.as<int32_t>(),
                                                    cl.T, bv->w_visit.as<int32_t>(), bv->w_plan.as<vaq::BitvecClusterPlan>(), k,
                                                    bv->id_base, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return ws.finish();
}

// both exact cluster entries: the queries and the answer are the device's and the work goes on st, or the host's
int naive_entry(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *ori_queries, int nq, int k, int method, int atleast,
                int32_t *labels_out, float *distances_out, bool on_device, hipStream_t st) {
  if (int rc = check_query(bv, nq, k, method, ori_queries, labels_out, distances_out)) return rc;
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  ENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_refiner_rows(bv, rv)) return rc;
  if (int rc = check_clusters(bv, atleast)) return rc;
  if (rv.D != bv->cl.D) return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the centres D=%d", rv.D, bv->cl.D);
  if (nq == 0) return VAQHIP_OK;
  if (on_device) return naive_locked(bv, rv, ori_queries, nq, k, atleast, labels_out, distances_out, st);
  StagingBufs &w = bv->w;
  return through_staging(bv, {{&w.oq, ori_queries, rv.D * sizeof(float)}}, nq, k, labels_out, distances_out, [&] {
    return naive_locked(bv, rv, w.oq.as<float>(), nq, k, atleast, w.lout.as<int32_t>(), w.dout.as<float>(), bv->stream);
  });
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
  if (int rc = check_device_id(device_id)) return rc;
  vaqhip_bitvec *bv = new (std::nothrow) vaqhip_bitvec();
  if (!bv) return fail(VAQHIP_ENOMEM, "host allocation");
  bv->n_bits = n_bits;
  bv->W = W;
  bv->rows.elem = (int)sizeof(uint64_t);
  if (int rc = open_handle(bv, device_id)) {
    delete bv;
    return rc;
  }
  *out = bv;
  return VAQHIP_OK;
}

void vaqhip_bitvec_destroy(vaqhip_bitvec *bv) {
  if (!bv) return;
  DeviceGuard g(bv->device);
  (void)hipDeviceSynchronize();  // (queries enqueued on the callers' streams read the rows and the workspaces)
  close_handle(bv);
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
  ENTRY(bv);
  if (bv->N + n_new > 0x7fffffffLL - 1 || bv->id_base + bv->N + n_new > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints: id_base+n = %lld", (long long)(bv->id_base + bv->N + n_new));
  bv->drop_clusters();  // (the cluster state describes the rows as they were)
  HIP_TRY(bv->rows.reserve(vaq::fast_pad_rows(bv->N + n_new), bv->N, bv->W));
  // (rows past N are the padding: a query in flight may read them, but no answer depends on what they hold)
  if (int rc = write_rows(bv, rows, bv->N, n_new, false, nullptr)) return rc;
  bv->N += n_new;
  return VAQHIP_OK;
}

int vaqhip_bitvec_set_clusters(vaqhip_bitvec *bv, const float *centroids, int T, int D, const int32_t *clust_idx) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (!centroids) return fail(VAQHIP_EINVAL, "null pointer");
  if (T < 1 || T > vaq::BITVEC_CLUSTERS_MAX) return fail(VAQHIP_EINVAL, "T=%d centres outside 1..%d", T, vaq::BITVEC_CLUSTERS_MAX);
  if (D < 1 || D > vaq::BITVEC_CLUSTERS_MAX_DIM)
    return fail(VAQHIP_EINVAL, "D=%d outside 1..%d (the refiner's row limit)", D, vaq::BITVEC_CLUSTERS_MAX_DIM);
  ENTRY(bv);
  return bitvec_set_clusters_locked(bv, centroids, T, D, clust_idx);
}

}  // extern "C"

// the body of vaqhip_bitvec_set_clusters behind its refusals of T and D (vaqhip_bitvec.h)
int vaqhost::bitvec_set_clusters_locked(vaqhip_bitvec *bv, const float *centroids, int T, int D, const int32_t *clust_idx) {
  const int64_t N = bv->N, n_pad = vaq::fast_pad_rows(N);
  if (N > 0 && !clust_idx) return fail(VAQHIP_EINVAL, "null pointer");
  // a stable counting sort of the rows by cluster: start[c] is the first image row of cluster c, member[g] the row
  std::vector<int32_t> start((size_t)T + 1, 0), member((size_t)std::max<int64_t>(N, 1));
  for (int64_t i = 0; i < N; i++) {
    if (clust_idx[i] < 0 || clust_idx[i] >= T)
      return fail(VAQHIP_EINVAL, "clust_idx[%lld]=%d outside 0..%d", (long long)i, clust_idx[i], T - 1);
    start[(size_t)clust_idx[i] + 1]++;
  }
  for (int c = 0; c < T; c++) start[(size_t)c + 1] += start[c];
  {
    std::vector<int32_t> next(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < N; i++) member[(size_t)next[clust_idx[i]]++] = (int32_t)i;
  }
  std::vector<float> centres_t((size_t)D * T);  // dimension-major: lane = centre reads adjacent floats
  for (int c = 0; c < T; c++)
    for (int d = 0; d < D; d++) centres_t[(size_t)d * T + c] = centroids[(size_t)c * D + d];
  BitvecClusters &cl = bv->cl;
  HIP_TRY(hipDeviceSynchronize());  // (a query enqueued on any stream may still read the old state)
  cl.set = false;
  HIP_TRY(cl.centres_t.ensure(centres_t.size() * sizeof(float)));
  HIP_TRY(cl.start.ensure(start.size() * sizeof(int32_t)));
  HIP_TRY(cl.member.ensure(member.size() * sizeof(int32_t)));
  HIP_TRY(cl.image.ensure((size_t)n_pad * bv->rows.row_bytes(bv->W)));
  HIP_TRY(hipMemcpy(cl.centres_t.p, centres_t.data(), centres_t.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(cl.start.p, start.data(), start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(cl.member.p, member.data(), member.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(vaq::launch_bitvec_cluster_gather(bv->rows.buf.as<uint64_t>(), cl.member.as<int32_t>(), N, n_pad, bv->W,
                                            cl.image.as<uint64_t>(), bv->stream));
  HIP_TRY(hipStreamSynchronize(bv->stream));
  cl.T = T;
  cl.D = D;
  cl.set = true;
  return VAQHIP_OK;
}

extern "C" {

int64_t vaqhip_bitvec_size(vaqhip_bitvec *bv) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  std::lock_guard<std::mutex> lk(bv->mu);
  return bv->N;
}

int vaqhip_bitvec_set_option(vaqhip_bitvec *bv, const char *key, int64_t value) {
  if (!bv || !key) return fail(VAQHIP_EINVAL, "null pointer");
  const bool refresh = std::strcmp(key, "ti_refresh") == 0;
  if (!refresh && std::strcmp(key, "dist_chunk_bytes") != 0) return fail(VAQHIP_EINVAL, "unknown option '%s'", key);
  if (refresh && (value < 1 || value > vaq::BITVEC_TI_POOL))
    return fail(VAQHIP_EINVAL, "ti_refresh=%lld: 1 .. %d", (long long)value, vaq::BITVEC_TI_POOL);
  if (value < 1 || value > ((int64_t)1 << 40)) return fail(VAQHIP_EINVAL, "dist_chunk_bytes=%lld: 1 .. 2^40", (long long)value);
  std::lock_guard<std::mutex> lk(bv->mu);
  if (refresh) bv->ti_refresh = (int)value;
  else bv->dist_chunk_bytes = value;
  return VAQHIP_OK;
}

int vaqhip_bitvec_query_device(vaqhip_bitvec *bv, const uint64_t *d_queries, int nq, int k, int method, int32_t *d_labels_out,
                               float *d_distances_out, void *stream) {
  if (int rc = check_query(bv, nq, k, method, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  ENTRY(bv);
  return query_locked(bv, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_query(vaqhip_bitvec *bv, const uint64_t *queries, int nq, int k, int method, int32_t *labels_out,
                        float *distances_out) {
  if (int rc = check_query(bv, nq, k, method, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  ENTRY(bv);
  StagingBufs &w = bv->w;
  return through_staging(bv, {{&w.q, queries, bv->W * sizeof(uint64_t)}}, nq, k, labels_out, distances_out, [&] {
    return query_locked(bv, w.q.as<uint64_t>(), nq, k, w.lout.as<int32_t>(), w.dout.as<float>(), bv->stream);
  });
}

int vaqhip_bitvec_query_rerank_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *d_bit_queries,
                                      const float *d_ori_queries, int nq, int k, int factor, int32_t *d_labels_out,
                                      float *d_distances_out, void *stream) {
  return rerank_entry(bv, r, d_bit_queries, d_ori_queries, nq, k, factor, d_labels_out, d_distances_out, true,
                      static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_query_rerank(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *bit_queries, const float *ori_queries,
                               int nq, int k, int factor, int32_t *labels_out, float *distances_out) {
  return rerank_entry(bv, r, bit_queries, ori_queries, nq, k, factor, labels_out, distances_out, false, nullptr);
}

int vaqhip_bitvec_query_clusters(vaqhip_bitvec *bv, const uint64_t *bit_queries, const float *ori_queries, int nq, int k,
                                 int method, int atleast_cluster, int32_t *labels_out, float *distances_out) {
  return clusters_entry(bv, nullptr, false, bit_queries, ori_queries, nq, k, 1, method, atleast_cluster, labels_out,
                        distances_out, false, nullptr);
}
int vaqhip_bitvec_query_clusters_device(vaqhip_bitvec *bv, const uint64_t *d_bit_queries, const float *d_ori_queries, int nq,
                                        int k, int method, int atleast_cluster, int32_t *d_labels_out, float *d_distances_out,
                                        void *stream) {
  return clusters_entry(bv, nullptr, false, d_bit_queries, d_ori_queries, nq, k, 1, method, atleast_cluster, d_labels_out,
                        d_distances_out, true, static_cast<hipStream_t>(stream));
}
int vaqhip_bitvec_query_rerank_clusters(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *bit_queries,
                                        const float *ori_queries, int nq, int k, int factor, int atleast_cluster,
                                        int32_t *labels_out, float *distances_out) {
  return clusters_entry(bv, r, true, bit_queries, ori_queries, nq, k, factor, VAQHIP_BITVEC_SORT, atleast_cluster, labels_out,
                        distances_out, false, nullptr);
}
int vaqhip_bitvec_query_rerank_clusters_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *d_bit_queries,
                                               const float *d_ori_queries, int nq, int k, int factor, int atleast_cluster,
                                               int32_t *d_labels_out, float *d_distances_out, void *stream) {
  return clusters_entry(bv, r, true, d_bit_queries, d_ori_queries, nq, k, factor, VAQHIP_BITVEC_SORT, atleast_cluster,
                        d_labels_out, d_distances_out, true, static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_query_naive_clusters(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *ori_queries, int nq, int k,
                                       int method, int atleast_cluster, int32_t *labels_out, float *distances_out) {
  return naive_entry(bv, r, ori_queries, nq, k, method, atleast_cluster, labels_out, distances_out, false, nullptr);
}
int vaqhip_bitvec_query_naive_clusters_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *d_ori_queries, int nq, int k,
                                              int method, int atleast_cluster, int32_t *d_labels_out, float *d_distances_out,
                                              void *stream) {
  return naive_entry(bv, r, d_ori_queries, nq, k, method, atleast_cluster, d_labels_out, d_distances_out, true,
                     static_cast<hipStream_t>(stream));
}

}  // extern "C"
