// vaqhip_bitvec_ti.cpp -- the triangle-inequality form of the Hamming engine's exact queries (include/vaqhip.h):
// vaqhip_bitvec_set_ti_clusters_from_refiner (computeTriangleInequalityClusters: the refiner's rows assigned and grouped
// on the device) and vaqhip_bitvec_query_naive_ti[_device] (queryNaiveTriangleInequality: the plan, then the pruned walk
// over the refiner's raw rows).  Kernels in vaq_bitvec_ti.hip and vaq_cluster_index.hip.
#include "vaqhip_bitvec.h"

#include <climits>

#include "vaq_cluster_index.h"

using namespace vaqhost;

namespace {

// what one buffer of the state becomes once a build has succeeded
void adopt(DevBuf &dst, DevBuf &src) {
  std::swap(dst.p, src.p);
  std::swap(dst.cap, src.cap);
}

// the refusals of a query that need no handle, before any device work; nq == 0 passes (no array is looked at)
int check_ti_query(const vaqhip_bitvec *bv, const vaqhip_refiner *r, int nq, int k, int method, const void *q, const void *l,
                   const void *d) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (nq < 0 || k < 1) return fail(VAQHIP_EINVAL, "bad sizes (nq=%d k=%d)", nq, k);
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (method < VAQHIP_BITVEC_HEAP || method > VAQHIP_BITVEC_SORT_EARLY_ABANDON)
    return fail(VAQHIP_EINVAL, "method=%d is no QueryMethod", method);
  if (method == VAQHIP_BITVEC_SORT)
    return fail(VAQHIP_EUNSUPPORTED, "QueryMethod::Sort: the reference's insertion sort never compares against the last element "
                "while its list fills, so its bound is not the k-th best distance; only QueryMethod::Heap is provided");
  if (method != VAQHIP_BITVEC_HEAP)
    return fail(VAQHIP_EUNSUPPORTED, "the early-abandon methods: queryNaiveTriangleInequality has an empty branch for "
                "HeapEarlyAbandon and none for SortEarlyAbandon; only QueryMethod::Heap is provided");
  if (nq > 0 && (!q || !l || !d)) return fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

// queryNaiveTriangleInequality for nq queries on the device, enqueued on st: per chunk of queries the centres in
// ascending distance, then the pruned walk and the selection in one
int ti_locked(vaqhip_bitvec *bv, const RefinerView &rv, const float *d_oq, int nq, int k, int32_t *d_labels, float *d_dist,
              int64_t *d_eval, hipStream_t st) {
  const BitvecTiClusters &ti = bv->ti;
  const int64_t per_query = (int64_t)ti.T * (sizeof(int32_t) + sizeof(float));
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, (int64_t)QUERY_CHUNK, bv->dist_chunk_bytes / per_query}));
  WS_SCOPE(ws, bv, st);
  HIP_TRY(bv->w_visit.ensure((size_t)chunk * ti.T * sizeof(int32_t)));
  HIP_TRY(bv->w_qcc.ensure((size_t)chunk * ti.T * sizeof(float)));
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    const float *oq = d_oq + (size_t)q0 * ti.D;
    HIP_TRY(vaq::launch_bitvec_ti_plan(oq, n, ti.D, ti.centres_t.as<float>(), ti.T, bv->w_visit.as<int32_t>(),
                                       bv->w_qcc.as<float>(), st));
    HIP_TRY(vaq::launch_bitvec_ti_select(oq, n, ti.D, rv.rows, rv.N, ti.start.as<int32_t>(), ti.member.as<int32_t>(),
                                         ti.xcc.as<float>(), ti.T, bv->w_visit.as<int32_t>(), bv->w_qcc.as<float>(), k,
                                         bv->ti_refresh, bv->id_base, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k,
                                         d_eval ? d_eval + q0 : nullptr, st));
  }
  return ws.finish();
}

// both query entries: the queries and the answer are the device's and the work goes on st, or the host's
int ti_entry(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *ori_queries, int nq, int k, int method, int32_t *labels_out,
             float *distances_out, int64_t *evaluated_out, bool on_device, hipStream_t st) {
  if (int rc = check_ti_query(bv, r, nq, k, method, ori_queries, labels_out, distances_out)) return rc;
  ENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (!bv->ti.set)
    return fail(VAQHIP_ESTATE, "no triangle-inequality state: call vaqhip_bitvec_set_ti_clusters_from_refiner once the rows "
                "are in place (a set or an append of rows drops it)");
  if (int rc = check_refiner_rows(bv, rv)) return rc;
  if (rv.D != bv->ti.D) return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the centres D=%d", rv.D, bv->ti.D);
  if (nq == 0) return VAQHIP_OK;
  if (on_device) return ti_locked(bv, rv, ori_queries, nq, k, labels_out, distances_out, evaluated_out, st);
  StagingBufs &w = bv->w;
  if (evaluated_out) HIP_TRY(bv->w_eval.ensure((size_t)nq * sizeof(int64_t)));
  int64_t *d_eval = evaluated_out ? bv->w_eval.as<int64_t>() : nullptr;
  int rc = 0;
  HIP_TRY(through_staging(w, bv->stream, {{&w.oq, ori_queries, rv.D * sizeof(float)}}, nq, nq, k, labels_out, distances_out, rc,
                          [&](int) {
    return ti_locked(bv, rv, w.oq.as<float>(), nq, k, w.lout.as<int32_t>(), w.dout.as<float>(), d_eval, bv->stream);
  }));
  // (the staging has waited for the stream: the counts are there)
  if (rc == 0 && evaluated_out) HIP_TRY(hipMemcpy(evaluated_out, d_eval, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost));
  return rc;
}

}  // namespace

extern "C" {

int vaqhip_bitvec_set_ti_clusters_from_refiner(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *centroids, int T, int D) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (int rc = bitvec_check_centres(centroids, T, D)) return rc;
  ENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_refiner_rows(bv, rv)) return rc;
  if (rv.D != D) return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the centres D=%d", rv.D, D);
  const int64_t N = bv->N, n1 = std::max<int64_t>(N, 1);
  hipStream_t st = bv->stream;
  // the new state is built beside the old one, which stays if the build is refused
  std::vector<float> centres_t((size_t)D * T);  // dimension-major: lane = centre reads adjacent floats
  for (int c = 0; c < T; c++)
    for (int d = 0; d < D; d++) centres_t[(size_t)d * T + c] = centroids[(size_t)c * D + d];
  const size_t cen_bytes = centres_t.size() * sizeof(float);
  DevBuf n_cen, n_start, n_member, n_xcc, d_cen, d_idx, d_dist, keys_in, keys_out, vals, temp, d_bad;
  HIP_TRY(n_cen.ensure(cen_bytes));
  HIP_TRY(n_start.ensure(((size_t)T + 1) * sizeof(int32_t)));
  HIP_TRY(n_member.ensure((size_t)n1 * sizeof(int32_t)));
  HIP_TRY(n_xcc.ensure((size_t)n1 * sizeof(float)));
  HIP_TRY(d_cen.ensure(cen_bytes));
  HIP_TRY(d_idx.ensure((size_t)n1 * sizeof(int32_t)));
  HIP_TRY(d_dist.ensure((size_t)n1 * sizeof(float)));
  HIP_TRY(keys_in.ensure((size_t)n1 * sizeof(uint64_t)));
  HIP_TRY(keys_out.ensure((size_t)n1 * sizeof(uint64_t)));
  HIP_TRY(vals.ensure((size_t)n1 * sizeof(uint32_t)));
  HIP_TRY(d_bad.ensure(sizeof(int32_t)));
  size_t temp_bytes = 0;
  if (N > 0)
    HIP_TRY(vaq::bitvec_ti_sort(nullptr, temp_bytes, keys_in.as<uint64_t>(), keys_out.as<uint64_t>(), vals.as<uint32_t>(),
                                n_member.as<int32_t>(), N, T, st));
  HIP_TRY(temp.ensure(std::max<size_t>(temp_bytes, 16)));
  int32_t first_bad = INT32_MAX;
  HIP_TRY(hipMemcpyAsync(n_cen.p, centres_t.data(), cen_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_cen.p, centroids, cen_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_bad.p, &first_bad, sizeof(first_bad), hipMemcpyHostToDevice, st));
  // computeClusterIndex's rule, unchanged: the first of the nearest centres by squared distance
  HIP_TRY(vaq::launch_cluster_index(rv.rows, N, D, d_cen.as<float>(), T, d_idx.as<int32_t>(), d_dist.as<float>(), st));
  HIP_TRY(vaq::launch_bitvec_ti_keys(d_idx.as<int32_t>(), d_dist.as<float>(), N, keys_in.as<uint64_t>(), vals.as<uint32_t>(),
                                     d_bad.as<int32_t>(), st));
  HIP_TRY(hipMemcpyAsync(&first_bad, d_bad.p, sizeof(first_bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (first_bad != INT32_MAX)
    return fail(VAQHIP_EINVAL, "row %d has no centre at a distance below FLT_MAX (a NaN or an overflow in every sum): the "
                "reference would give it to centre 0 with no true distance; the triangle-inequality state is left as it was",
                first_bad);
  if (N > 0)
    HIP_TRY(vaq::bitvec_ti_sort(temp.p, temp_bytes, keys_in.as<uint64_t>(), keys_out.as<uint64_t>(), vals.as<uint32_t>(),
                                n_member.as<int32_t>(), N, T, st));
  HIP_TRY(vaq::launch_bitvec_ti_bounds(keys_out.as<uint64_t>(), N, T, n_start.as<int32_t>(), n_xcc.as<float>(), st));
  HIP_TRY(hipDeviceSynchronize());  // (the build is done, and a query enqueued on any stream may still read the old state)
  BitvecTiClusters &ti = bv->ti;
  adopt(ti.centres_t, n_cen);
  adopt(ti.start, n_start);
  adopt(ti.member, n_member);
  adopt(ti.xcc, n_xcc);
  ti.T = T;
  ti.D = D;
  ti.set = true;
  return VAQHIP_OK;
}

int vaqhip_bitvec_query_naive_ti(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *ori_queries, int nq, int k, int method,
                                 int32_t *labels_out, float *distances_out, int64_t *evaluated_out) {
  return ti_entry(bv, r, ori_queries, nq, k, method, labels_out, distances_out, evaluated_out, false, nullptr);
}
int vaqhip_bitvec_query_naive_ti_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *d_ori_queries, int nq, int k,
                                        int method, int32_t *d_labels_out, float *d_distances_out, int64_t *d_evaluated_out,
                                        void *stream) {
  return ti_entry(bv, r, d_ori_queries, nq, k, method, d_labels_out, d_distances_out, d_evaluated_out, true,
                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
