// vaqhip_cluster_index.cpp -- the cluster of every raw row, made on the device (computeClusterIndex,
// utils/Experiment.hpp:372-392): vaqhip_refiner_cluster_index* over a refiner's resident rows, vaqhip_cluster_index*
// over rows that are in none, and vaqhip_bitvec_set_clusters_from_refiner, which assigns and then loads the cluster
// state as vaqhip_bitvec_set_clusters does.  Kernel in vaq_cluster_index.hip, statement in vaq_cluster_index.h.
#include "vaqhip_bitvec.h"

#include "vaq_cluster_index.h"

using namespace vaqhost;

namespace {

constexpr int64_t HOST_CHUNK_ROWS = (int64_t)1 << 20;  // rows per staged piece of the raw host forms

int check_rows(const void *X, int64_t n, const void *idx_out) {
  if (n < 0 || n > 0x7fffffffLL) return fail(VAQHIP_EINVAL, "n=%lld outside 0..2^31 - 1 (a cluster index is one int32 a row)", (long long)n);
  if (n > 0 && (!X || !idx_out)) return fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

// Rows on the device, centres and answer on the host: through the handle's staging on its stream, waited for.  The
// caller holds h->mu with the device current; dist_out may be null.
int assign_to_host(HandleCore *h, StagingBufs &w, vaq::RowsRef rows, int64_t n, int D, const float *centroids, int T,
                   int32_t *idx_out, float *dist_out) {
  const size_t cen_bytes = (size_t)T * D * sizeof(float);
  HIP_TRY(w.oq.ensure(cen_bytes));
  HIP_TRY(w.lout.ensure((size_t)n * sizeof(int32_t)));
  if (dist_out) HIP_TRY(w.dout.ensure((size_t)n * sizeof(float)));
  WS_SCOPE(ws, h, h->stream);
  HIP_TRY(hipMemcpyAsync(w.oq.p, centroids, cen_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(vaq::launch_cluster_index(rows, n, D, w.oq.as<float>(), T, w.lout.as<int32_t>(), dist_out ? w.dout.as<float>() : nullptr,
                                    h->stream));
  HIP_TRY(hipMemcpyAsync(idx_out, w.lout.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out, w.dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ws.finish();
}

// both refiner entries: the centres and the answer are the device's and the work goes on st, or the host's
int refiner_entry(vaqhip_refiner *r, const float *centroids, int T, int32_t *idx_out, float *dist_out, bool on_device,
                  hipStream_t st) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  HandleCore *h = refiner_core(r);
  ENTRY(h);
  const RefinerView rv = refiner_view(r);
  if (int rc = bitvec_check_centres(centroids, T, rv.D)) return rc;
  if (rv.N > 0 && !idx_out) return fail(VAQHIP_EINVAL, "null pointer");
  if (rv.N == 0) return VAQHIP_OK;
  if (!on_device) return assign_to_host(h, refiner_staging(r), rv.rows, rv.N, rv.D, centroids, T, idx_out, dist_out);
  HIP_TRY(vaq::launch_cluster_index(rv.rows, rv.N, rv.D, centroids, T, idx_out, dist_out, st));  // (no workspace: nothing to wait for)
  return VAQHIP_OK;
}

// the four entries over rows that are in no refiner
int raw_entry(int device_id, vaq::RowsRef X, int64_t n, int D, const float *centroids, int T, int32_t *idx_out, float *dist_out,
              bool on_device, hipStream_t st) {
  if (int rc = bitvec_check_centres(centroids, T, D)) return rc;
  if (int rc = check_rows(X.p, n, idx_out)) return rc;
  if (n == 0) return VAQHIP_OK;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  if (on_device) {
    HIP_TRY(vaq::launch_cluster_index(X, n, D, centroids, T, idx_out, dist_out, st));
    return VAQHIP_OK;
  }
  // the host form: the centres once, the rows in staged pieces (a dataset larger than the device goes through in batches)
  const int64_t chunk = std::min(n, HOST_CHUNK_ROWS);
  const size_t row_bytes = (size_t)D * X.elem, cen_bytes = (size_t)T * D * sizeof(float);
  DevBuf d_x, d_cen, d_idx, d_dist;
  HIP_TRY(d_x.ensure((size_t)chunk * row_bytes));
  HIP_TRY(d_cen.ensure(cen_bytes));
  HIP_TRY(d_idx.ensure((size_t)chunk * sizeof(int32_t)));
  if (dist_out) HIP_TRY(d_dist.ensure((size_t)chunk * sizeof(float)));
  CallStream cs;
  HIP_TRY(cs.open());
  HIP_TRY(hipMemcpyAsync(d_cen.p, centroids, cen_bytes, hipMemcpyHostToDevice, cs.s));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t m = std::min(chunk, n - r0);
    HIP_TRY(hipMemcpyAsync(d_x.p, static_cast<const char *>(X.p) + (size_t)r0 * row_bytes, (size_t)m * row_bytes,
                           hipMemcpyHostToDevice, cs.s));
    HIP_TRY(vaq::launch_cluster_index(vaq::RowsRef{d_x.p, X.elem}, m, D, d_cen.as<float>(), T, d_idx.as<int32_t>(),
                                      dist_out ? d_dist.as<float>() : nullptr, cs.s));
    HIP_TRY(hipMemcpyAsync(idx_out + r0, d_idx.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, cs.s));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out + r0, d_dist.p, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, cs.s));
    HIP_TRY(hipStreamSynchronize(cs.s));  // (the next piece overwrites the staging)
  }
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int64_t vaqhip_refiner_size(vaqhip_refiner *r) {
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  std::lock_guard<std::mutex> lk(refiner_mutex(r));
  return refiner_view(r).N;
}

int vaqhip_refiner_cluster_index(vaqhip_refiner *r, const float *centroids, int T, int32_t *clust_idx_out, float *dist_out) {
  return refiner_entry(r, centroids, T, clust_idx_out, dist_out, false, nullptr);
}
int vaqhip_refiner_cluster_index_device(vaqhip_refiner *r, const float *d_centroids, int T, int32_t *d_clust_idx_out,
                                        float *d_dist_out, void *stream) {
  return refiner_entry(r, d_centroids, T, d_clust_idx_out, d_dist_out, true, static_cast<hipStream_t>(stream));
}

int vaqhip_cluster_index(int device_id, const float *X, int64_t n, int D, const float *centroids, int T, int32_t *clust_idx_out,
                         float *dist_out) {
  return raw_entry(device_id, vaq::RowsRef{X, 4}, n, D, centroids, T, clust_idx_out, dist_out, false, nullptr);
}
int vaqhip_cluster_index_u8(int device_id, const uint8_t *X, int64_t n, int D, const float *centroids, int T,
                            int32_t *clust_idx_out, float *dist_out) {
  return raw_entry(device_id, vaq::RowsRef{X, 1}, n, D, centroids, T, clust_idx_out, dist_out, false, nullptr);
}
int vaqhip_cluster_index_device(int device_id, const float *d_X, int64_t n, int D, const float *d_centroids, int T,
                                int32_t *d_clust_idx_out, float *d_dist_out, void *stream) {
  return raw_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, d_centroids, T, d_clust_idx_out, d_dist_out, true,
                   static_cast<hipStream_t>(stream));
}
int vaqhip_cluster_index_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, const float *d_centroids, int T,
                                   int32_t *d_clust_idx_out, float *d_dist_out, void *stream) {
  return raw_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, d_centroids, T, d_clust_idx_out, d_dist_out, true,
                   static_cast<hipStream_t>(stream));
}

int vaqhip_bitvec_set_clusters_from_refiner(vaqhip_bitvec *bv, vaqhip_refiner *r, const float *centroids, int T, int D) {
  if (!bv) return fail(VAQHIP_EINVAL, "bitvec engine is null");
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (int rc = bitvec_check_centres(centroids, T, D)) return rc;
  ENTRY(bv);
  std::lock_guard<std::mutex> rlk(refiner_mutex(r));
  const RefinerView rv = refiner_view(r);
  if (int rc = check_refiner_rows(bv, rv)) return rc;
  if (rv.D != D) return fail(VAQHIP_EINVAL, "the refiner's rows have D=%d, the centres D=%d", rv.D, D);
  std::vector<int32_t> idx((size_t)bv->N);
  if (bv->N > 0)
    if (int rc = assign_to_host(bv, bv->w, rv.rows, rv.N, D, centroids, T, idx.data(), nullptr)) return rc;
  for (int64_t i = 0; i < bv->N; i++)
    if (idx[(size_t)i] < 0)
      return fail(VAQHIP_EINVAL, "row %lld has no centre at a distance below FLT_MAX (a NaN or an overflow in every sum): the "
                  "reference would index clusterMembers[-1]; the cluster state is left as it was", (long long)i);
  return bitvec_set_clusters_locked(bv, centroids, T, D, idx.data());
}

}  // extern "C"
