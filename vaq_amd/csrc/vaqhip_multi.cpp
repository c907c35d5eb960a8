// vaqhip_multi.cpp -- the multi-GPU form of the index behind the C ABI (include/vaqhip.h,
// "multi-device"): SURVEY.md section 8(b) rows 1-3 / 8(e).  This file: its life, its rows and its settings;
// the search is vaqhip_multi_search.cpp, the k-means of clusterTI vaqhip_multi_kmeans.cpp.
//
// One process drives the GPUs of a node, one host thread per device.  The code rows are cut
// into contiguous shards (shard g = rows [g * ceil(N/G), (g+1) * ceil(N/G))), every shard is an
// ordinary vaqhip_index on its device with id_base = its first row, and every setting goes to every shard.
// Shards are contiguous in label order and a single index orders by (distance, label) too, which is what lets
// the search merge the shards' answers into the single-index result bit for bit.
// The reference's precedent for shard-and-merge: BitVecEngine.cpp:1034-1132 (merge :1114-1126).
#include "vaqhip_multi.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

using namespace vaqhost;

static thread_local std::string g_merr;

int vaqhost::mfail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_merr = buf;
  return code;
}

// every shard regroups its own rows under the same centres, all of them at once; mx->mu is held
int vaqhost::set_ti_clusters_on_shards(vaqhip_multi *mx, const float *clusters, int T, int seg_num) {
  return on_shards(mx, [&](int, Shard &s) { return vaqhip_index_set_ti_clusters(s.ix, clusters, T, seg_num); });
}

extern "C" {

const char *vaqhip_multi_last_error(void) { return g_merr.c_str(); }

int vaqhip_multi_create(vaqhip_multi **out, int D, int M, const int *bits, const float *const *centroids,
                        const float *eig, int n_devices, const int *device_ids, unsigned flags) {
  if (!out) return mfail(VAQHIP_EINVAL, "out is null");
  *out = nullptr;
  if (n_devices < 1 || n_devices > VAQHIP_MAX_DEVICES || !device_ids)
    return mfail(VAQHIP_EINVAL, "n_devices=%d outside 1..%d (or no device list)", n_devices, VAQHIP_MAX_DEVICES);
  vaqhip_multi *mx = new (std::nothrow) vaqhip_multi();
  if (!mx) return mfail(VAQHIP_ENOMEM, "host allocation");
  mx->D = D;
  mx->M = M;
  mx->G = n_devices;
  mx->seq = (flags & VAQHIP_SUM_SEQUENTIAL) != 0;
  mx->sh.resize(n_devices);
  for (int g = 0; g < n_devices; g++)
    for (int h = 0; h < g; h++)
      if (device_ids[g] == device_ids[h]) mx->distinct = false;
  for (int g = 0; g < n_devices; g++) {
    Shard &s = mx->sh[g];
    s.device = device_ids[g];
    if (const int rc = forward(vaqhip_index_create_ex(&s.ix, D, M, bits, centroids, eig, s.device, flags))) {
      vaqhip_multi_destroy(mx);
      return rc;
    }
    if (g == 0) mx->bits.assign(bits, bits + M);  // (the first shard's creation has checked bits and M)
    // ("exact_ties" with TI is a property of ONE index: a shard among several keeps the default tie contract)
    if (n_devices > 1) vaqhip_internal_set_sharded(s.ix, 1);
    bool ok = hipSetDevice(s.device) == hipSuccess && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
    if (g == 0) {
      for (auto &e : mx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&mx->user_ready, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&mx->consumed, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&mx->finished, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&mx->flagged, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
      vaqhip_multi_destroy(mx);
      return mfail(VAQHIP_EHIP, "stream / event creation on device %d failed", s.device);
    }
  }
  mx->pool.start(n_devices);
  *out = mx;
  return VAQHIP_OK;
}

void vaqhip_multi_destroy(vaqhip_multi *mx) {
  if (!mx) return;
  mx->pool.stop();
  for (auto &s : mx->sh) {
    (void)hipSetDevice(s.device);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(s.comm);
    for (DevBuf *b : {&s.d_queries, &s.d_packed, &s.d_gathered, &s.d_list, &s.d_state_in, &s.d_state_out}) b->release();
    for (hipEvent_t e : s.link_done) (void)hipEventDestroy(e);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    if (s.ix) vaqhip_index_destroy(s.ix);
  }
  if (!mx->sh.empty()) (void)hipSetDevice(mx->sh[0].device);
  for (DevBuf *b : {&mx->d_out_labels, &mx->d_final, &mx->d_head}) b->release();
  for (auto &e : mx->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {mx->user_ready, mx->consumed, mx->finished, mx->flagged})
    if (e) (void)hipEventDestroy(e);
  delete mx;
}

int vaqhip_multi_set_codes_u16(vaqhip_multi *mx, const uint16_t *codes, int64_t N, int64_t id_base) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (N < 0 || (N > 0 && !codes) || id_base < 0) return mfail(VAQHIP_EINVAL, "bad codes/N/id_base");
  std::lock_guard<std::mutex> lk(mx->mu);
  for (int g = 0; g < mx->G; g++) shard_cut(N, mx->G, g, &mx->sh[g].lo, &mx->sh[g].n);
  // every shard uploads, sorts and packs its rows on its own device, all of them at once
  if (const int rc = on_shards(mx, [&](int, Shard &s) {
        return vaqhip_index_set_codes_u16(s.ix, codes + s.lo * mx->M, s.n, id_base + s.lo);
      }))
    return rc;
  mx->N = N;
  mx->id_base = id_base;
  mx->has_codes = true;
  return VAQHIP_OK;
}

int vaqhip_multi_add_codes_u16(vaqhip_multi *mx, const uint16_t *codes, int64_t n_new) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (n_new < 0 || (n_new > 0 && !codes)) return mfail(VAQHIP_EINVAL, "bad codes/N");
  std::lock_guard<std::mutex> lk(mx->mu);
  // labels are global row numbers and shards are contiguous ranges of them, so new rows (which
  // continue the numbering) extend the LAST shard; set_codes re-balances
  Shard &s = mx->sh[mx->G - 1];
  if (const int rc = forward(vaqhip_index_add_codes_u16(s.ix, codes, n_new))) return rc;
  s.n += n_new;
  mx->N += n_new;
  mx->has_codes = true;
  return VAQHIP_OK;
}

int vaqhip_multi_set_ti_clusters(vaqhip_multi *mx, const float *clusters, int T, int seg_num) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  return set_ti_clusters_on_shards(mx, clusters, T, seg_num);
}

int vaqhip_multi_set_method(vaqhip_multi *mx, unsigned methods, float visit) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  // FAST on its own is taken once every shard holds the SAME quantisation, i.e. after one of the two multi calls
  // that replicate it; before that the index keeps refusing the method, as it always has
  if ((methods & VAQHIP_METHOD_FAST) && !(methods & (VAQHIP_METHOD_TI | VAQHIP_METHOD_EA | VAQHIP_METHOD_HEAP)) && !mx->fast_q)
    return mfail(VAQHIP_EUNSUPPORTED, "method FAST on a multi index needs vaqhip_multi_set_lut_quantization or "
                                      "vaqhip_multi_learn_quantization first");
  return each_shard(mx, [&](vaqhip_index *ix) { return vaqhip_index_set_method(ix, methods, visit); });
}

int vaqhip_multi_set_lut_quantization(vaqhip_multi *mx, const float *offsets, const float *scale) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (!offsets || !scale) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  // every shard quantises its tables by the same map
  if (const int rc = each_shard(mx, [&](vaqhip_index *ix) { return vaqhip_index_set_lut_quantization(ix, offsets, scale); }))
    return rc;
  mx->fast_q = true;
  return VAQHIP_OK;
}

int vaqhip_multi_set_lut_quantiles(vaqhip_multi *mx, const float *quantiles) {
  if (!mx || !quantiles) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  // vaqhip_index_set_lut_quantiles's checks, once, on the host: every shard was created from the same arguments
  constexpr int MAX_Q = 257;
  if (!mx->seq) return mfail(VAQHIP_EINVAL, "quantiles belong to a VAQHIP_SUM_SEQUENTIAL index (BitVecEngine's scalar quantisers)");
  if (mx->D != mx->M) return mfail(VAQHIP_EINVAL, "D=%d != M=%d: the engine has one quantiser per dimension", mx->D, mx->M);
  for (int s = 0; s < mx->M; s++) {
    if (mx->bits[(size_t)s] > 8) return mfail(VAQHIP_EINVAL, "bits[%d]=%d > 8: Q has at most 257 entries", s, mx->bits[(size_t)s]);
    for (int j = 0; j <= (1 << mx->bits[(size_t)s]); j++)
      if (quantiles[(size_t)s * MAX_Q + j] != quantiles[(size_t)s * MAX_Q + j])
        return mfail(VAQHIP_EINVAL, "quantiles[%d][%d] is NaN", s, j);
  }
  DeviceGuard keep(DeviceGuard::restore_only);
  // shard after shard: one that fails leaves those before it with Q (idempotent state: a repeated call heals it)
  if (const int rc = each_shard(mx, [&](vaqhip_index *ix) { return vaqhip_index_set_lut_quantiles(ix, quantiles); })) return rc;
  mx->lut_q = true;
  return VAQHIP_OK;
}

int vaqhip_multi_learn_quantization(vaqhip_multi *mx, const float *X, int64_t n, int projected, float sample_ratio,
                                    float *offsets_out, float *scale_out) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  // learnt once, on shard 0 (every shard holds the same codebooks and rotation, and the rows play no part),
  // then replicated: the values are the single index's, bit for bit
  std::vector<float> off((size_t)mx->M), sc((size_t)mx->M);
  int rc = vaqhip_learn_quantization(mx->sh[0].ix, X, n, projected, sample_ratio, off.data(), sc.data());
  for (int g = 1; !rc && g < mx->G; g++) rc = vaqhip_index_set_lut_quantization(mx->sh[g].ix, off.data(), sc.data());
  if (forward(rc)) return rc;
  mx->fast_q = true;
  if (offsets_out) std::memcpy(offsets_out, off.data(), off.size() * sizeof(float));
  if (scale_out) std::memcpy(scale_out, sc.data(), sc.size() * sizeof(float));
  return VAQHIP_OK;
}

int vaqhip_multi_set_option(vaqhip_multi *mx, const char *key, int64_t value) {
  if (!mx || !key) return mfail(VAQHIP_EINVAL, "null pointer");
  if (std::strcmp(key, "encode_chunk_rows") == 0) return set_encode_chunk_rows(mx, value);
  std::lock_guard<std::mutex> lk(mx->mu);
  if (std::strcmp(key, "exchange") == 0) {
    if (value < 0 || value > 2) return mfail(VAQHIP_EINVAL, "exchange must be 0 (auto), 1 (RCCL) or 2 (copies)");
    if (value == EX_RCCL && !mx->distinct)
      return mfail(VAQHIP_EINVAL, "RCCL needs distinct devices (the list names a GPU twice)");
    mx->exchange = (int)value;
    return VAQHIP_OK;
  }
  if (std::strcmp(key, "exact_batch") == 0) {
    if (value < 0 || value > (1 << 20)) return mfail(VAQHIP_EINVAL, "exact_batch must be 0 (auto) or a number of list entries");
    mx->opt_exact_batch = (int)value;
    return VAQHIP_OK;
  }
  if (const int rc = each_shard(mx, [&](vaqhip_index *ix) { return vaqhip_set_option(ix, key, value); })) return rc;
  // (every shard holds the option too: one shard alone answers by its own replay, and the chain is only
  //  taken where the option has an effect on every shard)
  if (std::strcmp(key, "exact_ties") == 0) mx->opt_exact = value != 0;
  if (std::strcmp(key, "timing") == 0) mx->opt_timing = value != 0;
  return VAQHIP_OK;
}

int vaqhip_multi_get_info(const vaqhip_multi *mx, vaqhip_multi_info *out) {
  if (!mx || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);  // (a search in flight writes these)
  *out = mx->last;
  out->n_devices = mx->G;
  out->N = mx->N;
  out->id_base = mx->id_base;
  for (int g = 0; g < VAQHIP_MAX_DEVICES; g++) {
    out->device_ids[g] = g < mx->G ? mx->sh[g].device : -1;
    out->shard_rows[g] = g < mx->G ? mx->sh[g].n : 0;
  }
  return VAQHIP_OK;
}

vaqhip_index *vaqhip_multi_shard(vaqhip_multi *mx, int g) {
  if (!mx || g < 0 || g >= mx->G) return nullptr;
  return mx->sh[g].ix;
}

} // extern "C"
