// vaqhip_multi_kmeans.cpp -- vaqhip_multi_cluster_ti_kmeans: the k-means of clusterTI over the shards of a
// multi-device index, and its timing getter.
#include "vaqhip_multi.h"

#include <chrono>
#include <cstring>

#include "kmeans_sample.h"
#include "vaq_kmeans.h"

using namespace vaqhost;

extern "C" {

// The k-means of clusterTI over all rows of the shards ("Across shards"): the sample and
// the seeds are the single index's over rows 0..N-1 in global order; every shard reads its part of the sample
// from its packed rows, the host puts the parts together, the fit runs with the assign step cut over the shards'
// devices (vaq::kmeans_fit), and the centres go to every shard as vaqhip_multi_set_ti_clusters gives them.
int vaqhip_multi_cluster_ti_kmeans(vaqhip_multi *mx, int T, int seg_num, int max_iter, float *clusters_out,
                                   int *iters_out, int *nan_rows_out) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (T < 1 || max_iter < 1) return mfail(VAQHIP_EINVAL, "T=%d max_iter=%d", T, max_iter);
  std::lock_guard<std::mutex> lk(mx->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  const int G = mx->G;
  for (int g = 0; g < G; g++)
    if (const int rc = vaqhip_internal_kmeans_check(mx->sh[g].ix, T, seg_num))
      return mfail(rc, "shard %d (device %d): %s", g, mx->sh[g].device, vaqhip_last_error());
  const int64_t N = mx->N;
  if (T > N)  // (the sample is min(N, 256 * T) rows: never fewer than T unless N is)
    return mfail(VAQHIP_EINVAL, "T=%d centres from %lld rows (the reference reads out of bounds)", T, (long long)N);
  const auto t0 = std::chrono::steady_clock::now();
  const int rows = vaq::kmeans_sample_rows(N, T);
  const bool sampled = N > rows;
  std::vector<int> sample;
  if (sampled) sample = vaq::permutation_head(N, rows);
  int64_t lo[VAQHIP_MAX_DEVICES], cnt[VAQHIP_MAX_DEVICES];
  for (int g = 0; g < G; g++) {
    lo[g] = mx->sh[g].lo;
    cnt[g] = mx->sh[g].n;
  }
  const std::vector<vaq::KmeansShardSample> split = vaq::kmeans_split_sample(sample, lo, cnt, G);

  // gather: every shard its part of the sample, on its own device; the parts meet in sample order on the host
  std::vector<uint16_t> scodes((size_t)rows * seg_num);
  std::vector<std::vector<uint16_t>> piece((size_t)G);
  int rc = on_shards(mx, [&](int g, Shard &s) {
    if (!sampled)  // all rows: the shard's rows lie at sample positions [lo, lo + n)
      return vaqhip_internal_kmeans_gather(s.ix, nullptr, (int)s.n, seg_num, scodes.data() + (size_t)s.lo * seg_num);
    const std::vector<int> &local = split[(size_t)g].local;
    piece[(size_t)g].resize(std::max<size_t>(local.size() * seg_num, 1));
    return vaqhip_internal_kmeans_gather(s.ix, local.data(), (int)local.size(), seg_num, piece[(size_t)g].data());
  });
  if (rc) return rc;
  for (int g = 0; sampled && g < G; g++) {
    const std::vector<int> &pos = split[(size_t)g].pos;
    for (size_t i = 0; i < pos.size(); i++)
      std::memcpy(&scodes[(size_t)pos[i] * seg_num], &piece[(size_t)g][i * seg_num], (size_t)seg_num * sizeof(uint16_t));
  }

  // fit: shard 0's device holds the sample and the centres, every shard's device assigns its slice
  vaq::KmeansDev devs[VAQHIP_MAX_DEVICES];
  int L = 0;
  for (int g = 0; g < G; g++) {
    const void *sub = nullptr;
    if ((rc = forward(vaqhip_internal_kmeans_tables(mx->sh[g].ix, &sub, &devs[g].cent, &L)))) return rc;
    devs[g].device = mx->sh[g].device;
    devs[g].st = mx->sh[g].stream;
    devs[g].sub = static_cast<const vaq::SubDesc *>(sub);
  }
  const int dd = seg_num * L;
  std::vector<float> means((size_t)T * dd);
  const std::vector<int> seeds = vaq::permutation_head(rows, T);
  int iters = 0, no_centre = 0;
  vaq::KmeansPhases ph;
  {
    Shard &s = mx->sh[0];
    auto on0 = [&](hipError_t e, const char *what) {
      return e == hipSuccess ? 0 : mfail(hip_code(e), "shard 0 (device %d): %s: %s", s.device, what, hipGetErrorString(e));
    };
    if ((rc = on0(hipSetDevice(s.device), "hipSetDevice"))) return rc;
    DevBuf d_scodes, d_means;  // (freed with shard 0's device current: kmeans_fit leaves it so)
    if ((rc = on0(d_scodes.ensure(scodes.size() * sizeof(uint16_t)), "sample buffer")) ||
        (rc = on0(d_means.ensure(means.size() * sizeof(float)), "centre buffer")) ||
        (rc = on0(hipMemcpyAsync(d_scodes.p, scodes.data(), scodes.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s.stream),
                  "sample upload")))
      return rc;
    int failed = 0;
    const hipError_t e = vaq::kmeans_fit(devs, G, d_scodes.as<uint16_t>(), rows, seg_num, L, seeds.data(), T, max_iter,
                                         d_means.as<float>(), &iters, &no_centre, mx->opt_timing ? &ph : nullptr, &failed);
    if (e != hipSuccess) {
      (void)hipSetDevice(s.device);
      return mfail(hip_code(e), "shard %d (device %d): k-means: %s", failed, mx->sh[failed].device, hipGetErrorString(e));
    }
    if ((rc = on0(hipMemcpy(means.data(), d_means.p, means.size() * sizeof(float), hipMemcpyDeviceToHost), "centres")))
      return rc;
  }
  mx->km_last = vaqhip_kmeans_timing{};
  mx->km_last.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  mx->km_last.assign_ms = (float)ph.assign_ms;
  mx->km_last.accumulate_ms = (float)ph.accumulate_ms;
  mx->km_last.update_ms = (float)ph.update_ms;
  mx->km_last.iterations = iters;
  mx->km_last.rows = rows;
  mx->km_last.dims = dd;
  mx->km_last.clusters = T;
  if (no_centre)
    return mfail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  if (clusters_out) std::memcpy(clusters_out, means.data(), means.size() * sizeof(float));
  if (iters_out) *iters_out = iters;
  if (nan_rows_out) *nan_rows_out = vaq::nan_rows(means.data(), T, dd);
  return set_ti_clusters_on_shards(mx, means.data(), T, seg_num);
}

int vaqhip_multi_last_kmeans_timing(vaqhip_multi *mx, vaqhip_kmeans_timing *out) {
  if (!mx || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  *out = mx->km_last;
  return VAQHIP_OK;
}

} // extern "C"
