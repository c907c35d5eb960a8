// vaqhip_multi_lutfit.cpp -- the sharded quantile fit of include/vaqhip.h (vaqhip_multi_lut_fit_quantiles,
// vaqhip_multi_refiner_lut_fit_quantiles): vaqhip_lut_fit_quantiles's result, bit for bit, with the training rows cut
// over the devices and no device ever holding n x D.
//
// A column's fit is a function of the column SORTED, and a keys-only radix sort does not depend on the order its keys
// arrived in.  So dimension d is owned by device d % G (lutfit_multi_plan.h), and per round of G consecutive dimensions:
//   1 columns  every shard turns its resident rows into the round's column slices of sortable keys, the projection
//              fused (lutfit_project_columns_kernel), into a scratch of G x n_g words
//   2 copy     every shard sends slice w to owner w's key buffer at word lo_g (hipMemcpyPeerAsync; device-to-device
//              where both shards name one GPU)
//   3 fit      every owner runs the single fit's column pipeline on its n keys (lut_fit_column_from_keys: the body
//              lut_fit_columns runs too) into its own slot for that dimension
// Steps 1-2 and step 3 are two phases on the shards' workers (job_pool.h, on_shards): every worker synchronises its
// stream before it reports, and the caller starts a phase only when every shard has succeeded in the one before, so a
// failing shard ends the call and an owner never sorts a buffer that is still being written.  (Round t + 1's columns
// could overlap round t's fit with a second key buffer per owner; not done.)  After the last round the owners' slots
// and every shard's non-finite flag go to the host; the outputs are written only when no flag is set.
// The workers, streams, events and buffers are the call's own: the host form has no handle to keep them in, and the
// refiner form only reads the refiner's rows (r->mu held; set_rows and add_rows copy synchronously).
#include "vaqhip_multi_refiner.h"

#include <chrono>
#include <cstring>

#include "lutfit_multi_plan.h"
#include "vaq_lutfit.h"
#include "vaq_lutfit_dev.h"

using namespace vaqhost;
namespace lf = vaq::lutfit;
namespace lp = vaq::lutfit_plan;

namespace {

thread_local vaqhip_multi_lut_fit_timing g_fit_last = {};

enum { PH_COLUMNS, PH_COPY, PH_SORT, PH_QUANTILE, PH_MEANS, PH_COUNT };

struct FitShard {
  int device = 0;
  std::string err;
  hipStream_t stream = nullptr;
  vaq::RowsRef d_rows = {nullptr, 4};  // the shard's n_g x D rows on its device, float or byte, read in place every round
  DevBuf slice, eig, cols, bad;   // host form: the uploaded rows (n_g x D of the call's element); eigvec; [W][n_g] keys; the non-finite flag
  vaq::LutFitColumnWork work;     // as an owner: the column in flight
  DevBuf cent, q;                 //   and its slots, [slots][256] and [slots][257]
  std::vector<float> h_cent, h_q;
  int h_bad = 0;
  hipEvent_t t[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // columns start, end, copied; the fit's 4
  float ms[PH_COUNT] = {0, 0, 0, 0, 0};  // summed over the rounds
};

// what on_shards runs over: G, pool, sh[] with device and err
struct FitRun {
  int G = 0;
  std::vector<FitShard> sh;
  vaq::JobPool pool;
  lp::Plan plan;
  const int *bits = nullptr;
  vaq::RowsRef X = {nullptr, 4};  // host form: the call's matrix, float or byte
  const float *eig = nullptr;  // host pointer or null
  // by the calling thread, whichever way the call ended: the workers first, then every device's streams and buffers
  ~FitRun() {
    pool.stop();
    for (FitShard &s : sh) {
      if (!s.stream && !s.t[0] && !s.slice.p && !s.eig.p && !s.cols.p && !s.bad.p && !s.work.keys.p && !s.cent.p) continue;
      if (hipSetDevice(s.device) != hipSuccess) continue;
      if (s.stream) (void)hipStreamSynchronize(s.stream);
      release_all({&s.slice, &s.eig, &s.cols, &s.bad, &s.cent, &s.q});
      s.work.release();
      destroy_events(s.t);
      if (s.stream) (void)hipStreamDestroy(s.stream);
    }
  }
};

// the single fit's refusals (vaqhip_lutfit.cpp, check_fit_args) with its codes
int check_fit_args(int64_t n, int D, const int *bits, const void *cent, const void *q) {
  if (!bits || !cent || !q) return mfail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return mfail(VAQHIP_EINVAL, "n=%lld: centroidsQuantile reads Z.front() of an empty column", (long long)n);
  if (n >= ((int64_t)1 << 31)) return mfail(VAQHIP_EINVAL, "n=%lld: the reference counts a bucket in an int", (long long)n);
  if (D < 1) return mfail(VAQHIP_EINVAL, "D=%d", D);
  if (D > 4096) return mfail(VAQHIP_EUNSUPPORTED, "D=%d > 4096", D);
  for (int d = 0; d < D; d++)
    if (bits[d] < 1 || bits[d] > 8) return mfail(VAQHIP_EINVAL, "bits[%d]=%d outside 1..8 (centroidsMat has 256 rows)", d, bits[d]);
  return VAQHIP_OK;
}

// every shard: its stream and events, its rows (host form: uploaded once), eigvec, its scratch; every owner: its buffers
int setup_shard(FitRun &f, int g, FitShard &s) {
  const lp::Plan &p = f.plan;
  const size_t D = (size_t)p.D;
  if (hipSetDevice(s.device) != hipSuccess) {
    s.err = "hipSetDevice failed (no CPU path)";
    return VAQHIP_ENODEVICE;
  }
  MHIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  MHIP(ensure_events(s.t));
  const int64_t n_g = p.cnt[g];
  if (n_g > 0) {
    if (f.X.p) {
      const size_t bytes = (size_t)n_g * D * (size_t)f.X.elem;
      MHIP(s.slice.ensure(bytes));
      MHIP(hipMemcpyAsync(s.slice.p, vaq::rows_at(f.X, (size_t)p.lo[g] * D).p, bytes, hipMemcpyHostToDevice, s.stream));
      s.d_rows = vaq::RowsRef{s.slice.p, f.X.elem};
    }
    if (f.eig) {
      MHIP(s.eig.ensure(D * D * sizeof(float)));
      MHIP(hipMemcpyAsync(s.eig.p, f.eig, D * D * sizeof(float), hipMemcpyHostToDevice, s.stream));
    }
    MHIP(s.cols.ensure((size_t)lp::shard_scratch_words(p, g) * sizeof(uint32_t)));
    MHIP(s.bad.ensure(sizeof(int)));
    MHIP(hipMemsetAsync(s.bad.p, 0, sizeof(int), s.stream));
  }
  const int slots = lp::owned_dims(g, p.D, p.G);
  if (slots > 0) {
    MHIP(s.work.ensure(lp::owner_key_words(p), s.stream));
    MHIP(s.cent.ensure((size_t)slots * lf::MAX_CENT * sizeof(float)));
    MHIP(s.q.ensure((size_t)slots * lf::MAX_Q * sizeof(float)));
    MHIP(hipMemsetAsync(s.cent.p, 0, (size_t)slots * lf::MAX_CENT * sizeof(float), s.stream));  // rows >= N stay 0 (:853)
  }
  MHIP(hipStreamSynchronize(s.stream));
  return 0;
}

// steps 1 and 2 of round t on shard g's worker
int columns_and_copy(FitRun &f, int t, int g, FitShard &s) {
  const lp::Plan &p = f.plan;
  const int64_t n_g = p.cnt[g];
  if (n_g == 0) return 0;  // (an empty shard contributes no word)
  const int d0 = lp::round_first(t, p.G), W = lp::round_width(t, p.D, p.G);
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventRecord(s.t[0], s.stream));
  MHIP(vaq::launch_lutfit_project_columns(s.d_rows, n_g, p.D, f.eig ? s.eig.as<float>() : nullptr, d0, W, s.cols.as<uint32_t>(),
                                          s.bad.as<int>(), s.stream));
  MHIP(hipEventRecord(s.t[1], s.stream));
  for (int w = 0; w < W; w++) {
    FitShard &o = f.sh[(size_t)lp::owner_of(d0 + w, p.G)];
    const uint32_t *src = s.cols.as<uint32_t>() + lp::slice_src_word(p, g, w);
    uint32_t *dst = o.work.keys.as<uint32_t>() + lp::slice_dst_word(p, g);
    const size_t bytes = (size_t)n_g * sizeof(uint32_t);
    if (o.device == s.device) MHIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s.stream));
    else MHIP(hipMemcpyPeerAsync(dst, o.device, src, s.device, bytes, s.stream));
  }
  MHIP(hipEventRecord(s.t[2], s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  float ms = 0.0f;
  MHIP(hipEventElapsedTime(&ms, s.t[0], s.t[1]));
  s.ms[PH_COLUMNS] += ms;
  MHIP(hipEventElapsedTime(&ms, s.t[1], s.t[2]));
  s.ms[PH_COPY] += ms;
  return 0;
}

// step 3 of round t on owner g's worker
int fit_owned_column(FitRun &f, int t, int g, FitShard &s) {
  const lp::Plan &p = f.plan;
  if (g >= lp::round_width(t, p.D, p.G)) return 0;  // (idle this round)
  const int d = lp::round_first(t, p.G) + g;
  MHIP(hipSetDevice(s.device));
  MHIP(vaq::lut_fit_column_from_keys(s.work, p.n, f.bits[d], s.q.as<float>() + (size_t)t * lf::MAX_Q,
                                     s.cent.as<float>() + (size_t)t * lf::MAX_CENT, s.t + 3, s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  for (int ph = 0; ph < 3; ph++) {
    float ms = 0.0f;
    MHIP(hipEventElapsedTime(&ms, s.t[3 + ph], s.t[4 + ph]));
    s.ms[PH_SORT + ph] += ms;
  }
  return 0;
}

// every shard's flag and every owner's slots to the host
int gather_shard(FitRun &f, int g, FitShard &s) {
  const lp::Plan &p = f.plan;
  const int slots = lp::owned_dims(g, p.D, p.G);
  if (p.cnt[g] == 0 && slots == 0) return 0;
  MHIP(hipSetDevice(s.device));
  if (p.cnt[g] > 0) MHIP(hipMemcpyAsync(&s.h_bad, s.bad.p, sizeof(int), hipMemcpyDeviceToHost, s.stream));
  if (slots > 0) {
    s.h_cent.resize((size_t)slots * lf::MAX_CENT);
    s.h_q.resize((size_t)slots * lf::MAX_Q);
    MHIP(hipMemcpyAsync(s.h_cent.data(), s.cent.p, s.h_cent.size() * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    MHIP(hipMemcpyAsync(s.h_q.data(), s.q.p, s.h_q.size() * sizeof(float), hipMemcpyDeviceToHost, s.stream));
  }
  MHIP(hipStreamSynchronize(s.stream));
  return 0;
}

// f.G, f.sh[g].device (and d_rows in the refiner form) and f.plan are set; everything has been refused that can be
int run_fit(FitRun &f, float *centroids_out, float *quantiles_out) {
  const auto t0 = std::chrono::steady_clock::now();
  const lp::Plan &p = f.plan;
  f.pool.start(f.G);
  if (const int rc = on_shards(&f, [&](int g, FitShard &s) { return setup_shard(f, g, s); })) return rc;
  for (int t = 0; t < lp::rounds(p.D, p.G); t++) {
    if (const int rc = on_shards(&f, [&](int g, FitShard &s) { return columns_and_copy(f, t, g, s); })) return rc;
    if (const int rc = on_shards(&f, [&](int g, FitShard &s) { return fit_owned_column(f, t, g, s); })) return rc;
  }
  if (const int rc = on_shards(&f, [&](int g, FitShard &s) { return gather_shard(f, g, s); })) return rc;
  for (const FitShard &s : f.sh)
    if (s.h_bad)
      return mfail(VAQHIP_EINVAL, "a training value is NaN or infinite%s: std::sort has no defined result on it",
                   f.eig ? " after the projection" : "");
  for (int d = 0; d < p.D; d++) {
    const FitShard &o = f.sh[(size_t)lp::owner_of(d, p.G)];
    const size_t slot = (size_t)lp::slot_of(d, p.G);
    std::memcpy(centroids_out + (size_t)d * lf::MAX_CENT, o.h_cent.data() + slot * lf::MAX_CENT, lf::MAX_CENT * sizeof(float));
    std::memcpy(quantiles_out + (size_t)d * lf::MAX_Q, o.h_q.data() + slot * lf::MAX_Q, lf::MAX_Q * sizeof(float));
  }
  vaqhip_multi_lut_fit_timing tm = {};
  for (const FitShard &s : f.sh) {
    tm.columns_ms = std::max(tm.columns_ms, s.ms[PH_COLUMNS]);
    tm.copy_ms = std::max(tm.copy_ms, s.ms[PH_COPY]);
    tm.sort_ms = std::max(tm.sort_ms, s.ms[PH_SORT]);
    tm.quantile_ms = std::max(tm.quantile_ms, s.ms[PH_QUANTILE]);
    tm.means_ms = std::max(tm.means_ms, s.ms[PH_MEANS]);
  }
  tm.rows = p.n;
  tm.dims = p.D;
  tm.n_devices = p.G;
  tm.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_fit_last = tm;
  return VAQHIP_OK;
}

// the host form over float or byte rows: every shard uploads its slice as the elements the caller holds
int fit_host(int n_devices, const int *device_ids, vaq::RowsRef X, int64_t n, int D, const int *bits, const float *eigvec,
             float *centroids_out, float *quantiles_out) {
  if (!X.p || !device_ids) return mfail(VAQHIP_EINVAL, "null pointer");
  if (const int rc = check_fit_args(n, D, bits, centroids_out, quantiles_out)) return rc;
  if (n_devices < 1 || n_devices > VAQHIP_MAX_DEVICES)
    return mfail(VAQHIP_EINVAL, "n_devices=%d outside 1..%d", n_devices, VAQHIP_MAX_DEVICES);
  DeviceGuard keep(DeviceGuard::restore_only);  // (declared first: it puts the device back after f has released)
  FitRun f;
  f.G = n_devices;
  f.sh.resize((size_t)n_devices);
  for (int g = 0; g < n_devices; g++) f.sh[(size_t)g].device = device_ids[g];
  if (!lp::plan_host(n_devices, D, n, &f.plan)) return mfail(VAQHIP_EINVAL, "bad n_devices/D/n");
  f.bits = bits;
  f.X = X;
  f.eig = eigvec;
  return run_fit(f, centroids_out, quantiles_out);
}

}  // namespace

extern "C" {

int vaqhip_multi_lut_fit_quantiles(int n_devices, const int *device_ids, const float *X, int64_t n, int D, const int *bits,
                                   const float *eigvec, float *centroids_out, float *quantiles_out) {
  return fit_host(n_devices, device_ids, vaq::RowsRef{X, 4}, n, D, bits, eigvec, centroids_out, quantiles_out);
}
int vaqhip_multi_lut_fit_quantiles_u8(int n_devices, const int *device_ids, const uint8_t *X, int64_t n, int D,
                                      const int *bits, const float *eigvec, float *centroids_out, float *quantiles_out) {
  return fit_host(n_devices, device_ids, vaq::RowsRef{X, 1}, n, D, bits, eigvec, centroids_out, quantiles_out);
}

int vaqhip_multi_refiner_lut_fit_quantiles(vaqhip_multi_refiner *r, const int *bits, const float *eigvec,
                                           float *centroids_out, float *quantiles_out) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (!bits || !centroids_out || !quantiles_out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return mfail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_multi_refiner_set_rows first");
  if (const int rc = check_fit_args(r->N, r->D, bits, centroids_out, quantiles_out)) return rc;
  DeviceGuard keep(DeviceGuard::restore_only);  // (declared first: it puts the device back after f has released)
  FitRun f;
  f.G = r->G;
  f.sh.resize((size_t)r->G);
  int64_t cnt[VAQHIP_MAX_DEVICES];
  for (int g = 0; g < r->G; g++) {
    const ResidentRows rows = resident_rows(r, g);
    f.sh[(size_t)g].device = r->sh[g].device;
    f.sh[(size_t)g].d_rows = rows.rows;  // (float or byte: the column kernel reads either in place)
    cnt[g] = rows.n;
  }
  if (!lp::plan_from_counts(r->G, r->D, cnt, &f.plan)) return mfail(VAQHIP_EINVAL, "bad shard counts");
  f.bits = bits;
  f.eig = eigvec;
  return run_fit(f, centroids_out, quantiles_out);
}

int vaqhip_multi_last_lut_fit_timing(vaqhip_multi_lut_fit_timing *out) {
  if (!out) return mfail(VAQHIP_EINVAL, "null pointer");
  *out = g_fit_last;
  return VAQHIP_OK;
}

}  // extern "C"
