// vaqhip_multi_lutfit.cpp -- the sharded quantile fit of include/vaqhip.h (vaqhip_multi_lut_fit_quantiles,
// vaqhip_multi_refiner_lut_fit_quantiles): vaqhip_lut_fit_quantiles's result, bit for bit, with the training rows cut
// over the devices and no device ever holding n x D.
//
// A column's fit is a function of the column SORTED, and a keys-only radix sort does not depend on the order its keys
// arrived in.  So dimension d is owned by device d % G (lutfit_multi_plan.h), and per round of G consecutive dimensions:
//   1 columns  every shard turns its resident rows into the round's column slices of sortable keys, the projection
//              fused (lutfit_project_columns_kernel), into a scratch of G x n_g words
//   2 copy     every shard sends slice w to owner w's key buffer at word lo_g (copy_between, vaqhip_multi.h)
//   3 fit      every owner runs the single fit's column pipeline on its n keys (lut_fit_column_from_keys: the body
//              lut_fit_columns runs too) into its own slot for that dimension
// Steps 1-2 and step 3 are two phases on the shards' workers (job_pool.h, on_shards): every worker synchronises its
// stream before it reports, and the caller starts a phase only when every shard has succeeded in the one before, so a
// failing shard ends the call and an owner never sorts a buffer that is still being written.  (Round t + 1's columns
// could overlap round t's fit with a second key buffer per owner; not done.)  After the last round the owners' slots
// and every shard's non-finite flag go to the host; the outputs are written only when no flag is set.
// The workers, streams, events and buffers are the call's own (vaqhip_shard_run.h: the run, the start of a shard's
// setup and the teardown): the host form has no handle to keep them in, and the refiner form only reads the refiner's
// rows (r->mu held; set_rows and add_rows copy synchronously).  What is here is the plan, the phases and the gather.
#include "vaqhip_shard_run.h"

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

struct FitShard : RunShard {
  DevBuf cols, bad;               // [W][n_g] keys; the non-finite flag
  vaq::LutFitColumnWork work;     // as an owner: the column in flight
  DevBuf cent, q;                 //   and its slots, [slots][256] and [slots][257]
  std::vector<float> h_cent, h_q;
  int h_bad = 0;
  hipEvent_t t[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // columns start, end, copied; the fit's 4
  float ms[PH_COUNT] = {0, 0, 0, 0, 0};  // summed over the rounds
  void release() { release_all({&cols, &bad, &cent, &q}), work.release(), destroy_events(t); }
};

// the call's run (vaqhip_shard_run.h) with what this fit adds
struct FitRun : ShardRun<FitShard> {
  lp::Plan plan;
  const int *bits = nullptr;
};

// every shard: its stream and events, its rows (host form: uploaded once), eigvec, its scratch; every owner: its buffers
int setup_shard(FitRun &f, int g, FitShard &s) {
  const lp::Plan &p = f.plan;
  const int64_t n_g = p.cnt[g];
  if (const int rc = f.open(s, p.lo[g], n_g, p.D)) return rc;
  MHIP(ensure_events(s.t));
  if (n_g > 0) {
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
    MHIP(copy_between(dst, o.device, src, s.device, (size_t)n_g * sizeof(uint32_t), s.stream));
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
  tm.columns_ms = f.max_ms(PH_COLUMNS);
  tm.copy_ms = f.max_ms(PH_COPY);
  tm.sort_ms = f.max_ms(PH_SORT);
  tm.quantile_ms = f.max_ms(PH_QUANTILE);
  tm.means_ms = f.max_ms(PH_MEANS);
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
  if (const int rc = forward(vaqhip_internal_lut_fit_check(X.p, n, D, bits, centroids_out, quantiles_out))) return rc;
  FitRun f;
  if (const int rc = f.from_devices(n_devices, device_ids)) return rc;
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
  // (the rows are the refiner's: any non-null pointer stands for them in the single fit's checks)
  if (const int rc = forward(vaqhip_internal_lut_fit_check(r, r->N, r->D, bits, centroids_out, quantiles_out))) return rc;
  FitRun f;
  int64_t cnt[VAQHIP_MAX_DEVICES];
  f.from_refiner(r, cnt);  // (float or byte rows: the column kernel reads either in place)
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
