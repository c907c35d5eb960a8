// vaqhip_multi_codebooks.cpp -- the sharded codebook fit of include/vaqhip.h (vaqhip_multi_fit_codebooks[_u8],
// vaqhip_multi_refiner_fit_codebooks): vaqhip_fit_codebooks's result, bit for bit, with the training rows cut over the
// devices and no device ever holding n x D rows, nor a projected copy of them.
//
// No value of subspace s is computed from another subspace's, so every subspace has one owner device
// (fit_codebooks_multi_plan.h) and an owner fits its subspaces alone, over a compact matrix of just their columns:
//   1 columns  every shard writes, per owner, the packed [rows it contributes][D_w] block of that owner's columns
//              (launch_codebook_columns: a byte widened where it is loaded, the projection fused as one fmaf chain per
//              value) -- its rows of the sample, or all of its rows for an owner of a subspace that does not sample
//   2 copy     every shard sends each block to its owner (copy_between, vaqhip_multi.h): a block of all rows to row
//              lo_g of the owner's n x D_w matrix, a sample block to the owner's staging area behind the blocks of the
//              shards before it
//   3 fit      every owner places the staged rows at their positions in its sample matrix (an owner that holds all rows
//              gathers the sample of its other subspaces from them instead, as the single fit does) and runs the single
//              fit from there on, unchanged: vaq::codebooks_lloyd with D = D_w, its sub-plan and no eigvec
// Steps 1-2 and step 3 are two phases on the shards' workers (job_pool.h, on_shards): every worker synchronises its
// stream before it reports, and the caller starts a phase only when every shard has succeeded in the one before, so a
// failing shard ends the call and an owner never reads a matrix that is still being written.  The outputs are written
// only when every owner has succeeded and no row was left without a centre.
// The workers, streams, events and buffers are the call's own (vaqhip_shard_run.h: the run, the start of a shard's
// setup and the teardown): the host form has no handle to keep them in, and the refiner form only reads the refiner's
// rows (r->mu held; set_rows and add_rows copy synchronously).  What is here is the plan, the sample a host form picks,
// the phases and the outputs.
// One device (G == 1) is the single fit itself; there is no exchange.
#include "vaqhip_shard_run.h"

#include <chrono>
#include <cstring>

#include "fit_codebooks_multi_plan.h"
#include "vaq_codebooks.h"

using namespace vaqhost;
namespace cm = vaq::cbfit_multi;
namespace cb = vaq::cbfit;

namespace {

thread_local vaqhip_multi_fit_codebooks_timing g_cbm_last = {};

enum { PH_COLUMNS, PH_COPY, PH_PLACE, PH_COUNT };

struct CbShard : RunShard {
  bool picked = false;         // host form, every subspace samples: d_rows are its sample rows, in sample order
  DevBuf subs, local, blocks;  // the owners' subspaces [M]; local rows; packed blocks
  // as an owner: the sample and full matrices, the staging area with its positions, the permutation head an owner of all
  // rows gathers by, the centres
  DevBuf Ps, Pf, stage, pos, perm, means;
  std::vector<float> h_means;
  std::vector<int> iters;
  int no_centre = 0;
  vaq::CodebookPhases ph;
  hipEvent_t t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // columns start, end, copied; place start, end
  float ms[PH_COUNT] = {0, 0, 0};
  void release() { release_all({&subs, &local, &blocks, &Ps, &Pf, &stage, &pos, &perm, &means}), destroy_events(t); }
};

// the call's run (vaqhip_shard_run.h) with what this fit adds
struct CbRun : ShardRun<CbShard> {
  cm::Plan plan;
  int D = 0, max_iter = 0;
  int sub_at[VAQHIP_MAX_DEVICES + 1] = {};  // where owner w's subspaces start in the list every shard holds
  bool timing = false;
};

// (declared behind the host memory a stream copies from: the stream is idle before that memory goes, on every return)
struct SyncOnLeave {
  hipStream_t &st;
  ~SyncOnLeave() {
    if (st) (void)hipStreamSynchronize(st);
  }
};

// every shard: its stream and events, its rows (host form: uploaded once), eigvec, the lists, its blocks; every owner:
// its matrices
int setup_shard(CbRun &f, int g, CbShard &s) {
  const cm::Plan &p = f.plan;
  const cm::ShardPart &sp = p.shard[(size_t)g];
  std::vector<char> picked_rows;  // the sample rows a host form picks, and
  std::vector<int> list;          //   an owner's positions: the host's until the stream is synchronised
  SyncOnLeave idle_on_return{s.stream};
  // every subspace samples: only this slice's rows of the sample go up, in the sample's order
  s.picked = f.X.p && p.whole.sampled && sp.cnt > 0;
  if (const int rc = f.open(s, sp.lo, sp.cnt, f.D, !s.picked)) return rc;
  MHIP(ensure_events(s.t));
  if (sp.cnt > 0) {
    if (s.picked) {
      const size_t row_bytes = (size_t)f.D * (size_t)f.X.elem;
      picked_rows.resize(std::max<size_t>(sp.local.size() * row_bytes, 1));
      const char *base = static_cast<const char *>(f.X.p) + (size_t)sp.lo * row_bytes;
      for (size_t i = 0; i < sp.local.size(); i++)
        std::memcpy(picked_rows.data() + i * row_bytes, base + (size_t)sp.local[i] * row_bytes, row_bytes);
      MHIP(s.slice.ensure(picked_rows.size()));
      if (!sp.local.empty())
        MHIP(hipMemcpyAsync(s.slice.p, picked_rows.data(), sp.local.size() * row_bytes, hipMemcpyHostToDevice, s.stream));
      s.d_rows = vaq::RowsRef{s.slice.p, f.X.elem};
    }
    std::vector<int> subs;
    for (const cm::Owner &o : p.owner) subs.insert(subs.end(), o.subs.begin(), o.subs.end());
    MHIP(s.subs.ensure(subs.size() * sizeof(int)));
    MHIP(hipMemcpy(s.subs.p, subs.data(), subs.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!s.picked && !sp.local.empty()) {
      MHIP(s.local.ensure(sp.local.size() * sizeof(int)));
      MHIP(hipMemcpyAsync(s.local.p, sp.local.data(), sp.local.size() * sizeof(int), hipMemcpyHostToDevice, s.stream));
    }
    MHIP(s.blocks.ensure(std::max<size_t>((size_t)cm::scratch_floats(p, g) * sizeof(float), 16)));
  }
  const cm::Owner &o = p.owner[(size_t)g];
  if (!o.idle()) {
    const size_t Dw = (size_t)o.D_w, S = (size_t)o.plan.gathered;
    MHIP(s.means.ensure((size_t)o.plan.n_cent * p.L * sizeof(float)));
    if (S > 0) MHIP(s.Ps.ensure(S * Dw * sizeof(float)));
    if (o.full()) {
      MHIP(s.Pf.ensure((size_t)p.n * Dw * sizeof(float)));
      if (S > 0) list = vaq::permutation_head(p.n, (int64_t)S);  // it gathers its own sample from all rows
    } else {
      MHIP(s.stage.ensure(S * Dw * sizeof(float)));
      for (int h = 0; h < p.G; h++) {
        const std::vector<int> &pos = p.shard[(size_t)h].pos;
        list.insert(list.end(), pos.begin(), pos.begin() + cm::sample_count(p, h, g));
      }
    }
    if (!list.empty()) {
      DevBuf &b = o.full() ? s.perm : s.pos;
      MHIP(b.ensure(list.size() * sizeof(int)));
      MHIP(hipMemcpyAsync(b.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s.stream));
    }
  }
  MHIP(hipStreamSynchronize(s.stream));
  return 0;
}

// steps 1 and 2 on shard g's worker
int columns_and_copy(CbRun &f, int g, CbShard &s) {
  const cm::Plan &p = f.plan;
  const cm::ShardPart &sp = p.shard[(size_t)g];
  if (sp.cnt == 0) return 0;  // (an empty shard contributes no row)
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventRecord(s.t[0], s.stream));
  for (int w = 0; w < p.G; w++) {
    const cm::Owner &o = p.owner[(size_t)w];
    const int64_t rows = cm::block_rows(p, g, w);
    if (rows == 0) continue;
    // all of its rows for an owner of a full subspace; else its rows of the sample, through the local-row list (the
    // rows a host form picked ARE that list's rows, in its order)
    const int *d_local = o.full() || s.picked ? nullptr : s.local.as<int>();
    MHIP(vaq::launch_codebook_columns(s.d_rows, f.D, f.eig ? s.eig.as<float>() : nullptr, d_local, 0, rows,
                                      s.subs.as<int>() + f.sub_at[w], p.L, o.D_w, s.blocks.as<float>() + cm::block_at(p, g, w),
                                      s.stream));
  }
  MHIP(hipEventRecord(s.t[1], s.stream));
  for (int w = 0; w < p.G; w++) {
    const cm::Owner &o = p.owner[(size_t)w];
    const int64_t rows = cm::block_rows(p, g, w);
    if (rows == 0) continue;
    CbShard &os = f.sh[(size_t)w];
    const float *src = s.blocks.as<float>() + cm::block_at(p, g, w);
    float *dst = o.full() ? os.Pf.as<float>() + (size_t)sp.lo * o.D_w : os.stage.as<float>() + (size_t)cm::stage_row(p, g, w) * o.D_w;
    MHIP(copy_between(dst, os.device, src, s.device, (size_t)rows * o.D_w * sizeof(float), s.stream));
  }
  MHIP(hipEventRecord(s.t[2], s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  MHIP(hipEventElapsedTime(&s.ms[PH_COLUMNS], s.t[0], s.t[1]));
  MHIP(hipEventElapsedTime(&s.ms[PH_COPY], s.t[1], s.t[2]));
  return 0;
}

// step 3 on owner g's worker: its sample in place, the single fit from there on, its centres to the host
int fit_owned(CbRun &f, int g, CbShard &s) {
  const cm::Plan &p = f.plan;
  const cm::Owner &o = p.owner[(size_t)g];
  if (o.idle()) return 0;
  const auto began = std::chrono::steady_clock::now();
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventRecord(s.t[3], s.stream));
  if (!o.full())
    MHIP(vaq::launch_codebook_place(s.stage.as<float>(), s.pos.as<int>(), o.plan.gathered, o.D_w, s.Ps.as<float>(), s.stream));
  else
    MHIP(vaq::launch_codebook_gather(s.Pf.as<float>(), o.D_w, s.perm.as<int>(), o.plan.gathered, s.Ps.as<float>(), s.stream));
  MHIP(hipEventRecord(s.t[4], s.stream));
  s.iters.assign(o.subs.size(), 0);
  MHIP(vaq::codebooks_lloyd(o.plan.gathered > 0 ? s.Ps.as<float>() : nullptr, o.full() ? s.Pf.as<float>() : nullptr, o.D_w,
                            p.L, o.plan, f.max_iter, s.means.as<float>(), s.iters.data(), &s.no_centre,
                            f.timing ? &s.ph : nullptr, began, s.stream));  // synchronises
  s.h_means.resize((size_t)o.plan.n_cent * p.L);
  MHIP(hipMemcpyAsync(s.h_means.data(), s.means.p, s.h_means.size() * sizeof(float), hipMemcpyDeviceToHost, s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  MHIP(hipEventElapsedTime(&s.ms[PH_PLACE], s.t[3], s.t[4]));
  return 0;
}

// f.G, f.sh[g].device (and d_rows in the refiner form), f.plan and f.D are set; everything has been refused that can be
int run_fit(CbRun &f, float *centroids_out, int *iters_out, int *nan_rows_out) {
  const cm::Plan &p = f.plan;
  for (int w = 0; w < p.G; w++) f.sub_at[w + 1] = f.sub_at[w] + (int)p.owner[(size_t)w].subs.size();
  f.timing = vaqhip_internal_fit_codebooks_timing_on() != 0;
  f.pool.start(f.G);
  if (const int rc = on_shards(&f, [&](int g, CbShard &s) { return setup_shard(f, g, s); })) return rc;
  if (const int rc = on_shards(&f, [&](int g, CbShard &s) { return columns_and_copy(f, g, s); })) return rc;
  if (const int rc = on_shards(&f, [&](int g, CbShard &s) { return fit_owned(f, g, s); })) return rc;
  for (const CbShard &s : f.sh)
    if (s.no_centre)
      return mfail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  vaqhip_multi_fit_codebooks_timing tm = {};
  for (int w = 0; w < p.G; w++) {
    const cm::Owner &o = p.owner[(size_t)w];
    const CbShard &s = f.sh[(size_t)w];
    tm.owner_subspaces[w] = (int)o.subs.size();
    for (size_t i = 0; i < o.subs.size(); i++) {
      const cb::Sub &mine = o.plan.sub[i], &sd = p.whole.sub[(size_t)o.subs[i]];
      const float *m = s.h_means.data() + (size_t)mine.cent_off * p.L;
      std::memcpy(centroids_out + (size_t)sd.cent_off * p.L, m, (size_t)sd.k * p.L * sizeof(float));
      if (iters_out) iters_out[o.subs[i]] = s.iters[i];
      if (nan_rows_out) nan_rows_out[o.subs[i]] = vaq::nan_rows(m, sd.k, p.L);
      tm.iterations = std::max(tm.iterations, s.iters[i]);
    }
    tm.assign_ms = std::max(tm.assign_ms, (float)s.ph.assign_ms);
    tm.accumulate_ms = std::max(tm.accumulate_ms, (float)s.ph.accumulate_ms);
    tm.update_ms = std::max(tm.update_ms, (float)s.ph.update_ms);
  }
  tm.columns_ms = f.max_ms(PH_COLUMNS);
  tm.copy_ms = f.max_ms(PH_COPY);
  tm.place_ms = f.max_ms(PH_PLACE);
  tm.subspaces = p.M;
  tm.dims = f.D;
  tm.rows = p.n;
  tm.sample_rows = p.whole.sample;
  tm.n_devices = p.G;
  g_cbm_last = tm;  // (total_ms: WallClock, once the run has been taken down)
  return VAQHIP_OK;
}

// total_ms of a sharded call: from its declaration, before the run, to its end behind ~CbRun -- planning, the phases and
// the release of every worker, stream and buffer, as a clock around the call would show
struct WallClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  bool ok = false;
  ~WallClock() {
    if (ok) g_cbm_last.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

// the timing of a call that one device served: the single fit's figures
void timing_from_single() {
  vaqhip_fit_codebooks_timing t = {};
  (void)vaqhip_last_fit_codebooks_timing(&t);
  vaqhip_multi_fit_codebooks_timing tm = {};
  tm.total_ms = t.total_ms;
  tm.assign_ms = t.assign_ms;
  tm.accumulate_ms = t.accumulate_ms;
  tm.update_ms = t.update_ms;
  tm.iterations = t.iterations;
  tm.subspaces = t.subspaces;
  tm.dims = t.dims;
  tm.rows = t.rows;
  tm.sample_rows = t.sample_rows;
  tm.n_devices = 1;
  tm.owner_subspaces[0] = t.subspaces;
  g_cbm_last = tm;
}

// the host form over float or byte rows
int fit_host(int n_devices, const int *device_ids, vaq::RowsRef X, int64_t n, int D, int M, const int *bits,
             const float *eigvec, int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  if (!device_ids) return mfail(VAQHIP_EINVAL, "null pointer");
  if (const int rc = forward(vaqhip_internal_fit_codebooks_check(X.p, n, D, M, bits, max_iter, centroids_out))) return rc;
  WallClock wall;
  CbRun f;
  if (const int rc = f.from_devices(n_devices, device_ids)) return rc;
  if (n_devices == 1) {  // the single fit itself
    const int rc = forward(X.elem == 1 ? vaqhip_fit_codebooks_u8(device_ids[0], static_cast<const uint8_t *>(X.p), n, D, M, bits,
                                                                 eigvec, max_iter, centroids_out, iters_out, nan_rows_out)
                                       : vaqhip_fit_codebooks(device_ids[0], static_cast<const float *>(X.p), n, D, M, bits,
                                                              eigvec, max_iter, centroids_out, iters_out, nan_rows_out));
    if (!rc) timing_from_single();
    return rc;
  }
  if (!cm::plan_host(n_devices, n, D, M, bits, &f.plan)) return mfail(VAQHIP_EINVAL, "bad n_devices/n/D/M");
  f.D = D;
  f.max_iter = max_iter;
  f.X = X;
  f.eig = eigvec;
  const int rc = run_fit(f, centroids_out, iters_out, nan_rows_out);
  wall.ok = rc == VAQHIP_OK;
  return rc;
}

}  // namespace

extern "C" {

int vaqhip_multi_fit_codebooks(int n_devices, const int *device_ids, const float *X, int64_t n, int D, int M, const int *bits,
                               const float *eigvec, int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host(n_devices, device_ids, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out,
                  nan_rows_out);
}
int vaqhip_multi_fit_codebooks_u8(int n_devices, const int *device_ids, const uint8_t *X, int64_t n, int D, int M,
                                  const int *bits, const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                  int *nan_rows_out) {
  return fit_host(n_devices, device_ids, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out,
                  nan_rows_out);
}

int vaqhip_multi_refiner_fit_codebooks(vaqhip_multi_refiner *r, int M, const int *bits, const float *eigvec, int max_iter,
                                       float *centroids_out, int *iters_out, int *nan_rows_out) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N == 0) return mfail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_multi_refiner_set_rows first");
  // (the rows are the refiner's: any non-null pointer stands for them in the single fit's checks)
  if (const int rc = forward(vaqhip_internal_fit_codebooks_check(r, r->N, r->D, M, bits, max_iter, centroids_out))) return rc;
  if (r->G == 1) {  // the single fit itself, over the one shard's resident rows
    const ResidentRows rows = resident_rows(r, 0);
    const int rc = forward(vaqhip_internal_fit_codebooks_rows_device(r->sh[0].device, rows.rows.p, rows.rows.elem, rows.n, r->D,
                                                                     M, bits, eigvec, max_iter, centroids_out, iters_out,
                                                                     nan_rows_out));
    if (!rc) timing_from_single();
    return rc;
  }
  WallClock wall;
  CbRun f;
  int64_t cnt[VAQHIP_MAX_DEVICES];
  f.from_refiner(r, cnt);  // (float or byte rows: the column kernel reads either in place)
  if (!cm::plan_from_counts(r->G, cnt, r->D, M, bits, &f.plan) || f.plan.n != r->N) return mfail(VAQHIP_EINVAL, "bad shard counts");
  f.D = r->D;
  f.max_iter = max_iter;
  f.eig = eigvec;
  const int rc = run_fit(f, centroids_out, iters_out, nan_rows_out);
  wall.ok = rc == VAQHIP_OK;
  return rc;
}

int vaqhip_multi_last_fit_codebooks_timing(vaqhip_multi_fit_codebooks_timing *out) {
  if (!out) return mfail(VAQHIP_EINVAL, "null pointer");
  *out = g_cbm_last;
  return VAQHIP_OK;
}

}  // extern "C"
