// vaqhip_multi_refiner_search.cpp -- the exhaustive form of the multi-device refiner (vaqhip_multi_refiner_search:
// every resident row a candidate, in row order): what vaqhip_refiner_search returns over the same rows, slot for slot.
// Unlike the refine form (vaqhip_multi_refiner.cpp), its selection DOES depend on other shards' rows under
// "exact_ties", so it ends in a chain of replays.  Per set of queries:
//   A select     every shard with rows: the single form's select + merge over its own rows (vaqhip_exhaust_plan.h), a
//                [nq][k1] list per shard; on the shards' workers
//   B gather     the lists next to shard 0's, one merge by (distance, label) there: the answer without "exact_ties"
//   C flag       on the MERGED k + 1 lists: queries without equal distances are copied out, the others listed
//   D chain      the listed queries through the reference's heap, shard after shard in row order; the raw heap
//                arrays travel by peer copy, the last shard with rows reorders, shard 0 places the slots
// B to D are enqueued by the calling thread in chain order, so an event is always recorded before its wait is enqueued.
// With one shard the call is the single refiner's launches (xs_search_set) on the caller's stream.
#include "vaqhip_multi_refiner.h"
#include "vaq_exact.h"
#include "vaq_exhaust_launch.h"
#include "vaq_merge.h"

using namespace vaqhost;

namespace {

// the gathered lists of one set, in bytes on the first device (the set is cut to fit; every shard's own candidate
// lists are bounded by XS_LIST_BYTES as in the single form)
constexpr size_t XS_GATHER_BYTES = (size_t)256 << 20;

bool xs_takes_part(int g, const RShard &s) { return g == 0 || s.n > 0; }  // (shard 0 hosts the merge even without rows)

// Phase A of a set, on the shard's worker: buffers, the queries, select + merge over the shard's own rows
int xs_enqueue_shard(vaqhip_multi_refiner *r, int g, RShard &s) {
  if (!xs_takes_part(g, s)) return 0;  // (owns no label: no list, no link)
  const SearchCall &c = r->xc;
  SearchShardBufs &x = s.xs;  // this shard's and
  SearchFirstBufs &x0 = r->x;  //   (g == 0) the first device's
  const int n = c.nq, D = r->D, k1 = c.k1;
  const bool exact = c.chain, timing = r->opt.timing != 0;
  MHIP(hipSetDevice(s.device));
  // the last set's gather, merge and chain may still read the old buffers: `finished` follows all of them
  FitList fit;
  if (g == 0) {
    fit.want(x0.gl, c.lists * c.lists_bytes(), "gl");
    fit.want(x0.gd, c.lists * c.lists_bytes(), "gd");
    fit.want(x0.ms_d, c.scratch_bytes(), "ms_d");
    fit.want(x0.ms_id, c.scratch_bytes(), "ms_id");
    if (exact) {
      fit.want(x0.k1_l, c.lists_bytes(), "k1_l");
      fit.want(x0.k1_d, c.lists_bytes(), "k1_d");
      fit.want(x0.list, c.list_bytes(), "list");
    }
  } else {
    fit.want(s.d_q, c.query_bytes(D), "d_q");
    fit.want(x.l, c.lists_bytes(), "l");
    fit.want(x.d, c.lists_bytes(), "d");
    if (exact) fit.want(x.list, c.list_bytes(), "list");
  }
  if (exact)
    for (DevBuf *b : {&x.hin_v, &x.hin_i, &x.hout_v, &x.hout_i}) fit.want(*b, c.state_bytes(), "heap state");
  MFIT(fit, r->finished, !x.work.fits(x.plan, k1, false));
  MHIP(x.work.fit(x.plan, k1, false, false));
  if (timing) MHIP(ensure_events(x.t));
  // the previous set has been read (never recorded: no wait); the caller's inputs are there
  MHIP(hipStreamWaitEvent(s.stream, r->finished, 0));
  MHIP(hipStreamWaitEvent(s.stream, r->user_ready, 0));
  if (timing) MHIP(hipEventRecord(x.t[0], s.stream));
  const float *dq = c.d_q0;
  int32_t *out_l = x0.gl.as<int32_t>();  // shard 0: list 0 of the gathered lists
  float *out_d = x0.gd.as<float>();
  if (g > 0) {
    MHIP(hipMemcpyPeerAsync(s.d_q.p, s.device, c.d_q0, r->sh[0].device, c.query_bytes(D), s.stream));
    dq = s.d_q.as<float>();
    out_l = x.l.as<int32_t>();
    out_d = x.d.as<float>();
  }
  const XsRows rows = {s.rows.rows(), s.n, r->id_base + s.lo, D};
  MHIP(xs_select_merge(x.work, x.plan, rows, dq, n, k1, out_l, out_d, s.stream, timing ? x.t[1] : nullptr, &x.wgs, &x.qg));
  if (timing) MHIP(hipEventRecord(x.t[2], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

// Phases B and C, by the calling thread on the first device, once every shard's part is enqueued
int xs_gather_merge_flag(vaqhip_multi_refiner *r, int32_t *d_lout, float *d_dout) {
  RShard &s = r->sh[0];
  const SearchCall &c = r->xc;
  const int n = c.nq, k = c.k, k1 = c.k1;
  const bool exact = c.chain, timing = r->opt.timing != 0;
  const size_t plane = c.plane();
  MHIP(hipSetDevice(s.device));
  if (timing) MHIP(ensure_events(r->x.t));
  for (int g = 1; g < r->G; g++)
    if (r->sh[g].n > 0) MHIP(hipStreamWaitEvent(s.stream, r->sh[g].done, 0));
  if (timing) MHIP(hipEventRecord(r->x.t[0], s.stream));
  for (int g = 1; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (u.n == 0) continue;
    const size_t at = (size_t)c.slot[g] * plane;
    MHIP(hipMemcpyPeerAsync(r->x.gl.as<int32_t>() + at, s.device, u.xs.l.p, u.device, c.lists_bytes(), s.stream));
    MHIP(hipMemcpyPeerAsync(r->x.gd.as<float>() + at, s.device, u.xs.d.p, u.device, c.lists_bytes(), s.stream));
  }
  if (timing) MHIP(hipEventRecord(r->x.t[1], s.stream));
  int32_t *m_l = exact ? r->x.k1_l.as<int32_t>() : d_lout;
  float *m_d = exact ? r->x.k1_d.as<float>() : d_dout;
  MHIP(vaq::launch_merge(r->x.gd.as<float>(), r->x.gl.as<int>(), nullptr, c.lists, (int64_t)plane, (int64_t)k1, n, k1, 0, 1,
                         m_l, m_d, nullptr, r->x.ms_d.as<float>(), r->x.ms_id.as<int>(), s.stream));
  if (timing) MHIP(hipEventRecord(r->x.t[2], s.stream));
  if (exact) {
    int *list = r->x.list.as<int>();
    MHIP(vaq::launch_exact_flag(n, k, m_l, m_d, d_lout, d_dout, list, reinterpret_cast<unsigned *>(list + n), s.stream));
    MHIP(hipEventRecord(r->flagged, s.stream));
  }
  if (timing) MHIP(hipEventRecord(r->x.t[3], s.stream));
  return 0;
}

// One link of phase D on shard g, by the calling thread: the list, the heap arrays of the link before (prev < 0: none),
// the replay over the shard's rows.  Enqueued in chain order: `flagged` and the previous link's event are recorded.
int xs_link(vaqhip_multi_refiner *r, int g, int prev, int32_t *d_lout, float *d_dout) {
  RShard &s = r->sh[g];
  const SearchCall &c = r->xc;
  const int n = c.nq, k = c.k, dev0 = r->sh[0].device;
  const bool timing = r->opt.timing != 0, last = g == c.last;
  const size_t state = c.state_bytes();
  MHIP(hipSetDevice(s.device));
  const float *dq = c.d_q0;
  const int *list = r->x.list.as<int>();
  if (g > 0) {  // (shard 0's stream holds the flag step itself)
    MHIP(hipStreamWaitEvent(s.stream, r->flagged, 0));
    MHIP(hipMemcpyPeerAsync(s.xs.list.p, s.device, r->x.list.p, dev0, c.list_bytes(), s.stream));
    dq = s.d_q.as<float>();  // (there since phase A)
    list = s.xs.list.as<int>();
  }
  if (prev >= 0) {
    const RShard &u = r->sh[prev];
    MHIP(hipStreamWaitEvent(s.stream, u.link, 0));
    MHIP(hipMemcpyPeerAsync(s.xs.hin_v.p, s.device, u.xs.hout_v.p, u.device, state, s.stream));
    MHIP(hipMemcpyPeerAsync(s.xs.hin_i.p, s.device, u.xs.hout_i.p, u.device, state, s.stream));
  }
  if (timing) MHIP(hipEventRecord(s.xs.t[3], s.stream));
  const bool direct = last && g == 0;  // (all rows on the first shard: its link writes the caller's buffers)
  MHIP(vaq::launch_exhaust_replay_link(dq, n, r->D, s.rows.rows(), s.n, r->id_base + s.lo, k, list,
                                       reinterpret_cast<const unsigned *>(list + n), prev >= 0 ? s.xs.hin_v.as<float>() : nullptr,
                                       prev >= 0 ? s.xs.hin_i.as<int>() : nullptr, direct ? nullptr : s.xs.hout_v.as<float>(),
                                       direct ? nullptr : s.xs.hout_i.as<int>(), last ? 1 : 0, direct ? d_lout : nullptr,
                                       direct ? d_dout : nullptr, s.stream));
  if (timing) MHIP(hipEventRecord(s.xs.t[4], s.stream));
  MHIP(hipEventRecord(s.link, s.stream));
  return 0;
}

// the end of a set on the first device: with a chain, the last link's slots placed at their queries
int xs_finish(vaqhip_multi_refiner *r, bool chain, int32_t *d_lout, float *d_dout, hipStream_t user) {
  RShard &s = r->sh[0];
  const SearchCall &c = r->xc;
  const int n = c.nq, k = c.k;
  MHIP(hipSetDevice(s.device));
  if (chain && c.last > 0) {
    const RShard &u = r->sh[c.last];
    const size_t state = c.state_bytes();
    const int *list = r->x.list.as<int>();
    MHIP(hipStreamWaitEvent(s.stream, u.link, 0));
    MHIP(hipMemcpyPeerAsync(s.xs.hin_v.p, s.device, u.xs.hout_v.p, u.device, state, s.stream));
    MHIP(hipMemcpyPeerAsync(s.xs.hin_i.p, s.device, u.xs.hout_i.p, u.device, state, s.stream));
    MHIP(vaq::launch_exhaust_scatter(n, k, list, reinterpret_cast<const unsigned *>(list + n), s.xs.hin_v.as<float>(),
                                     s.xs.hin_i.as<int>(), d_lout, d_dout, s.stream));
  }
  if (r->opt.timing) MHIP(hipEventRecord(r->x.t[4], s.stream));
  MHIP(hipEventRecord(r->finished, s.stream));
  MHIP(hipStreamWaitEvent(user, r->finished, 0));
  return 0;
}

// option "timing": waits for the set and adds its figures (the slowest shard's select, merge and link)
int xs_read_timing(vaqhip_multi_refiner *r, bool chain) {
  RShard &s = r->sh[0];
  const SearchCall &c = r->xc;
  vaqhip_multi_refiner_search_timing &t = r->x_timing;
  auto span = [](hipEvent_t a, hipEvent_t b, float *ms) { return hipEventElapsedTime(ms, a, b); };
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventSynchronize(r->finished));
  float sel = 0, mer = 0, rep = 0, ms = 0;
  for (int g = 0; g < r->G; g++) {
    RShard &u = r->sh[g];
    if (!xs_takes_part(g, u)) continue;
    MHIP(hipSetDevice(u.device));
    MHIP(span(u.xs.t[0], u.xs.t[1], &ms));
    sel = std::max(sel, ms);
    MHIP(span(u.xs.t[1], u.xs.t[2], &ms));
    mer = std::max(mer, ms);
    if (chain && u.n > 0) {
      MHIP(span(u.xs.t[3], u.xs.t[4], &ms));
      rep = std::max(rep, ms);
    }
  }
  MHIP(hipSetDevice(s.device));
  t.select_ms += sel;
  t.merge_ms += mer;
  t.replay_ms += rep;
  MHIP(span(r->x.t[0], r->x.t[1], &ms));
  t.gather_ms += ms;
  MHIP(span(r->x.t[1], r->x.t[2], &ms));
  t.cross_merge_ms += ms;
  MHIP(span(r->x.t[2], r->x.t[3], &ms));
  t.flag_ms += ms;
  MHIP(span(r->x.t[3], r->x.t[4], &ms));
  if (chain) {
    t.chain_ms += ms;
    unsigned listed = 0;
    MHIP(hipMemcpy(&listed, r->x.list.as<int>() + c.nq, sizeof(unsigned), hipMemcpyDeviceToHost));
    t.listed_queries += (int)listed;
  }
  return 0;
}

// As refine_device_locked: device pointers on the first device, enqueue only, `user` waits for the outputs; r->mu held
int search_device_locked(vaqhip_multi_refiner *r, const float *d_q, int nq, int k, int32_t *d_lout, float *d_dout,
                         hipStream_t user) {
  RShard &s = r->sh[0];
  SearchCall &c = r->xc;
  bool any_cap = false;
  for (const RShard &u : r->sh) any_cap |= u.rows.cap_rows > 0;
  if (r->N == 0 && !any_cap) return mfail(VAQHIP_ESTATE, "no rows were set");
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  const bool exact = r->opt.exact != 0, timing = r->opt.timing != 0;
  s.err.clear();
  r->x_timing = {};
  r->x_timing.register_form = r->D <= (int)vaq::exhaust_register_max_dim();
  if (r->G == 1) {  // the single refiner's launches, at their cost, on the caller's stream
    auto body = [&]() -> int {
      MHIP(s.xs.work.size_for(s.device, r->D, s.rows.elem));
      const int k1 = exact ? k + 1 : k;
      const XsPlan pl = xs_plan(s.xs.work, r->N, r->opt.splits, nq, k1);
      MHIP(s.xs.work.fit(pl, k1, exact, timing));
      MHIP(hipStreamWaitEvent(user, r->finished, 0));  // (the workspace is shared by the callers' streams)
      const XsRows rows = {s.rows.rows(), r->N, r->id_base, r->D};
      vaqhip_refiner_search_timing t1 = {};
      hipError_t e = hipSuccess;
      int sets = 0;
      for (int q0 = 0; q0 < nq && e == hipSuccess; q0 += pl.chunk, sets++)
        e = xs_search_set(s.xs.work, pl, rows, d_q + (size_t)q0 * r->D, std::min(pl.chunk, nq - q0), k, exact,
                          d_lout + (size_t)q0 * k, d_dout + (size_t)q0 * k, user, timing ? &t1 : nullptr);
      (void)hipEventRecord(r->finished, user);  // (also after a failure: work may be enqueued already)
      MHIP(e);
      vaqhip_multi_refiner_search_timing &t = r->x_timing;
      t.select_ms = t1.select_ms;
      t.merge_ms = t1.merge_ms;
      t.flag_ms = t1.flag_ms;
      t.replay_ms = t1.replay_ms;
      t.listed_queries = t1.listed_queries;
      t.splits = pl.S;
      t.workgroups = t1.workgroups;
      t.queries_per_group = t1.queries_per_group;
      t.chain_shards = r->N > 0 ? 1 : 0;
      t.sets = sets;
      return 0;
    };
    const int rc = body();
    return rc ? mfail(rc, "device %d: %s", s.device, s.err.c_str()) : VAQHIP_OK;
  }
  if (r->dirty) drain(r);
  // the call's plan: the lists gathered, the chain's ends, one set size for every shard
  int first = -1;
  c.lists = 0;
  c.last = 0;
  for (int g = 0; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (!xs_takes_part(g, u)) continue;
    c.slot[g] = c.lists++;
    if (u.n > 0) {
      if (first < 0) first = g;
      c.last = g;
    }
  }
  const bool chain = exact && first >= 0;  // (no rows at all: every slot is -1 / FLT_MAX under either rule)
  const int k1 = chain ? k + 1 : k;
  c.chain = chain;
  c.k = k;
  c.k1 = k1;
  int set = std::min(nq, SET_QUERIES);
  set = (int)std::min<size_t>((size_t)set, std::max<size_t>(1, XS_GATHER_BYTES / ((size_t)c.lists * k1 * 8)));
  auto plan = [&](int max_chunk) -> int {
    for (int g = 0; g < r->G; g++) {
      RShard &u = r->sh[g];
      if (!xs_takes_part(g, u)) continue;
      if (hipSetDevice(u.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", u.device);
      const hipError_t e = u.xs.work.size_for(u.device, r->D, u.rows.elem);
      if (e != hipSuccess) return mfail(hip_code(e), "device %d: %s", u.device, hipGetErrorString(e));
      u.xs.plan = xs_plan(u.xs.work, u.n, r->opt.splits, nq, k1, max_chunk);
      set = std::min(set, u.xs.plan.chunk);
    }
    return VAQHIP_OK;
  };
  if (const int rc = plan(set)) return rc;  // every shard's own bound ...
  if (const int rc = plan(set)) return rc;  // ... and the smallest of them for all: equal sets of one size
  set = r->sh[0].xs.plan.chunk;
  r->x_timing.splits = r->sh[std::max(first, 0)].xs.plan.S;
  r->x_timing.chain_shards = first < 0 ? 0 : c.lists - (r->sh[0].n > 0 ? 0 : 1);
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  if (hipEventRecord(r->user_ready, user) != hipSuccess) return mfail(VAQHIP_EHIP, "recording the caller's stream");
  for (int q0 = 0; q0 < nq; q0 += set) {
    c.nq = std::min(set, nq - q0);
    c.d_q0 = d_q + (size_t)q0 * r->D;
    int32_t *lo = d_lout + (size_t)q0 * k;
    float *d_o = d_dout + (size_t)q0 * k;
    int rc = on_shards(r, [&](int g, RShard &u) { return xs_enqueue_shard(r, g, u); });
    auto step = [&](int g, int step_rc) {  // a step of the calling thread failed on shard g
      return step_rc ? mfail(step_rc, "shard %d (device %d): %s", g, r->sh[g].device, r->sh[g].err.c_str()) : 0;
    };
    if (!rc) {
      s.err.clear();
      rc = step(0, xs_gather_merge_flag(r, lo, d_o));
    }
    for (int g = 0, prev = -1; !rc && chain && g < r->G; g++) {
      if (r->sh[g].n == 0) continue;  // (a shard without rows is no link)
      r->sh[g].err.clear();
      rc = step(g, xs_link(r, g, prev, lo, d_o));
      prev = g;
    }
    if (!rc) rc = step(0, xs_finish(r, chain, lo, d_o, user));
    if (!rc && timing) rc = step(0, xs_read_timing(r, chain));
    if (rc) {
      r->dirty = true;  // (`finished` may not follow what was enqueued: the next call drains first)
      return rc;
    }
    r->x_timing.sets++;
    r->x_timing.workgroups = r->sh[std::max(first, 0)].xs.wgs;
    r->x_timing.queries_per_group = r->sh[std::max(first, 0)].xs.qg;
  }
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_multi_refiner_search_device(vaqhip_multi_refiner *r, const float *d_queries, int nq, int k, int32_t *d_labels_out,
                                       float *d_distances_out, void *stream) {
  if (const int rc = check_search(MULTI_REFINER, r, nq, k, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return search_device_locked(r, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_multi_refiner_search(vaqhip_multi_refiner *r, const float *queries, int nq, int k, int32_t *labels_out,
                                float *distances_out) {
  if (const int rc = check_search(MULTI_REFINER, r, nq, k, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  // (under "timing" the figures are the last staged set's: the bench and the tests stay within one)
  return through_staging(r, queries, nq, nullptr, 0, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return search_device_locked(r, r->w.q.as<float>(), n, k, r->w.lout.as<int32_t>(), r->w.dout.as<float>(), st);
  });
}

int vaqhip_multi_refiner_last_search_timing(vaqhip_multi_refiner *r, vaqhip_multi_refiner_search_timing *out) {
  if (!r || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  *out = r->x_timing;
  return VAQHIP_OK;
}

}  // extern "C"
