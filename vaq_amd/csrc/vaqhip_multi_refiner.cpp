// vaqhip_multi_refiner.cpp -- the multi-device refiner of include/vaqhip.h: the raw rows VAQ::refine reads
// (VAQ.cpp:849-876) cut over the GPUs of a node like the code rows of vaqhip_multi, and the single refiner's answer
// over them, slot for slot.
//
// A candidate's distance depends on the query and the candidate's own row only; the selection depends on the R
// (distance, label) pairs in candidate order only.  So every shard computes the distances of the candidates it holds
// (refine_dist_kernel: the single refiner's reduction) into its [nq][R] plane, the planes go to the first device, and
// ONE selection runs there over the R gathered distances in the original candidate order (refine_select_kernel: the
// single refiner's selection).  No chain of replays, unlike the search: nothing a shard computes depends on another.
//
// One process, one worker per shard (job_pool.h); a phase is enqueued by every worker at once and the caller goes on
// only when all of them succeeded (on_shards), so a failing shard ends the call and cannot hang it.  Per set of
// queries:
//   1 broadcast  queries and candidate labels from the first device to shards 1.. (hipMemcpyPeerAsync behind the
//                caller's stream's event; shard 0 reads the caller's buffers in place)
//   2 distances  refine_dist_kernel on every shard's own stream (a shard without rows launches nothing)
//   3 gather     shard 0's stream waits for every shard's event and copies the planes of shards 1.. next to its own
//   4 select     refine_select_kernel there, straight into the caller's buffers; the caller's stream waits for it
// Every wait is a stream wait on an event.  With one shard the call is launch_refine_rows on the caller's stream.
// The exhaustive form (every resident row a candidate) is vaqhip_multi_refiner_search.cpp.
#include "vaqhip_multi_refiner.h"
#include "vaq_refine.h"

#include <cstring>

using namespace vaqhost;

void vaqhost::drain(vaqhip_multi_refiner *r) {
  for (RShard &s : r->sh)
    if (hipSetDevice(s.device) == hipSuccess) (void)hipStreamSynchronize(s.stream);
  (void)hipSetDevice(r->sh[0].device);
  r->dirty = false;
}

namespace {

// the three timing events of the set in flight among `rf`'s (null without option "timing"); `s` takes the text
int set_events(const vaqhip_multi_refiner *r, EventList &ev, RShard &s, hipEvent_t *&t) {
  t = nullptr;
  if (!r->opt.timing) return 0;
  if (ev.ensure(3 * (size_t)(r->set.set_no + 1)) != hipSuccess) {
    s.err = "hipEventCreate failed";
    return VAQHIP_EHIP;
  }
  t = &ev.e[3 * (size_t)r->set.set_no];
  return 0;
}

// Phases 1 and 2 of a set, on the shard's worker: buffers, the broadcast, the distances.
int enqueue_shard(vaqhip_multi_refiner *r, int g, RShard &s) {
  const RefineSet &c = r->set;
  const int D = r->D;
  MHIP(hipSetDevice(s.device));
  hipEvent_t *t;
  if (const int rc = set_events(r, s.rf.t, s, t)) return rc;
  // the last set's gather and select (on shard 0's stream) may still read the old buffers: `finished` follows them
  FitList fit;
  if (g == 0) fit.want(r->rf.planes, r->G * c.plane_bytes(), "planes");
  else if (s.n > 0) {
    fit.want(s.d_q, c.query_bytes(D), "d_q");
    fit.want(s.rf.lin, c.plane_bytes(), "lin");
    fit.want(s.rf.plane, c.plane_bytes(), "plane");
  }
  MFIT(fit, r->finished);
  // the previous set has been read (never recorded: no wait); the caller's inputs are there
  MHIP(hipStreamWaitEvent(s.stream, r->finished, 0));
  MHIP(hipStreamWaitEvent(s.stream, r->user_ready, 0));
  if (t) MHIP(hipEventRecord(t[0], s.stream));
  const float *dq = c.d_q0;
  const int32_t *dl = c.d_lin0;
  float *plane = r->rf.planes.as<float>();  // shard 0: plane 0 of the gathered buffer
  if (g > 0 && s.n > 0) {
    const int dev0 = r->sh[0].device;
    MHIP(hipMemcpyPeerAsync(s.d_q.p, s.device, c.d_q0, dev0, c.query_bytes(D), s.stream));
    MHIP(hipMemcpyPeerAsync(s.rf.lin.p, s.device, c.d_lin0, dev0, c.plane_bytes(), s.stream));
    dq = s.d_q.as<float>();
    dl = s.rf.lin.as<int32_t>();
    plane = s.rf.plane.as<float>();
  }
  if (t) MHIP(hipEventRecord(t[1], s.stream));
  MHIP(vaq::launch_refine_dist(dq, c.nq, D, s.rows.rows(), s.n, r->id_base + s.lo, dl, c.R, plane, s.stream));
  if (t) MHIP(hipEventRecord(t[2], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

// Phases 3 and 4, by the calling thread on the first device, once every shard's part is enqueued
int gather_and_select(vaqhip_multi_refiner *r, int k, int32_t *d_lout, float *d_dout, hipStream_t user) {
  RShard &s = r->sh[0];
  const RefineSet &c = r->set;
  MHIP(hipSetDevice(s.device));
  hipEvent_t *t;
  if (const int rc = set_events(r, r->rf.t, s, t)) return rc;
  for (int g = 1; g < r->G; g++) MHIP(hipStreamWaitEvent(s.stream, r->sh[g].done, 0));
  if (t) MHIP(hipEventRecord(t[0], s.stream));
  float *planes = r->rf.planes.as<float>();
  for (int g = 1; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (u.n > 0)  // (an empty shard owns no label: its plane is never read)
      MHIP(hipMemcpyPeerAsync(planes + (size_t)g * c.plane(), s.device, u.rf.plane.p, u.device, c.plane_bytes(), s.stream));
  }
  if (t) MHIP(hipEventRecord(t[1], s.stream));
  MHIP(vaq::launch_refine_select(c.d_lin0, c.nq, planes, c.plane(), r->bounds, c.R, k, r->opt.exact, d_lout, d_dout, s.stream));
  if (t) MHIP(hipEventRecord(t[2], s.stream));
  MHIP(hipEventRecord(r->finished, s.stream));
  MHIP(hipStreamWaitEvent(user, r->finished, 0));
  return 0;
}

// Device pointers on the first device, enqueue only; r->mu held.  The outputs are written behind `user`'s earlier
// work and `user` is made to wait for them.
int refine_device_locked(vaqhip_multi_refiner *r, const float *d_q, int nq, const int32_t *d_lin, int R, int k,
                         int32_t *d_lout, float *d_dout, hipStream_t user) {
  RShard &s0 = r->sh[0];
  if (hipSetDevice(s0.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s0.device);
  const bool timing = r->opt.timing != 0;
  r->last_sets = 0;
  r->last_single = r->G == 1;
  if (r->G == 1) {  // the single refiner's call, at its cost
    hipError_t e = hipSuccess;
    if (timing && r->rf.t.ensure(3) != hipSuccess) return mfail(VAQHIP_EHIP, "hipEventCreate failed");
    if (timing) e = hipEventRecord(r->rf.t[0], user);
    if (e == hipSuccess)
      e = vaq::launch_refine_rows(d_q, nq, r->D, s0.rows.rows(), r->N, r->id_base, d_lin, R, k, r->opt.exact, d_lout, d_dout, user);
    if (e == hipSuccess && timing) e = hipEventRecord(r->rf.t[1], user);
    if (e != hipSuccess) return mfail(hip_code(e), "refine on device %d: %s", s0.device, hipGetErrorString(e));
    r->last_sets = timing ? 1 : 0;
    return VAQHIP_OK;
  }
  if (r->dirty) drain(r);
  if (hipEventRecord(r->user_ready, user) != hipSuccess) return mfail(VAQHIP_EHIP, "recording the caller's stream");
  for (int q0 = 0, set_no = 0; q0 < nq; q0 += SET_QUERIES, set_no++) {
    r->set = RefineSet{d_q + (size_t)q0 * r->D, d_lin + (size_t)q0 * R, std::min(SET_QUERIES, nq - q0), R, set_no};
    int rc = on_shards(r, [&](int g, RShard &s) { return enqueue_shard(r, g, s); });
    if (!rc) {
      s0.err.clear();
      rc = gather_and_select(r, k, d_lout + (size_t)q0 * k, d_dout + (size_t)q0 * k, user);
      if (rc) mfail(rc, "gather / select on device %d: %s", s0.device, s0.err.c_str());
    }
    if (rc) {
      r->dirty = true;  // (`finished` may not follow what was enqueued: the next call drains first)
      return rc;
    }
    if (timing) r->last_sets = set_no + 1;
  }
  return VAQHIP_OK;
}

// the index and the refiner of a fused call must describe the same rows on the same devices
int check_pair(vaqhip_multi *mx, const vaqhip_multi_refiner *r, int R) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (R > VAQHIP_MAX_K) return mfail(VAQHIP_EUNSUPPORTED, "R=%d > %d (the search returns the candidates)", R, VAQHIP_MAX_K);
  vaqhip_multi_info inf;
  if (const int rc = vaqhip_multi_get_info(mx, &inf)) return rc;
  if (const int rc = check_same_devices(mx, r)) return rc;
  if (inf.N != r->N || inf.id_base != r->id_base)
    return mfail(VAQHIP_ESTATE, "the index holds %lld rows from label %lld, the refiner %lld from %lld", (long long)inf.N,
                 (long long)inf.id_base, (long long)r->N, (long long)r->id_base);
  return VAQHIP_OK;
}

// search with k = R into the refiner's candidate buffers on the first device, refine from there; r->mu held
int search_refine_locked(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *d_q, int nq, int R, int k,
                         int32_t *d_lout, float *d_dout, hipStream_t st) {
  RShard &s = r->sh[0];
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  if (r->dirty) drain(r);
  const size_t bytes = (size_t)nq * R * 4;
  if (bytes > r->w.cand_l.cap) {  // (the last fused call's shards and select read the old buffers)
    hipError_t e = hipEventSynchronize(r->finished);
    if (e == hipSuccess) e = r->w.cand_l.ensure(bytes);
    if (e == hipSuccess) e = r->w.cand_d.ensure(bytes);
    if (e != hipSuccess) return mfail(hip_code(e), "candidate buffers on device %d: %s", s.device, hipGetErrorString(e));
  }
  if (const int rc = vaqhip_multi_search_device(mx, d_q, nq, R, 0, r->w.cand_l.as<int32_t>(), r->w.cand_d.as<float>(), st))
    return rc;
  return refine_device_locked(r, d_q, nq, r->w.cand_l.as<int32_t>(), R, k, d_lout, d_dout, st);
}

// The row calls, for either element type (elem: 4 or 1).  A set replaces the rows and their type on every shard; an
// append keeps the type of the rows there are, and a refiner without rows takes either.
int set_rows_any(vaqhip_multi_refiner *r, const void *X, int elem, int64_t N, int64_t id_base) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (N < 0 || (N > 0 && !X)) return mfail(VAQHIP_EINVAL, "bad rows");
  if (const int rc = check_labels_fit(MULTI_REFINER, N, id_base)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  const vaq::RefineBounds cut = vaq::refine_cut(N, r->G, id_base);
  if (rows_elem(r) != elem) {  // (the rows there are go either way: a failure below leaves none, not rows misread)
    for (RShard &s : r->sh) s.lo = s.n = 0, s.rows.retype(elem, r->D);
    r->N = 0;
    r->bounds = vaq::refine_cut(0, r->G, r->id_base);
  }
  // every shard uploads its own rows, all of them at once
  if (const int rc = on_shards(r, [&](int g, RShard &s) {
        MHIP(hipSetDevice(s.device));
        const int64_t lo = cut.b[g] - id_base, n = cut.b[g + 1] - cut.b[g];
        const size_t rb = s.rows.row_bytes(r->D);
        s.n = 0;
        MHIP(s.rows.reserve(n, RowStore::DROP, r->D));
        MHIP(hipDeviceSynchronize());
        if (n > 0) MHIP(hipMemcpy(s.rows.buf.p, static_cast<const char *>(X) + (size_t)lo * rb, (size_t)n * rb, hipMemcpyHostToDevice));
        s.lo = lo;
        s.n = n;
        return 0;
      })) {
    // (shards that did upload hold rows of a dataset the others do not: nothing is resident)
    for (RShard &s : r->sh) s.lo = s.n = 0;
    r->N = 0;
    r->bounds = vaq::refine_cut(0, r->G, r->id_base);
    return rc;
  }
  r->N = N;
  r->id_base = id_base;
  r->bounds = cut;
  return VAQHIP_OK;
}

int add_rows_any(vaqhip_multi_refiner *r, const void *X, int elem, int64_t n_new) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (n_new < 0 || (n_new > 0 && !X)) return mfail(VAQHIP_EINVAL, "bad rows");
  if (n_new == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  if (r->N > 0 && rows_elem(r) != elem)
    return mfail(VAQHIP_ESTATE, "the multi refiner holds %s rows: append rows of that type (nothing is converted)",
                 rows_elem(r) == 1 ? "uint8" : "float32");
  if (const int rc = check_labels_fit(MULTI_REFINER, r->N + n_new, r->id_base)) return rc;
  for (RShard &u : r->sh) u.rows.retype(elem, r->D);  // (only without rows does this change anything)
  // the new rows continue the numbering, so they extend the LAST shard, as vaqhip_multi_add_codes_u16 does
  RShard &s = r->sh[r->G - 1];
  DeviceGuard g(s.device);
  if (!g.ok) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  s.err.clear();
  auto body = [&]() -> int {
    const size_t rb = s.rows.row_bytes(r->D);
    MHIP(s.rows.reserve(s.n + n_new, s.n, r->D));
    // (rows past s.n are read by no launch in flight: no wait is needed before they are written)
    MHIP(hipMemcpy(s.rows.buf.as<char>() + (size_t)s.n * rb, X, (size_t)n_new * rb, hipMemcpyHostToDevice));
    return 0;
  };
  if (const int rc = body()) return mfail(rc, "shard %d (device %d): %s", r->G - 1, s.device, s.err.c_str());
  s.n += n_new;
  r->N += n_new;
  vaq::refine_grow_last(r->bounds, n_new);
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_multi_refiner_create(vaqhip_multi_refiner **out, int D, int n_devices, const int *device_ids) {
  if (!out) return mfail(VAQHIP_EINVAL, "out is null");
  *out = nullptr;
  if (D <= 0) return mfail(VAQHIP_EINVAL, "D=%d", D);
  if (n_devices < 1 || n_devices > VAQHIP_MAX_DEVICES || !device_ids)
    return mfail(VAQHIP_EINVAL, "n_devices=%d outside 1..%d (or no device list)", n_devices, VAQHIP_MAX_DEVICES);
  if ((size_t)D > vaq::refine_rows_max_dim())
    return mfail(VAQHIP_EUNSUPPORTED, "D=%d: the query row must fit the workgroup's LDS (%zu floats)", D,
                 vaq::refine_rows_max_dim());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return mfail(VAQHIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
  for (int g = 0; g < n_devices; g++)
    if (device_ids[g] < 0 || device_ids[g] >= ndev) return mfail(VAQHIP_EINVAL, "device_ids[%d]=%d of %d", g, device_ids[g], ndev);
  vaqhip_multi_refiner *r = new (std::nothrow) vaqhip_multi_refiner();
  if (!r) return mfail(VAQHIP_ENOMEM, "host allocation");
  DeviceGuard keep(DeviceGuard::restore_only);
  r->D = D;
  r->G = n_devices;
  r->sh.resize(n_devices);
  r->bounds = vaq::refine_cut(0, n_devices, 0);
  for (int g = 0; g < n_devices; g++) {
    RShard &s = r->sh[g];
    s.device = device_ids[g];
    bool ok = hipSetDevice(s.device) == hipSuccess && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&s.link, hipEventDisableTiming) == hipSuccess;
    if (g == 0)
      ok = ok && hipEventCreateWithFlags(&r->user_ready, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&r->finished, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&r->flagged, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      vaqhip_multi_refiner_destroy(r);
      return mfail(VAQHIP_ENODEVICE, "stream / event creation on device %d failed", s.device);
    }
  }
  r->pool.start(n_devices);
  *out = r;
  return VAQHIP_OK;
}

void vaqhip_multi_refiner_destroy(vaqhip_multi_refiner *r) {
  if (!r) return;
  DeviceGuard keep(DeviceGuard::restore_only);
  r->pool.stop();
  for (RShard &s : r->sh) {
    (void)hipSetDevice(s.device);
    (void)hipDeviceSynchronize();  // (refines enqueued on the callers' streams read the rows)
    s.release();
    for (hipEvent_t e : {s.done, s.link})
      if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (!r->sh.empty()) (void)hipSetDevice(r->sh[0].device);
  r->w.release(), r->rf.release(), r->x.release();
  for (hipEvent_t e : {r->user_ready, r->finished, r->flagged})
    if (e) (void)hipEventDestroy(e);
  delete r;
}

int vaqhip_multi_refiner_set_rows(vaqhip_multi_refiner *r, const float *X, int64_t N, int64_t id_base) {
  return set_rows_any(r, X, 4, N, id_base);
}
int vaqhip_multi_refiner_add_rows(vaqhip_multi_refiner *r, const float *X, int64_t n_new) { return add_rows_any(r, X, 4, n_new); }
int vaqhip_multi_refiner_set_rows_u8(vaqhip_multi_refiner *r, const uint8_t *X, int64_t N, int64_t id_base) {
  return set_rows_any(r, X, 1, N, id_base);
}
int vaqhip_multi_refiner_add_rows_u8(vaqhip_multi_refiner *r, const uint8_t *X, int64_t n_new) {
  return add_rows_any(r, X, 1, n_new);
}

int vaqhip_multi_refiner_elem_size(vaqhip_multi_refiner *r) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  std::lock_guard<std::mutex> lk(r->mu);
  return rows_elem(r);
}

int vaqhip_multi_refiner_set_option(vaqhip_multi_refiner *r, const char *key, int64_t value) {
  return set_option(MULTI_REFINER, r, key, value);
}

int vaqhip_multi_refiner_refine_device(vaqhip_multi_refiner *r, const float *d_queries, int nq, const int32_t *d_labels_in,
                                       int R, int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (const int rc = check_sizes(MULTI_REFINER, r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries || !d_labels_in || !d_labels_out || !d_distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return refine_device_locked(r, d_queries, nq, d_labels_in, R, k, d_labels_out, d_distances_out,
                              static_cast<hipStream_t>(stream));
}

int vaqhip_multi_refiner_refine(vaqhip_multi_refiner *r, const float *queries, int nq, const int32_t *labels_in, int R,
                                int k, int32_t *labels_out, float *distances_out) {
  if (const int rc = check_sizes(MULTI_REFINER, r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !labels_in || !labels_out || !distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return through_staging(r, queries, nq, labels_in, R, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return refine_device_locked(r, r->w.q.as<float>(), n, r->w.lin.as<int32_t>(), R, k, r->w.lout.as<int32_t>(),
                                r->w.dout.as<float>(), st);
  });
}

int vaqhip_multi_search_refine_device(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *d_queries_raw, int nq, int R,
                                      int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (const int rc = check_sizes(MULTI_REFINER, r, nq, R, k)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  if (const int rc = check_pair(mx, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries_raw || !d_labels_out || !d_distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard keep(DeviceGuard::restore_only);
  return search_refine_locked(mx, r, d_queries_raw, nq, R, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_multi_search_refine(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *queries_raw, int nq, int R, int k,
                               int32_t *labels_out, float *distances_out) {
  if (const int rc = check_sizes(MULTI_REFINER, r, nq, R, k)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  if (const int rc = check_pair(mx, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries_raw || !labels_out || !distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard keep(DeviceGuard::restore_only);
  return through_staging(r, queries_raw, nq, nullptr, R, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return search_refine_locked(mx, r, r->w.q.as<float>(), n, R, k, r->w.lout.as<int32_t>(), r->w.dout.as<float>(), st);
  });
}

int vaqhip_multi_refiner_get_info(vaqhip_multi_refiner *r, vaqhip_multi_refiner_info *out) {
  if (!r || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  std::memset(out, 0, sizeof *out);
  out->n_devices = r->G;
  out->D = r->D;
  out->N = r->N;
  out->id_base = r->id_base;
  out->exact_ties = r->opt.exact;
  out->set_queries = SET_QUERIES;
  for (int g = 0; g < VAQHIP_MAX_DEVICES; g++) {
    out->device_ids[g] = g < r->G ? r->sh[g].device : -1;
    out->shard_rows[g] = g < r->G ? r->sh[g].n : 0;
  }
  // The phase times of the last call made under "timing" = 1, summed over its sets; broadcast and distances are
  // those of the slowest shard.  Waits for that call.
  auto span = [](hipEvent_t a, hipEvent_t b, float *ms) {
    *ms = 0;
    return hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(ms, a, b) == hipSuccess;
  };
  bool ok = true;
  float ms = 0;
  if (r->last_single && r->last_sets) {
    ok = hipSetDevice(r->sh[0].device) == hipSuccess && span(r->rf.t[0], r->rf.t[1], &ms);
    out->last_distances_ms = ms;  // (one kernel: the distances and the selection together)
  } else {
    for (int i = 0; ok && i < r->last_sets; i++) {
      float bc = 0, di = 0;
      for (int g = 0; ok && g < r->G; g++) {
        const RShard &s = r->sh[g];
        ok = hipSetDevice(s.device) == hipSuccess && span(s.rf.t[3 * i], s.rf.t[3 * i + 1], &ms);
        bc = std::max(bc, ms);
        ok = ok && span(s.rf.t[3 * i + 1], s.rf.t[3 * i + 2], &ms);
        di = std::max(di, ms);
      }
      out->last_broadcast_ms += bc;
      out->last_distances_ms += di;
      ok = ok && hipSetDevice(r->sh[0].device) == hipSuccess && span(r->rf.t[3 * i], r->rf.t[3 * i + 1], &ms);
      out->last_gather_ms += ms;
      ok = ok && span(r->rf.t[3 * i + 1], r->rf.t[3 * i + 2], &ms);
      out->last_select_ms += ms;
    }
  }
  if (!ok) return mfail(VAQHIP_EHIP, "reading the timing events");
  out->last_sets = r->last_sets;
  return VAQHIP_OK;
}

}  // extern "C"
