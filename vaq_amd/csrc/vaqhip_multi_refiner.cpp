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
//
// The exhaustive form (vaqhip_multi_refiner_search: every resident row a candidate, in row order) is the second half
// of this file.  Its selection DOES depend on other shards' rows under "exact_ties", so it ends in a chain of replays:
//   A select     every shard with rows: the single form's select + merge over its own rows (vaqhip_exhaust_plan.h), a
//                [nq][k1] list per shard; on the shards' workers
//   B gather     the lists next to shard 0's, one merge by (distance, label) there: the answer without "exact_ties"
//   C flag       on the MERGED k + 1 lists: queries without equal distances are copied out, the others listed
//   D chain      the listed queries through the reference's heap, shard after shard in row order; the raw heap
//                arrays travel by peer copy, the last shard with rows reorders, shard 0 places the slots
// B to D are enqueued by the calling thread in chain order, so an event is always recorded before its wait is enqueued.
#include "vaqhip_multi.h"

#include <cstring>

#include "vaq_kernels.h"
#include "vaqhip_exhaust_plan.h"

using namespace vaqhost;

namespace vaqhost __attribute__((visibility("hidden"))) {

struct RShard {
  int device = 0;
  int64_t lo = 0, n = 0;  // rows [lo, lo + n) of the dataset
  int64_t cap_rows = 0;   // rows the allocation holds (appends grow the last shard geometrically)
  DevBuf d_rows;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // this shard's plane of the current set is complete
  DevBuf d_q, d_lin;          // shards 1..: the set's queries and candidate labels
  DevBuf d_plane;             // shards 1..: float [nq][R]; shard 0 writes into the gathered planes
  std::vector<hipEvent_t> t;  // option "timing": 3 events per set (start, broadcast done, distances done)
  // the exhaustive form: this device's workspace and its plan for the call in flight; shards 1..: the shard's
  // [set][k1] lists (shard 0 writes into the gathered lists) and the replay list with its count; the chain's state,
  // [set][k] raw heap arrays in and out (shard 0's x_hin receives the last link's finished slots)
  XsWork xs;
  XsPlan xpl = {1, 1, 1};
  int x_wgs = 0, x_qg = 0;
  DevBuf x_l, x_d, x_list;
  DevBuf x_hin_v, x_hin_i, x_hout_v, x_hout_i;
  hipEvent_t link = nullptr;  // this shard's link of the chain is complete
  hipEvent_t xt[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // "timing": start, selected, merged; link start, end
  std::string err;
};

}  // namespace vaqhost

struct vaqhip_multi_refiner {
  __attribute__((visibility("hidden"))) ~vaqhip_multi_refiner() = default;
  int D = 0, G = 0;
  std::vector<RShard> sh;
  int64_t N = 0, id_base = 0;
  vaq::RefineBounds bounds = {};
  int opt_exact = 0, opt_timing = 0;
  int opt_splits = 0;  // "exhaustive_splits": per shard, 0 = automatic
  std::mutex mu;  // one call at a time
  vaq::JobPool pool;
  // on the first device
  DevBuf d_planes;                        // float [G][set][R]
  DevBuf w_q, w_lin, w_lout, w_dout;      // the host forms' staging
  DevBuf w_cand_l, w_cand_d;              // the fused call's candidates
  hipEvent_t user_ready = nullptr;        // recorded on the caller's stream: its inputs are there
  hipEvent_t finished = nullptr;          // the last set's select is complete: every buffer of the set has been read
  bool dirty = false;                     // a call failed part-way: `finished` does not cover what it enqueued
  std::vector<hipEvent_t> t;              // option "timing": 3 events per set (gather start, gathered, selected)
  int last_sets = 0;                      // sets of the last call that carry timing events
  bool last_single = false;               //   it was the one-shard form (t[0], t[1] around the kernel)
  // the exhaustive form, on the first device: the gathered [lists][set][k1] labels and distances, the cross-shard
  // merge's scratch, the merged k + 1 lists and the replay list with its count
  DevBuf x_gl, x_gd, x_ms_d, x_ms_id, x_k1_l, x_k1_d, x_list;
  hipEvent_t flagged = nullptr;  // the replay list of the current set is complete
  hipEvent_t xt[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // "timing": gather start, gathered, merged, flagged, placed
  vaqhip_multi_refiner_search_timing x_timing = {};
  int x_k = 0, x_k1 = 0, x_lists = 0;     // of the search in flight: k, entries per list, lists gathered
  int x_slot[VAQHIP_MAX_DEVICES] = {};    //   where shard g's list sits among them
  int x_last = 0;                         //   the last shard that holds rows (0 when none does)
  bool x_chain = false;                   //   "exact_ties" and some shard holds rows: k1 = k + 1, flag step, chain
  // the set in flight
  const float *d_q0 = nullptr;
  const int32_t *d_lin0 = nullptr;
  int nq = 0, R = 0, set_no = 0;
  size_t plane() const { return (size_t)nq * R; }
};

namespace {

constexpr int REFINE_MAX_R = 2048;
// Queries per set: the planes of one set take G * SET_QUERIES * R * 4 bytes on the first device (512 MB at
// G = 8, R = 1024).  Results do not depend on it: a query's answer depends on its own candidates only.
constexpr int SET_QUERIES = VAQHIP_MULTI_REFINER_SET;

int check_sizes(const vaqhip_multi_refiner *r, int nq, int R, int k) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (nq < 0 || R <= 0 || k <= 0) return mfail(VAQHIP_EINVAL, "bad sizes (nq=%d R=%d k=%d)", nq, R, k);
  if (R > REFINE_MAX_R || k > R) return mfail(VAQHIP_EUNSUPPORTED, "need k <= R <= %d (R=%d k=%d)", REFINE_MAX_R, R, k);
  return VAQHIP_OK;
}

int check_labels_fit(int64_t N, int64_t id_base) {
  if (id_base < 0) return mfail(VAQHIP_EINVAL, "id_base < 0");
  if (N > 0x7fffffffLL - 1 || id_base + N > 0x7fffffffLL)
    return mfail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld", (long long)(id_base + N));
  return VAQHIP_OK;
}

// `n` timing events more where the vector is short
int fit_events(std::vector<hipEvent_t> &v, size_t n) {
  while (v.size() < n) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return VAQHIP_EHIP;
    v.push_back(e);
  }
  return 0;
}

// room for `rows` rows on the shard whose device is current; keep: the first s.n rows survive the move
int reserve_rows(vaqhip_multi_refiner *r, RShard &s, int64_t rows, bool keep) {
  if (rows <= s.cap_rows) return 0;
  const int64_t want = keep ? std::max(rows, s.cap_rows + s.cap_rows / 2) : rows;
  DevBuf nb;
  MHIP(nb.ensure((size_t)want * r->D * sizeof(float)));
  MHIP(hipDeviceSynchronize());  // (a refine enqueued on any stream may still read the old rows)
  if (keep && s.n > 0) MHIP(hipMemcpy(nb.p, s.d_rows.p, (size_t)s.n * r->D * sizeof(float), hipMemcpyDeviceToDevice));
  std::swap(nb.p, s.d_rows.p);
  std::swap(nb.cap, s.d_rows.cap);
  s.cap_rows = want;
  return 0;
}

// every stream idle: after a call that failed part-way, before anything it may still read is freed or reused
void drain(vaqhip_multi_refiner *r) {
  for (RShard &s : r->sh)
    if (hipSetDevice(s.device) == hipSuccess) (void)hipStreamSynchronize(s.stream);
  (void)hipSetDevice(r->sh[0].device);
  r->dirty = false;
}

// Phases 1 and 2 of a set, on the shard's worker: buffers, the broadcast, the distances.
int enqueue_shard(vaqhip_multi_refiner *r, int g, RShard &s) {
  const int nq = r->nq, R = r->R, D = r->D;
  const bool timing = r->opt_timing != 0;
  MHIP(hipSetDevice(s.device));
  if (timing && fit_events(s.t, 3 * (size_t)(r->set_no + 1))) {
    s.err = "hipEventCreate failed";
    return VAQHIP_EHIP;
  }
  hipEvent_t *t = timing ? &s.t[3 * (size_t)r->set_no] : nullptr;
  // Growing frees the old buffer, which the last set's gather and select (on shard 0's stream) may still read:
  // `finished` follows all of them.  In steady state nothing grows and nothing here waits.
  struct Fit { DevBuf *b; size_t bytes; } fit[3];
  int n = 0;
  if (g == 0) fit[n++] = Fit{&r->d_planes, (size_t)r->G * r->plane() * sizeof(float)};
  else if (s.n > 0) {
    fit[n++] = Fit{&s.d_q, (size_t)nq * D * sizeof(float)};
    fit[n++] = Fit{&s.d_lin, r->plane() * sizeof(int32_t)};
    fit[n++] = Fit{&s.d_plane, r->plane() * sizeof(float)};
  }
  bool grows = false;
  for (int i = 0; i < n; i++) grows |= fit[i].bytes > fit[i].b->cap;
  if (grows) MHIP(hipEventSynchronize(r->finished));
  for (int i = 0; i < n; i++) MHIP(fit[i].b->ensure(fit[i].bytes));
  // the previous set has been read (never recorded: no wait); the caller's inputs are there
  MHIP(hipStreamWaitEvent(s.stream, r->finished, 0));
  MHIP(hipStreamWaitEvent(s.stream, r->user_ready, 0));
  if (t) MHIP(hipEventRecord(t[0], s.stream));
  const float *dq = r->d_q0;
  const int32_t *dl = r->d_lin0;
  float *plane = r->d_planes.as<float>();  // shard 0: plane 0 of the gathered buffer
  if (g > 0 && s.n > 0) {
    const int dev0 = r->sh[0].device;
    MHIP(hipMemcpyPeerAsync(s.d_q.p, s.device, r->d_q0, dev0, (size_t)nq * D * sizeof(float), s.stream));
    MHIP(hipMemcpyPeerAsync(s.d_lin.p, s.device, r->d_lin0, dev0, r->plane() * sizeof(int32_t), s.stream));
    dq = s.d_q.as<float>();
    dl = s.d_lin.as<int32_t>();
    plane = s.d_plane.as<float>();
  }
  if (t) MHIP(hipEventRecord(t[1], s.stream));
  MHIP(vaq::launch_refine_dist(dq, nq, D, s.d_rows.as<float>(), s.n, r->id_base + s.lo, dl, R, plane, s.stream));
  if (t) MHIP(hipEventRecord(t[2], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

// Phases 3 and 4, by the calling thread on the first device, once every shard's part is enqueued
int gather_and_select(vaqhip_multi_refiner *r, int k, int32_t *d_lout, float *d_dout, hipStream_t user) {
  RShard &s = r->sh[0];
  const bool timing = r->opt_timing != 0;
  MHIP(hipSetDevice(s.device));
  if (timing && fit_events(r->t, 3 * (size_t)(r->set_no + 1))) {
    s.err = "hipEventCreate failed";
    return VAQHIP_EHIP;
  }
  hipEvent_t *t = timing ? &r->t[3 * (size_t)r->set_no] : nullptr;
  for (int g = 1; g < r->G; g++) MHIP(hipStreamWaitEvent(s.stream, r->sh[g].done, 0));
  if (t) MHIP(hipEventRecord(t[0], s.stream));
  float *planes = r->d_planes.as<float>();
  for (int g = 1; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (u.n > 0)  // (an empty shard owns no label: its plane is never read)
      MHIP(hipMemcpyPeerAsync(planes + (size_t)g * r->plane(), s.device, u.d_plane.p, u.device, r->plane() * sizeof(float),
                              s.stream));
  }
  if (t) MHIP(hipEventRecord(t[1], s.stream));
  MHIP(vaq::launch_refine_select(r->d_lin0, r->nq, planes, r->plane(), r->bounds, r->R, k, r->opt_exact, d_lout, d_dout,
                                 s.stream));
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
  const bool timing = r->opt_timing != 0;
  r->last_sets = 0;
  r->last_single = r->G == 1;
  if (r->G == 1) {  // the single refiner's call, at its cost
    hipError_t e = hipSuccess;
    if (timing && fit_events(r->t, 3)) return mfail(VAQHIP_EHIP, "hipEventCreate failed");
    if (timing) e = hipEventRecord(r->t[0], user);
    if (e == hipSuccess)
      e = vaq::launch_refine_rows(d_q, nq, r->D, s0.d_rows.as<float>(), r->N, r->id_base, d_lin, R, k, r->opt_exact, d_lout,
                                  d_dout, user);
    if (e == hipSuccess && timing) e = hipEventRecord(r->t[1], user);
    if (e != hipSuccess) return mfail(hip_code(e), "refine on device %d: %s", s0.device, hipGetErrorString(e));
    r->last_sets = timing ? 1 : 0;
    return VAQHIP_OK;
  }
  if (r->dirty) drain(r);
  if (hipEventRecord(r->user_ready, user) != hipSuccess) return mfail(VAQHIP_EHIP, "recording the caller's stream");
  for (int q0 = 0, set_no = 0; q0 < nq; q0 += SET_QUERIES, set_no++) {
    r->nq = std::min(SET_QUERIES, nq - q0);
    r->R = R;
    r->set_no = set_no;
    r->d_q0 = d_q + (size_t)q0 * r->D;
    r->d_lin0 = d_lin + (size_t)q0 * R;
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

// the host form of a device call: sets of SET_QUERIES through the staging buffers on the first device
template <class Call> int through_staging(vaqhip_multi_refiner *r, const float *queries, int nq, const int32_t *labels_in,
                                          int R, int k, int32_t *labels_out, float *distances_out, Call &&call) {
  RShard &s = r->sh[0];
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  const int chunk = std::min(nq, SET_QUERIES);
  if (r->dirty) drain(r);
  s.err.clear();
  auto body = [&]() -> int {
    MHIP(hipEventSynchronize(r->finished));  // (the staging may grow: nothing reads it any more)
    MHIP(r->w_q.ensure((size_t)chunk * r->D * sizeof(float)));
    if (labels_in) MHIP(r->w_lin.ensure((size_t)chunk * R * sizeof(int32_t)));
    MHIP(r->w_lout.ensure((size_t)chunk * k * sizeof(int32_t)));
    MHIP(r->w_dout.ensure((size_t)chunk * k * sizeof(float)));
    hipStream_t st = s.stream;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
      const int n = std::min(chunk, nq - q0);
      MHIP(hipSetDevice(s.device));
      MHIP(hipMemcpyAsync(r->w_q.p, queries + (size_t)q0 * r->D, (size_t)n * r->D * sizeof(float), hipMemcpyHostToDevice, st));
      if (labels_in)
        MHIP(hipMemcpyAsync(r->w_lin.p, labels_in + (size_t)q0 * R, (size_t)n * R * sizeof(int32_t), hipMemcpyHostToDevice, st));
      if (const int rc = call(n, st)) return rc;
      MHIP(hipSetDevice(s.device));
      MHIP(hipMemcpyAsync(labels_out + (size_t)q0 * k, r->w_lout.p, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      MHIP(hipMemcpyAsync(distances_out + (size_t)q0 * k, r->w_dout.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
      MHIP(hipStreamSynchronize(st));
    }
    return 0;
  };
  const int rc = body();
  if (rc && !s.err.empty()) return mfail(rc, "device %d: %s", s.device, s.err.c_str());
  return rc;
}

// the index and the refiner of a fused call must describe the same rows on the same devices
int check_pair(vaqhip_multi *mx, const vaqhip_multi_refiner *r, int R) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (R > VAQHIP_MAX_K) return mfail(VAQHIP_EUNSUPPORTED, "R=%d > %d (the search returns the candidates)", R, VAQHIP_MAX_K);
  vaqhip_multi_info inf;
  if (const int rc = vaqhip_multi_get_info(mx, &inf)) return rc;
  if (mx->D != r->D) return mfail(VAQHIP_EINVAL, "the index has D=%d, the refiner D=%d", mx->D, r->D);
  bool same = inf.n_devices == r->G;
  for (int g = 0; same && g < r->G; g++) same = inf.device_ids[g] == r->sh[g].device;
  if (!same) return mfail(VAQHIP_EINVAL, "the index and the refiner name different device lists");
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
  if (bytes > r->w_cand_l.cap) {  // (the last fused call's shards and select read the old buffers)
    hipError_t e = hipEventSynchronize(r->finished);
    if (e == hipSuccess) e = r->w_cand_l.ensure(bytes);
    if (e == hipSuccess) e = r->w_cand_d.ensure(bytes);
    if (e != hipSuccess) return mfail(hip_code(e), "candidate buffers on device %d: %s", s.device, hipGetErrorString(e));
  }
  if (const int rc = vaqhip_multi_search_device(mx, d_q, nq, R, 0, r->w_cand_l.as<int32_t>(), r->w_cand_d.as<float>(), st))
    return rc;
  return refine_device_locked(r, d_q, nq, r->w_cand_l.as<int32_t>(), R, k, d_lout, d_dout, st);
}


// ---- the exhaustive form across shards ----
// the gathered lists of one set, in bytes on the first device (the set is cut to fit; every shard's own candidate
// lists are bounded by XS_LIST_BYTES as in the single form)
constexpr size_t XS_GATHER_BYTES = (size_t)256 << 20;

int check_search(const vaqhip_multi_refiner *r, int nq, int k, const void *a, const void *b, const void *c) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (nq < 0 || k < 1) return mfail(VAQHIP_EINVAL, "bad sizes (nq=%d k=%d)", nq, k);
  if (k > VAQHIP_MAX_K) return mfail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (nq > 0 && (!a || !b || !c)) return mfail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

bool xs_takes_part(int g, const RShard &s) { return g == 0 || s.n > 0; }  // (shard 0 hosts the merge even without rows)

// Phase A of a set, on the shard's worker: buffers, the queries, select + merge over the shard's own rows
int xs_enqueue_shard(vaqhip_multi_refiner *r, int g, RShard &s) {
  if (!xs_takes_part(g, s)) return 0;  // (owns no label: no list, no link)
  const int n = r->nq, D = r->D, k = r->x_k, k1 = r->x_k1;
  const bool exact = r->x_chain, timing = r->opt_timing != 0;
  MHIP(hipSetDevice(s.device));
  // Growing frees a buffer the last set's gather, merge and chain may still read: `finished` follows all of them.
  const size_t lists = (size_t)n * k1 * 4, state = (size_t)n * k * 4, list = ((size_t)n + 1) * 4;
  struct Fit { DevBuf *b; size_t bytes; } fit[16];
  int nf = 0;
  if (g == 0) {
    const size_t ms = vaq::merge_scratch_elems(r->x_lists, n, k1) * 4;
    for (DevBuf *b : {&r->x_gl, &r->x_gd}) fit[nf++] = Fit{b, (size_t)r->x_lists * lists};
    for (DevBuf *b : {&r->x_ms_d, &r->x_ms_id}) fit[nf++] = Fit{b, ms};
    if (exact) {
      for (DevBuf *b : {&r->x_k1_l, &r->x_k1_d}) fit[nf++] = Fit{b, lists};
      fit[nf++] = Fit{&r->x_list, list};
    }
  } else {
    fit[nf++] = Fit{&s.d_q, (size_t)n * D * sizeof(float)};
    for (DevBuf *b : {&s.x_l, &s.x_d}) fit[nf++] = Fit{b, lists};
    if (exact) fit[nf++] = Fit{&s.x_list, list};
  }
  if (exact)
    for (DevBuf *b : {&s.x_hin_v, &s.x_hin_i, &s.x_hout_v, &s.x_hout_i}) fit[nf++] = Fit{b, state};
  bool grows = !s.xs.fits(s.xpl, k1, false);
  for (int i = 0; i < nf; i++) grows |= fit[i].bytes > fit[i].b->cap;
  if (grows) MHIP(hipEventSynchronize(r->finished));
  for (int i = 0; i < nf; i++) MHIP(fit[i].b->ensure(fit[i].bytes));
  MHIP(s.xs.fit(s.xpl, k1, false, false));
  if (timing)
    for (hipEvent_t &e : s.xt)
      if (!e) MHIP(hipEventCreate(&e));
  // the previous set has been read (never recorded: no wait); the caller's inputs are there
  MHIP(hipStreamWaitEvent(s.stream, r->finished, 0));
  MHIP(hipStreamWaitEvent(s.stream, r->user_ready, 0));
  if (timing) MHIP(hipEventRecord(s.xt[0], s.stream));
  const float *dq = r->d_q0;
  int32_t *out_l = r->x_gl.as<int32_t>();  // shard 0: list 0 of the gathered lists
  float *out_d = r->x_gd.as<float>();
  if (g > 0) {
    MHIP(hipMemcpyPeerAsync(s.d_q.p, s.device, r->d_q0, r->sh[0].device, (size_t)n * D * sizeof(float), s.stream));
    dq = s.d_q.as<float>();
    out_l = s.x_l.as<int32_t>();
    out_d = s.x_d.as<float>();
  }
  const XsRows rows = {s.d_rows.as<float>(), s.n, r->id_base + s.lo, D};
  MHIP(xs_select_merge(s.xs, s.xpl, rows, dq, n, k1, out_l, out_d, s.stream, timing ? s.xt[1] : nullptr, &s.x_wgs, &s.x_qg));
  if (timing) MHIP(hipEventRecord(s.xt[2], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

// Phases B and C, by the calling thread on the first device, once every shard's part is enqueued
int xs_gather_merge_flag(vaqhip_multi_refiner *r, int32_t *d_lout, float *d_dout) {
  RShard &s = r->sh[0];
  const int n = r->nq, k = r->x_k, k1 = r->x_k1;
  const bool exact = r->x_chain, timing = r->opt_timing != 0;
  const size_t plane = (size_t)n * k1;
  MHIP(hipSetDevice(s.device));
  if (timing)
    for (hipEvent_t &e : r->xt)
      if (!e) MHIP(hipEventCreate(&e));
  for (int g = 1; g < r->G; g++)
    if (r->sh[g].n > 0) MHIP(hipStreamWaitEvent(s.stream, r->sh[g].done, 0));
  if (timing) MHIP(hipEventRecord(r->xt[0], s.stream));
  for (int g = 1; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (u.n == 0) continue;
    const size_t at = (size_t)r->x_slot[g] * plane;
    MHIP(hipMemcpyPeerAsync(r->x_gl.as<int32_t>() + at, s.device, u.x_l.p, u.device, plane * 4, s.stream));
    MHIP(hipMemcpyPeerAsync(r->x_gd.as<float>() + at, s.device, u.x_d.p, u.device, plane * 4, s.stream));
  }
  if (timing) MHIP(hipEventRecord(r->xt[1], s.stream));
  int32_t *m_l = exact ? r->x_k1_l.as<int32_t>() : d_lout;
  float *m_d = exact ? r->x_k1_d.as<float>() : d_dout;
  MHIP(vaq::launch_merge(r->x_gd.as<float>(), r->x_gl.as<int>(), nullptr, r->x_lists, (int64_t)plane, (int64_t)k1, n, k1, 0, 1,
                         m_l, m_d, nullptr, r->x_ms_d.as<float>(), r->x_ms_id.as<int>(), s.stream));
  if (timing) MHIP(hipEventRecord(r->xt[2], s.stream));
  if (exact) {
    int *list = r->x_list.as<int>();
    MHIP(vaq::launch_exact_flag(n, k, m_l, m_d, d_lout, d_dout, list, reinterpret_cast<unsigned *>(list + n), s.stream));
    MHIP(hipEventRecord(r->flagged, s.stream));
  }
  if (timing) MHIP(hipEventRecord(r->xt[3], s.stream));
  return 0;
}

// One link of phase D on shard g, by the calling thread: the list, the heap arrays of the link before (prev < 0: none),
// the replay over the shard's rows.  Enqueued in chain order: `flagged` and the previous link's event are recorded.
int xs_link(vaqhip_multi_refiner *r, int g, int prev, int32_t *d_lout, float *d_dout) {
  RShard &s = r->sh[g];
  const int n = r->nq, k = r->x_k, dev0 = r->sh[0].device;
  const bool timing = r->opt_timing != 0, last = g == r->x_last;
  const size_t state = (size_t)n * k * 4;
  MHIP(hipSetDevice(s.device));
  const float *dq = r->d_q0;
  const int *list = r->x_list.as<int>();
  if (g > 0) {  // (shard 0's stream holds the flag step itself)
    MHIP(hipStreamWaitEvent(s.stream, r->flagged, 0));
    MHIP(hipMemcpyPeerAsync(s.x_list.p, s.device, r->x_list.p, dev0, ((size_t)n + 1) * 4, s.stream));
    dq = s.d_q.as<float>();  // (there since phase A)
    list = s.x_list.as<int>();
  }
  if (prev >= 0) {
    const RShard &u = r->sh[prev];
    MHIP(hipStreamWaitEvent(s.stream, u.link, 0));
    MHIP(hipMemcpyPeerAsync(s.x_hin_v.p, s.device, u.x_hout_v.p, u.device, state, s.stream));
    MHIP(hipMemcpyPeerAsync(s.x_hin_i.p, s.device, u.x_hout_i.p, u.device, state, s.stream));
  }
  if (timing) MHIP(hipEventRecord(s.xt[3], s.stream));
  const bool direct = last && g == 0;  // (all rows on the first shard: its link writes the caller's buffers)
  MHIP(vaq::launch_exhaust_replay_link(dq, n, r->D, s.d_rows.as<float>(), s.n, r->id_base + s.lo, k, list,
                                       reinterpret_cast<const unsigned *>(list + n), prev >= 0 ? s.x_hin_v.as<float>() : nullptr,
                                       prev >= 0 ? s.x_hin_i.as<int>() : nullptr, direct ? nullptr : s.x_hout_v.as<float>(),
                                       direct ? nullptr : s.x_hout_i.as<int>(), last ? 1 : 0, direct ? d_lout : nullptr,
                                       direct ? d_dout : nullptr, s.stream));
  if (timing) MHIP(hipEventRecord(s.xt[4], s.stream));
  MHIP(hipEventRecord(s.link, s.stream));
  return 0;
}

// the end of a set on the first device: with a chain, the last link's slots placed at their queries
int xs_finish(vaqhip_multi_refiner *r, bool chain, int32_t *d_lout, float *d_dout, hipStream_t user) {
  RShard &s = r->sh[0];
  const int n = r->nq, k = r->x_k;
  MHIP(hipSetDevice(s.device));
  if (chain && r->x_last > 0) {
    const RShard &u = r->sh[r->x_last];
    const size_t state = (size_t)n * k * 4;
    const int *list = r->x_list.as<int>();
    MHIP(hipStreamWaitEvent(s.stream, u.link, 0));
    MHIP(hipMemcpyPeerAsync(s.x_hin_v.p, s.device, u.x_hout_v.p, u.device, state, s.stream));
    MHIP(hipMemcpyPeerAsync(s.x_hin_i.p, s.device, u.x_hout_i.p, u.device, state, s.stream));
    MHIP(vaq::launch_exhaust_scatter(n, k, list, reinterpret_cast<const unsigned *>(list + n), s.x_hin_v.as<float>(),
                                     s.x_hin_i.as<int>(), d_lout, d_dout, s.stream));
  }
  if (r->opt_timing) MHIP(hipEventRecord(r->xt[4], s.stream));
  MHIP(hipEventRecord(r->finished, s.stream));
  MHIP(hipStreamWaitEvent(user, r->finished, 0));
  return 0;
}

// option "timing": waits for the set and adds its figures (the slowest shard's select, merge and link)
int xs_read_timing(vaqhip_multi_refiner *r, bool chain) {
  RShard &s = r->sh[0];
  vaqhip_multi_refiner_search_timing &t = r->x_timing;
  auto span = [](hipEvent_t a, hipEvent_t b, float *ms) { return hipEventElapsedTime(ms, a, b); };
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventSynchronize(r->finished));
  float sel = 0, mer = 0, rep = 0, ms = 0;
  for (int g = 0; g < r->G; g++) {
    RShard &u = r->sh[g];
    if (!xs_takes_part(g, u)) continue;
    MHIP(hipSetDevice(u.device));
    MHIP(span(u.xt[0], u.xt[1], &ms));
    sel = std::max(sel, ms);
    MHIP(span(u.xt[1], u.xt[2], &ms));
    mer = std::max(mer, ms);
    if (chain && u.n > 0) {
      MHIP(span(u.xt[3], u.xt[4], &ms));
      rep = std::max(rep, ms);
    }
  }
  MHIP(hipSetDevice(s.device));
  t.select_ms += sel;
  t.merge_ms += mer;
  t.replay_ms += rep;
  MHIP(span(r->xt[0], r->xt[1], &ms));
  t.gather_ms += ms;
  MHIP(span(r->xt[1], r->xt[2], &ms));
  t.cross_merge_ms += ms;
  MHIP(span(r->xt[2], r->xt[3], &ms));
  t.flag_ms += ms;
  MHIP(span(r->xt[3], r->xt[4], &ms));
  if (chain) t.chain_ms += ms;
  if (chain) {
    unsigned listed = 0;
    MHIP(hipMemcpy(&listed, r->x_list.as<int>() + r->nq, sizeof(unsigned), hipMemcpyDeviceToHost));
    t.listed_queries += (int)listed;
  }
  return 0;
}

// Device pointers on the first device, enqueue only; r->mu held.  As refine_device_locked.
int search_device_locked(vaqhip_multi_refiner *r, const float *d_q, int nq, int k, int32_t *d_lout, float *d_dout,
                         hipStream_t user) {
  RShard &s = r->sh[0];
  bool any_cap = false;
  for (const RShard &u : r->sh) any_cap |= u.cap_rows > 0;
  if (r->N == 0 && !any_cap) return mfail(VAQHIP_ESTATE, "no rows were set");
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  const bool exact = r->opt_exact != 0, timing = r->opt_timing != 0;
  s.err.clear();
  r->x_timing = {};
  r->x_timing.register_form = r->D <= (int)vaq::exhaust_register_max_dim();
  if (r->G == 1) {  // the single refiner's launches, at their cost, on the caller's stream
    auto body = [&]() -> int {
      MHIP(s.xs.size_for(s.device, r->D));
      const int k1 = exact ? k + 1 : k;
      const XsPlan pl = xs_plan(s.xs, r->N, r->opt_splits, nq, k1);
      MHIP(s.xs.fit(pl, k1, exact, timing));
      MHIP(hipStreamWaitEvent(user, r->finished, 0));  // (the workspace is shared by the callers' streams)
      const XsRows rows = {s.d_rows.as<float>(), r->N, r->id_base, r->D};
      vaqhip_refiner_search_timing t1 = {};
      hipError_t e = hipSuccess;
      int sets = 0;
      for (int q0 = 0; q0 < nq && e == hipSuccess; q0 += pl.chunk, sets++)
        e = xs_search_set(s.xs, pl, rows, d_q + (size_t)q0 * r->D, std::min(pl.chunk, nq - q0), k, exact,
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
  r->x_lists = 0;
  r->x_last = 0;
  for (int g = 0; g < r->G; g++) {
    const RShard &u = r->sh[g];
    if (!xs_takes_part(g, u)) continue;
    r->x_slot[g] = r->x_lists++;
    if (u.n > 0) {
      if (first < 0) first = g;
      r->x_last = g;
    }
  }
  const bool chain = exact && first >= 0;  // (no rows at all: every slot is -1 / FLT_MAX under either rule)
  const int k1 = chain ? k + 1 : k;
  r->x_chain = chain;
  r->x_k = k;
  r->x_k1 = k1;
  int set = std::min(nq, SET_QUERIES);
  set = (int)std::min<size_t>((size_t)set, std::max<size_t>(1, XS_GATHER_BYTES / ((size_t)r->x_lists * k1 * 8)));
  auto plan = [&](int max_chunk) -> int {
    for (int g = 0; g < r->G; g++) {
      RShard &u = r->sh[g];
      if (!xs_takes_part(g, u)) continue;
      if (hipSetDevice(u.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", u.device);
      const hipError_t e = u.xs.size_for(u.device, r->D);
      if (e != hipSuccess) return mfail(hip_code(e), "device %d: %s", u.device, hipGetErrorString(e));
      u.xpl = xs_plan(u.xs, u.n, r->opt_splits, nq, k1, max_chunk);
      set = std::min(set, u.xpl.chunk);
    }
    return VAQHIP_OK;
  };
  if (const int rc = plan(set)) return rc;  // every shard's own bound ...
  if (const int rc = plan(set)) return rc;  // ... and the smallest of them for all: equal sets of one size
  set = r->sh[0].xpl.chunk;
  r->x_timing.splits = r->sh[std::max(first, 0)].xpl.S;
  r->x_timing.chain_shards = first < 0 ? 0 : r->x_lists - (r->sh[0].n > 0 ? 0 : 1);
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  if (hipEventRecord(r->user_ready, user) != hipSuccess) return mfail(VAQHIP_EHIP, "recording the caller's stream");
  for (int q0 = 0; q0 < nq; q0 += set) {
    r->nq = std::min(set, nq - q0);
    r->d_q0 = d_q + (size_t)q0 * r->D;
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
    r->x_timing.workgroups = r->sh[std::max(first, 0)].x_wgs;
    r->x_timing.queries_per_group = r->sh[std::max(first, 0)].x_qg;
  }
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
    for (DevBuf *b : {&s.d_rows, &s.d_q, &s.d_lin, &s.d_plane, &s.x_l, &s.x_d, &s.x_list, &s.x_hin_v, &s.x_hin_i, &s.x_hout_v,
                      &s.x_hout_i})
      b->release();
    s.xs.release();
    for (hipEvent_t e : s.t) (void)hipEventDestroy(e);
    for (hipEvent_t e : s.xt)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {s.done, s.link})
      if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (!r->sh.empty()) (void)hipSetDevice(r->sh[0].device);
  for (DevBuf *b : {&r->d_planes, &r->w_q, &r->w_lin, &r->w_lout, &r->w_dout, &r->w_cand_l, &r->w_cand_d, &r->x_gl, &r->x_gd,
                    &r->x_ms_d, &r->x_ms_id, &r->x_k1_l, &r->x_k1_d, &r->x_list})
    b->release();
  for (hipEvent_t e : r->t) (void)hipEventDestroy(e);
  for (hipEvent_t e : r->xt)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {r->user_ready, r->finished, r->flagged})
    if (e) (void)hipEventDestroy(e);
  delete r;
}

int vaqhip_multi_refiner_set_rows(vaqhip_multi_refiner *r, const float *X, int64_t N, int64_t id_base) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (N < 0 || (N > 0 && !X)) return mfail(VAQHIP_EINVAL, "bad rows");
  if (const int rc = check_labels_fit(N, id_base)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  const vaq::RefineBounds cut = vaq::refine_cut(N, r->G, id_base);
  // every shard uploads its own rows, all of them at once
  if (const int rc = on_shards(r, [&](int g, RShard &s) {
        MHIP(hipSetDevice(s.device));
        const int64_t lo = cut.b[g] - id_base, n = cut.b[g + 1] - cut.b[g];
        s.n = 0;
        if (const int rc = reserve_rows(r, s, n, false)) return rc;
        MHIP(hipDeviceSynchronize());
        if (n > 0) MHIP(hipMemcpy(s.d_rows.p, X + (size_t)lo * r->D, (size_t)n * r->D * sizeof(float), hipMemcpyHostToDevice));
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

int vaqhip_multi_refiner_add_rows(vaqhip_multi_refiner *r, const float *X, int64_t n_new) {
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  if (n_new < 0 || (n_new > 0 && !X)) return mfail(VAQHIP_EINVAL, "bad rows");
  if (n_new == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  if (const int rc = check_labels_fit(r->N + n_new, r->id_base)) return rc;
  // the new rows continue the numbering, so they extend the LAST shard, as vaqhip_multi_add_codes_u16 does
  RShard &s = r->sh[r->G - 1];
  DeviceGuard g(s.device);
  if (!g.ok) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  s.err.clear();
  auto body = [&]() -> int {
    if (const int rc = reserve_rows(r, s, s.n + n_new, true)) return rc;
    // (rows past s.n are read by no launch in flight: no wait is needed before they are written)
    MHIP(hipMemcpy(s.d_rows.as<float>() + (size_t)s.n * r->D, X, (size_t)n_new * r->D * sizeof(float), hipMemcpyHostToDevice));
    return 0;
  };
  if (const int rc = body()) return mfail(rc, "shard %d (device %d): %s", r->G - 1, s.device, s.err.c_str());
  s.n += n_new;
  r->N += n_new;
  vaq::refine_grow_last(r->bounds, n_new);
  return VAQHIP_OK;
}

int vaqhip_multi_refiner_set_option(vaqhip_multi_refiner *r, const char *key, int64_t value) {
  if (!r || !key) return mfail(VAQHIP_EINVAL, "null pointer");
  const bool exact = std::strcmp(key, "exact_ties") == 0, timing = std::strcmp(key, "timing") == 0,
             splits = std::strcmp(key, "exhaustive_splits") == 0;
  if (!exact && !timing && !splits) return mfail(VAQHIP_EINVAL, "unknown option '%s'", key);
  if (splits && (value < 0 || value > 64))  // (refused before the refiner is touched)
    return mfail(VAQHIP_EINVAL, "exhaustive_splits=%lld: 0 (automatic) or 1..64", (long long)value);
  std::lock_guard<std::mutex> lk(r->mu);
  if (exact) r->opt_exact = value != 0;
  else if (timing) r->opt_timing = value != 0;
  else r->opt_splits = (int)value;
  return VAQHIP_OK;
}

int vaqhip_multi_refiner_refine_device(vaqhip_multi_refiner *r, const float *d_queries, int nq, const int32_t *d_labels_in,
                                       int R, int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (const int rc = check_sizes(r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries || !d_labels_in || !d_labels_out || !d_distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return refine_device_locked(r, d_queries, nq, d_labels_in, R, k, d_labels_out, d_distances_out,
                              static_cast<hipStream_t>(stream));
}

int vaqhip_multi_refiner_refine(vaqhip_multi_refiner *r, const float *queries, int nq, const int32_t *labels_in, int R,
                                int k, int32_t *labels_out, float *distances_out) {
  if (const int rc = check_sizes(r, nq, R, k)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !labels_in || !labels_out || !distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return through_staging(r, queries, nq, labels_in, R, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return refine_device_locked(r, r->w_q.as<float>(), n, r->w_lin.as<int32_t>(), R, k, r->w_lout.as<int32_t>(),
                                r->w_dout.as<float>(), st);
  });
}

int vaqhip_multi_search_refine_device(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *d_queries_raw, int nq, int R,
                                      int k, int32_t *d_labels_out, float *d_distances_out, void *stream) {
  if (const int rc = check_sizes(r, nq, R, k)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  if (const int rc = check_pair(mx, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!d_queries_raw || !d_labels_out || !d_distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard keep(DeviceGuard::restore_only);
  return search_refine_locked(mx, r, d_queries_raw, nq, R, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_multi_search_refine(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *queries_raw, int nq, int R, int k,
                               int32_t *labels_out, float *distances_out) {
  if (const int rc = check_sizes(r, nq, R, k)) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  if (const int rc = check_pair(mx, r, R)) return rc;
  if (nq == 0) return VAQHIP_OK;
  if (!queries_raw || !labels_out || !distances_out) return mfail(VAQHIP_EINVAL, "null pointer");
  DeviceGuard keep(DeviceGuard::restore_only);
  return through_staging(r, queries_raw, nq, nullptr, R, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return search_refine_locked(mx, r, r->w_q.as<float>(), n, R, k, r->w_lout.as<int32_t>(), r->w_dout.as<float>(), st);
  });
}

int vaqhip_multi_refiner_search_device(vaqhip_multi_refiner *r, const float *d_queries, int nq, int k, int32_t *d_labels_out,
                                       float *d_distances_out, void *stream) {
  if (const int rc = check_search(r, nq, k, d_queries, d_labels_out, d_distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  return search_device_locked(r, d_queries, nq, k, d_labels_out, d_distances_out, static_cast<hipStream_t>(stream));
}

int vaqhip_multi_refiner_search(vaqhip_multi_refiner *r, const float *queries, int nq, int k, int32_t *labels_out,
                                float *distances_out) {
  if (const int rc = check_search(r, nq, k, queries, labels_out, distances_out)) return rc;
  if (nq == 0) return VAQHIP_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  // (under "timing" the figures are the last staged set's: the bench and the tests stay within one)
  return through_staging(r, queries, nq, nullptr, 0, k, labels_out, distances_out, [&](int n, hipStream_t st) {
    return search_device_locked(r, r->w_q.as<float>(), n, k, r->w_lout.as<int32_t>(), r->w_dout.as<float>(), st);
  });
}

int vaqhip_multi_refiner_last_search_timing(vaqhip_multi_refiner *r, vaqhip_multi_refiner_search_timing *out) {
  if (!r || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  *out = r->x_timing;
  return VAQHIP_OK;
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
  out->exact_ties = r->opt_exact;
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
    ok = hipSetDevice(r->sh[0].device) == hipSuccess && span(r->t[0], r->t[1], &ms);
    out->last_distances_ms = ms;  // (one kernel: the distances and the selection together)
  } else {
    for (int i = 0; ok && i < r->last_sets; i++) {
      float bc = 0, di = 0;
      for (int g = 0; ok && g < r->G; g++) {
        const RShard &s = r->sh[g];
        ok = hipSetDevice(s.device) == hipSuccess && span(s.t[3 * i], s.t[3 * i + 1], &ms);
        bc = std::max(bc, ms);
        ok = ok && span(s.t[3 * i + 1], s.t[3 * i + 2], &ms);
        di = std::max(di, ms);
      }
      out->last_broadcast_ms += bc;
      out->last_distances_ms += di;
      ok = ok && hipSetDevice(r->sh[0].device) == hipSuccess && span(r->t[3 * i], r->t[3 * i + 1], &ms);
      out->last_gather_ms += ms;
      ok = ok && span(r->t[3 * i + 1], r->t[3 * i + 2], &ms);
      out->last_select_ms += ms;
    }
  }
  if (!ok) return mfail(VAQHIP_EHIP, "reading the timing events");
  out->last_sets = r->last_sets;
  return VAQHIP_OK;
}

}  // extern "C"
