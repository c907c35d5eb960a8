// vaqhip_multi_refiner.h -- what the two host files of the multi-device refiner share: the shard, the handle, the set
// of each form in flight (every buffer of a set is sized by it) and the two steps both forms take.  Buffers are
// grouped by form and device.  Private to vaqhip_multi_refiner.cpp (life cycle, rows, options, the refine form, the
// fused call) and vaqhip_multi_refiner_search.cpp (the exhaustive form); the builds from a refiner's rows (vaqhip_multi_encode.cpp,
// vaqhip_multi_learn.cpp, the sharded fits through vaqhip_shard_run.h) take resident_rows() and the pair checks.
#ifndef VAQHIP_MULTI_REFINER_H
#define VAQHIP_MULTI_REFINER_H
#include "vaqhip_multi.h"

#include "refine_owner.h"
#include "vaq_merge.h"
#include "vaqhip_refine_common.h"

namespace vaqhost __attribute__((visibility("hidden"))) {

// Queries per set: the planes of one set take G * SET_QUERIES * R * 4 bytes on the first device (512 MB at
// G = 8, R = 1024).  Results do not depend on it: a query's answer depends on its own candidates only.
constexpr int SET_QUERIES = VAQHIP_MULTI_REFINER_SET;
constexpr RefineHost MULTI_REFINER = {mfail, "multi refiner"};

// the refine form on a shard (shards 1..; shard 0 reads the caller's labels and writes into the gathered planes): the
// set's candidate labels and their float [nq][R] plane.  t: option "timing", per set start, broadcast, distances done
struct RefineShardBufs {
  DevBuf lin, plane;
  EventList t;
  void release() { release_all({&lin, &plane}), t.release(); }
};

// the refine form on the first device: the gathered float [G][set][R].  t: per set gather start, gathered, selected
struct RefineFirstBufs {
  DevBuf planes;
  EventList t;
  void release() { planes.release(), t.release(); }
};

// the exhaustive form on one shard: the device's workspace and its plan for the call in flight; shards 1..: the
// shard's [set][k1] lists (shard 0 writes into the gathered lists) and the replay list with its count; the chain's
// state, [set][k] raw heap arrays in and out (shard 0's hin receives the last link's finished slots)
struct SearchShardBufs {
  XsWork work;
  XsPlan plan = {1, 1, 1};
  int wgs = 0, qg = 0;
  DevBuf l, d, list, hin_v, hin_i, hout_v, hout_i;
  hipEvent_t t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // "timing": start, selected, merged; link start, end
  void release() { work.release(), release_all({&l, &d, &list, &hin_v, &hin_i, &hout_v, &hout_i}), destroy_events(t); }
};

// the exhaustive form on the first device: the gathered [lists][set][k1] labels and distances, the cross-shard
// merge's scratch, the merged k + 1 lists and the replay list with its count
struct SearchFirstBufs {
  DevBuf gl, gd, ms_d, ms_id, k1_l, k1_d, list;
  hipEvent_t t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // "timing": gather start, gathered, merged, flagged, placed
  void release() { release_all({&gl, &gd, &ms_d, &ms_id, &k1_l, &k1_d, &list}), destroy_events(t); }
};

struct RShard {
  int device = 0;
  int64_t lo = 0, n = 0;  // rows [lo, lo + n) of the dataset
  RowStore rows;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // this shard's plane (its lists) of the current set is complete
  hipEvent_t link = nullptr;  // this shard's link of the chain is complete
  DevBuf d_q;                 // shards 1..: the set's queries, either form
  RefineShardBufs rf;
  SearchShardBufs xs;
  std::string err;
  void release() { release_all({&rows.buf, &d_q}), rf.release(), xs.release(); }  // its device current and synchronised
};

// The refine form's set in flight: refine_device_locked fills it per set, every phase reads it.
struct RefineSet {
  const float *d_q0 = nullptr;  // on the first device, as the labels
  const int32_t *d_lin0 = nullptr;
  int nq = 0, R = 0, set_no = 0;
  size_t plane() const { return (size_t)nq * R; }  // entries of one shard's plane, of the set's labels
  size_t plane_bytes() const { return plane() * 4; }
  size_t query_bytes(int D) const { return (size_t)nq * D * sizeof(float); }
};

// The exhaustive form's call in flight: search_device_locked fills the plan once and nq, d_q0 per set.
struct SearchCall {
  int k = 0, k1 = 0, lists = 0;      // k, entries per list, lists gathered
  int slot[VAQHIP_MAX_DEVICES] = {};  //   where shard g's list sits among them
  int last = 0;                       //   the last shard that holds rows (0 when none does)
  bool chain = false;                 // "exact_ties" and some shard holds rows: k1 = k + 1, flag step, chain
  int nq = 0;                         // the set in flight, its queries on the first device
  const float *d_q0 = nullptr;
  size_t plane() const { return (size_t)nq * k1; }                   // entries of one shard's [nq][k1] lists
  size_t lists_bytes() const { return plane() * 4; }                 //   labels or distances
  size_t state_bytes() const { return (size_t)nq * k * 4; }          // one raw heap array of the chain
  size_t list_bytes() const { return ((size_t)nq + 1) * 4; }         // the replay list and its count
  size_t scratch_bytes() const { return vaq::merge_scratch_elems(lists, nq, k1) * 4; }  // of the cross-shard merge
  size_t query_bytes(int D) const { return (size_t)nq * D * sizeof(float); }
};

}  // namespace vaqhost

struct vaqhip_multi_refiner {
  __attribute__((visibility("hidden"))) ~vaqhip_multi_refiner() = default;
  int D = 0, G = 0;
  std::vector<vaqhost::RShard> sh;
  int64_t N = 0, id_base = 0;
  vaq::RefineBounds bounds = {};
  vaqhost::RefineOptions opt;
  std::mutex mu;  // one call at a time
  vaq::JobPool pool;
  hipEvent_t user_ready = nullptr;  // recorded on the caller's stream: its inputs are there
  hipEvent_t finished = nullptr;    // the last set's select (chain) is complete: every buffer of the set has been read
  hipEvent_t flagged = nullptr;     // the exhaustive form's replay list of the current set is complete
  bool dirty = false;               // a call failed part-way: `finished` does not cover what it enqueued
  vaqhost::StagingBufs w;
  vaqhost::RefineFirstBufs rf;
  vaqhost::RefineSet set;
  int last_sets = 0;         // sets of the last refine that carry timing events
  bool last_single = false;  //   it was the one-shard form (t[0], t[1] around the kernel)
  vaqhost::SearchFirstBufs x;
  vaqhost::SearchCall xc;
  vaqhip_multi_refiner_search_timing x_timing = {};
};

namespace vaqhost __attribute__((visibility("hidden"))) {

// the element size of the rows the refiner holds (4 or 1): every shard's store carries it, set together (r->mu held)
inline int rows_elem(const vaqhip_multi_refiner *r) { return r->sh[0].rows.elem; }

// every stream idle: after a call that failed part-way, before anything it may still read is freed or reused
void drain(vaqhip_multi_refiner *r);

// An index and a refiner that stand for the same rows: one D, one device list (neither changes after create).
inline int check_same_devices(const vaqhip_multi *mx, const vaqhip_multi_refiner *r) {
  if (mx->D != r->D) return mfail(VAQHIP_EINVAL, "the index has D=%d, the refiner D=%d", mx->D, r->D);
  bool same = mx->G == r->G;
  for (int g = 0; same && g < r->G; g++) same = mx->sh[g].device == r->sh[g].device;
  if (!same) return mfail(VAQHIP_EINVAL, "the index and the refiner name different device lists");
  return VAQHIP_OK;
}

// what a build of the index from the refiner's rows refuses (vaqhip_multi_encode*_from_refiner,
// vaqhip_multi_learn_quantization_from_refiner): the above, and a refiner without rows.  r->mu held.
inline int check_refiner_pair(const vaqhip_multi *mx, const vaqhip_multi_refiner *r) {
  if (const int rc = check_same_devices(mx, r)) return rc;
  if (r->N == 0) return mfail(VAQHIP_ESTATE, "the refiner holds no rows: vaqhip_multi_refiner_set_rows first");
  return VAQHIP_OK;
}

// Shard g's resident rows for the builds across the shards (vaqhip_multi_encode.cpp, vaqhip_shard_run.h), which read
// them in place on the shard's device: n rows of D floats or bytes (rows.elem), the first with label first_label.  r->mu held; set_rows and
// add_rows copy synchronously, so the rows are complete.
struct ResidentRows { vaq::RowsRef rows; int64_t n, first_label; };
inline ResidentRows resident_rows(const vaqhip_multi_refiner *r, int g) {
  const RShard &s = r->sh[g];
  return ResidentRows{s.rows.rows(), s.n, r->id_base + s.lo};
}

// The host form of a device call: sets of SET_QUERIES through the staging buffers on the first device (r->w); r->mu held
template <class Call> int through_staging(vaqhip_multi_refiner *r, const float *queries, int nq, const int32_t *labels_in,
                                          int R, int k, int32_t *labels_out, float *distances_out, Call &&call) {
  RShard &s = r->sh[0];
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", s.device);
  if (r->dirty) drain(r);
  s.err.clear();
  int rc = 0;
  hipError_t e = hipEventSynchronize(r->finished);  // (the staging may grow: nothing reads it any more)
  if (e == hipSuccess)  // (a call that succeeds leaves the first device current: its last step runs there)
    e = through_staging(r->w, s.stream, r->D, std::min(nq, SET_QUERIES), queries, nq, labels_in, R, k, labels_out, distances_out,
                        rc, [&](int n) { return call(n, s.stream); });
  if (e != hipSuccess) return mfail(hip_code(e), "device %d: %s", s.device, hipGetErrorString(e));
  if (rc && !s.err.empty()) return mfail(rc, "device %d: %s", s.device, s.err.c_str());
  return rc;
}

}  // namespace vaqhost
#endif
