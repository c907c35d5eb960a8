// vaqhip_multi.h -- what the host files of the multi-device index share: the shard, the index with the
// geometry of the search in flight, the error hand-over, the grow path of a phase's buffers, the two loops over
// shards and the copy between two shards' devices.  Private to vaqhip_multi.cpp (life cycle, codes, setters),
// vaqhip_multi_search.cpp (the search), vaqhip_multi_kmeans.cpp (the k-means of clusterTI), the builds across the
// shards -- vaqhip_multi_encode.cpp, vaqhip_multi_learn.cpp, and vaqhip_multi_lutfit.cpp and vaqhip_multi_codebooks.cpp,
// whose call-owned run (vaqhip_shard_run.h) is what on_shards works on there -- and,
// through vaqhip_multi_refiner.h, the refiner over sharded raw rows (vaqhip_multi_refiner.cpp,
// vaqhip_multi_refiner_search.cpp), which takes the error hand-over, the grow path and on_shards from here; they see a
// shard's index through include/vaqhip.h and vaqhip_internal.h only.
#ifndef VAQHIP_MULTI_H
#define VAQHIP_MULTI_H
#include "vaqhip.h"
#include "vaqhip_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <mutex>
#include <string>
#include <vector>

#include "job_pool.h"
#include "vaqhip_dev.h"
#include "vaqhip_rccl.h"

// (hidden: none of this joins the library's exported symbols)
namespace vaqhost __attribute__((visibility("hidden"))) {

enum Exchange { EX_AUTO = 0, EX_RCCL = 1, EX_COPIES = 2 };

struct Shard {
  vaqhip_index *ix = nullptr;
  int device = 0;
  int64_t lo = 0, n = 0;  // rows [lo, lo + n) of the database
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // this shard's packed result is complete
  DevBuf d_queries;   // float [nq][D]
  DevBuf d_packed;    // int32 [2][nq][k]: labels, distance bits (FAST: + the head plane, [nq][kk] uint16)
  DevBuf d_gathered;  // int32 [G][packed] (every device under RCCL; shard 0 with copies)
  ncclComm_t comm = nullptr;
  // "exact_ties" across shards: the replay list (word 0 = count, entries from byte 16), the heap states
  // this shard's links start from and leave ([entry][2][k] words; shard 0's d_state_in receives the LAST
  // shard's), one event per batch of the list; int32 words
  DevBuf d_list, d_state_in, d_state_out;
  std::vector<hipEvent_t> link_done;
  std::string err;  // what the shard's last phase failed with
};

} // namespace vaqhost

struct vaqhip_multi {
  // (its members have destructors: declared so that it can be hidden, the exported symbols stay as they were)
  __attribute__((visibility("hidden"))) ~vaqhip_multi() = default;
  int D = 0, M = 0, G = 0;
  bool seq = false;  // VAQHIP_SUM_SEQUENTIAL: every shard is a queryLUT index
  std::vector<int> bits;  // [M], as every shard was created with
  std::vector<vaqhost::Shard> sh;
  bool distinct = true;  // no device named twice
  int exchange = vaqhost::EX_AUTO;
  bool comms_ready = false;
  int64_t N = 0, id_base = 0;
  // one call at a time (mu); every phase of it runs on the shards' worker threads (job_pool.h), and the
  // caller only goes on to the next phase -- the collective -- when every shard has succeeded
  mutable std::mutex mu;
  vaq::JobPool pool;
  // the search in flight (vaqhip_multi_search.cpp): plan_call fills what holds for the whole call, plan_set
  // the rest per set of queries; every phase reads it, and every buffer is sized by it alone
  struct __attribute__((visibility("hidden"))) Call {
    const float *queries = nullptr;     // host pointer, or
    const float *d_queries0 = nullptr;  // device pointer on shard 0's device (vaqhip_multi_search_device)
    int nq = 0, k = 0, projected = 0;
    bool rccl = false;             // the exchange goes over RCCL (with one shard: the one-rank collective)
    bool chain = false;            // "exact_ties" across shards: the chain runs (then k is the caller's k + 1)
    int n_batches = 0, batch = 0;  //   of the set's replay list
    int entry = 0;                 //   int32 words of one list entry's heap state
    bool fast = false;             // FAST's sharded form
    int kk = 0;                    //   min(k, N): rows of the head
    // the buffers of one set, in int32 words unless named bytes
    size_t plane() const { return (size_t)nq * k; }                // one [nq][k] plane of a shard's list
    size_t pair_bytes() const { return 2 * plane() * 4; }          // labels and distances: the merged lists
    size_t head_at() const { return 2 * plane(); }                 // where FAST's head plane starts in a packed buffer
    size_t packed() const { return head_at() + (fast ? ((size_t)nq * kk + 1) / 2 : 0); }  // one shard's packed buffer
    size_t packed_bytes() const { return packed() * 4; }
    size_t head_bytes() const { return (size_t)nq * std::max(kk, 1) * 2; }  // the gathered head
    size_t query_bytes(int D) const { return (size_t)nq * D * 4; }
    size_t list_bytes() const { return 16 + (size_t)nq * 4; }      // the replay list
    size_t state_bytes() const { return (size_t)nq * entry * 4; }  // the heap states of a whole list
    int k_out() const { return chain ? k - 1 : k; }                // the caller's k, and
    size_t out_plane() const { return (size_t)nq * k_out(); }      //   a plane of the answer
  } call;
  // what outlives a call: events and buffers on shard 0's device, options
  hipEvent_t user_ready = nullptr;     // recorded on the caller's stream: the queries are there
  hipEvent_t consumed = nullptr;       // shard 0 has read every shard's packed result (copies) / merged
  hipEvent_t finished = nullptr;       // the result is in the caller's device buffers
  hipEvent_t flagged = nullptr;        // "exact_ties": the replay list of the current set is complete
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start, searched, gathered, merged
  vaqhost::DevBuf d_out_labels;   // int32 [nq][k] labels, then
  float *d_out_dist = nullptr;    //   float [nq][k] distances (inside d_out_labels)
  vaqhost::DevBuf d_final;        // "exact_ties": int32 [2][nq][k] the current set's answer (labels, distances)
  vaqhost::DevBuf d_head;         // FAST: uint16 [nq][kk] the gathered head distances
  int opt_exact = 0, opt_exact_batch = 0;
  bool fast_q = false;            // a quantisation was given to every shard (vaqhip_multi_set_lut_quantization / learn)
  int opt_timing = 0;             // option "timing", as the shards hold it
  vaqhip_kmeans_timing km_last = {};  // the last vaqhip_multi_cluster_ti_kmeans
  // the encode across the shards (vaqhip_multi_encode.cpp)
  bool has_codes = false;             // a set or an add has given the shards rows (an empty matrix counts)
  int64_t opt_encode_chunk = 0;       // option "encode_chunk_rows", 0 = the default
  vaqhip_multi_encode_timing enc_last = {};
  bool lut_q = false;                 // vaqhip_multi_set_lut_quantiles has given every shard Q (the _lut encoders need it)
  vaqhip_multi_info last = {};
};

namespace vaqhost __attribute__((visibility("hidden"))) {

// sets vaqhip_multi_last_error()'s text for this thread (vaqhip_multi.cpp) and returns `code`
int mfail(int code, const char *fmt, ...);

inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP; }

// a HIP call of shard `s` failed: the text goes to the shard, the code to the caller
#define MHIP(expr)                                               \
  do {                                                           \
    hipError_t e_ = (expr);                                      \
    if (e_ != hipSuccess) {                                      \
      s.err = std::string(#expr) + ": " + hipGetErrorString(e_); \
      return vaqhost::hip_code(e_);                              \
    }                                                            \
  } while (0)

// a single-index call (vaqhip_*) failed on shard `s`, on this thread
#define MIX(expr)                   \
  do {                              \
    const int rc_ = (expr);         \
    if (rc_) {                      \
      s.err = vaqhip_last_error();  \
      return rc_;                   \
    }                               \
  } while (0)

// The buffers a phase needs, fitted together.  Growing frees the old buffer, and hipFree waits for the work of the
// buffer's own device only, while a stream of ANOTHER device may still read it.  So when any entry would grow (or
// `also`: something else of the caller's will), fit() first waits for `read`, the event the owner records behind
// every such reader, and then ensures all of them.  In steady state nothing grows and nothing waits.  It returns the
// first HIP error; `failed` then names the buffer (null: the wait failed) and text() says both.
struct FitList {
  static constexpr int CAP = 16;  // (the longest list today: 11, phase A of the exhaustive form on the first device)
  struct Entry { DevBuf *b; size_t bytes; const char *name; } e[CAP];
  int n = 0;
  const char *failed = nullptr;
  void want(DevBuf &b, size_t bytes, const char *name) {
    assert(n < CAP);
    if (n < CAP) e[n++] = Entry{&b, bytes, name};
  }
  hipError_t fit(hipEvent_t read, bool also = false) {
    bool grows = also;
    for (int i = 0; i < n; i++) grows |= e[i].bytes > e[i].b->cap;
    if (grows)
      if (const hipError_t r = hipEventSynchronize(read)) return r;
    for (int i = 0; i < n; i++) {
      failed = e[i].name;
      if (const hipError_t r = e[i].b->ensure(e[i].bytes)) return r;
    }
    failed = nullptr;
    return hipSuccess;
  }
  std::string text(hipError_t r) const {
    return std::string(failed ? failed : "the wait before a buffer grows") + (failed ? ".ensure: " : ": ") + hipGetErrorString(r);
  }
};

// fits the list of shard `s`, as MHIP
#define MFIT(list, ...)                             \
  do {                                              \
    const hipError_t e_ = (list).fit(__VA_ARGS__);  \
    if (e_ != hipSuccess) {                         \
      s.err = (list).text(e_);                      \
      return vaqhost::hip_code(e_);                 \
    }                                               \
  } while (0)

// job(g, shard) on every shard's worker at once.  A job that fails and leaves the shard's text empty says that a
// single-index call failed: the text is then that call's, taken on the worker's thread.  The first failing shard
// is reported.  (Owner: vaqhip_multi, the multi-device refiner or a call's ShardRun -- G, pool and sh[] with device and
// err.)
template <class Owner, class Job> int on_shards(Owner *mx, Job &&job) {
  const int rc = mx->pool.run([&](int g) -> int {
    auto &s = mx->sh[g];
    s.err.clear();
    const int r = job(g, s);
    if (r && s.err.empty()) s.err = vaqhip_last_error();
    return r;
  });
  for (int g = 0; rc && g < mx->G; g++)
    if (mx->pool.rc(g)) return mfail(mx->pool.rc(g), "shard %d (device %d): %s", g, mx->sh[g].device, mx->sh[g].err.c_str());
  return VAQHIP_OK;
}

// `bytes` from src on src_device to dst on dst_device, behind `stream`: a plain device-to-device copy where both shards
// name one GPU, a peer copy otherwise.  (The search and the refiner copy between shards 1.. and the first device with
// hipMemcpyPeerAsync throughout; that is their own decision.)
inline hipError_t copy_between(void *dst, int dst_device, const void *src, int src_device, size_t bytes, hipStream_t stream) {
  if (dst_device == src_device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
  return hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, stream);
}

// the code of a single-index call made on the calling thread, with its text when it failed
inline int forward(int rc) { return rc ? mfail(rc, "%s", vaqhip_last_error()) : rc; }

// call(index) on shard after shard, up to the first that fails
template <class F> int each_shard(vaqhip_multi *mx, F &&call) {
  for (Shard &s : mx->sh)
    if (const int rc = forward(call(s.ix))) return rc;
  return VAQHIP_OK;
}

// vaqhip_multi_set_ti_clusters with mx->mu held (vaqhip_multi.cpp): the k-means ends with it
int set_ti_clusters_on_shards(vaqhip_multi *mx, const float *clusters, int T, int seg_num);

// the cut of N rows over G shards: shard g = rows [g * ceil(N / G), (g + 1) * ceil(N / G))
inline void shard_cut(int64_t N, int G, int g, int64_t *lo, int64_t *n) {
  const int64_t per = (N + G - 1) / G;
  *lo = std::min<int64_t>(N, (int64_t)g * per);
  *n = std::min<int64_t>(N, (int64_t)(g + 1) * per) - *lo;
}

// option "encode_chunk_rows" of vaqhip_multi_set_option (vaqhip_multi_encode.cpp): refuses before it locks
int set_encode_chunk_rows(vaqhip_multi *mx, int64_t value);

} // namespace vaqhost
#endif
