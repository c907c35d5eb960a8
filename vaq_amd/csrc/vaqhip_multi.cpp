// vaqhip_multi.cpp -- the multi-GPU form of the index behind the C ABI (include/vaqhip.h,
// "multi-device"): SURVEY.md section 8(b) rows 1-3 / 8(e).
//
// One process drives the GPUs of a node, one host thread per device.  The code rows are cut
// into contiguous shards (shard g = rows [g * ceil(N/G), (g+1) * ceil(N/G))), every shard is an
// ordinary vaqhip_index on its device with id_base = its first row, every device answers ALL
// queries on its shard, and ONE exchange step finishes the search: an all-gather of the packed
// per-shard results [2][nq][k] (labels, distance bits) over RCCL -- ncclAllGather on communicators
// made by ncclCommInitAll, i.e. xGMI between the GPUs of the node -- followed by the k-min merge
// kernel by (distance, label).  Shards are contiguous in label order and a single index orders by
// (distance, label) too, so the merged result equals the single-index result bit for bit.
// The reference's precedent for shard-and-merge: BitVecEngine.cpp:1034-1132 (merge :1114-1126).
//
// RCCL is loaded with dlopen at the first multi-device search (libvaqhip.so itself does not link
// it): inside a Python process PyTorch's own copy is already mapped and is the one that gets used.
// When the device list names one GPU several times (logical shards: how the exchange and merge
// are tested on a one-GPU box) RCCL cannot be used -- it refuses duplicate devices -- and the
// gather is done with device-to-device copies instead; same buffers, same merge.
//
// Option "exact_ties" with more than one shard ("exact_ties across shards"): the reference's
// heap after the rows of shards 0..g is shard g's replay started from the heap shards 0..g-1 left, so
// per set of queries (A) every shard scans with k + 1 by the smallest-label rule, the exchange and merge
// above give the global k + 1 list on shard 0, the flag kernel copies the untied queries out and lists
// the tied ones; the list goes to every shard; (B) batch by batch of the list, shard g waits for shard
// g-1's event, takes the heap state by peer copy, runs its link (vaq_exact.hip) and records its own event;
// shard 0 reorders the state the last shard left into the caller's slots.  Every wait is a stream wait on
// an event; no kernel waits for another.
//
// Method FAST with more than one shard ("FAST across shards"): its answer is ordered by
// (dist, seq), and seq depends on std::sort's permutation of the first kk = min(k, N) rows of the WHOLE index
// (the head), so every shard hands over two things in its packed buffer -- the distances of the head rows it
// holds (never truncated: at most k in all) and the top-k of its other rows by (dist, row) -- and shard 0, after
// the one all-gather, sorts the gathered head as the single index does and takes the first k of the stable merge
// by distance of "head, then the shards' lists in shard order".
#include "vaqhip.h"
#include "vaqhip_internal.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "job_pool.h"
#include "kmeans_sample.h"
#include "vaq_kernels.h"
#include "vaqhip_dev.h"

namespace {

using vaqhost::DevBuf;
using vaqhost::DeviceGuard;

int mfail(int code, const char *fmt, ...);

// ---- RCCL, resolved at run time -------------------------------------------------------------
typedef struct ncclComm *ncclComm_t;
typedef int ncclResult_t;  // ncclSuccess == 0
enum { NCCL_INT32 = 2 };   // ncclInt32 / ncclInt (rccl.h: ncclDataType_t)
struct Rccl {
  void *h = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string where;
};
Rccl g_rccl;
std::mutex g_rccl_mu;

bool load_rccl(std::string *err) {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (g_rccl.h) return true;
  const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *n : names)  // a copy that is already mapped (PyTorch's) wins
    if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) { g_rccl.where = std::string(n) + " (already loaded)"; break; }
  if (!h)
    for (const char *n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) { g_rccl.where = n; break; }
  if (!h) {
    *err = std::string("RCCL not found: ") + dlerror();
    return false;
  }
  Rccl r;
  r.h = h;
  r.where = g_rccl.where;
#define VAQ_SYM(field, name)                                              \
  *reinterpret_cast<void **>(&r.field) = dlsym(h, name);                  \
  if (!r.field) { *err = std::string("RCCL symbol missing: ") + name; return false; }
  VAQ_SYM(CommInitAll, "ncclCommInitAll")
  VAQ_SYM(CommDestroy, "ncclCommDestroy")
  VAQ_SYM(AllGather, "ncclAllGather")
  VAQ_SYM(GroupStart, "ncclGroupStart")
  VAQ_SYM(GroupEnd, "ncclGroupEnd")
  VAQ_SYM(GetErrorString, "ncclGetErrorString")
#undef VAQ_SYM
  g_rccl = r;
  return true;
}

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

} // namespace

struct vaqhip_multi {
  // (its members have destructors now: declared so that it can be hidden, the exported symbols stay as they were)
  __attribute__((visibility("hidden"))) ~vaqhip_multi() = default;
  int D = 0, M = 0, G = 0;
  bool seq = false;  // VAQHIP_SUM_SEQUENTIAL: every shard is a queryLUT index
  std::vector<Shard> sh;
  bool distinct = true;  // no device named twice
  int exchange = EX_AUTO;
  bool comms_ready = false;
  int64_t N = 0, id_base = 0;
  // one call at a time (mu); every phase of it runs on the shards' worker threads (job_pool.h), and the
  // caller only goes on to the next phase -- the collective -- when every shard has succeeded
  mutable std::mutex mu;
  vaq::JobPool pool;
  // the search in flight: filled by multi_search_common per set of queries, read by every phase
  struct Call {
    const float *queries = nullptr;     // host pointer, or
    const float *d_queries0 = nullptr;  // device pointer on shard 0's device (vaqhip_multi_search_device)
    int nq = 0, k = 0, projected = 0, use_rccl = 0;
    bool chain = false;            // "exact_ties" across shards: the chain runs (then k is the caller's k + 1)
    int n_batches = 0, batch = 0;  //   of the set's replay list
    int entry = 0;                 //   int32 words of one list entry's heap state
    bool fast = false;             // FAST's sharded form
    int kk = 0;                    //   min(k, N): rows of the head
    size_t pk = 0;                 // int32 words of one shard's packed buffer: 2 * nq * k (+ the head plane)
  } call;
  // what outlives a call: events and buffers on shard 0's device, options
  hipEvent_t user_ready = nullptr;     // recorded on the caller's stream: the queries are there
  hipEvent_t consumed = nullptr;       // shard 0 has read every shard's packed result (copies) / merged
  hipEvent_t finished = nullptr;       // the result is in the caller's device buffers
  hipEvent_t flagged = nullptr;        // "exact_ties": the replay list of the current set is complete
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start, searched, gathered, merged
  DevBuf d_out_labels;            // int32 [nq][k] labels, then
  float *d_out_dist = nullptr;    //   float [nq][k] distances (inside d_out_labels)
  DevBuf d_final;                 // "exact_ties": int32 [2][nq][k] the current set's answer (labels, distances)
  DevBuf d_head;                  // FAST: uint16 [nq][kk] the gathered head distances
  int opt_exact = 0, opt_exact_batch = 0;
  bool fast_q = false;            // a quantisation was given to every shard (vaqhip_multi_set_lut_quantization / learn)
  int opt_timing = 0;             // option "timing", as the shards hold it
  vaqhip_kmeans_timing km_last = {};  // the last vaqhip_multi_cluster_ti_kmeans
  vaqhip_multi_info last = {};
};

namespace {

thread_local std::string g_merr;

int mfail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_merr = buf;
  return code;
}

#define MHIP(expr)                                                                         \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      s.err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
      return e_ == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP;                      \
    }                                                                                      \
  } while (0)

// DevBuf::ensure with the shard's error text, where MHIP's own return does not fit
int ensure(Shard &s, DevBuf &b, size_t bytes) {
  MHIP(b.ensure(bytes));
  return 0;
}

// one shard's part of a search; runs on that shard's worker thread with its device current
int run_shard(vaqhip_multi *mx, int g) {
  Shard &s = mx->sh[g];
  const vaqhip_multi::Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k;
  const size_t plane = (size_t)nq * k;
  MHIP(hipSetDevice(s.device));
  MHIP(s.d_queries.ensure((size_t)nq * mx->D * 4));
  MHIP(s.d_packed.ensure(c.pk * 4));
  const bool holds_all = c.use_rccl || g == 0;
  if (G > 1 && holds_all) MHIP(s.d_gathered.ensure((size_t)G * c.pk * 4));
  if (c.fast && g == 0) MHIP(mx->d_head.ensure((size_t)nq * std::max(c.kk, 1) * 2));
  if (g == 0) {
    MHIP(mx->d_out_labels.ensure(2 * plane * 4));
    mx->d_out_dist = reinterpret_cast<float *>(mx->d_out_labels.as<int32_t>() + plane);
  }
  if (c.chain) {
    const size_t state = (size_t)nq * c.entry * 4;
    MHIP(s.d_list.ensure(16 + (size_t)nq * 4));
    MHIP(s.d_state_in.ensure(state));
    MHIP(s.d_state_out.ensure(state));
    if (g == 0) MHIP(mx->d_final.ensure(state));
    while ((int)s.link_done.size() < c.n_batches) {
      hipEvent_t e = nullptr;
      MHIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      s.link_done.push_back(e);
    }
  }
  // (the previous search's exchange -- and chain -- has read this shard's buffers: never recorded = no wait)
  MHIP(hipStreamWaitEvent(s.stream, mx->consumed, 0));
  if (g == 0) MHIP(hipEventRecord(mx->ev[0], s.stream));
  float *dq = s.d_queries.as<float>();
  int32_t *packed = s.d_packed.as<int32_t>();
  if (c.d_queries0) {
    // device entry: the queries sit on shard 0's device; every shard takes its copy over the fabric
    MHIP(hipStreamWaitEvent(s.stream, mx->user_ready, 0));
    MHIP(hipMemcpyPeerAsync(dq, s.device, c.d_queries0, mx->sh[0].device, (size_t)nq * mx->D * 4, s.stream));
  } else {
    MHIP(hipMemcpyAsync(dq, c.queries, (size_t)nq * mx->D * 4, hipMemcpyHostToDevice, s.stream));
  }
  int32_t *labels = G == 1 ? mx->d_out_labels.as<int32_t>() : packed;
  float *dist = G == 1 ? mx->d_out_dist : reinterpret_cast<float *>(packed + plane);
  const int rc = c.fast ? vaqhip_internal_search_fast_shard_device(s.ix, dq, nq, k, c.projected, s.lo, c.kk, labels, dist,
                                                                   reinterpret_cast<uint16_t *>(packed + 2 * plane), s.stream)
                 : c.chain ? vaqhip_internal_search_plain_device(s.ix, dq, nq, k, c.projected, labels, dist, s.stream)
                           : vaqhip_search_device(s.ix, dq, nq, k, c.projected, labels, dist, s.stream);
  if (rc) {
    s.err = vaqhip_last_error();
    return rc;
  }
  if (g == 0) MHIP(hipEventRecord(mx->ev[1], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

// The exchange step, issued by the CALLING thread once every shard's search is enqueued without error:
// one ncclAllGather per device inside a group (nq * k * 8 bytes per rank over xGMI; FAST: + nq * kk * 2).  A shard that
// failed has returned before this point and no collective was enqueued anywhere, so nothing can be
// left waiting for a peer that never arrives.
int exchange_rccl(vaqhip_multi *mx) {
  ncclResult_t nr = g_rccl.GroupStart();
  if (nr != 0) return mfail(VAQHIP_EHIP, "ncclGroupStart: %s", g_rccl.GetErrorString(nr));
  ncclResult_t first = 0;
  for (int g = 0; g < mx->G; g++) {
    Shard &s = mx->sh[g];
    if (hipSetDevice(s.device) != hipSuccess) { first = first ? first : -1; continue; }
    nr = g_rccl.AllGather(s.d_packed.p, s.d_gathered.p, mx->call.pk, NCCL_INT32, s.comm, s.stream);
    if (nr != 0 && !first) first = nr;
  }
  nr = g_rccl.GroupEnd();
  if (first != 0) return mfail(VAQHIP_EHIP, "ncclAllGather: %s", first > 0 ? g_rccl.GetErrorString(first) : "hipSetDevice");
  if (nr != 0) return mfail(VAQHIP_EHIP, "ncclGroupEnd: %s", g_rccl.GetErrorString(nr));
  return 0;
}

// after every shard has enqueued its part: gather by copies when RCCL is not in play, merge on
// shard 0's device
int gather_and_merge(vaqhip_multi *mx) {
  Shard &s = mx->sh[0];
  const vaqhip_multi::Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k;
  const size_t plane = (size_t)nq * k;
  int32_t *gathered = s.d_gathered.as<int32_t>(), *out_labels = mx->d_out_labels.as<int32_t>();
  MHIP(hipSetDevice(s.device));
  if (G > 1) {
    if (!c.use_rccl) {
      for (int g = 0; g < G; g++) {
        MHIP(hipStreamWaitEvent(s.stream, mx->sh[g].done, 0));
        MHIP(hipMemcpyPeerAsync(gathered + (size_t)g * c.pk, s.device, mx->sh[g].d_packed.p, mx->sh[g].device,
                                c.pk * 4, s.stream));
      }
    }
    MHIP(hipEventRecord(mx->ev[2], s.stream));
    int rc;
    if (c.fast) {
      // the head rows' distances from the planes of the shards that hold them, then the head's std::sort and
      // the stable merge "head, then the shards' lists in shard order"
      int start[VAQHIP_MAX_DEVICES + 1];
      for (int g = 0; g <= G; g++) start[g] = g < G ? (int)std::min<int64_t>(mx->sh[g].lo, c.kk) : c.kk;
      uint16_t *head = mx->d_head.as<uint16_t>();
      rc = vaqhip_internal_fast_head_gather_device(s.device, reinterpret_cast<const uint16_t *>(gathered + 2 * plane),
                                                   (int64_t)(2 * c.pk), G, start, nq, c.kk, head, s.stream);
      if (!rc)
        rc = vaqhip_merge_fast_device(s.device, head, c.kk, c.kk, mx->id_base,
                                      reinterpret_cast<const float *>(gathered + plane), gathered, G,
                                      (int64_t)c.pk, (int64_t)k, nq, k, out_labels, mx->d_out_dist, s.stream);
    } else {
      rc = vaqhip_merge_topk_strided_device(
          s.device, reinterpret_cast<const float *>(gathered + plane), gathered, G, (int64_t)c.pk,
          (int64_t)k, nq, k, out_labels, mx->d_out_dist, s.stream);
    }
    if (rc) {
      s.err = vaqhip_last_error();
      return rc;
    }
  } else {
    MHIP(hipEventRecord(mx->ev[2], s.stream));
  }
  return 0;
}

// "exact_ties" across shards, after the merge of the k + 1 lists (mx->call.k): flag on shard 0, the list to
// every shard, the chain of links batch by batch, heap_reorder on shard 0 -> mx->d_final [2][nq][k].
// Issued by the calling thread; everything is enqueued, nothing waited for.  A failure part-way leaves
// streams that wait only for events already recorded (or never recorded: no wait).
#define MIX(expr)                                 \
  do {                                            \
    const int rc_ = (expr);                       \
    if (rc_) {                                    \
      s.err = vaqhip_last_error();                \
      return rc_;                                 \
    }                                             \
  } while (0)
int chain_on_shard0(vaqhip_multi *mx) {
  Shard &s = mx->sh[0];
  const vaqhip_multi::Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k - 1;
  const size_t plane = (size_t)nq * k, entry = (size_t)c.entry;
  int32_t *fl = mx->d_final.as<int32_t>();
  float *fd = reinterpret_cast<float *>(fl + plane);
  const size_t list_bytes = 16 + (size_t)nq * 4;
  // a shard's replay list: the count in word 0, the entries from byte 16
  auto list_count = [](const Shard &t) { return t.d_list.as<unsigned>(); };
  auto list_entries = [](const Shard &t) { return reinterpret_cast<int *>(t.d_list.as<int32_t>() + 4); };
  MIX(vaqhip_internal_exact_flag_device(s.device, nq, k, mx->d_out_labels.as<int32_t>(), mx->d_out_dist, fl, fd,
                                        list_entries(s), list_count(s), s.stream));
  MHIP(hipEventRecord(mx->flagged, s.stream));
  for (int g = 1; g < G; g++) {
    Shard &t = mx->sh[g];
    MHIP(hipSetDevice(t.device));
    MHIP(hipStreamWaitEvent(t.stream, mx->flagged, 0));
    MHIP(hipMemcpyPeerAsync(t.d_list.p, t.device, s.d_list.p, s.device, list_bytes, t.stream));
  }
  // Batches are enqueued in order on every shard's stream: on distinct GPUs shard g works on batch b
  // while shard g + 1 works on batch b - 1.  Entries beyond the device-side count exit at once.
  for (int b = 0; b < c.n_batches; b++) {
    const int e0 = b * c.batch, ne = std::min(c.batch, nq - e0);
    for (int g = 0; g < G; g++) {
      Shard &t = mx->sh[g];
      MHIP(hipSetDevice(t.device));
      if (g > 0) {
        const Shard &u = mx->sh[g - 1];
        MHIP(hipStreamWaitEvent(t.stream, u.link_done[b], 0));
        MHIP(hipMemcpyPeerAsync(t.d_state_in.as<int32_t>() + e0 * entry, t.device, u.d_state_out.as<int32_t>() + e0 * entry,
                                u.device, ne * entry * 4, t.stream));
      }
      MIX(vaqhip_internal_exact_link_device(t.ix, k, t.lo, list_entries(t), list_count(t), e0, ne,
                                            g > 0 ? t.d_state_in.as<int32_t>() : nullptr, t.d_state_out.as<int32_t>(),
                                            t.stream));
      MHIP(hipEventRecord(t.link_done[b], t.stream));
    }
  }
  const Shard &last = mx->sh[G - 1];
  MHIP(hipSetDevice(s.device));
  MHIP(hipStreamWaitEvent(s.stream, last.link_done[c.n_batches - 1], 0));
  MHIP(hipMemcpyPeerAsync(s.d_state_in.p, s.device, last.d_state_out.p, last.device, nq * entry * 4, s.stream));
  MIX(vaqhip_internal_exact_finish_device(s.device, s.d_state_in.as<int32_t>(), list_entries(s), list_count(s), nq,
                                          mx->seq ? 1 : 0, k, fl, fd, s.stream));
  return 0;
}
#undef MIX

// the result (k per query, on shard 0's device) to the caller: device buffers behind the caller's
// stream, or the host
int deliver(vaqhip_multi *mx, const int32_t *src_labels, const float *src_dist, int k, int32_t *labels, float *distances,
            hipStream_t user) {
  Shard &s = mx->sh[0];
  const int G = mx->G;
  const size_t plane = (size_t)mx->call.nq * k;
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventRecord(mx->ev[3], s.stream));
  MHIP(hipEventRecord(mx->consumed, s.stream));
  if (mx->call.d_queries0) {
    // device entry: results into the caller's buffers on shard 0's device; the caller's stream waits
    // for them, the host does not
    MHIP(hipMemcpyAsync(labels, src_labels, plane * 4, hipMemcpyDeviceToDevice, s.stream));
    MHIP(hipMemcpyAsync(distances, src_dist, plane * 4, hipMemcpyDeviceToDevice, s.stream));
    MHIP(hipEventRecord(mx->finished, s.stream));
    MHIP(hipStreamWaitEvent(user, mx->finished, 0));
    return 0;
  }
  MHIP(hipMemcpyAsync(labels, src_labels, plane * 4, hipMemcpyDeviceToHost, s.stream));
  MHIP(hipMemcpyAsync(distances, src_dist, plane * 4, hipMemcpyDeviceToHost, s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  for (int g = 1; g < G; g++) {  // (their collective / copies are complete before anyone reuses the buffers)
    MHIP(hipSetDevice(mx->sh[g].device));
    MHIP(hipStreamSynchronize(mx->sh[g].stream));
  }
  MHIP(hipSetDevice(s.device));
  float ms[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++) MHIP(hipEventElapsedTime(&ms[i], mx->ev[i], mx->ev[i + 1]));
  mx->last.last_search_ms = ms[0];
  mx->last.last_exchange_ms = ms[1];
  mx->last.last_merge_ms = ms[2];
  return 0;
}

int finish_on_shard0(vaqhip_multi *mx, int32_t *labels, float *distances, hipStream_t user) {
  if (int rc = gather_and_merge(mx)) return rc;
  const vaqhip_multi::Call &c = mx->call;
  if (!c.chain) return deliver(mx, mx->d_out_labels.as<int32_t>(), mx->d_out_dist, c.k, labels, distances, user);
  if (int rc = chain_on_shard0(mx)) return rc;
  const int k = c.k - 1;
  const int32_t *fl = mx->d_final.as<int32_t>();
  return deliver(mx, fl, reinterpret_cast<const float *>(fl + (size_t)c.nq * k), k, labels, distances, user);
}

int ensure_comms(vaqhip_multi *mx) {
  if (mx->comms_ready) return 0;
  std::string err;
  if (!load_rccl(&err)) return mfail(VAQHIP_ENODEVICE, "%s", err.c_str());
  std::vector<ncclComm_t> comms(mx->G);
  std::vector<int> devs(mx->G);
  for (int g = 0; g < mx->G; g++) devs[g] = mx->sh[g].device;
  const ncclResult_t nr = g_rccl.CommInitAll(comms.data(), mx->G, devs.data());
  if (nr != 0) return mfail(VAQHIP_EHIP, "ncclCommInitAll(%d devices): %s", mx->G, g_rccl.GetErrorString(nr));
  for (int g = 0; g < mx->G; g++) mx->sh[g].comm = comms[g];
  mx->comms_ready = true;
  return 0;
}

} // namespace

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
    const int rc = vaqhip_index_create_ex(&s.ix, D, M, bits, centroids, eig, s.device, flags);
    if (rc) {
      g_merr = vaqhip_last_error();
      vaqhip_multi_destroy(mx);
      return rc;
    }
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
  const int64_t per = (N + mx->G - 1) / mx->G;  // contiguous shards of ceil(N / G) rows
  for (int g = 0; g < mx->G; g++) {
    Shard &s = mx->sh[g];
    s.lo = std::min<int64_t>(N, (int64_t)g * per);
    s.n = std::min<int64_t>(N, (int64_t)(g + 1) * per) - s.lo;
  }
  // every shard uploads, sorts and packs its rows on its own device, all of them at once
  const int rc = mx->pool.run([&](int g) -> int {
    Shard &s = mx->sh[g];
    s.err.clear();
    const int r = vaqhip_index_set_codes_u16(s.ix, codes + s.lo * mx->M, s.n, id_base + s.lo);
    if (r) s.err = vaqhip_last_error();
    return r;
  });
  if (rc)
    for (int g = 0; g < mx->G; g++)
      if (mx->pool.rc(g)) return mfail(mx->pool.rc(g), "shard %d (device %d): %s", g, mx->sh[g].device, mx->sh[g].err.c_str());
  mx->N = N;
  mx->id_base = id_base;
  return VAQHIP_OK;
}

int vaqhip_multi_add_codes_u16(vaqhip_multi *mx, const uint16_t *codes, int64_t n_new) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (n_new < 0 || (n_new > 0 && !codes)) return mfail(VAQHIP_EINVAL, "bad codes/N");
  std::lock_guard<std::mutex> lk(mx->mu);
  // labels are global row numbers and shards are contiguous ranges of them, so new rows (which
  // continue the numbering) extend the LAST shard; set_codes re-balances
  Shard &s = mx->sh[mx->G - 1];
  const int rc = vaqhip_index_add_codes_u16(s.ix, codes, n_new);
  if (rc) {
    g_merr = vaqhip_last_error();
    return rc;
  }
  s.n += n_new;
  mx->N += n_new;
  return VAQHIP_OK;
}

// every shard regroups its own rows under the same centres, all of them at once; mx->mu is held
static int set_ti_clusters_on_shards(vaqhip_multi *mx, const float *clusters, int T, int seg_num) {
  const int rc = mx->pool.run([&](int g) -> int {
    Shard &s = mx->sh[g];
    s.err.clear();
    const int r = vaqhip_index_set_ti_clusters(s.ix, clusters, T, seg_num);
    if (r) s.err = vaqhip_last_error();
    return r;
  });
  if (rc)
    for (int g = 0; g < mx->G; g++)
      if (mx->pool.rc(g)) return mfail(mx->pool.rc(g), "shard %d (device %d): %s", g, mx->sh[g].device, mx->sh[g].err.c_str());
  return VAQHIP_OK;
}

int vaqhip_multi_set_ti_clusters(vaqhip_multi *mx, const float *clusters, int T, int seg_num) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  return set_ti_clusters_on_shards(mx, clusters, T, seg_num);
}

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
  int rc = mx->pool.run([&](int g) -> int {
    Shard &s = mx->sh[g];
    s.err.clear();
    int r;
    if (sampled) {
      const std::vector<int> &local = split[(size_t)g].local;
      piece[(size_t)g].resize(std::max<size_t>(local.size() * seg_num, 1));
      r = vaqhip_internal_kmeans_gather(s.ix, local.data(), (int)local.size(), seg_num, piece[(size_t)g].data());
    } else {  // all rows: the shard's rows lie at sample positions [lo, lo + n)
      r = vaqhip_internal_kmeans_gather(s.ix, nullptr, (int)s.n, seg_num, scodes.data() + (size_t)s.lo * seg_num);
    }
    if (r) s.err = vaqhip_last_error();
    return r;
  });
  if (rc)
    for (int g = 0; g < G; g++)
      if (mx->pool.rc(g)) return mfail(mx->pool.rc(g), "shard %d (device %d): %s", g, mx->sh[g].device, mx->sh[g].err.c_str());
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
    if ((rc = vaqhip_internal_kmeans_tables(mx->sh[g].ix, &sub, &devs[g].cent, &L))) return mfail(rc, "%s", vaqhip_last_error());
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
      return e == hipSuccess ? 0
                             : mfail(e == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP, "shard 0 (device %d): %s: %s",
                                     s.device, what, hipGetErrorString(e));
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
      return mfail(e == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP, "shard %d (device %d): k-means: %s", failed,
                   mx->sh[failed].device, hipGetErrorString(e));
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
  int nan_rows = 0;
  for (int c = 0; c < T; c++) {
    bool nan = false;
    for (int j = 0; j < dd; j++) nan |= std::isnan(means[(size_t)c * dd + j]);
    nan_rows += nan;
  }
  if (clusters_out) std::memcpy(clusters_out, means.data(), means.size() * sizeof(float));
  if (iters_out) *iters_out = iters;
  if (nan_rows_out) *nan_rows_out = nan_rows;
  return set_ti_clusters_on_shards(mx, means.data(), T, seg_num);
}

int vaqhip_multi_last_kmeans_timing(vaqhip_multi *mx, vaqhip_kmeans_timing *out) {
  if (!mx || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  *out = mx->km_last;
  return VAQHIP_OK;
}

int vaqhip_multi_set_method(vaqhip_multi *mx, unsigned methods, float visit) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  // FAST on its own is taken once every shard holds the SAME quantisation, i.e. after one of the two multi calls
  // that replicate it; before that the index keeps refusing the method, as it always has
  if ((methods & VAQHIP_METHOD_FAST) && !(methods & (VAQHIP_METHOD_TI | VAQHIP_METHOD_EA | VAQHIP_METHOD_HEAP)) && !mx->fast_q)
    return mfail(VAQHIP_EUNSUPPORTED, "method FAST on a multi index needs vaqhip_multi_set_lut_quantization or "
                                      "vaqhip_multi_learn_quantization first");
  for (auto &s : mx->sh) {
    const int rc = vaqhip_index_set_method(s.ix, methods, visit);
    if (rc) {
      g_merr = vaqhip_last_error();
      return rc;
    }
  }
  return VAQHIP_OK;
}

int vaqhip_multi_set_lut_quantization(vaqhip_multi *mx, const float *offsets, const float *scale) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (!offsets || !scale) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  for (auto &s : mx->sh) {  // every shard quantises its tables by the same map
    const int rc = vaqhip_index_set_lut_quantization(s.ix, offsets, scale);
    if (rc) {
      g_merr = vaqhip_last_error();
      return rc;
    }
  }
  mx->fast_q = true;
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
  if (rc) {
    g_merr = vaqhip_last_error();
    return rc;
  }
  mx->fast_q = true;
  if (offsets_out) std::memcpy(offsets_out, off.data(), off.size() * sizeof(float));
  if (scale_out) std::memcpy(scale_out, sc.data(), sc.size() * sizeof(float));
  return VAQHIP_OK;
}

int vaqhip_multi_set_option(vaqhip_multi *mx, const char *key, int64_t value) {
  if (!mx || !key) return mfail(VAQHIP_EINVAL, "null pointer");
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
  for (auto &s : mx->sh) {
    const int rc = vaqhip_set_option(s.ix, key, value);
    if (rc) {
      g_merr = vaqhip_last_error();
      return rc;
    }
  }
  // (every shard holds the option too: one shard alone answers by its own replay, and the chain is only
  //  taken where the option has an effect on every shard)
  if (std::strcmp(key, "exact_ties") == 0) mx->opt_exact = value != 0;
  if (std::strcmp(key, "timing") == 0) mx->opt_timing = value != 0;
  return VAQHIP_OK;
}

// one set of queries (mx->call): the shards' searches, the exchange, the merge
// (and the chain) on shard 0, the result to the caller
static int search_set(vaqhip_multi *mx, bool rccl, int32_t *labels, float *distances, hipStream_t user) {
  // phase 1: every shard uploads (or copies) the queries and enqueues its search
  const int rc1 = mx->pool.run([&](int g) -> int {
    mx->sh[g].err.clear();
    return run_shard(mx, g);
  });
  if (rc1) {
    // Nothing of the exchange has been enqueued: the shards that did succeed have complete, ordinary
    // work on their streams, and the index stays usable (and destroyable).
    for (int g = 0; g < mx->G; g++)
      if (mx->pool.rc(g))
        return mfail(mx->pool.rc(g), "shard %d (device %d): %s", g, mx->sh[g].device, mx->sh[g].err.c_str());
  }
  // phase 2: the exchange, only now that every shard is known to take part
  if (mx->call.use_rccl) {
    const int rc = exchange_rccl(mx);
    if (rc) return rc;
  }
  if (rccl && mx->G == 1) {
    // one rank: the collective degenerates to a copy; run it anyway so that a one-GPU box
    // proves the RCCL binding (communicator, stream, datatype) end to end
    Shard &s = mx->sh[0];
    const size_t plane = (size_t)mx->call.nq * mx->call.k;
    if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_EHIP, "hipSetDevice");
    if (ensure(s, s.d_gathered, 2 * plane * 4)) return mfail(VAQHIP_ENOMEM, "%s", s.err.c_str());
    const ncclResult_t nr = g_rccl.AllGather(mx->d_out_labels.p, s.d_gathered.p, 2 * plane, NCCL_INT32, s.comm, s.stream);
    if (nr != 0) return mfail(VAQHIP_EHIP, "ncclAllGather: %s", g_rccl.GetErrorString(nr));
    if (hipMemcpyAsync(mx->d_out_labels.p, s.d_gathered.p, 2 * plane * 4, hipMemcpyDeviceToDevice, s.stream) != hipSuccess)
      return mfail(VAQHIP_EHIP, "copy back from the gathered buffer");
  }
  Shard &s0 = mx->sh[0];
  const int rc = finish_on_shard0(mx, labels, distances, user);
  if (rc) return mfail(rc, "exchange / merge on device %d: %s", s0.device, s0.err.c_str());
  return VAQHIP_OK;
}

static int multi_search_common(vaqhip_multi *mx, const float *queries, const float *d_queries0, hipStream_t user, int nq, int k,
                               int projected, int32_t *labels, float *distances) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (nq < 0 || k <= 0) return mfail(VAQHIP_EINVAL, "nq=%d k=%d", nq, k);
  if (nq == 0) return VAQHIP_OK;
  if ((!queries && !d_queries0) || !labels || !distances) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  vaqhip_multi::Call &c = mx->call;
  // FAST over several shards: the head-and-lists form (one shard alone answers as the single index does)
  c.fast = mx->G > 1;
  for (int g = 0; c.fast && g < mx->G; g++) c.fast = vaqhip_internal_fast_in_force(mx->sh[g].ix) != 0;
  if (c.fast && k > VAQHIP_MAX_K) return mfail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  // (the other methods leave shard 0's device current, as they always have)
  DeviceGuard keep(DeviceGuard::restore_only, c.fast);
  // RCCL when the GPUs are distinct and there is something to exchange (or when asked for by
  // option, which also exercises it on one device); device-to-device copies otherwise
  bool rccl = mx->exchange == EX_RCCL || (mx->exchange == EX_AUTO && mx->distinct && mx->G > 1);
  if (rccl) {
    const int rc = ensure_comms(mx);
    if (rc) return rc;
  }
  // a one-shard index asked to use RCCL still goes through the collective (G == 1 skips packing)
  c.use_rccl = rccl && mx->G > 1;
  c.projected = projected;
  if (d_queries0) {
    if (hipSetDevice(mx->sh[0].device) != hipSuccess || hipEventRecord(mx->user_ready, user) != hipSuccess)
      return mfail(VAQHIP_EHIP, "recording the caller's stream");
  }
  // "exact_ties" over several shards: the chain, where the option has an effect on a single index too
  // (not TI, not FAST, k < VAQHIP_MAX_K); one set of queries at a time, because every link reads the lookup
  // tables its shard built for the set
  c.chain = mx->opt_exact && mx->G > 1;
  for (int g = 0; c.chain && g < mx->G; g++) c.chain = vaqhip_internal_exact_applies(mx->sh[g].ix, k) != 0;
  if (c.chain) c.entry = vaqhip_internal_exact_state_words(mx->sh[0].ix, k);
  const int set = c.chain ? std::min(nq, vaqhip_internal_query_chunk()) : nq;
  for (int q0 = 0; q0 < nq; q0 += set) {
    const int n = std::min(set, nq - q0);
    c.queries = queries ? queries + (size_t)q0 * mx->D : nullptr;
    c.d_queries0 = d_queries0 ? d_queries0 + (size_t)q0 * mx->D : nullptr;
    c.nq = n;
    c.k = c.chain ? k + 1 : k;
    // appends may have grown N past k, or the head with it: both are taken from the rows as they are now
    c.kk = c.fast ? (int)std::min<int64_t>(k, mx->N) : 0;
    c.pk = 2 * (size_t)n * c.k + (c.fast ? ((size_t)n * c.kk + 1) / 2 : 0);
    if (c.chain) {
      // batches of the replay list, chosen from the set's size (the count of tied queries lives on the device)
      int b = mx->opt_exact_batch > 0 ? mx->opt_exact_batch : std::max(64, (n + 15) / 16);
      b = std::max(b, (n + 255) / 256);
      c.batch = b;
      c.n_batches = (n + b - 1) / b;
    }
    const int rc = search_set(mx, rccl, labels + (size_t)q0 * k, distances + (size_t)q0 * k, user);
    if (rc) return rc;
  }
  mx->last.exchange = rccl ? EX_RCCL : (mx->G == 1 ? 0 : EX_COPIES);
  return VAQHIP_OK;
}

int vaqhip_multi_search(vaqhip_multi *mx, const float *queries, int nq, int k, int projected, int32_t *labels,
                        float *distances) {
  return multi_search_common(mx, queries, nullptr, nullptr, nq, k, projected, labels, distances);
}

int vaqhip_multi_search_device(vaqhip_multi *mx, const float *d_queries, int nq, int k, int projected, int32_t *d_labels,
                               float *d_distances, void *stream) {
  return multi_search_common(mx, nullptr, d_queries, static_cast<hipStream_t>(stream), nq, k, projected, d_labels,
                             d_distances);
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
