// vaqhip_multi_search.cpp -- a search of the multi-device index (vaqhip_multi.h): everything between
// vaqhip_multi_search / vaqhip_multi_search_device and the result.
//
// Every device answers ALL queries on its shard, and ONE exchange step finishes the search: an all-gather
// of the packed per-shard results [2][nq][k] (labels, distance bits) over RCCL -- ncclAllGather on
// communicators made by ncclCommInitAll, i.e. xGMI between the GPUs of the node -- followed by the k-min
// merge kernel by (distance, label), which equals the single-index result bit for bit.  When the device
// list names one GPU several times (logical shards: how the exchange and merge are tested on a one-GPU box)
// RCCL cannot be used -- it refuses duplicate devices -- and the gather is done with device-to-device copies
// instead; same buffers, same merge.
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
#include "vaqhip_multi.h"

using namespace vaqhost;
using Call = vaqhip_multi::Call;

namespace {

// Phase 1, first half, on the shard's worker with its device current: the buffers of this set fit and its
// events exist.  In steady state nothing grows and nothing here waits.
int fit_buffers(vaqhip_multi *mx, int g, Shard &s) {
  const Call &c = mx->call;
  const int G = mx->G;
  FitList fit;
  fit.want(s.d_queries, c.query_bytes(mx->D), "d_queries");
  fit.want(s.d_packed, c.packed_bytes(), "d_packed");
  if (G > 1 && (c.rccl || g == 0)) fit.want(s.d_gathered, G * c.packed_bytes(), "d_gathered");  // who holds every shard's
  if (c.fast && g == 0) fit.want(mx->d_head, c.head_bytes(), "d_head");
  if (g == 0) fit.want(mx->d_out_labels, c.pair_bytes(), "d_out_labels");
  if (c.chain) {
    fit.want(s.d_list, c.list_bytes(), "d_list");
    fit.want(s.d_state_in, c.state_bytes(), "d_state_in");
    fit.want(s.d_state_out, c.state_bytes(), "d_state_out");
    if (g == 0) fit.want(mx->d_final, c.state_bytes(), "d_final");
  }
  MHIP(hipSetDevice(s.device));
  // The last search's copies out of d_packed, d_state_out and d_list run on ANOTHER device's stream, and after the
  // device entry nobody has waited for them.  `consumed` follows all of them (never recorded, or recorded before a
  // host entry returned: no wait).  A search that failed on shard 0 after phase 1 may not have recorded it:
  // search_set leaves every stream idle instead.
  MFIT(fit, mx->consumed);
  if (g == 0) mx->d_out_dist = reinterpret_cast<float *>(mx->d_out_labels.as<int32_t>() + c.plane());
  while (c.chain && (int)s.link_done.size() < c.n_batches) {
    hipEvent_t e = nullptr;
    MHIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s.link_done.push_back(e);
  }
  return 0;
}

// Phase 1, second half, same worker: the queries to the shard and its search, enqueued on its stream.  (A failing
// search leaves the shard's text empty: on_shards takes it from the single index.)
int enqueue_shard(vaqhip_multi *mx, int g, Shard &s) {
  const Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k;
  // (the previous search's exchange -- and chain -- has read this shard's buffers: never recorded = no wait)
  MHIP(hipStreamWaitEvent(s.stream, mx->consumed, 0));
  if (g == 0) MHIP(hipEventRecord(mx->ev[0], s.stream));
  float *dq = s.d_queries.as<float>();
  int32_t *packed = s.d_packed.as<int32_t>();
  if (c.d_queries0) {
    // device entry: the queries sit on shard 0's device; every shard takes its copy over the fabric
    MHIP(hipStreamWaitEvent(s.stream, mx->user_ready, 0));
    MHIP(hipMemcpyPeerAsync(dq, s.device, c.d_queries0, mx->sh[0].device, c.query_bytes(mx->D), s.stream));
  } else {
    MHIP(hipMemcpyAsync(dq, c.queries, c.query_bytes(mx->D), hipMemcpyHostToDevice, s.stream));
  }
  int32_t *labels = G == 1 ? mx->d_out_labels.as<int32_t>() : packed;
  float *dist = G == 1 ? mx->d_out_dist : reinterpret_cast<float *>(packed + c.plane());
  const int rc = c.fast ? vaqhip_internal_search_fast_shard_device(s.ix, dq, nq, k, c.projected, s.lo, c.kk, labels, dist,
                                                                   reinterpret_cast<uint16_t *>(packed + c.head_at()), s.stream)
                 : c.chain ? vaqhip_internal_search_plain_device(s.ix, dq, nq, k, c.projected, labels, dist, s.stream)
                           : vaqhip_search_device(s.ix, dq, nq, k, c.projected, labels, dist, s.stream);
  if (rc) return rc;
  if (g == 0) MHIP(hipEventRecord(mx->ev[1], s.stream));
  MHIP(hipEventRecord(s.done, s.stream));
  return 0;
}

int ensure_comms(vaqhip_multi *mx) {
  if (mx->comms_ready) return 0;
  std::string err;
  if (!load_rccl(&err)) return mfail(VAQHIP_ENODEVICE, "%s", err.c_str());
  std::vector<ncclComm_t> comms(mx->G);
  std::vector<int> devs(mx->G);
  for (int g = 0; g < mx->G; g++) devs[g] = mx->sh[g].device;
  const ncclResult_t nr = g_rccl.CommInitAll(comms.data(), mx->G, devs.data());
  if (nr != ncclSuccess) return mfail(VAQHIP_EHIP, "ncclCommInitAll(%d devices): %s", mx->G, g_rccl.GetErrorString(nr));
  for (int g = 0; g < mx->G; g++) mx->sh[g].comm = comms[g];
  mx->comms_ready = true;
  return 0;
}

// The exchange step, issued by the CALLING thread once every shard's search is enqueued without error:
// one ncclAllGather per device inside a group (nq * k * 8 bytes per rank over xGMI; FAST: + nq * kk * 2).  A shard that
// failed has returned before this point and no collective was enqueued anywhere, so nothing can be
// left waiting for a peer that never arrives.
int exchange_rccl(vaqhip_multi *mx) {
  ncclResult_t nr = g_rccl.GroupStart();
  if (nr != ncclSuccess) return mfail(VAQHIP_EHIP, "ncclGroupStart: %s", g_rccl.GetErrorString(nr));
  int first = 0;  // the first failure: an ncclResult_t, or -1 for hipSetDevice
  for (int g = 0; g < mx->G; g++) {
    Shard &s = mx->sh[g];
    if (hipSetDevice(s.device) != hipSuccess) { first = first ? first : -1; continue; }
    nr = g_rccl.AllGather(s.d_packed.p, s.d_gathered.p, mx->call.packed(), ncclInt32, s.comm, s.stream);
    if (nr != ncclSuccess && !first) first = nr;
  }
  nr = g_rccl.GroupEnd();
  if (first != 0)
    return mfail(VAQHIP_EHIP, "ncclAllGather: %s", first > 0 ? g_rccl.GetErrorString((ncclResult_t)first) : "hipSetDevice");
  if (nr != ncclSuccess) return mfail(VAQHIP_EHIP, "ncclGroupEnd: %s", g_rccl.GetErrorString(nr));
  return 0;
}

// One shard asked to use RCCL: the collective degenerates to a copy; run it anyway so that a one-GPU box
// proves the RCCL binding (communicator, stream, datatype) end to end.  (One shard does not pack: its lists
// are the merged lists already.)
int allgather_one_rank(vaqhip_multi *mx) {
  Shard &s = mx->sh[0];
  const Call &c = mx->call;
  if (hipSetDevice(s.device) != hipSuccess) return mfail(VAQHIP_EHIP, "hipSetDevice");
  const hipError_t e = s.d_gathered.ensure(c.pair_bytes());
  if (e != hipSuccess) return mfail(VAQHIP_ENOMEM, "b.ensure(bytes): %s", hipGetErrorString(e));
  const ncclResult_t nr = g_rccl.AllGather(mx->d_out_labels.p, s.d_gathered.p, c.packed(), ncclInt32, s.comm, s.stream);
  if (nr != ncclSuccess) return mfail(VAQHIP_EHIP, "ncclAllGather: %s", g_rccl.GetErrorString(nr));
  if (hipMemcpyAsync(mx->d_out_labels.p, s.d_gathered.p, c.pair_bytes(), hipMemcpyDeviceToDevice, s.stream) != hipSuccess)
    return mfail(VAQHIP_EHIP, "copy back from the gathered buffer");
  return 0;
}

// after every shard has enqueued its part: gather by copies when RCCL is not in play, merge on
// shard 0's device
int gather_and_merge(vaqhip_multi *mx) {
  Shard &s = mx->sh[0];
  const Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k;
  int32_t *gathered = s.d_gathered.as<int32_t>(), *out_labels = mx->d_out_labels.as<int32_t>();
  MHIP(hipSetDevice(s.device));
  if (G > 1 && !c.rccl) {
    for (int g = 0; g < G; g++) {
      MHIP(hipStreamWaitEvent(s.stream, mx->sh[g].done, 0));
      MHIP(hipMemcpyPeerAsync(gathered + g * c.packed(), s.device, mx->sh[g].d_packed.p, mx->sh[g].device, c.packed_bytes(),
                              s.stream));
    }
  }
  MHIP(hipEventRecord(mx->ev[2], s.stream));
  if (G == 1) return 0;
  const float *gathered_dist = reinterpret_cast<const float *>(gathered + c.plane());
  if (c.fast) {
    // the head rows' distances from the planes of the shards that hold them, then the head's std::sort and
    // the stable merge "head, then the shards' lists in shard order"
    int start[VAQHIP_MAX_DEVICES + 1];
    for (int g = 0; g <= G; g++) start[g] = g < G ? (int)std::min<int64_t>(mx->sh[g].lo, c.kk) : c.kk;
    uint16_t *head = mx->d_head.as<uint16_t>();
    MIX(vaqhip_internal_fast_head_gather_device(s.device, reinterpret_cast<const uint16_t *>(gathered + c.head_at()),
                                                (int64_t)(2 * c.packed()) /* in uint16 */, G, start, nq, c.kk, head, s.stream));
    MIX(vaqhip_merge_fast_device(s.device, head, c.kk, c.kk, mx->id_base, gathered_dist, gathered, G, (int64_t)c.packed(),
                                 (int64_t)k, nq, k, out_labels, mx->d_out_dist, s.stream));
  } else {
    MIX(vaqhip_merge_topk_strided_device(s.device, gathered_dist, gathered, G, (int64_t)c.packed(), (int64_t)k, nq, k,
                                         out_labels, mx->d_out_dist, s.stream));
  }
  return 0;
}

// "exact_ties" across shards, after the merge of the k + 1 lists (mx->call.k): flag on shard 0, the list to
// every shard, the chain of links batch by batch, heap_reorder on shard 0 -> mx->d_final [2][nq][k].
// Issued by the calling thread; everything is enqueued, nothing waited for.  A failure part-way leaves
// streams that wait only for events already recorded (or never recorded: no wait).
int chain_on_shard0(vaqhip_multi *mx) {
  Shard &s = mx->sh[0];
  const Call &c = mx->call;
  const int G = mx->G, nq = c.nq, k = c.k_out();
  const size_t entry = (size_t)c.entry;
  int32_t *fl = mx->d_final.as<int32_t>();
  float *fd = reinterpret_cast<float *>(fl + c.out_plane());
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
    MHIP(hipMemcpyPeerAsync(t.d_list.p, t.device, s.d_list.p, s.device, c.list_bytes(), t.stream));
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
  MHIP(hipMemcpyPeerAsync(s.d_state_in.p, s.device, last.d_state_out.p, last.device, c.state_bytes(), s.stream));
  MIX(vaqhip_internal_exact_finish_device(s.device, s.d_state_in.as<int32_t>(), list_entries(s), list_count(s), nq,
                                          mx->seq ? 1 : 0, k, fl, fd, s.stream));
  return 0;
}

// the result (the caller's k per query, on shard 0's device) to the caller: device buffers behind the
// caller's stream, or the host
int deliver(vaqhip_multi *mx, const int32_t *src_labels, const float *src_dist, int32_t *labels, float *distances,
            hipStream_t user) {
  Shard &s = mx->sh[0];
  const size_t bytes = mx->call.out_plane() * 4;
  MHIP(hipSetDevice(s.device));
  MHIP(hipEventRecord(mx->ev[3], s.stream));
  MHIP(hipEventRecord(mx->consumed, s.stream));
  if (mx->call.d_queries0) {
    // device entry: results into the caller's buffers on shard 0's device; the caller's stream waits
    // for them, the host does not
    MHIP(hipMemcpyAsync(labels, src_labels, bytes, hipMemcpyDeviceToDevice, s.stream));
    MHIP(hipMemcpyAsync(distances, src_dist, bytes, hipMemcpyDeviceToDevice, s.stream));
    MHIP(hipEventRecord(mx->finished, s.stream));
    MHIP(hipStreamWaitEvent(user, mx->finished, 0));
    return 0;
  }
  MHIP(hipMemcpyAsync(labels, src_labels, bytes, hipMemcpyDeviceToHost, s.stream));
  MHIP(hipMemcpyAsync(distances, src_dist, bytes, hipMemcpyDeviceToHost, s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  for (int g = 1; g < mx->G; g++) {  // (their collective / copies are complete before anyone reuses the buffers)
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

// phase 3, on shard 0's device by the calling thread: merge, chain, result
int finish_on_shard0(vaqhip_multi *mx, int32_t *labels, float *distances, hipStream_t user) {
  if (int rc = gather_and_merge(mx)) return rc;
  if (!mx->call.chain) return deliver(mx, mx->d_out_labels.as<int32_t>(), mx->d_out_dist, labels, distances, user);
  if (int rc = chain_on_shard0(mx)) return rc;
  const int32_t *fl = mx->d_final.as<int32_t>();
  return deliver(mx, fl, reinterpret_cast<const float *>(fl + mx->call.out_plane()), labels, distances, user);
}

// one set of queries (mx->call): the shards' searches, the exchange, the merge
// (and the chain) on shard 0, the result to the caller
int search_set(vaqhip_multi *mx, int32_t *labels, float *distances, hipStream_t user) {
  // phase 1: every shard uploads (or copies) the queries and enqueues its search.  When one fails, nothing of the
  // exchange has been enqueued: the shards that did succeed have complete, ordinary work on their streams, and
  // the index stays usable (and destroyable).
  if (int rc = on_shards(mx, [&](int g, Shard &s) {
        const int r = fit_buffers(mx, g, s);
        return r ? r : enqueue_shard(mx, g, s);
      }))
    return rc;
  // phase 2: the exchange, only now that every shard is known to take part (copies: part of phase 3)
  if (mx->call.rccl)
    if (int rc = mx->G > 1 ? exchange_rccl(mx) : allgather_one_rank(mx)) return rc;
  // phase 3
  const int rc = finish_on_shard0(mx, labels, distances, user);
  if (rc) {
    // `consumed` may not have been recorded while copies between devices are enqueued: leave every stream idle, so
    // that the next search may grow its buffers whatever this one left (fit_buffers).  Everything enqueued up to
    // here is complete work; a collective that failed to start (above) is not waited for.
    for (Shard &s : mx->sh)
      if (hipSetDevice(s.device) == hipSuccess) (void)hipStreamSynchronize(s.stream);
    (void)hipSetDevice(mx->sh[0].device);
    return mfail(rc, "exchange / merge on device %d: %s", mx->sh[0].device, mx->sh[0].err.c_str());
  }
  return VAQHIP_OK;
}

// what holds for the whole call; decisions only, nothing is issued
int plan_call(vaqhip_multi *mx, int k, int projected) {
  Call &c = mx->call;
  const int G = mx->G;
  c.projected = projected;
  // FAST over several shards: the head-and-lists form (one shard alone answers as the single index does)
  c.fast = G > 1;
  for (int g = 0; c.fast && g < G; g++) c.fast = vaqhip_internal_fast_in_force(mx->sh[g].ix) != 0;
  if (c.fast && k > VAQHIP_MAX_K) return mfail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  // RCCL when the GPUs are distinct and there is something to exchange (or when asked for by option: a
  // one-shard index then still goes through the collective); device-to-device copies otherwise
  c.rccl = mx->exchange == EX_RCCL || (mx->exchange == EX_AUTO && mx->distinct && G > 1);
  // "exact_ties" over several shards: the chain, where the option has an effect on a single index too
  // (not TI, not FAST, k < VAQHIP_MAX_K)
  c.chain = mx->opt_exact && G > 1;
  for (int g = 0; c.chain && g < G; g++) c.chain = vaqhip_internal_exact_applies(mx->sh[g].ix, k) != 0;
  if (c.chain) c.entry = vaqhip_internal_exact_state_words(mx->sh[0].ix, k);
  return VAQHIP_OK;
}

// the numbers of one set: queries [q0, q0 + n) of the call
void plan_set(vaqhip_multi *mx, const float *queries, const float *d_queries0, int q0, int n, int k) {
  Call &c = mx->call;
  c.queries = queries ? queries + (size_t)q0 * mx->D : nullptr;
  c.d_queries0 = d_queries0 ? d_queries0 + (size_t)q0 * mx->D : nullptr;
  c.nq = n;
  c.k = c.chain ? k + 1 : k;
  // appends may have grown N past k, or the head with it: both are taken from the rows as they are now
  c.kk = c.fast ? (int)std::min<int64_t>(k, mx->N) : 0;
  if (c.chain) {
    // batches of the replay list, chosen from the set's size (the count of tied queries lives on the device)
    int b = mx->opt_exact_batch > 0 ? mx->opt_exact_batch : std::max(64, (n + 15) / 16);
    b = std::max(b, (n + 255) / 256);
    c.batch = b;
    c.n_batches = (n + b - 1) / b;
  }
}

int multi_search_common(vaqhip_multi *mx, const float *queries, const float *d_queries0, hipStream_t user, int nq, int k,
                        int projected, int32_t *labels, float *distances) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (nq < 0 || k <= 0) return mfail(VAQHIP_EINVAL, "nq=%d k=%d", nq, k);
  if (nq == 0) return VAQHIP_OK;
  if ((!queries && !d_queries0) || !labels || !distances) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  const Call &c = mx->call;
  if (int rc = plan_call(mx, k, projected)) return rc;
  // Known quirk: only FAST puts the caller's device back; the other methods leave shard 0's device current, as they
  // always have.  Callers can observe that, so it stays.
  DeviceGuard keep(DeviceGuard::restore_only, c.fast);
  if (c.rccl)
    if (int rc = ensure_comms(mx)) return rc;
  if (d_queries0) {
    if (hipSetDevice(mx->sh[0].device) != hipSuccess || hipEventRecord(mx->user_ready, user) != hipSuccess)
      return mfail(VAQHIP_EHIP, "recording the caller's stream");
  }
  // the chain takes one set of queries at a time, because every link reads the lookup tables its shard built for the set
  const int set = c.chain ? std::min(nq, vaqhip_internal_query_chunk()) : nq;
  for (int q0 = 0; q0 < nq; q0 += set) {
    plan_set(mx, queries, d_queries0, q0, std::min(set, nq - q0), k);
    if (int rc = search_set(mx, labels + (size_t)q0 * k, distances + (size_t)q0 * k, user)) return rc;
  }
  mx->last.exchange = c.rccl ? EX_RCCL : (mx->G == 1 ? 0 : EX_COPIES);
  return VAQHIP_OK;
}

} // namespace

extern "C" {

int vaqhip_multi_search(vaqhip_multi *mx, const float *queries, int nq, int k, int projected, int32_t *labels,
                        float *distances) {
  return multi_search_common(mx, queries, nullptr, nullptr, nq, k, projected, labels, distances);
}

int vaqhip_multi_search_device(vaqhip_multi *mx, const float *d_queries, int nq, int k, int projected, int32_t *d_labels,
                               float *d_distances, void *stream) {
  return multi_search_common(mx, nullptr, d_queries, static_cast<hipStream_t>(stream), nq, k, projected, d_labels,
                             d_distances);
}

} // extern "C"
