// vaqhip_index.h -- what the host files of the single-device index share: the index itself, its device
// buffers (vaqhip_dev.h), the entry preamble, the workspace scope, the launch plan and the few functions
// that cross files -- among them the one encode driver (EncodeRule, encode_rows_locked and its two entries: defined in
// vaqhip_api.cpp, called there for vaqhip_encode* and from vaqhip_lutfit.cpp for vaqhip_encode_lut*).  Private to
// vaqhip_api.cpp, vaqhip_plan.cpp, vaqhip_search.cpp, vaqhip_codes.cpp, vaqhip_fast.cpp and vaqhip_lutfit.cpp (vaqhip_refiner.cpp takes
// fail(), HIP_TRY and the device types from here and reaches the index through include/vaqhip.h): the multi-device host
// (vaqhip_multi*.cpp) sees the index through include/vaqhip.h and vaqhip_internal.h only.
#ifndef VAQHIP_INDEX_H
#define VAQHIP_INDEX_H
#include "vaqhip.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "vaq_common.h"
#include "vaq_scan_bm.h"
#include "vaq_scan_params.h"
#include "vaqhip_dev.h"
#include "vaqhip_internal.h"

// (hidden: none of this joins the library's exported symbols)
namespace vaqhost __attribute__((visibility("hidden"))) {

// sets vaqhip_last_error()'s text for this thread (vaqhip_api.cpp) and returns `code`
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(e_ == hipErrorOutOfMemory ? VAQHIP_ENOMEM : VAQHIP_EHIP, "%s: %s", #expr, \
                  hipGetErrorString(e_));                                                 \
  } while (0)

constexpr int QUERY_CHUNK = 16384;             // queries per internal launch set
// (launch_cost_order pays from about one residency of workgroups on: 7 per CU)
constexpr int COST_ORDER_MIN_QUERIES = 1024;
// option "defer_units" (vaqhip_plan.cpp): workgroups per query of the second launch, queries it takes at most
constexpr int DEFER_SLICES = 2, DEFER_CAP = 2048;

// ---- bucket-major rounds (vaq_scan_bm.hip): shared by the one-call search and the staged one ----
struct BmRoundInfo {
  int chunk, n, cap, qb, units;
};

struct StagedState {
  bool open = false;
  vaq::BmParams bp;
  vaq::ScanParams sp;
  BmRoundInfo bi;
  int k = 0, defer_cap = 0, nr = 0, r_next = 0;
  int limits[4] = {0, 0, 0, 0};
  int32_t *labels = nullptr;
  float *dist = nullptr;
};

} // namespace vaqhost

struct vaqhip_index {
  using DevBuf = vaqhost::DevBuf;
  int D = 0, M = 0, L = 0;
  int max_bits = 0, min_bits = 0, total_bits = 0, W = 0, layout = 0, lut_floats = 0;
  int device = 0, n_cu = 256;
  std::vector<int> bits;
  std::vector<vaq::SubDesc> sub;
  DevBuf d_cent, d_cent_t, d_eig, d_sub, d_first_sub, d_codes, d_perm, d_bstart;
  // byte codes bucketed by the whole first code: rows of a bucket are ordered by the rest of the
  // second code too, d_sub holds the first row of every (first code, second code) run
  // (sub_fine = bits of the second code below the bucket key; 0 = no such order, e.g. after an append)
  DevBuf d_substart;
  int sub_fine = 0;
  bool has_eig = false;
  int seq = 0;  // 1: BitVecEngine::queryLUT's sequential row sum
  int bucket_shift = 0, bucket_t = 0, n_buckets = 1;  // bucketed row order (set with the codes)
  int64_t N = -1, id_base = 0;
  int64_t N_keyed = 0;  // rows the bucket key width was chosen for (appends rebuild once N outgrows it 4x)
  // triangle-inequality form (VAQ::clusterTI): rows grouped by cluster instead of by first
  // code; d_bstart then holds the cluster starts, n_buckets = ti_T, bucket_shift = 0
  int ti_T = 0, ti_seg = 0;
  float ti_visit = 1.0f;              // mVisit
  unsigned methods = VAQHIP_METHOD_HEAP;
  DevBuf d_ti_clusters, d_ti_clusters_t, d_ti_xcc, w_ti_order, w_ti_qcc, w_ti_nvisit;
  // workspace (grow-only, reused across searches)
  DevBuf w_q, w_qproj, w_lut, w_part_d, w_part_id, w_part_cnt, w_labels, w_dist, w_stage, w_lutref, w_thr, w_ms_d, w_ms_id, w_order, w_qorder;
  DevBuf w_cost;   // [nq] cost keys of launch_cost_order
  DevBuf w_defer;  // [0] entries asked for, then DEFER_CAP records (best-first form, queries cut in two)
  // bucket-major second pass: plan arrays, per-bucket query lists, candidates, per-query words
  DevBuf w_bm_small, w_bm_mask, w_bm_qlist, w_bm_cand_d, w_bm_cand_id, w_bm_query, w_bm_thr64;
  // option "exact_ties": original row -> bucketed row (built at the first such search after the codes change),
  // the scan's k + 1 results, the replay list
  DevBuf d_inv, d_rowbucket, w_ex_labels, w_ex_dist, w_ex_list;
  // ... on a TI index: position in the reference's member order -> index row (vaq::ti_build_walk), built at the
  // first such search after the rows were (re)grouped
  DevBuf d_ti_walk;
  bool ti_walk_valid = false;
  bool sharded = false;  // one shard of several (vaqhip_internal_set_sharded): no TI replay, the shards merge by (distance, label)
  vaqhost::StagedState staged;  // vaqhip_search_begin_device .. vaqhip_search_finish_device
  // FAST (max bits <= 4): the codes again in ORIGINAL row order as nibbles (vaq_fast.h), rows padded to
  // FAST_ROW_PAD with code 0; mOffsets / mScale on the host and the device; per-call workspaces
  DevBuf d_fast_codes, d_fast_off, d_fast_scale, w_fast_small, w_fast_dist, w_fast_order, w_fast_scratch;
  bool fast_ok = false;   // the index can hold FAST codes (max bits <= 4, groups of four, not sequential)
  bool fast_q = false;    // a quantisation is set
  // the FAST code image exists only while FAST is the method in force: built at the first FAST search
  // after the codes or the method changed, kept current by set/add codes while FAST stays in force,
  // released (with the FAST workspaces) when another method is set
  int64_t fast_rows = -1;  // rows the image holds, -1 = no image
  int64_t fast_cap = 0;    // rows its allocation holds (multiple of FAST_ROW_PAD)
  std::vector<float> fast_off, fast_scale;
  bool inv_valid = false;
  // a sequential-sum index that can encode (vaqhip_index_set_lut_quantiles): Q[D][257] of
  // BitVecEngine::binaryEncodingLUT on the host, its prefix maxima packed on the device (vaq_lutfit.h)
  std::vector<float> lut_q;
  DevBuf d_lut_pm;
  hipStream_t stream = nullptr;
  // The workspaces above are shared by every call on this index.  Host-side enqueues are
  // serialised by `mu`, but `_device` entry points run on the caller's stream: the last enqueue
  // that used the workspaces leaves an event, and a call on a DIFFERENT stream makes its stream
  // wait for it first (same stream: in order anyway).
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  // options
  int opt_qb = 0, opt_slices = 0, opt_timing = 0, opt_ea = 3, opt_nwaves = 0, opt_seed = 1, opt_hot = 16, opt_seed_frac = 64, opt_order = 0, opt_bucket_bits = 0, opt_no_skip = 0, opt_bf = 1, opt_group = 1, opt_defer = 0, opt_cost_order = 1, opt_bm = 1, opt_bm_cap = 0, opt_bm_units = 0, opt_bm_qb = 0, opt_bm_nwaves = 0, opt_sub_order = 1, opt_bm_sub = 1, opt_bm_boot = 1, opt_bm_round = 6, opt_exact = 0;
  // timing: a ring of 5-event sets, one per search since the last read
  static constexpr int EV_SETS = 256;
  std::vector<hipEvent_t> ev;   // EV_SETS * 6, created on first use
  int ev_used = 0;              // searches recorded since the last vaqhip_last_timing
  vaqhip_timing last = {};
  vaqhip_kmeans_timing km_last = {};  // the last vaqhip_index_cluster_ti_kmeans
  vaqhip_learn_timing learn_last = {};  // the last device-form learnQuantization (vaqhip_learn.cpp)
  std::mutex mu;
};

namespace vaqhost __attribute__((visibility("hidden"))) {

struct Plan {
  int qb, ea, kp, ccap, qcap, nwaves, n_slices;
  int lds_subs, lut_lds_entries;  // LUT tables staged in LDS (a prefix of the subspaces)
  int ti_cap = 0;                 // TI form: visiting-list entries staged at a time
  int64_t slice_rows;
  size_t lds;
  // sampling pre-pass that seeds the shared thresholds (0 slices = none)
  int seed_slices;
  int64_t seed_rows, seed_stride;
  bool ordered;  // slices dispatched best-first per query batch
  bool bf = false;  // best-first scan form (vaq_scan_bf.h)
  int bf_carry = 0;
  int bf_pool = 0;
  int defer_units = 0;  // > 0: expensive queries are cut in two (ScanParams::defer_*)
  bool cost_order = false;  // one best-first workgroup per query: expensive queries are dispatched first
  bool bm = false;          // bucket-major rounds (vaq_scan_bm.hip)
  bool bm_boot = false;     //   thresholds from a sample instead of a capped best-first pass
  int bm_qb = 0, bm_nwaves = 0, bm_cap = 0;
};

// vaqhip_plan.cpp
int make_plan(const vaqhip_index *ix, int nq, int k, Plan *pl);
int make_ti_plan(const vaqhip_index *ix, int nq, int k, Plan *pl);
// vaqhip_search.cpp: the preamble of every search.  `method_err`: what the method in force has against the
// index's state, or nullptr.  nq == 0 passes (the caller returns VAQHIP_OK before it touches a pointer)
int check_search_args(const vaqhip_index *ix, const float *d_queries, int nq, int k, const int32_t *d_labels,
                      const float *d_dist, const char *method_err);
// vaqhip_fast.cpp
struct FastShardPart;
bool fast_only(const vaqhip_index *ix);
int search_fast(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected, int32_t *d_labels,
                float *d_dist, hipStream_t st, const FastShardPart *part = nullptr);
void fast_release(vaqhip_index *ix);
int fast_codes_update(vaqhip_index *ix, const uint16_t *d_u16, int64_t row_begin, int64_t row_end, hipStream_t st);
// vaqhip_index_set_lut_quantization with the index locked and its device current
int set_quantization_locked(vaqhip_index *ix, const float *off, const float *scale);
// vaqhip_api.cpp: rows of either element type to codes -- the one driver behind vaqhip_encode* (encode_rule_vaq) and
// vaqhip_encode_lut* (encode_rule_lut, entries in vaqhip_lutfit.cpp).  A rule says what differs between the two
struct EncodeRule {
  bool lut;                                  // encodeToLUTCode: ESTATE without quantiles (before the n == 0 return)
  bool (*project)(const vaqhip_index *ix);   // do unprojected rows need launch_project?
  hipError_t (*launch)(const vaqhip_index *ix, const float *xp, int64_t m, uint16_t *d_codes, hipStream_t st);
};
EncodeRule encode_rule_vaq();
EncodeRule encode_rule_lut();
// the refusals both entries start with: null index, bad arguments, the rule's own; n == 0 passes
int check_encode_args(const vaqhip_index *ix, const EncodeRule &rule, const void *X, int64_t n, const void *codes);
// the chunk loop, on `st`: caller holds ix->mu and has the device current
int encode_rows_locked(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef d_X, int64_t n, int projected,
                       uint16_t *d_codes, hipStream_t st);
int encode_device_entry(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef d_X, int64_t n, int projected,
                        uint16_t *d_codes, void *stream);
int encode_host_entry(vaqhip_index *ix, const EncodeRule &rule, vaq::RowsRef X, int64_t n, int projected, uint16_t *codes);
// vaqhip_learn.cpp: vaqhip_learn_quantization[_u8]_device's body, which vaqhip_refiner.cpp calls over its resident
// rows (n x D on the index's device, complete); takes the index's lock itself
int learn_rows_device(vaqhip_index *ix, vaq::RowsRef d_X, int64_t n, int projected, float ratio, float *offsets_out,
                      float *scale_out);
// vaqhip_codebooks.cpp: vaqhip_fit_codebooks[_u8]'s body from the upload on -- or, by `form`, that of the hierarchical
// (subspaces above 8 bits in two stages) or the binary form (as a tree of 2-centre fits) --, which vaqhip_refiner.cpp
// calls over its resident rows (n x D on `device`, complete); eigvec and the outputs are the host's
enum class CodebookForm { FLAT = 0, HIER, BIN };
int fit_codebooks_rows_device(CodebookForm form, int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                              const float *eigvec, int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out);
// vaqhip_train.cpp: vaqhip_train_moment's and vaqhip_train_rotation's bodies over rows resident on `device`, which
// vaqhip_refiner.cpp calls over its resident rows (complete); the outputs are the host's
int train_moment_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, double *cov_out, float *cov_f_out);
int train_rotation_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, int bit_budget, int min_bits,
                               int max_bits, float percent_var, float *eigvec_out, float *eigenvalues_out, int *bits_out,
                               int *highest_subs_out);

// The preamble of an entry point: the index's lock, then its device current (put back when the scope ends).
// rc: VAQHIP_OK, or what the entry returns at once -- ENTRY(ix) declares it and does so, as HIP_TRY would.
#define ENTRY(ix) Entry entry_(ix); if (entry_.rc) return entry_.rc
struct Entry {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  int rc;
  explicit Entry(vaqhip_index *ix)
      : lk(ix->mu), g(ix->device),
        rc(g.ok ? VAQHIP_OK : fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", ix->device)) {}
};

// Around the enqueueing of work that touches the index's shared workspaces on stream `st`: construction makes
// `st` wait for the last such work on another stream (rc: its code), finish() leaves the event for the next call
// and is the success path.  A return before finish() is a failure with work possibly enqueued already: the
// destructor leaves the event all the same, without touching the failure's code and text.
// WS_SCOPE(ws, ix, st) declares the scope and returns its code at once when the construction failed.
// Owner: the index, or another handle that keeps the same three members (ws_event, ws_stream, ws_used) for workspaces
// of its own (vaqhip_bitvec.cpp); the macro's argument names it.
#define WS_SCOPE(name, ix, st) WsScope name(ix, st); if (name.rc) return name.rc
template <class Owner> struct WsScope {
  Owner *ix;
  hipStream_t st;
  bool open = false;
  int rc;
  WsScope(Owner *ix, hipStream_t st) : ix(ix), st(st), rc(acquire()) { open = rc == VAQHIP_OK; }
  WsScope(const WsScope &) = delete;
  ~WsScope() {
    if (open && hipEventRecord(ix->ws_event, st) == hipSuccess) mark();
  }
  int finish() {
    open = false;
    HIP_TRY(hipEventRecord(ix->ws_event, st));
    mark();
    return VAQHIP_OK;
  }

 private:
  int acquire() {
    if (!ix->ws_event) HIP_TRY(hipEventCreateWithFlags(&ix->ws_event, hipEventDisableTiming));
    if (ix->ws_used && st != ix->ws_stream) HIP_TRY(hipStreamWaitEvent(st, ix->ws_event, 0));
    return VAQHIP_OK;
  }
  void mark() {
    ix->ws_stream = st;
    ix->ws_used = true;
  }
};

inline int ensure_events(vaqhip_index *ix) {
  if (!ix->ev.empty()) return VAQHIP_OK;
  std::vector<hipEvent_t> ev(vaqhip_index::EV_SETS * 6);
  for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
  ix->ev.swap(ev);
  return VAQHIP_OK;
}

} // namespace vaqhost
#endif
