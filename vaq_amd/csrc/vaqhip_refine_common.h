// vaqhip_refine_common.h -- what the two refiner hosts share (vaqhip_refiner.cpp: one device; vaqhip_multi_refiner*.cpp:
// the rows cut over shards): the checks of a call, the options, the store of one device's raw rows, the staging of the
// host forms, and (vaqhip_exhaust_plan.h) the exhaustive form's plan.  A check takes the host it speaks for, so that
// its text lands in that host's thread-local (vaqhip_last_error / vaqhip_multi_last_error) under that host's name.
#ifndef VAQHIP_REFINE_COMMON_H
#define VAQHIP_REFINE_COMMON_H
#include "vaqhip.h"

#include <cstring>
#include <mutex>

#include "vaqhip_exhaust_plan.h"

namespace vaqhost __attribute__((visibility("hidden"))) {

constexpr int REFINE_MAX_R = 2048;

struct RefineHost { int (*fail)(int, const char *, ...); const char *name; };  // name: "refiner", "multi refiner"

inline int check_sizes(const RefineHost &h, const void *r, int nq, int R, int k) {
  if (!r) return h.fail(VAQHIP_EINVAL, "%s is null", h.name);
  if (nq < 0 || R <= 0 || k <= 0) return h.fail(VAQHIP_EINVAL, "bad sizes (nq=%d R=%d k=%d)", nq, R, k);
  if (R > REFINE_MAX_R || k > R) return h.fail(VAQHIP_EUNSUPPORTED, "need k <= R <= %d (R=%d k=%d)", REFINE_MAX_R, R, k);
  return VAQHIP_OK;
}

inline int check_labels_fit(const RefineHost &h, int64_t N, int64_t id_base) {
  if (id_base < 0) return h.fail(VAQHIP_EINVAL, "id_base < 0");
  if (N > 0x7fffffffLL - 1 || id_base + N > 0x7fffffffLL)
    return h.fail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld", (long long)(id_base + N));
  return VAQHIP_OK;
}

inline int check_search(const RefineHost &h, const void *r, int nq, int k, const void *a, const void *b, const void *c) {
  if (!r) return h.fail(VAQHIP_EINVAL, "%s is null", h.name);
  if (nq < 0 || k < 1) return h.fail(VAQHIP_EINVAL, "bad sizes (nq=%d k=%d)", nq, k);
  if (k > VAQHIP_MAX_K) return h.fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (nq > 0 && (!a || !b || !c)) return h.fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

// "exact_ties", "timing" (events around the phases), "exhaustive_splits" (per shard, 0 = automatic)
struct RefineOptions { int exact = 0, timing = 0, splits = 0; };

// vaqhip_[multi_]refiner_set_option: a bad key or value is refused before the refiner is touched
template <class Refiner> int set_option(const RefineHost &h, Refiner *r, const char *key, int64_t value) {
  if (!r || !key) return h.fail(VAQHIP_EINVAL, "null pointer");
  const bool exact = std::strcmp(key, "exact_ties") == 0, timing = std::strcmp(key, "timing") == 0,
             splits = std::strcmp(key, "exhaustive_splits") == 0;
  if (!exact && !timing && !splits) return h.fail(VAQHIP_EINVAL, "unknown option '%s'", key);
  if (splits && (value < 0 || value > 64))
    return h.fail(VAQHIP_EINVAL, "exhaustive_splits=%lld: 0 (automatic) or 1..64", (long long)value);
  std::lock_guard<std::mutex> lk(r->mu);
  (exact ? r->opt.exact : timing ? r->opt.timing : r->opt.splits) = splits ? (int)value : value != 0;
  return VAQHIP_OK;
}

// One device's raw rows: grow-only, appends grow it geometrically.  Used with its device current.
// The rows are of one element type, float32 or uint8 (elem: the element's size, 4 or 1); retype() changes it when no
// row is kept.
struct RowStore {
  DevBuf buf;
  int64_t cap_rows = 0;  // rows the allocation holds
  int elem = 4;
  static constexpr int64_t DROP = -1;
  vaq::RowsRef rows() const { return vaq::RowsRef{buf.p, elem}; }
  size_t row_bytes(int D) const { return (size_t)D * elem; }
  // the rows to come are of `elem_size` bytes an element: the allocation stays and holds more or fewer of them.  The
  // caller keeps no row across the change (a set, or an append to none); no device work.
  void retype(int elem_size, int D) {
    if (elem_size == elem) return;
    elem = elem_size;
    cap_rows = (int64_t)(buf.cap / row_bytes(D));
  }
  // room for `rows` rows of D elements; keep_n >= 0: an append, the first keep_n survive, growth by half at least; DROP: none
  hipError_t reserve(int64_t rows, int64_t keep_n, int D) {
    if (rows <= cap_rows) return hipSuccess;
    const int64_t want = keep_n >= 0 ? std::max(rows, cap_rows + cap_rows / 2) : rows;
    DevBuf nb;
    XS_TRY(nb.ensure((size_t)want * row_bytes(D)));
    XS_TRY(hipDeviceSynchronize());  // (a refine enqueued on any stream may still read the old rows)
    if (keep_n > 0) XS_TRY(hipMemcpy(nb.p, buf.p, (size_t)keep_n * row_bytes(D), hipMemcpyDeviceToDevice));
    std::swap(nb.p, buf.p);
    std::swap(nb.cap, buf.cap);
    cap_rows = want;
    return hipSuccess;
  }
};

// the workspaces of the host forms (queries, candidate labels, the answer) and the fused call's candidates
struct StagingBufs {
  DevBuf q, lin, lout, dout, cand_l, cand_d;
  void release() { release_all({&q, &lin, &lout, &dout, &cand_l, &cand_d}); }
};

// The host form of a device call: chunks of `chunk` queries through `w` on stream st; labels_in may be null.  call(n)
// runs one staged chunk from w.q (w.lin) into w.lout, w.dout and returns the host's code; a code other than 0 ends
// the loop and is left in rc.  Returns the first HIP error.
template <class Call> hipError_t through_staging(StagingBufs &w, hipStream_t st, int D, int chunk, const float *queries, int nq,
                                                 const int32_t *labels_in, int R, int k, int32_t *labels_out,
                                                 float *distances_out, int &rc, Call &&call) {
  XS_TRY(w.q.ensure((size_t)chunk * D * sizeof(float)));
  if (labels_in) XS_TRY(w.lin.ensure((size_t)chunk * R * sizeof(int32_t)));
  XS_TRY(w.lout.ensure((size_t)chunk * k * sizeof(int32_t)));
  XS_TRY(w.dout.ensure((size_t)chunk * k * sizeof(float)));
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    XS_TRY(hipMemcpyAsync(w.q.p, queries + (size_t)q0 * D, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, st));
    if (labels_in)
      XS_TRY(hipMemcpyAsync(w.lin.p, labels_in + (size_t)q0 * R, (size_t)n * R * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = call(n)) != 0) return hipSuccess;
    XS_TRY(hipMemcpyAsync(labels_out + (size_t)q0 * k, w.lout.p, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XS_TRY(hipMemcpyAsync(distances_out + (size_t)q0 * k, w.dout.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
    XS_TRY(hipStreamSynchronize(st));
  }
  return hipSuccess;
}

}  // namespace vaqhost

// What another handle's call reads of a single-device refiner (vaqhip_bitvec.cpp: the rerank over its resident rows).
// Defined in vaqhip_refiner.cpp.  The caller holds refiner_mutex(r) from refiner_view(r) until the work that reads the
// rows is enqueued: a set or an append waits for the device before it moves them.
struct vaqhip_refiner;
namespace vaqhost __attribute__((visibility("hidden"))) {
struct RefinerView {
  vaq::RowsRef rows;
  int64_t N, id_base;
  int device, D;
};
std::mutex &refiner_mutex(vaqhip_refiner *r);
RefinerView refiner_view(const vaqhip_refiner *r);
}  // namespace vaqhost
#endif
