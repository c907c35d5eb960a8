// vaqhip_shard_run.h -- what a call that runs across shards with state of its own shares: the call-owned run of the
// sharded fits (vaqhip_multi_lutfit.cpp, vaqhip_multi_codebooks.cpp: workers, streams and buffers that live for one
// call, because the host form has no handle to keep them in) and the teardown every such call ends with, which
// vaqhip_multi_encode.cpp and vaqhip_multi_learn.cpp take too for their per-call scratch on a handle's streams.
#ifndef VAQHIP_SHARD_RUN_H
#define VAQHIP_SHARD_RUN_H
#include "vaqhip_multi_refiner.h"

namespace vaqhost __attribute__((visibility("hidden"))) {

// where one shard's part of a call lives: its device and the stream that may still touch it
struct ShardAt { int device; hipStream_t stream; };

// The teardown of per-call state, part[g] on shard g at at(g), by the calling thread once the workers are through,
// whichever way the call ended: EVERY stream idle before ANYTHING is freed, then part[g].release() with shard g's
// device current.  After a failure part-way a later shard's stream may still hold a copy into an earlier shard's
// buffers, and hipFree waits for the work of the buffer's own device only (vaqhip_multi.h, FitList).  A part that
// holds nothing (held()) is left alone, its device with it.
template <class Part, class At> void idle_then_release(std::vector<Part> &part, At &&at) {
  for (size_t g = 0; g < part.size(); g++)
    if (part[g].held() && hipSetDevice(at((int)g).device) == hipSuccess) (void)hipStreamSynchronize(at((int)g).stream);
  for (size_t g = 0; g < part.size(); g++)
    if (part[g].held()) {
      (void)hipSetDevice(at((int)g).device);
      part[g].release();
    }
}

// what every shard of a call-owned run holds; the file's own shard struct extends it with its buffers, its events and
// a release() for those
struct RunShard {
  int device = 0;
  std::string err;
  hipStream_t stream = nullptr;        // the call's own: made by open(), destroyed by the teardown
  vaq::RowsRef d_rows = {nullptr, 4};  // the shard's rows on its device, float or byte: resident, or uploaded (slice)
  DevBuf slice, eig;                   // host form: the uploaded rows of the call's element; eigvec
  bool held() const { return stream != nullptr; }  // (open() makes the stream before anything else)
};

// What on_shards runs over (G, pool, sh[] with device and err), owned by one call.  S extends RunShard.
template <class S> struct ShardRun {
  DeviceGuard keep{DeviceGuard::restore_only};  // (first: it puts the caller's device back after everything is released)
  int G = 0;
  std::vector<S> sh;
  vaq::JobPool pool;
  vaq::RowsRef X = {nullptr, 4};  // host form: the call's matrix, float or byte
  const float *eig = nullptr;     // host pointer or null

  // the host form's shards
  int from_devices(int n_devices, const int *device_ids) {
    if (n_devices < 1 || n_devices > VAQHIP_MAX_DEVICES)
      return mfail(VAQHIP_EINVAL, "n_devices=%d outside 1..%d", n_devices, VAQHIP_MAX_DEVICES);
    G = n_devices;
    sh.resize((size_t)G);
    for (int g = 0; g < G; g++) sh[(size_t)g].device = device_ids[g];
    return VAQHIP_OK;
  }

  // the refiner form's: its devices, its resident rows read in place, their counts to cnt[G] (r->mu held)
  void from_refiner(const vaqhip_multi_refiner *r, int64_t *cnt) {
    G = r->G;
    sh.resize((size_t)G);
    for (int g = 0; g < G; g++) {
      const ResidentRows rows = resident_rows(r, g);
      sh[(size_t)g].device = r->sh[g].device;
      sh[(size_t)g].d_rows = rows.rows;
      cnt[g] = rows.n;
    }
  }

  // The start of a shard's setup, on its worker: the device current, the stream, and for a shard of n > 0 rows the
  // host form's rows [lo, lo + n) as the elements the caller holds (`rows_up` false: the caller uploads its own
  // choice of them) and eigvec.  Enqueues only.
  int open(S &s, int64_t lo, int64_t n, int D, bool rows_up = true) const {
    if (hipSetDevice(s.device) != hipSuccess) {
      s.err = "hipSetDevice failed (no CPU path)";
      return VAQHIP_ENODEVICE;
    }
    MHIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (n == 0) return 0;
    if (X.p && rows_up) {
      const size_t bytes = (size_t)n * D * (size_t)X.elem;
      MHIP(s.slice.ensure(bytes));
      MHIP(hipMemcpyAsync(s.slice.p, vaq::rows_at(X, (size_t)lo * D).p, bytes, hipMemcpyHostToDevice, s.stream));
      s.d_rows = vaq::RowsRef{s.slice.p, X.elem};
    }
    if (eig) {
      MHIP(s.eig.ensure((size_t)D * D * sizeof(float)));
      MHIP(hipMemcpyAsync(s.eig.p, eig, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice, s.stream));
    }
    return 0;
  }

  // a phase's time over the call: the slowest shard's (S holds ms[])
  float max_ms(int phase) const {
    float m = 0.0f;
    for (const S &s : sh) m = std::max(m, s.ms[phase]);
    return m;
  }

  // the workers first; then idle_then_release over the shards that were opened: the shard's own buffers and events
  // (S::release); the base's buffers and the stream last
  ~ShardRun() {
    pool.stop();
    idle_then_release(sh, [&](int g) { return ShardAt{sh[(size_t)g].device, sh[(size_t)g].stream}; });
    for (S &s : sh) {
      if (!s.held() || hipSetDevice(s.device) != hipSuccess) continue;
      release_all({&s.slice, &s.eig});
      (void)hipStreamDestroy(s.stream);
      s.stream = nullptr;
    }
  }
};

}  // namespace vaqhost
#endif
