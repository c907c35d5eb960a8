// vaqhip_handle.h -- what a single-device handle of include/vaqhip.h is made of (vaqhip_index, vaqhip_refiner,
// vaqhip_bitvec): the error text of the thread, the members every handle keeps (HandleCore), the preamble of an entry
// point, the scope around work on the handle's shared workspaces, and the steps of a create and a destroy that the
// handles have in common.  It holds nothing of vaqhip_index.
#ifndef VAQHIP_HANDLE_H
#define VAQHIP_HANDLE_H
#include "vaqhip.h"

#include <hip/hip_runtime.h>
#include <mutex>

#include "vaqhip_dev.h"

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

struct HandleCore {
  int device = 0;
  hipStream_t stream = nullptr;  // of the host forms
  // The handle's workspaces are shared by every call on it.  Host-side enqueues are serialised by `mu`, but
  // `_device` entry points run on the caller's stream: the last enqueue that used the workspaces leaves an
  // event, and a call on a DIFFERENT stream makes its stream wait for it first (same stream: in order anyway).
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  std::mutex mu;
};

// The preamble of an entry point: the handle's lock, then its device current (put back when the scope ends).
// rc: VAQHIP_OK, or what the entry returns at once -- ENTRY(h) declares it and does so, as HIP_TRY would.
#define ENTRY(h) Entry entry_(h); if (entry_.rc) return entry_.rc
struct Entry {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  int rc;
  explicit Entry(HandleCore *h)
      : lk(h->mu), g(h->device),
        rc(g.ok ? VAQHIP_OK : fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", h->device)) {}
};

// Around the enqueueing of work that touches the handle's shared workspaces on stream `st`: construction makes
// `st` wait for the last such work on another stream (rc: its code), finish() leaves the event for the next call
// and is the success path.  A return before finish() is a failure with work possibly enqueued already: the
// destructor leaves the event all the same, without touching the failure's code and text.
// WS_SCOPE(ws, h, st) declares the scope and returns its code at once when the construction failed.
#define WS_SCOPE(name, h, st) WsScope name(h, st); if (name.rc) return name.rc
struct WsScope {
  HandleCore *h;
  hipStream_t st;
  bool open = false;
  int rc;
  WsScope(HandleCore *h, hipStream_t st) : h(h), st(st), rc(acquire()) { open = rc == VAQHIP_OK; }
  WsScope(const WsScope &) = delete;
  ~WsScope() {
    if (open && hipEventRecord(h->ws_event, st) == hipSuccess) mark();
  }
  int finish() {
    open = false;
    HIP_TRY(hipEventRecord(h->ws_event, st));
    mark();
    return VAQHIP_OK;
  }

 private:
  int acquire() {
    if (!h->ws_event) HIP_TRY(hipEventCreateWithFlags(&h->ws_event, hipEventDisableTiming));
    if (h->ws_used && st != h->ws_stream) HIP_TRY(hipStreamWaitEvent(st, h->ws_event, 0));
    return VAQHIP_OK;
  }
  void mark() {
    h->ws_stream = st;
    h->ws_used = true;
  }
};

// what every create refuses of its device_id
inline int check_device_id(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VAQHIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
  if (device_id < 0 || device_id >= ndev) return fail(VAQHIP_EINVAL, "device_id=%d of %d", device_id, ndev);
  return VAQHIP_OK;
}

// a new handle's device and, on it, its stream
inline int open_handle(HandleCore *h, int device_id) {
  h->device = device_id;
  DeviceGuard g(device_id);
  const hipError_t e = g.ok ? hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) : hipErrorInvalidDevice;
  if (e != hipSuccess) return fail(VAQHIP_ENODEVICE, "device %d: %s", device_id, hipGetErrorString(e));
  return VAQHIP_OK;
}

// the end of a handle's stream and event: its device current, and whatever may still run on them waited for
inline void close_handle(HandleCore *h) {
  if (h->stream) (void)hipStreamDestroy(h->stream);
  if (h->ws_event) (void)hipEventDestroy(h->ws_event);
}

} // namespace vaqhost
#endif
