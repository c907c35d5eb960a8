// vaqhip_dev.h -- what every host of the library owns device state with: a grow-only device buffer, the
// events of an option "timing" and the guard of the current device.  Shared by the single-index host files
// (through vaqhip_index.h), the multi-device host files (through vaqhip_multi.h) and the two kernel files that
// allocate scratch (vaq_codes.hip, vaq_ti.hip).  It holds nothing of vaqhip_index.
#ifndef VAQHIP_DEV_H
#define VAQHIP_DEV_H
#include <hip/hip_runtime.h>
#include <cstddef>
#include <initializer_list>
#include <vector>

// (hidden: none of this joins the library's exported symbols)
namespace vaqhost __attribute__((visibility("hidden"))) {

// Freed by release() or the destructor, with the CALLER's current device: the owner makes the buffer's
// device current (and its streams idle) first.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) {  // one owner: moved into a container, never copied or assigned
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(DevBuf &&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // grow-only; the old contents are not kept
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Creates those of e[0..n) that are still null: the events of an option "timing", made when it is first used.
inline hipError_t ensure_events(hipEvent_t *e, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!e[i])
      if (const hipError_t r = hipEventCreate(&e[i])) return r;
  return hipSuccess;
}

inline void destroy_events(hipEvent_t *e, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (e[i]) (void)hipEventDestroy(e[i]);
    e[i] = nullptr;
  }
}

template <size_t N> hipError_t ensure_events(hipEvent_t (&e)[N]) { return ensure_events(e, N); }
template <size_t N> void destroy_events(hipEvent_t (&e)[N]) { destroy_events(e, N); }

// The events of an option "timing" where their number grows with the call: the first n exist after ensure(n).
struct EventList {
  std::vector<hipEvent_t> e;
  hipError_t ensure(size_t n) {
    while (e.size() < n) e.push_back(nullptr);
    return ensure_events(e.data(), n);
  }
  hipEvent_t operator[](size_t i) const { return e[i]; }
  void release() { destroy_events(e.data(), e.size()); }
};

// A stream of one call's own: non-blocking, made by open() with the device current, synchronised and destroyed when it
// leaves scope.  Declared behind what the stream's work reads and writes.
struct CallStream {
  hipStream_t s = nullptr;
  CallStream() = default;
  CallStream(const CallStream &) = delete;
  CallStream &operator=(const CallStream &) = delete;
  hipError_t open() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  ~CallStream() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
};

inline void release_all(std::initializer_list<DevBuf *> bufs) {
  for (DevBuf *b : bufs) b->release();
}

// Makes `dev` current and puts the caller's device back when the scope ends; the restore-only form
// leaves the current device alone and only puts it back (`active` false: not even that).
struct DeviceGuard {
  enum RestoreOnly { restore_only };
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  explicit DeviceGuard(RestoreOnly, bool active = true) : ok(true) {
    if (active && hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

} // namespace vaqhost
#endif
