// What the library allocates through the HIP runtime, owned by type: device buffers, pinned host buffers, events, streams.  Each
// is freed by its destructor, so a scene, a context or a local gives back what it holds wherever it ends -- no list to extend.
// Non-copyable, movable.  Host only.
// NO OBJECT OF THESE TYPES MAY HAVE STATIC STORAGE DURATION: its destructor would run after the HIP runtime has shut down and
// must not call into it.  They live in scenes, contexts and locals ("Ownership").
#ifndef MIRT_DEV_MEM_H
#define MIRT_DEV_MEM_H

#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdio>

#include "../../include/mirt.h"

namespace mirt {

int hip_fail(hipError_t e, const char* what, const char* file, int line);   // sets the last-error string, returns MIRT_ERR_HIP

namespace detail {
struct DeviceMem {
  static hipError_t take(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void give(void* p) { (void)hipFree(p); }
  static constexpr const char* what = "hipMalloc";
};
struct PinnedMem {
  static hipError_t take(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void give(void* p) { (void)hipHostFree(p); }
  static constexpr const char* what = "hipHostMalloc";
};

// An allocation and its capacity in elements of T.  After any failed allocation: empty, capacity 0.
template <class T, class Mem>
class Buf {
public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept
  {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~Buf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }
  void reset()
  {
    if (p_) Mem::give(p_);
    p_ = nullptr; cap_ = 0;
  }
  // Free, then allocate n elements (n = 0: stay empty).  The runtime's status, nothing reported: for the caller that can do
  // without the buffer.
  hipError_t alloc_raw(size_t n)
  {
    reset();
    if (n == 0) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = Mem::take(&p, sizeof(T) * n);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p); cap_ = n;
    return hipSuccess;
  }
  // The same, a failure reported: MIRT_OK or MIRT_ERR_HIP.  The caller has made sure that nothing still uses the old block.
  // (The message names the CALLER's file and line -- the defaults are evaluated where the call is written -- and the runtime
  // call, with the buffer's `name` where the caller gives one: "hipMalloc(heap)".)
  int alloc(size_t n, const char* name = nullptr, const char* file = __builtin_FILE(), int line = __builtin_LINE())
  {
    const hipError_t e = alloc_raw(n);
    if (e == hipSuccess) return MIRT_OK;
    char what[96];
    snprintf(what, sizeof(what), name ? "%s(%s)" : "%s", Mem::what, name);
    return hip_fail(e, what, file, line);
  }
  // A buffer that only grows, used by the work on one stream.  Below `need` elements: wait for that stream -- an earlier call
  // on it may still be using the smaller block -- free it, allocate `need`.  (A buffer that work on OTHER streams reads waits
  // for more at its site, then calls alloc.)
  int grow(size_t need, hipStream_t stream, const char* name = nullptr, const char* file = __builtin_FILE(), int line = __builtin_LINE())
  {
    if (cap_ >= need) return MIRT_OK;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize", file, line);
    return alloc(need, name, file, line);
  }

private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
} // namespace detail

template <class T> using DevBuf = detail::Buf<T, detail::DeviceMem>;         // hipMalloc / hipFree
template <class T> using PinnedBuf = detail::Buf<T, detail::PinnedMem>;      // hipHostMalloc / hipHostFree

class Event {
public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept
  {
    if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
    return *this;
  }
  ~Event() { reset(); }

  operator hipEvent_t() const { return e_; }
  void reset()
  {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  // creates the event if there is none (a failure names the caller's file and line, as Buf::alloc does)
  int create(unsigned flags = hipEventDefault, const char* file = __builtin_FILE(), int line = __builtin_LINE())
  {
    if (e_) return MIRT_OK;
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    if (e == hipSuccess) return MIRT_OK;
    e_ = nullptr;
    return hip_fail(e, "hipEventCreate", file, line);
  }

private:
  hipEvent_t e_ = nullptr;
};

class Stream {
public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept
  {
    if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; }
    return *this;
  }
  ~Stream() { reset(); }

  operator hipStream_t() const { return s_; }
  void reset()
  {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }
  // creates the stream if there is none (a failure names the caller's file and line)
  int create(unsigned flags, const char* file = __builtin_FILE(), int line = __builtin_LINE())
  {
    if (s_) return MIRT_OK;
    const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
    if (e == hipSuccess) return MIRT_OK;
    s_ = nullptr;
    return hip_fail(e, "hipStreamCreateWithFlags", file, line);
  }

private:
  hipStream_t s_ = nullptr;
};

} // namespace mirt

#define MIRT_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return mirt::hip_fail(e_, #call, __FILE__, __LINE__); } while (0)
// the same for a call that has reported its own failure and returns a MIRT_* status
#define MIRT_TRY(call) do { const int rc_ = (call); if (rc_ != MIRT_OK) return rc_; } while (0)

#endif
