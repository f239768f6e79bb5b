// dm_buf.h — the owners of what a handle allocates: device arrays, pinned
// host arrays, events, streams, timers, and the capacity of a group of arrays.
// Each frees in its destructor, cannot be copied, can be moved, and converts
// to the raw pointer / handle it owns, so the code that uses one reads as it
// would with the raw thing.  libdm allocates and frees memory, and creates and
// destroys events and streams, only here.
// Plain C++ over the HIP runtime API: no device code (tests/native/buf_main.cpp
// builds it with g++ against counting fakes of those calls).
#pragma once

#include <hip/hip_runtime_api.h>
#include <string.h>

#include <string>

#include "../../include/dm.h"

int dm_set_error(int code, const char* fmt, ...);  // dm_api.cpp

// Device array of T.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; n_ = o.n_;
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  // Exactly n elements (n <= 0: one): frees what it held first, contents are
  // not kept.  device >= 0: hipSetDevice(device) before the allocation.
  // DM_ERR_OOM / DM_ERR_HIP and an empty buffer on failure.
  int alloc(int64_t n, const char* what, int device = -1) {
    reset();
    if (n <= 0) n = 1;
    const size_t bytes = sizeof(T) * (size_t)n;
    hipError_t e = device >= 0 ? hipSetDevice(device) : hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) {
      p_ = nullptr;
      return dm_set_error(e == hipErrorOutOfMemory ? DM_ERR_OOM : DM_ERR_HIP, "hipMalloc(%s, %lld bytes): %s", what,
                          (long long)bytes, hipGetErrorString(e));
    }
    n_ = n;
    return DM_OK;
  }
  // alloc, then hipMemset to 0 (done on return); a failed fill is DM_ERR_HIP and an empty buffer too
  int alloc_zeroed(int64_t n, const char* what, int device = -1) {
    if (int rc = alloc(n, what, device)) return rc;
    const hipError_t e = hipMemset(p_, 0, sizeof(T) * (size_t)n_);
    if (e == hipSuccess) return DM_OK;
    reset();
    return dm_set_error(DM_ERR_HIP, "hipMemset(%s): %s (%d)", what, hipGetErrorString(e), (int)e);
  }
  // At least n elements: nothing when it already holds them, else alloc.
  int ensure(int64_t n, const char* what, int device = -1) { return n <= n_ ? DM_OK : alloc(n, what, device); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  int64_t size() const { return n_; }  // elements; 0 when empty
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  int64_t n_ = 0;
};

// Pinned host array of T (hipHostMalloc with `flags`).  With
// hipHostMallocMapped it also holds the array's device address.
template <class T>
class HostBuf {
 public:
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : p_(o.p_), d_(o.d_), n_(o.n_) { o.p_ = o.d_ = nullptr; o.n_ = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; d_ = o.d_; n_ = o.n_;
      o.p_ = o.d_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~HostBuf() { reset(); }

  // As DevBuf::alloc.  The contents are not initialised.
  int alloc(int64_t n, unsigned flags, const char* what) {
    reset();
    if (n <= 0) n = 1;
    hipError_t e = hipHostMalloc((void**)&p_, sizeof(T) * (size_t)n, flags);
    if (e != hipSuccess) {
      p_ = nullptr;
      return fail(e, "hipHostMalloc", what);
    }
    if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer((void**)&d_, p_, 0)) != hipSuccess) {
      reset();
      return fail(e, "hipHostGetDevicePointer", what);
    }
    n_ = n;
    return DM_OK;
  }
  int alloc_zeroed(int64_t n, unsigned flags, const char* what) {
    if (int rc = alloc(n, flags, what)) return rc;
    memset(p_, 0, sizeof(T) * (size_t)n_);
    return DM_OK;
  }
  int ensure(int64_t n, unsigned flags, const char* what) { return n <= n_ ? DM_OK : alloc(n, flags, what); }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = d_ = nullptr;
    n_ = 0;
  }
  int64_t size() const { return n_; }
  T* get() const { return p_; }
  T* dev() const { return d_; }  // the device address of a mapped array, else nullptr
  operator T*() const { return p_; }

 private:
  static int fail(hipError_t e, const char* call, const char* what) {
    return dm_set_error(e == hipErrorOutOfMemory ? DM_ERR_OOM : DM_ERR_HIP, "%s(%s): %s (%d)", call, what,
                        hipGetErrorString(e), (int)e);
  }
  T* p_ = nullptr;
  T* d_ = nullptr;
  int64_t n_ = 0;
};

// A DevBuf or HostBuf whose first K elements are a header: users point at
// the records behind it.
template <class Buf, int K>
struct Headed {
  Buf buf;
  // room for n records behind the header; the other arguments as Buf::alloc's
  template <class... A>
  int alloc(int64_t n, A... a) { return buf.alloc((n > 0 ? n : 1) + K, a...); }
  int64_t capacity() const { return buf.size() ? buf.size() - K : 0; }  // records
  auto base() const { return buf.get(); }
  auto records() const { return buf.get() ? buf.get() + K : nullptr; }
  auto records_dev() const { return buf.dev() ? buf.dev() + K : nullptr; }  // mapped HostBuf only
};

// The capacity kept beside a group of arrays that grow together.  Only a
// growth sets it, so it never names a size one of the arrays does not have.
class GroupCap {
 public:
  GroupCap& operator=(const GroupCap&) = delete;
  operator int64_t() const { return n_; }
  // alloc_all() allocates every array of the group for n.  The capacity is 0
  // while it runs and afterwards n only if it returned DM_OK.
  template <class F>
  int grow(int64_t n, F&& alloc_all) {
    n_ = 0;
    const int rc = alloc_all();
    if (rc == DM_OK) n_ = n;
    return rc;
  }

 private:
  int64_t n_ = 0;
};

// Owning event / stream, destroyed with the owner; DevEvent and DevStream
// below add the call that creates one.
template <class H, hipError_t (*Destroy)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(const HipHandle&) = delete;
  HipHandle& operator=(const HipHandle&) = delete;
  HipHandle(HipHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  HipHandle& operator=(HipHandle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~HipHandle() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  operator H() const { return h_; }

 protected:
  // after a creation call stored into h_: DM_OK, or a null handle and the error in dm_hip_check's words
  int created(hipError_t e, const char* call) {
    if (e == hipSuccess) return DM_OK;
    h_ = nullptr;
    return dm_set_error(e == hipErrorOutOfMemory ? DM_ERR_OOM : DM_ERR_HIP, "%s: %s (%d)", call,
                        hipGetErrorString(e), (int)e);
  }
  H h_ = nullptr;
};
// create() destroys the handle held, if any, first.
struct DevEvent : HipHandle<hipEvent_t, hipEventDestroy> {
  int create(unsigned flags) {
    reset();
    return created(hipEventCreateWithFlags(&h_, flags), "hipEventCreateWithFlags");
  }
};
struct DevStream : HipHandle<hipStream_t, hipStreamDestroy> {
  int create(unsigned flags, int priority) {
    reset();
    return created(hipStreamCreateWithPriority(&h_, flags, priority), "hipStreamCreateWithPriority");
  }
};

// One timed launch (dm_timer_begin / _end): the events around it on `stream`, dropped by dm_profile_read.
struct KernelTimer {
  std::string name;
  DevEvent start, stop;
  hipStream_t stream = nullptr;
};
