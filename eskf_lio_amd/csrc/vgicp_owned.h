// vgicp_owned.h — the owners behind the context's members: device memory, page-locked host memory, an event, the
// stream.  Each is move-only, frees what it holds when it goes, and converts to the raw pointer / handle, so reading
// call sites look as they did with raw members.  release() gives the handle up without freeing it.
// Plain C++17, no HIP include: the calls that allocate and free are a backend B (the HIP one is in vgicp_context.h, a
// counting one in tests/native/owned.cpp):
//   B::error, B::ok, B::event, B::stream              B::device_alloc(void**, bytes, fine_grained) / device_free(void*)
//   B::pinned_alloc(void**, bytes) / pinned_free(void*)   B::pinned_alias(void** device_address, void* host)
//   B::event_create(event*, timing) / event_destroy(event)   B::stream_create(stream*) / stream_destroy(stream)
#pragma once
#include <cstddef>

namespace vgicp::owned {

// alloc() FREES THE OLD BLOCK FIRST and only then allocates (a table of gigabytes is never held twice); when the
// allocation fails the owner is empty and the backend's error is returned.
template <class T, class B>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept { take(o); }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept { if (this != &o) { reset(); take(o); } return *this; }
  ~DeviceBuf() { reset(); }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t bytes() const { return bytes_; }
  void reset() { if (p_) B::device_free(p_); p_ = nullptr; bytes_ = 0; }
  T* release() { T* p = p_; p_ = nullptr; bytes_ = 0; return p; }
  typename B::error alloc(size_t bytes, bool fine_grained = false) {
    reset();
    void* p = nullptr;
    const typename B::error e = B::device_alloc(&p, bytes, fine_grained);
    if (e == B::ok) { p_ = static_cast<T*>(p); bytes_ = bytes; }
    return e;
  }

 private:
  void take(DeviceBuf& o) { bytes_ = o.bytes_; p_ = o.release(); }
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// Page-locked host memory.  alloc_mapped() also asks, once, for the address at which the device reads and writes the
// same bytes: dev() is that address until the next reset().
template <class T, class B>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept { take(o); }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); take(o); } return *this; }
  ~PinnedBuf() { reset(); }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  T* dev() const { return dev_; }
  size_t bytes() const { return bytes_; }
  void reset() { if (p_) B::pinned_free(p_); p_ = dev_ = nullptr; bytes_ = 0; }
  T* release() { T* p = p_; p_ = dev_ = nullptr; bytes_ = 0; return p; }
  typename B::error alloc(size_t bytes) {
    reset();
    void* p = nullptr;
    const typename B::error e = B::pinned_alloc(&p, bytes);
    if (e == B::ok) { p_ = static_cast<T*>(p); bytes_ = bytes; }
    return e;
  }
  typename B::error alloc_mapped(size_t bytes) {
    typename B::error e = alloc(bytes);
    if (e != B::ok) return e;
    void* d = nullptr;
    e = B::pinned_alias(&d, p_);
    if (e == B::ok) dev_ = static_cast<T*>(d);
    else reset();
    return e;
  }

 private:
  void take(PinnedBuf& o) { bytes_ = o.bytes_; dev_ = o.dev_; p_ = o.release(); }
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t bytes_ = 0;
};

template <class B>
class EventHandle {
 public:
  using H = typename B::event;
  EventHandle() = default;
  EventHandle(EventHandle&& o) noexcept : h_(o.release()) {}
  EventHandle& operator=(EventHandle&& o) noexcept { if (this != &o) { reset(); h_ = o.release(); } return *this; }
  ~EventHandle() { reset(); }
  operator H() const { return h_; }
  H get() const { return h_; }
  void reset() { if (h_) B::event_destroy(h_); h_ = H(); }
  H release() { H h = h_; h_ = H(); return h; }
  typename B::error create(bool timing = true) {
    reset();
    H h = H();
    const typename B::error e = B::event_create(&h, timing);
    if (e == B::ok) h_ = h;
    return e;
  }

 private:
  H h_ = H();
};

template <class B>
class StreamHandle {
 public:
  using H = typename B::stream;
  StreamHandle() = default;
  StreamHandle(StreamHandle&& o) noexcept : h_(o.release()) {}
  StreamHandle& operator=(StreamHandle&& o) noexcept { if (this != &o) { reset(); h_ = o.release(); } return *this; }
  ~StreamHandle() { reset(); }
  operator H() const { return h_; }
  H get() const { return h_; }
  void reset() { if (h_) B::stream_destroy(h_); h_ = H(); }
  H release() { H h = h_; h_ = H(); return h; }
  typename B::error create() {
    reset();
    H h = H();
    const typename B::error e = B::stream_create(&h);
    if (e == B::ok) h_ = h;
    return e;
  }

 private:
  H h_ = H();
};

}  // namespace vgicp::owned
