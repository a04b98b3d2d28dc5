// ShimSupport.hpp — what the three drop-in classes share and none of them owns: the error check of a C-ABI call, the
// developer's time slots (shim::Trace), the pool that keeps the storage of clouds which died inside the classes, and the
// process's default context.
#ifndef ESKF_LIO_SHIM_SUPPORT_HPP_
#define ESKF_LIO_SHIM_SUPPORT_HPP_

#include <chrono>
#if defined(__linux__)
#include <sys/mman.h>
#endif
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../vgicp_hip.h"
#include "ShimTypes.hpp"

namespace ESKF_LIO
{
namespace shim
{
inline void check(vgicp_ctx * ctx, int rc, const char * what)
{
  if (rc != VGICP_OK) {
    throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " +
            vgicp_last_error(ctx));
  }
}

// Developer aid: where a frame's host time goes inside the classes (tools/probe_eager.py through libvgicp_host.so).
// Off unless shim::trace().on is set; a disabled scope costs one predictable branch.
struct Trace
{
  enum Slot {ProcessEnqueue, ProcessWait, ProcessResize, ProcessDownload, ProcessStamp, AlignVerify, AlignCall,
    UpdateVerify, UpdateRest, UpdateInsert, UpdateShadow, Slots};   // (the last two are parts of UpdateRest)
  bool on = false;
  double seconds[Slots] = {0};
  uint64_t calls[Slots] = {0};
};
inline Trace & trace()
{
  static Trace t;
  return t;
}
struct TraceScope
{
  int slot;
  std::chrono::steady_clock::time_point t0;
  explicit TraceScope(int s)
  : slot(trace().on ? s : -1)
  {
    if (slot >= 0) {t0 = std::chrono::steady_clock::now();}
  }
  ~TraceScope()
  {
    if (slot >= 0) {
      trace().seconds[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      ++trace().calls[slot];
    }
  }
};

// Storage of clouds that died inside these classes (a cloud moved into updateLocalMap, src/Odometry.cpp:86, ends in the
// map's hands) is kept for the clouds to come: process() needs 72 bytes per kept point for the covariances of every
// frame, and a FRESH allocation of that size is what the C library maps anew and the kernel faults in page by page
// (measured: 0.44 ms of a 1.1 ms frame were `covariances_.resize()`); storage that was used before costs nothing.
// At most four vectors of each kind are kept; everything else is freed as before.
struct StoragePool
{
  std::mutex mutex;
  std::vector<std::vector<Vector3d>> points;
  std::vector<std::vector<Matrix3d>> covariances;
};
inline StoragePool & storagePool()
{
  static StoragePool pool;
  return pool;
}
// the cloud is about to be destroyed by its last owner: keep its buffers (four of a kind at most: a fifth replaces the
// smallest one kept when it is larger)
template<typename T>
inline void keepStorage(std::vector<T> & v, std::vector<std::vector<T>> & kept)
{
  if (!v.capacity()) {return;}
  v.clear();
  if (kept.size() < 4) {
    kept.emplace_back(std::move(v));
    return;
  }
  size_t smallest = 0;
  for (size_t i = 1; i < kept.size(); ++i) {
    if (kept[i].capacity() < kept[smallest].capacity()) {smallest = i;}
  }
  if (kept[smallest].capacity() < v.capacity()) {kept[smallest].swap(v);}
}
inline void recycleStorage(PointCloud & cloud)
{
  StoragePool & pool = storagePool();
  std::lock_guard<std::mutex> lk(pool.mutex);
  keepStorage(cloud.covariances_, pool.covariances);
  keepStorage(cloud.points_, pool.points);
}
// make room for n elements in v, out of the pool when v has none of its own (v's contents are not kept): the smallest
// kept buffer that is large enough
template<typename T>
inline void adoptStorage(std::vector<T> & v, std::vector<std::vector<T>> & kept, size_t n)
{
  if (v.capacity() >= n) {return;}
  {
    StoragePool & pool = storagePool();
    std::lock_guard<std::mutex> lk(pool.mutex);
    size_t best = kept.size();
    for (size_t i = 0; i < kept.size(); ++i) {
      if (kept[i].capacity() >= n && (best == kept.size() || kept[i].capacity() < kept[best].capacity())) {best = i;}
    }
    if (best != kept.size()) {
      v.swap(kept[best]);
      v.clear();
      kept.erase(kept.begin() + static_cast<std::ptrdiff_t>(best));
      return;
    }
  }
  // nothing to reuse (the clouds of the last frames are still with the shadow grid's worker, or were smaller): a fresh
  // allocation with room for the next frames' sizes (a scan's kept count moves by a few per cent from frame to frame:
  // an exact fit would send every other frame here), its pages brought in by ONE call instead of one fault each
  // (Linux >= 5.14; ignored where it is not known)
  v.reserve(n + n / 4 + 64);
#if defined(__linux__)
  const uintptr_t lo = (reinterpret_cast<uintptr_t>(v.data()) + 4095u) & ~uintptr_t(4095u);
  const uintptr_t hi = reinterpret_cast<uintptr_t>(v.data() + v.capacity()) & ~uintptr_t(4095u);
  if (hi > lo + (256u << 10)) {(void)madvise(reinterpret_cast<void *>(lo), hi - lo, 23 /* MADV_POPULATE_WRITE */);}
#endif
}

// One context per process, created on first use: device $VGICP_DEVICE (default 0), or — VGICP_DEVICES=0,1,2,3 — ONE
// context that drives several devices from this thread (vgicp_create_multi: replicated map, point-sharded align;
// an ordinal may repeat, "0,0", to split one device).  The reference's single caller thread (src/main.cpp:68-70)
// reaches the multi-GPU path through the unchanged ICP::align that way.
inline vgicp_ctx * defaultContext()
{
  static vgicp_ctx * ctx = [] {
      vgicp_ctx * c = nullptr;
      int rc;
      if (const char * list = std::getenv("VGICP_DEVICES")) {
        std::vector<int> ids;
        for (const char * p = list; *p; ) {
          char * end = nullptr;
          const long v = std::strtol(p, &end, 10);
          if (end == p) {break;}
          ids.push_back(static_cast<int>(v));
          p = (*end == ',') ? end + 1 : end;
        }
        if (ids.empty()) {throw std::runtime_error("VGICP_DEVICES names no device");}
        rc = vgicp_create_multi(ids.data(), static_cast<int>(ids.size()), &c);
      } else {
        int dev = 0;
        if (const char * env = std::getenv("VGICP_DEVICE")) {dev = std::atoi(env);}
        rc = vgicp_create(dev, &c);
      }
      if (rc != VGICP_OK) {
        throw std::runtime_error(std::string("vgicp_create failed: ") + vgicp_last_error(nullptr));
      }
      return c;
    }();
  return ctx;
}
}  // namespace shim
}  // namespace ESKF_LIO

#endif  // ESKF_LIO_SHIM_SUPPORT_HPP_
