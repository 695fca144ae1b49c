// ggrs_amd/csrc/host_batch.hpp — what the host side of every engine needs, once
// (engine.hip, p2p_engine.hip, spectator_engine.hip): error plumbing, the device
// scope, the owner of a batch's device resources, read-backs, the profiling
// event pool and the size of a launch.  Plain host C++ over the HIP runtime: no
// kernels.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ggrs_amd.h"
#include "session_record.hpp"

namespace rb {

// ---- errors.  A batch keeps its last message in `last_err`; a call without a batch (create, the
// rb_debug_* functions) leaves it in the engine's own thread-local, which rb_*_last_error(nullptr)
// reads: one per translation unit.
namespace {
thread_local std::string g_create_err;
inline rb_status fail(std::nullptr_t, rb_status st, const std::string& msg) {
  g_create_err = msg;
  return st;
}
template <class B>
rb_status fail(B* b, rb_status st, const std::string& msg) {
  if (!b) return fail(nullptr, st, msg);
  b->last_err = msg;
  return st;
}
}  // namespace
#define RB_TRY(b, expr)                                                                                          \
  do {                                                                                                           \
    hipError_t _e = (expr);                                                                                      \
    if (_e != hipSuccess) return rb::fail((b), RB_DEVICE_ERROR, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// hipSetDevice for the batch's calls, the caller's current device restored on every return
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// ---- The owner of device resources: everything a batch (or one call, as a local) allocates is
// made through it and freed by release_all(), so no engine lists its pointers a second time.
struct DeviceOwner {
  std::vector<void*> dev, host;
  std::vector<hipEvent_t> events;

  template <class T>
  hipError_t alloc(T*& p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) dev.push_back(q);
    p = static_cast<T*>(q);
    return e;
  }
  template <class T>
  hipError_t alloc_host(T*& p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, flags);
    if (e == hipSuccess) host.push_back(q);
    p = static_cast<T*>(q);
    return e;
  }
  hipError_t event(hipEvent_t& ev, unsigned flags = hipEventDefault) {
    const hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e == hipSuccess) events.push_back(ev);
    return e;
  }
  // a device buffer that regrows: freed now, p = nullptr
  template <class T>
  hipError_t release(T*& p) {
    const auto it = std::find(dev.begin(), dev.end(), static_cast<void*>(p));
    if (it == dev.end()) return hipSuccess;
    dev.erase(it);
    return hipFree(std::exchange(p, nullptr));
  }
  void release_all() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (void* q : host) (void)hipHostFree(q);
    for (void* q : dev) (void)hipFree(q);
    events.clear();
    host.clear();
    dev.clear();
  }
  DeviceOwner() = default;
  DeviceOwner(const DeviceOwner&) = delete;
  DeviceOwner& operator=(const DeviceOwner&) = delete;
  ~DeviceOwner() { release_all(); }
};

// ---- read-backs
// `rows` rows of Spad elements, after everything on the batch's stream, on the batch's device
template <class B, class T>
rb_status read_rows(B* b, const T* dev, size_t rows, std::vector<T>& host) {
  DeviceScope dev_scope(b->device);
  host.resize(rows * static_cast<size_t>(b->Spad));
  RB_TRY(b, hipMemcpyAsync(host.data(), dev, host.size() * sizeof(T), hipMemcpyDeviceToHost, b->stream));
  RB_TRY(b, hipStreamSynchronize(b->stream));
  return RB_OK;
}
// session s's words [L][NW] from a block of state planes of Spad sessions (word_index)
inline void session_words(const uint32_t* planes, int NW, int L, size_t Spad, int s, uint32_t* w) {
  for (int l = 0; l < L; ++l)
    for (int k = 0; k < NW; ++k) w[l * NW + k] = planes[word_index(NW, Spad * L, static_cast<size_t>(s) * L + l, k)];
}

// ---- Kernel timing (rb_profile_enable / rb_p2p_profile_enable): the events a launch records
// itself through hipExtLaunchKernel — the kernel's own start and end, with no marker packets of
// their own around it on the stream; both null when the batch is not profiling.
struct LaunchEv {
  hipEvent_t start = nullptr, stop = nullptr;
};
// The pool of event pairs, reused after take().
struct EventPool {
  DeviceOwner& res;
  std::vector<LaunchEv> ev;
  std::vector<int32_t> ticks;  // ticks covered by each timed launch
  size_t used = 0;
  static constexpr size_t kPairs = 256;  // made by enable()

  hipError_t grow() {
    LaunchEv p;
    hipError_t e = res.event(p.start);
    if (e == hipSuccess) e = res.event(p.stop);
    if (e == hipSuccess) {
      ev.push_back(p);
      ticks.push_back(0);
    }
    return e;
  }
  // The pool is created here, outside any timed region (a first hipEventCreate inside one costs
  // tens of microseconds of host time), and every new event recorded once: the runtime sets an
  // event's completion signal up at its first record, which would otherwise land in the first timed call.
  hipError_t enable(hipStream_t st) {
    const size_t fresh = ev.size();
    hipError_t e = hipSuccess;
    while (e == hipSuccess && ev.size() < kPairs) e = grow();
    for (size_t i = fresh; i < ev.size() && e == hipSuccess; ++i) {
      e = hipEventRecord(ev[i].start, st);
      if (e == hipSuccess) e = hipEventRecord(ev[i].stop, st);
    }
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  }
  // the next pair, creating one if the pool is used up; consumed only by commit()
  hipError_t next(LaunchEv& out) {
    if (used == ev.size())
      if (const hipError_t e = grow(); e != hipSuccess) return e;
    out = ev[used];
    return hipSuccess;
  }
  // the launch went out, covering n ticks
  void commit(int32_t n = 1) { ticks[used++] = n; }
  // the time, ticks and number of the launches since the last take
  hipError_t take(double* total_ms, int32_t* n_ticks, int32_t* launches) {
    double t = 0;
    int32_t tk = 0;
    if (used > 0)
      if (const hipError_t e = hipEventSynchronize(ev[used - 1].stop); e != hipSuccess) return e;
    for (size_t i = 0; i < used; ++i) {
      float ms = 0;
      if (const hipError_t e = hipEventElapsedTime(&ms, ev[i].start, ev[i].stop); e != hipSuccess) return e;
      t += ms;
      tk += ticks[i];
    }
    if (total_ms) *total_ms = t;
    if (n_ticks) *n_ticks = tk;
    if (launches) *launches = static_cast<int32_t>(used);
    used = 0;
    return hipSuccess;
  }
};

// ---- The size of a launch over `lanes` lanes in workgroups of `block`: its grid, and the waves it
// runs, the lanes past `lanes` included (they store a launch-clock start stamp before they return).
inline size_t launch_grid(size_t lanes, int block) { return (lanes + block - 1) / block; }
inline size_t launch_waves(size_t lanes, int block) { return launch_grid(lanes, block) * block / 64; }

}  // namespace rb
