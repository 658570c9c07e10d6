// Host stand-in for the HIP memory, stream and event calls smarts_amd/csrc/smx_handle.h makes, on top of the plain shim
// <hip/hip_runtime.h>.  Test infrastructure only (tests/native/host_handle.cpp): device memory is malloc'd and recorded,
// every use of it is checked against the record, streams and events are counted, and one counter makes the n-th call
// return an error.  A release (hipFree, a destroy) that is told to fail reports the error and releases all the same.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
struct ShimStream { int priority; };
struct ShimEvent { unsigned flags; };
typedef ShimStream* hipStream_t;
typedef ShimEvent* hipEvent_t;

struct ShimHip {
  std::map<const char*, size_t> live;  // device allocations: base -> bytes
  std::set<hipStream_t> streams;
  std::set<hipEvent_t> events;
  long calls = 0;        // HIP calls so far
  long fail_at = 0;      // the call (counted from 1) that returns an error; 0: none
  bool fired = false, fired_in_release = false;  // it did; ... and that call was a release, whose result the library ignores
  long mallocs = 0, memcpys = 0, memsets = 0, frees = 0, stream_creates = 0, event_creates = 0;
  long misuse = 0;       // a free of a pointer that is not live, a copy or fill outside one live allocation, ...
  void reset() {
    const char* keep = trace;
    *this = ShimHip();
    trace = keep;
  }
  const char* trace = nullptr;  // not null: every call is printed with its number, after this tag
  bool fails(const char* call, bool release = false) {
    ++calls;
    if (trace) std::printf("%4ld  %-32s %s\n", calls, call, trace);
    if (calls != fail_at) return false;
    fired = true, fired_in_release = release;
    return true;
  }
  // [p, p + n) lies inside one live allocation
  bool inside(const void* p, size_t n) const {
    auto it = live.upper_bound((const char*)p);
    if (it == live.begin()) return false;
    --it;
    return (const char*)p + n <= it->first + it->second;
  }
  void bad(const char* what) {
    ++misuse;
    std::printf("HIP misuse: %s\n", what);
  }
};
static ShimHip shim_hip;

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }
inline hipError_t hipSetDevice(int) { return shim_hip.fails("hipSetDevice") ? hipErrorInvalidValue : hipSuccess; }
inline hipError_t hipDeviceSynchronize() { return shim_hip.fails("hipDeviceSynchronize") ? hipErrorInvalidValue : hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t bytes) {
  ++shim_hip.mallocs;
  if (shim_hip.fails("hipMalloc")) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);  // (uninitialised on purpose: a read before the fill is the sanitizer's to see)
  shim_hip.live[(const char*)*p] = bytes;
  return hipSuccess;
}
template <class T>
inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc((void**)p, bytes); }
inline hipError_t hipFree(void* p) {
  ++shim_hip.frees;
  const bool failed = shim_hip.fails("hipFree", true);
  auto it = shim_hip.live.find((const char*)p);
  if (it == shim_hip.live.end()) {
    shim_hip.bad("hipFree of a pointer that is not a live allocation");
    return hipErrorInvalidValue;
  }
  shim_hip.live.erase(it);
  std::free(p);
  return failed ? hipErrorInvalidValue : hipSuccess;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  ++shim_hip.memcpys;
  if (shim_hip.fails("hipMemcpy")) return hipErrorInvalidValue;
  if (!shim_hip.inside(kind == hipMemcpyHostToDevice ? dst : src, bytes)) {
    shim_hip.bad("hipMemcpy outside one live allocation");
    return hipErrorInvalidValue;
  }
  if (bytes) std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipMemset(void* dst, int value, size_t bytes) {
  ++shim_hip.memsets;
  if (shim_hip.fails("hipMemset")) return hipErrorInvalidValue;
  if (!shim_hip.inside(dst, bytes)) {
    shim_hip.bad("hipMemset outside one live allocation");
    return hipErrorInvalidValue;
  }
  std::memset(dst, value, bytes);
  return hipSuccess;
}
inline hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) {
  if (shim_hip.fails("hipDeviceGetStreamPriorityRange")) return hipErrorInvalidValue;
  *least = 0, *greatest = -1;
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int priority) {
  ++shim_hip.stream_creates;
  if (shim_hip.fails("hipStreamCreateWithPriority")) return hipErrorOutOfMemory;
  *s = new ShimStream{priority};
  shim_hip.streams.insert(*s);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) {
  const bool failed = shim_hip.fails("hipStreamSynchronize", true);
  if (!shim_hip.streams.count(s)) shim_hip.bad("hipStreamSynchronize of a stream that is not live");
  return failed ? hipErrorInvalidValue : hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  const bool failed = shim_hip.fails("hipStreamDestroy", true);
  if (!shim_hip.streams.erase(s)) {
    shim_hip.bad("hipStreamDestroy of a stream that is not live");
    return hipErrorInvalidValue;
  }
  delete s;
  return failed ? hipErrorInvalidValue : hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  ++shim_hip.event_creates;
  if (shim_hip.fails("hipEventCreateWithFlags")) return hipErrorOutOfMemory;
  *e = new ShimEvent{flags};
  shim_hip.events.insert(*e);
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) {
  const bool failed = shim_hip.fails("hipEventDestroy", true);
  if (!shim_hip.events.erase(e)) {
    shim_hip.bad("hipEventDestroy of an event that is not live");
    return hipErrorInvalidValue;
  }
  delete e;
  return failed ? hipErrorInvalidValue : hipSuccess;
}
