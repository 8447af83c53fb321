// A stand-in for <hip/hip_runtime.h> that lets a plain host compiler build the host-side bookkeeping of csrc/common.h (tests/sim/host_checks.cpp):
// the handful of runtime calls common.h and the exchange headers make, those of common.h each appending its name and arguments to hip_stub::log.  Device memory is host memory, an event is
// a small heap block, a stream is whatever pointer the test makes up: AddressSanitizer then sees a leak, a double free or a use after release.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct hip_stub_event { int recorded; }* hipEvent_t;
typedef struct hip_stub_stream* hipStream_t;
constexpr unsigned hipEventDisableTiming = 2, hipHostMallocDefault = 0;

namespace hip_stub {
inline std::vector<std::string>& log() { static std::vector<std::string> l; return l; }
inline size_t& malloc_limit() { static size_t v = (size_t)1 << 30; return v; }      // a larger hipMalloc fails
inline void note(const char* what, const void* a = nullptr, const void* b = nullptr) {
    char s[96]; snprintf(s, sizeof(s), "%s %p %p", what, a, b); log().push_back(s);
}
}  // namespace hip_stub

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "stub error"; }
inline hipError_t hipMalloc(void** p, size_t n) {
    hip_stub::note("hipMalloc");
    if (n > hip_stub::malloc_limit()) return hipErrorOutOfMemory;
    *p = malloc(n); return hipSuccess;
}
inline hipError_t hipFree(void* p) { hip_stub::note("hipFree"); free(p); return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n); return hipSuccess; }
inline hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { hip_stub::note("hipEventCreate"); *e = new hip_stub_event{0}; return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) { hip_stub::note("hipEventDestroy", e); delete e; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { hip_stub::note("hipEventRecord", e, s); e->recorded = 1; return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t e) { hip_stub::note("hipEventSynchronize", e); (void)e->recorded; return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { hip_stub::note("hipStreamWaitEvent", s, e); (void)e->recorded; return hipSuccess; }
// what the rank threads of the exchange check call (csrc/group_exchange.h, csrc/rccl_standin.h): a copy is done when the call returns, so there is nothing to
// wait for; neither writes the log, which belongs to the main thread
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) { memcpy(dst, src, n); return hipSuccess; }
