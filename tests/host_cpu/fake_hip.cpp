// fake_hip.cpp -- the 28 hip* functions tm_host.cpp calls, over host memory,
// for one device 0 (tests/test_image_cpu.py).
//
// Device memory and pinned memory are malloc'd, byte for byte the size asked
// for, so AddressSanitizer sees every read and write past a "device" table or
// a staging buffer.  Copies are memcpy, streams and events are synchronous:
// everything queued has happened when the call returns.  A mapped host
// buffer's device address is its host address.  The sizes of the live
// allocations are kept, so that the launchers (fake_launch.cpp) and the audit
// can bound what a table may hold.
//
// One knob: fake_hip_busy_events(k) makes the next k hipEventQuery calls answer
// hipErrorNotReady, which is how the driver reaches tm_commit's wait loop, its
// forced path and lane_busy without a GPU.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "fake_hip.h"

namespace {

std::mutex g_mu;
std::map<uintptr_t, size_t> g_allocs;   // start -> bytes
std::atomic<uint64_t> g_busy{0};
struct Handle { uint32_t magic; };      // a stream or an event
constexpr uint32_t STREAM_MAGIC = 0x53545245u, EVENT_MAGIC = 0x45564e54u;

hipError_t fake_alloc(void **p, size_t bytes) {
    if (!p) return hipErrorInvalidValue;
    void *q = malloc(bytes ? bytes : 1);
    if (!q) return hipErrorOutOfMemory;
    // a fresh device allocation holds anything: a reader that trusts it is wrong
    memset(q, 0xA5, bytes ? bytes : 1);
    std::lock_guard<std::mutex> g(g_mu);
    g_allocs[reinterpret_cast<uintptr_t>(q)] = bytes;
    *p = q;
    return hipSuccess;
}

hipError_t fake_free(void *p) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> g(g_mu);
        auto it = g_allocs.find(reinterpret_cast<uintptr_t>(p));
        if (it == g_allocs.end()) {
            fprintf(stderr, "fake_hip: free of %p, which is no live allocation\n", p);
            abort();
        }
        g_allocs.erase(it);
    }
    free(p);
    return hipSuccess;
}

template <class H>
hipError_t make_handle(H *out, uint32_t magic) {
    if (!out) return hipErrorInvalidValue;
    Handle *h = static_cast<Handle *>(malloc(sizeof(Handle)));
    if (!h) return hipErrorOutOfMemory;
    h->magic = magic;
    *out = reinterpret_cast<H>(h);
    return hipSuccess;
}

template <class H>
void check_handle(H h, uint32_t magic, const char *what) {
    if (!h) return;   // the null stream
    if (reinterpret_cast<Handle *>(h)->magic != magic) {
        fprintf(stderr, "fake_hip: %s given a handle of another kind\n", what);
        abort();
    }
}

template <class H>
hipError_t drop_handle(H h, uint32_t magic, const char *what) {
    if (!h) return hipErrorInvalidHandle;
    check_handle(h, magic, what);
    reinterpret_cast<Handle *>(h)->magic = 0;
    free(h);
    return hipSuccess;
}

}  // namespace

extern "C" {

void fake_hip_busy_events(uint64_t k) { g_busy.store(k); }

size_t fake_hip_alloc_bytes(const void *p) {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_allocs.find(reinterpret_cast<uintptr_t>(p));
    return it == g_allocs.end() ? 0 : it->second;
}

size_t fake_hip_room(const void *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_allocs.upper_bound(a);
    if (it == g_allocs.begin()) return 0;
    --it;
    return a < it->first + it->second ? it->first + it->second - a : 0;
}

size_t fake_hip_live_allocs(void) {
    std::lock_guard<std::mutex> g(g_mu);
    return g_allocs.size();
}

// ---- the device

hipError_t hipGetDevice(int *d) { if (d) *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorNotReady: return "not ready";
    case hipErrorNotSupported: return "not supported by the CPU device fake";
    case hipErrorOutOfMemory: return "out of memory";
    default: return "fake HIP error";
    }
}
hipError_t hipDeviceGetAttribute(int *pi, hipDeviceAttribute_t, int dev) {
    if (!pi || dev != 0) return hipErrorInvalidValue;
    *pi = 1;
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p) {
    if (!a || !fake_hip_room(p)) return hipErrorInvalidValue;
    memset(a, 0, sizeof *a);
    a->type = hipMemoryTypeDevice;
    a->device = 0;
    a->devicePointer = const_cast<void *>(p);
    a->hostPointer = const_cast<void *>(p);
    return hipSuccess;
}

// ---- memory

hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipFree(void *p) { return fake_free(p); }
hipError_t hipHostFree(void *p) { return fake_free(p); }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned int) {
    if (!d || !fake_hip_room(h)) return hipErrorInvalidValue;
    *d = h;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
    if (n) memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind k, hipStream_t s) {
    check_handle(s, STREAM_MAGIC, "hipMemcpyAsync");
    return hipMemcpy(dst, src, n, k);
}
hipError_t hipMemset(void *dst, int v, size_t n) {
    if (n) memset(dst, v, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) {
    check_handle(s, STREAM_MAGIC, "hipMemsetAsync");
    return hipMemset(dst, v, n);
}

// ---- streams and events

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return make_handle(s, STREAM_MAGIC); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop_handle(s, STREAM_MAGIC, "hipStreamDestroy"); }
hipError_t hipStreamSynchronize(hipStream_t s) { check_handle(s, STREAM_MAGIC, "hipStreamSynchronize"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
    check_handle(s, STREAM_MAGIC, "hipStreamWaitEvent");
    check_handle(e, EVENT_MAGIC, "hipStreamWaitEvent");
    return e ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventCreate(hipEvent_t *e) { return make_handle(e, EVENT_MAGIC); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make_handle(e, EVENT_MAGIC); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop_handle(e, EVENT_MAGIC, "hipEventDestroy"); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    check_handle(e, EVENT_MAGIC, "hipEventRecord");
    check_handle(s, STREAM_MAGIC, "hipEventRecord");
    return e ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    check_handle(e, EVENT_MAGIC, "hipEventSynchronize");
    return e ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
    check_handle(a, EVENT_MAGIC, "hipEventElapsedTime");
    check_handle(b, EVENT_MAGIC, "hipEventElapsedTime");
    if (ms) *ms = 0.0f;
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e) {
    check_handle(e, EVENT_MAGIC, "hipEventQuery");
    if (!e) return hipErrorInvalidHandle;
    uint64_t k = g_busy.load();
    while (k && !g_busy.compare_exchange_weak(k, k - 1)) {}
    return k ? hipErrorNotReady : hipSuccess;
}

}  // extern "C"
