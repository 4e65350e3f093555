// host_runtime.hip -- the host-side state every translation unit leans on: the thread-local error text, the scratch pool, the
// stream pool, the lanes of the host-pointer entry points (host_lane.h), the caller-buffer registry's one instance
// (pin_registry.h) and the properties of a field / curve id.  No kernel and no extern "C" here: capi.hip holds the entry points.
#include <atomic>
#include <cstdarg>
#include <mutex>
#include <vector>

#include "common.h"
#include "ec.cuh"
#include "host_lane.h"
#include "pin_registry.h"

namespace plk {

std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}

// ---- scratch pool ----
struct ScratchEntry {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    bool in_call = false;   // between acquire and release on some host thread
    bool used = false;      // ev has been recorded at least once
};
static std::mutex g_scratch_mu;
static std::vector<ScratchEntry> g_scratch;

void* scratch_acquire(size_t bytes, hipStream_t stream) {
    if (bytes == 0) bytes = 16;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    ScratchEntry* best = nullptr;
    for (auto& e : g_scratch) {
        if (e.in_call || e.device != dev || e.bytes < bytes) continue;
        // a small request must not take (and keep) a buffer sized for a whole transform: at most 4x the request above 1 MiB
        if (e.bytes > ((size_t)1 << 20) && e.bytes / 4 > bytes) continue;
        const bool ordered = !e.used || e.stream == stream || hipEventQuery(e.ev) == hipSuccess;
        if (!ordered) continue;
        if (!best || e.bytes < best->bytes) best = &e;
    }
    if (best) {
        best->in_call = true;
        return best->p;
    }
    ScratchEntry e;
    e.bytes = bytes;
    e.device = dev;
    hipError_t err = hipMalloc(&e.p, bytes);
    if (err != hipSuccess) {
        set_error(err == hipErrorOutOfMemory ? PLK_ERR_OOM : PLK_ERR_HIP, "hipMalloc(%zu) for scratch failed: %s", bytes, hipGetErrorString(err));
        return nullptr;
    }
    if (hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(e.p);
        set_error(PLK_ERR_HIP, "hipEventCreate failed");
        return nullptr;
    }
    e.in_call = true;
    g_scratch.push_back(e);
    return e.p;
}

void scratch_release(void* p, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (auto& e : g_scratch)
        if (e.p == p) {
            (void)hipEventRecord(e.ev, stream);
            e.stream = stream;
            e.used = true;
            e.in_call = false;
            return;
        }
}

// every device of the group is quiet
static void group_quiesce() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < group_size(); ++d) {
        if (d && group_phys(d) == group_phys(d - 1)) continue;
        (void)hipSetDevice(group_phys(d));
        (void)hipDeviceSynchronize();
    }
    if (cur >= 0) (void)hipSetDevice(cur);
}

void scratch_clear() {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    group_quiesce();  // before the buffers go
    (void)hipDeviceSynchronize();
    for (auto& e : g_scratch) {
        if (e.in_call) continue;
        (void)hipFree(e.p);
        (void)hipEventDestroy(e.ev);
        e.p = nullptr;
    }
    std::vector<ScratchEntry> keep;
    for (auto& e : g_scratch)
        if (e.p) keep.push_back(e);
    g_scratch.swap(keep);
}

// ---- stream pool ----
struct PooledStream {
    hipStream_t s;
    int device;
    bool free;
};
static std::mutex g_spool_mu;
static std::vector<PooledStream> g_spool;

hipStream_t stream_pool_acquire() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_spool_mu);
    for (auto& e : g_spool)
        if (e.free && e.device == dev) {
            e.free = false;
            return e.s;
        }
    hipStream_t s = nullptr;
    hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (err != hipSuccess) {
        set_error(PLK_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(err));
        return nullptr;
    }
    g_spool.push_back({s, dev, false});
    return s;
}
void stream_pool_release(hipStream_t s) {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_spool_mu);
    for (auto& e : g_spool)
        if (e.s == s) e.free = true;
}

// ---- host-pointer entry points: one lane per (calling thread, logical device) - host_lane.h ----
static thread_local HostLane t_lanes[PLK_MAX_DEVICES];

int lane_get(HostLane*& out) {
    PLK_TRY(ensure_device());
    int dev = 0;
    PLK_HIP_TRY(hipGetDevice(&dev));
    HostLane& l = t_lanes[thread_logical_device()];
    if (l.stream && l.device != dev) l.drop_streams();  // the group was re-initialised over other devices
    if (!l.stream) {
        l.stream = stream_pool_acquire();
        if (!l.stream) return PLK_ERR_HIP;
        l.device = dev;
    }
    if (l.pin_used) (void)hipStreamSynchronize(l.stream);  // a call that failed half way may have left copies in flight
    l.pin_used = 0;
    out = &l;
    return PLK_OK;
}

// The caller-buffer registry (pin_registry.h has the rules and the code; host_lane.h the callers): here only its three outside
// effects - hipHostRegister as portable (every device of the group may copy from the range), hipHostUnregister, and "every device
// of the group quiet" - and the library's one instance, with the two-second wait limit.
struct HipPinPolicy {
    bool register_range(const uint8_t* lo, size_t bytes) {
        if (hipHostRegister(const_cast<uint8_t*>(lo), bytes, hipHostRegisterPortable) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    void unregister_range(const uint8_t* lo) { (void)hipHostUnregister(const_cast<uint8_t*>(lo)); }
    void quiesce() { group_quiesce(); }
};
static PinRegistry<HipPinPolicy>& pin_registry() {
    static PinRegistry<HipPinPolicy>* r = new PinRegistry<HipPinPolicy>(2000);  // never destroyed: thread-local lanes may outlive statics
    return *r;
}
bool pin_registry_acquire(const void* ptr, size_t bytes) { return pin_registry().acquire(ptr, bytes); }
void pin_registry_release(const void* ptr) { pin_registry().release(ptr); }

static std::atomic<unsigned long long> g_lane_copies[LANE_ROUTES];
void lane_count(int route) { g_lane_copies[route].fetch_add(1, std::memory_order_relaxed); }

int host_stats(unsigned long long* out, unsigned n) {
    const PinStats ps = pin_registry().stats();
    std::vector<unsigned long long> v(ps.branch, ps.branch + PIN_BRANCHES);
    v.push_back(ps.waits);
    v.push_back(ps.rechecks);
    for (int r = 0; r < LANE_ROUTES; ++r) v.push_back(g_lane_copies[r].load(std::memory_order_relaxed));
    for (unsigned i = 0; out && i < n && i < v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}

static int or_invalid_id(int rc) { return rc == PLK_NO_MATCH ? PLK_ERR_INVALID_ARG : rc; }
int field_limbs(int field) {
    return or_invalid_id(with_field(field, [](auto t) { return tag_t<decltype(t)>::NL / 2; }));
}
int curve_limbs(int curve) {
    return or_invalid_id(with_curve(curve, [](auto t) { return tag_t<decltype(t)>::FP::NL / 2; }));
}
int curve_scalar_field(int curve) {
    return or_invalid_id(with_curve(curve, [](auto t) { return tag_t<decltype(t)>::SP::FIELD_ID; }));
}
int curve_scalar_bits(int curve) {
    return or_invalid_id(with_curve(curve, [](auto t) { return tag_t<decltype(t)>::SP::BITS; }));
}

}  // namespace plk
