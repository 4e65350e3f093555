// pin_registry.h -- the caller-buffer registry of the host-pointer entry points (host_lane.h), as plain C++: no HIP type in it, so
// that tests/pin_registry_host.cpp runs the same code on the host against a model of the runtime.
//
// Registered caller ranges: NON-OVERLAPPING intervals, each with the threads that hold it.  A request inside a registered interval
// shares it; a request that extends or partly overlaps one never leaves a half-registered range behind (HIP resolves a pointer to the
// registered object it starts in - an asynchronous copy longer than that object is rejected, and the first holder's release would
// unregister pages under the second caller's DMA):
//  * held by OTHER threads: wait until they have released it, then register the union - for at most `wait_ms` in all (the library:
//    two seconds): holders that in turn wait for this thread (or for a lock its dispatcher holds) would otherwise never release; past
//    that the request fails and the caller's copies go without a registration;
//  * held by the calling thread alone (two overlapping buffers of one batched call, an in-place padded transform): every device
//    of the group is synchronised - the thread's own copies over the old interval are complete - and the interval is re-registered
//    as the union, the thread's holds carried over.
//
// The three outside effects are the Policy the registry is instantiated with:
//     bool register_range(const uint8_t* lo, size_t bytes);   // may fail
//     void unregister_range(const uint8_t* lo);                // the start address of an earlier successful register_range
//     void quiesce();                                          // "every device quiet"; called WITHOUT the registry's lock held
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

namespace plk {

// the route a call took: acquire() and release() report it, and the registry counts each
enum PinBranch : int {
    PIN_NONE = 0,
    PIN_FRESH,            // nothing in the way: registered, one hold
    PIN_REGISTER_FAILED,  // nothing in the way, the registration was refused: false
    PIN_SHARED,           // inside one registered interval: one more hold on it
    PIN_UNION,            // the calling thread's own intervals replaced by their union with the request, its holds carried over
    PIN_UNION_FAILED,     // ... the union's registration was refused: nothing of it is registered, the thread's holds are gone, false
    PIN_GAVE_UP,          // other threads' holds outlasted the wait limit: false, nothing changed
    PIN_RELEASED_LAST,    // release: the last hold, the interval was unregistered
    PIN_RELEASED_KEPT,    // release: other holds remain
    PIN_RELEASE_NOT_HELD, // release: the calling thread holds nothing on that interval, nothing changed
    PIN_RELEASE_UNKNOWN,  // release: the address lies in no interval, nothing changed
    PIN_BRANCHES
};
inline const char* pin_branch_name(int b) {
    static const char* const names[PIN_BRANCHES] = {"none",     "fresh",         "register-failed", "shared",           "union",          "union-failed",
                                                    "gave-up",  "released-last", "released-kept",   "release-not-held", "release-unknown"};
    return b >= 0 && b < PIN_BRANCHES ? names[b] : "?";
}
struct PinTrace {
    int branch = PIN_NONE;
    unsigned waits = 0;     // times the request slept for other threads' holds
    unsigned rechecks = 0;  // times the union path found the map changed under its synchronisation and looked again
};
struct PinStats {
    unsigned long long branch[PIN_BRANCHES] = {};
    unsigned long long waits = 0, rechecks = 0;
    unsigned waiting = 0;  // a gauge: requests asleep for other threads' holds right now
};
struct PinInterval {
    const uint8_t* lo;
    size_t bytes;
    std::map<std::thread::id, unsigned> holders;
};

template <class Policy>
class PinRegistry {
    struct Entry {
        size_t bytes;
        std::map<std::thread::id, unsigned> holders;
        unsigned refs() const {
            unsigned r = 0;
            for (const auto& h : holders) r += h.second;
            return r;
        }
    };
    using Map = std::map<const uint8_t*, Entry>;  // by start address; intervals never overlap
    using Hits = std::vector<typename Map::iterator>;

    Policy policy_;
    const long wait_ms_;
    mutable std::mutex mu_;
    std::condition_variable cv_;
    Map pins_;
    PinStats stats_;

    // the registered intervals that touch [lo, hi)
    Hits touching(const uint8_t* lo, const uint8_t* hi) {
        Hits hit;
        auto it = pins_.upper_bound(lo);
        if (it != pins_.begin()) --it;
        for (; it != pins_.end() && it->first < hi; ++it)
            if (it->first + it->second.bytes > lo) hit.push_back(it);
        return hit;
    }
    static bool held_by_others(const Hits& hit, std::thread::id me) {
        for (const auto& h : hit)
            for (const auto& who : h->second.holders)
                if (who.first != me && who.second) return true;
        return false;
    }
    bool done(PinTrace& t, PinTrace* out, int branch, bool rc) {
        t.branch = branch;
        ++stats_.branch[branch];
        stats_.waits += t.waits;
        stats_.rechecks += t.rechecks;
        if (out) *out = t;
        return rc;
    }

  public:
    explicit PinRegistry(long wait_ms = 2000, Policy policy = Policy()) : policy_(policy), wait_ms_(wait_ms) {}
    PinRegistry(const PinRegistry&) = delete;
    PinRegistry& operator=(const PinRegistry&) = delete;

    // true: registered (by this call or an earlier one), must be released by this thread with this address
    bool acquire(const void* ptr, size_t bytes, PinTrace* trace = nullptr) {
        PinTrace t;
        if (trace) *trace = t;
        if (!ptr || !bytes) return false;
        const uint8_t* lo = (const uint8_t*)ptr;
        const uint8_t* hi = lo + bytes;
        const std::thread::id me = std::this_thread::get_id();
        bool waited = false;
        std::chrono::steady_clock::time_point deadline;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            Hits hit = touching(lo, hi);
            if (hit.empty()) {
                if (!policy_.register_range(lo, bytes)) return done(t, trace, PIN_REGISTER_FAILED, false);  // exotic memory: the copies block the caller instead
                Entry e{bytes, {}};
                e.holders[me] = 1;
                pins_[lo] = e;
                return done(t, trace, PIN_FRESH, true);
            }
            if (hit.size() == 1 && hit[0]->first <= lo && hit[0]->first + hit[0]->second.bytes >= hi) {
                ++hit[0]->second.holders[me];
                return done(t, trace, PIN_SHARED, true);
            }
            if (held_by_others(hit, me)) {
                // Never wait unboundedly: two threads that each hold a range and ask for one overlapping the other's, or a
                // worker that waits here while its dispatcher holds the fan-out lock another holder is queued for, would wait for ever.  After
                // wait_ms in all the request goes on WITHOUT a registration of its own - the caller's copies then go through the lane's
                // staging buffer where the runtime rejects them (host_lane.h), as they do when a registration fails.
                if (!waited) deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(wait_ms_);
                waited = true;
                if (std::chrono::steady_clock::now() >= deadline) return done(t, trace, PIN_GAVE_UP, false);
                ++stats_.waiting;
#if defined(__SANITIZE_THREAD__)
                // ThreadSanitizer builds only (the host test): a wait on the steady clock is pthread_cond_clockwait, which the
                // ThreadSanitizer of GCC 11 does not know - it then believes the lock is held throughout the wait.  The limit is
                // still decided by the steady clock, above.
                (void)cv_.wait_until(lk, std::chrono::system_clock::now() + (deadline - std::chrono::steady_clock::now()));
#else
                (void)cv_.wait_until(lk, deadline);  // a release wakes us; then look again
#endif
                --stats_.waiting;
                ++t.waits;
                continue;
            }
            // every interval in the way is held by this thread alone: replace them by their union with the request
            const uint8_t* ulo = lo;
            const uint8_t* uhi = hi;
            unsigned mine = 1;
            for (auto& h : hit) {
                if (h->first < ulo) ulo = h->first;
                if (h->first + h->second.bytes > uhi) uhi = h->first + h->second.bytes;
                mine += h->second.refs();
            }
            lk.unlock();
            policy_.quiesce();  // this thread's copies over the old intervals are complete
            lk.lock();
            // Nobody else can have changed what is in the way meanwhile without waiting for us?  They can: a request INSIDE one of our
            // intervals takes a hold on it, and a request that touches none of them (in a gap the union bridges, or past an end the union
            // extends) registers a range of its own.  Our own intervals cannot have gone (we hold them), so the iterators are still valid:
            // look again whenever the set in the way is not the one the union was computed from.
            if (touching(lo, hi) != hit || held_by_others(hit, me)) {
                ++t.rechecks;
                continue;
            }
            for (auto& h : hit) {
                policy_.unregister_range(h->first);
                pins_.erase(h);
            }
            if (!policy_.register_range(ulo, (size_t)(uhi - ulo))) {
                // nothing of the union is registered now: this thread's earlier holds are gone with it (its copies go unregistered,
                // which is correct), and releases of them find no interval and do nothing
                cv_.notify_all();
                return done(t, trace, PIN_UNION_FAILED, false);
            }
            Entry e{(size_t)(uhi - ulo), {}};
            e.holders[me] = mine;
            pins_[ulo] = e;
            return done(t, trace, PIN_UNION, true);
        }
    }

    // ptr: any address a successful acquire was made with (it lies inside exactly one interval)
    void release(const void* ptr, PinTrace* trace = nullptr) {
        PinTrace t;
        const uint8_t* p = (const uint8_t*)ptr;
        std::lock_guard<std::mutex> lk(mu_);
        auto it = pins_.upper_bound(p);
        if (it == pins_.begin()) return (void)done(t, trace, PIN_RELEASE_UNKNOWN, false);
        --it;
        if (p >= it->first + it->second.bytes) return (void)done(t, trace, PIN_RELEASE_UNKNOWN, false);
        auto h = it->second.holders.find(std::this_thread::get_id());
        // not ours: a hold is released by the thread that took it (HostPin lives in one call object)
        if (h == it->second.holders.end()) return (void)done(t, trace, PIN_RELEASE_NOT_HELD, false);
        if (h->second && --h->second == 0) it->second.holders.erase(h);
        int branch = PIN_RELEASED_KEPT;
        if (it->second.refs() == 0) {
            policy_.unregister_range(it->first);
            pins_.erase(it);
            branch = PIN_RELEASED_LAST;
        }
        cv_.notify_all();
        (void)done(t, trace, branch, true);
    }

    PinStats stats() const {
        std::lock_guard<std::mutex> lk(mu_);
        return stats_;
    }
    std::vector<PinInterval> snapshot() const {
        std::lock_guard<std::mutex> lk(mu_);
        std::vector<PinInterval> v;
        for (const auto& e : pins_) v.push_back({e.first, e.second.bytes, e.second.holders});
        return v;
    }
    Policy& policy() { return policy_; }
};

}  // namespace plk
