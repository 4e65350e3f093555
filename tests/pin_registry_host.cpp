// pin_registry_host.cpp -- the caller-buffer registry of the host-pointer entry points (plonky_amd/csrc/pin_registry.h) on the host,
// against a model of the runtime.  Stand-alone: g++ -std=c++17 -pthread, with or without a sanitizer (tests/test_pin_registry_host.py).
//
// The model registrar records every register / unregister / "every device quiet" call, can be told to refuse the next registration,
// and runs a hook of the scenario's inside "every device quiet" (that is where the registry has dropped its lock, so the hook is how
// the concurrent cases become deterministic).  It checks, at every call of the registry and at the end of every scenario:
//   * live registrations never overlap (an overlapping registration is what the runtime would refuse);
//   * a range is never unregistered while another thread holds it; the holding thread itself unregisters it only inside an acquire,
//     after the synchronisation, and registers a range that covers it next (or loses exactly those holds when that is refused);
//   * an acquire that returned true lies inside exactly one live registration until its release;
//   * at quiescence every registration has been unregistered exactly once, and the registry's map is empty.
// Every scenario prints the branch the registry reports (PinTrace); the Python test compares the lines.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "pin_registry.h"

using namespace plk;

static const uint8_t* const BASE = (const uint8_t*)(uintptr_t)0x40000000;  // a fake address space: never dereferenced
static const uint8_t* at(size_t off) { return BASE + off; }

static std::mutex g_out_mu;
static int g_violations = 0;
static void violation(const char* fmt, ...) {
    std::lock_guard<std::mutex> lk(g_out_mu);
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (++g_violations <= 20) printf("VIOLATION: %s\n", buf);
}
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) violation(__VA_ARGS__); \
    } while (0)

struct Range {
    const uint8_t* lo;
    size_t bytes;
    const uint8_t* hi() const { return lo + bytes; }
    bool inside(const Range& o) const { return o.lo <= lo && hi() <= o.hi(); }
    bool touches(const Range& o) const { return lo < o.hi() && o.lo < hi(); }
};

struct Model {
    std::mutex mu;
    std::map<const uint8_t*, size_t> live;
    std::map<std::thread::id, std::vector<Range>> holds;  // a subset of the registry's holds at all times (see Harness)
    struct ThreadState {
        bool in_acquire = false, synced = false;
        std::vector<Range> pending;  // unregistered by this thread's union, not yet covered by a registration
    };
    std::map<std::thread::id, ThreadState> ts;
    unsigned long long registers = 0, refused = 0, unregisters = 0, syncs = 0;
    int fail_next = 0;
    std::function<void()> hook;
    bool keep_log = true;
    std::vector<std::string> log;

    void note(const char* what, const uint8_t* lo, size_t bytes) {
        if (!keep_log) return;
        char buf[64];
        if (lo)
            snprintf(buf, sizeof(buf), "%s %zu %zu", what, (size_t)(lo - BASE), bytes);
        else
            snprintf(buf, sizeof(buf), "%s", what);
        log.push_back(buf);
    }
    void lose_pending(std::thread::id me) {  // the union was refused: the thread's holds inside what it unregistered are gone
        ThreadState& st = ts[me];
        auto& mine = holds[me];
        for (const Range& p : st.pending)
            mine.erase(std::remove_if(mine.begin(), mine.end(), [&](const Range& h) { return h.inside(p); }), mine.end());
        st.pending.clear();
    }
};

struct ModelPolicy {
    Model* m = nullptr;
    bool register_range(const uint8_t* lo, size_t bytes) {
        std::lock_guard<std::mutex> lk(m->mu);
        const std::thread::id me = std::this_thread::get_id();
        const Range r{lo, bytes};
        if (m->fail_next > 0) {
            --m->fail_next;
            ++m->refused;
            m->note("refuse", lo, bytes);
            m->lose_pending(me);
            return false;
        }
        for (const auto& e : m->live)
            if (r.touches(Range{e.first, e.second})) {
                violation("registration [%zu, %zu) overlaps the live one [%zu, %zu)", (size_t)(lo - BASE), (size_t)(lo - BASE) + bytes,
                          (size_t)(e.first - BASE), (size_t)(e.first - BASE) + e.second);
                ++m->refused;
                m->lose_pending(me);
                return false;
            }
        for (const Range& p : m->ts[me].pending) CHECK(p.inside(r), "the union [%zu, +%zu) does not cover an interval it replaced", (size_t)(lo - BASE), bytes);
        m->ts[me].pending.clear();
        m->live[lo] = bytes;
        ++m->registers;
        m->note("register", lo, bytes);
        return true;
    }
    void unregister_range(const uint8_t* lo) {
        std::lock_guard<std::mutex> lk(m->mu);
        const std::thread::id me = std::this_thread::get_id();
        auto it = m->live.find(lo);
        if (it == m->live.end()) {
            violation("unregister of %zu, which is not registered (a second time?)", (size_t)(lo - BASE));
            return;
        }
        const Range r{lo, it->second};
        Model::ThreadState& st = m->ts[me];
        for (const auto& t : m->holds)
            for (const Range& h : t.second) {
                if (!h.touches(r)) continue;
                if (t.first != me)
                    violation("[%zu, +%zu) unregistered under another thread's hold [%zu, +%zu)", (size_t)(lo - BASE), r.bytes, (size_t)(h.lo - BASE), h.bytes);
                else if (!st.in_acquire)
                    violation("[%zu, +%zu) unregistered by a release while the thread still holds [%zu, +%zu)", (size_t)(lo - BASE), r.bytes,
                              (size_t)(h.lo - BASE), h.bytes);
            }
        if (st.in_acquire) {
            CHECK(st.synced, "the union path unregistered %zu before every device was quiet", (size_t)(lo - BASE));
            st.pending.push_back(r);
        }
        m->live.erase(it);
        ++m->unregisters;
        m->note("unregister", lo, r.bytes);
    }
    void quiesce() {
        std::function<void()> hook;
        {
            std::lock_guard<std::mutex> lk(m->mu);
            ++m->syncs;
            m->ts[std::this_thread::get_id()].synced = true;
            m->note("sync", nullptr, 0);
            hook.swap(m->hook);  // a hook runs once
        }
        if (hook) hook();
    }
};

struct Harness {
    Model m;
    PinRegistry<ModelPolicy> reg;
    explicit Harness(long wait_ms) : reg(wait_ms, ModelPolicy{&m}) {}

    // the model's holds are added AFTER the registry granted them and removed BEFORE the registry drops them: a subset at all times,
    // so that a hold the model sees under an unregistration is one the registry still counts
    bool acquire(size_t off, size_t bytes, PinTrace* trace = nullptr) {
        const std::thread::id me = std::this_thread::get_id();
        {
            std::lock_guard<std::mutex> lk(m.mu);
            Model::ThreadState& st = m.ts[me];
            st.in_acquire = true;
            st.synced = false;
            st.pending.clear();
        }
        PinTrace t;
        const bool ok = reg.acquire(at(off), bytes, &t);
        {
            std::lock_guard<std::mutex> lk(m.mu);
            Model::ThreadState& st = m.ts[me];
            st.in_acquire = false;
            CHECK(st.pending.empty(), "an acquire ended with an interval unregistered and nothing in its place");
            st.pending.clear();
            if (ok) m.holds[me].push_back(Range{at(off), bytes});
            CHECK(ok == (t.branch == PIN_FRESH || t.branch == PIN_SHARED || t.branch == PIN_UNION), "acquire returned %d on branch %s", (int)ok,
                  pin_branch_name(t.branch));
        }
        check_own();
        if (trace) *trace = t;
        return ok;
    }
    void release(size_t off, PinTrace* trace = nullptr) {
        const std::thread::id me = std::this_thread::get_id();
        {
            std::lock_guard<std::mutex> lk(m.mu);
            auto& mine = m.holds[me];
            for (auto it = mine.begin(); it != mine.end(); ++it)
                if (it->lo == at(off)) {
                    mine.erase(it);
                    break;
                }
        }
        reg.release(at(off), trace);
        check_own();
    }
    // does the calling thread hold `off` in the model (a hold lost to a refused union is gone from it)
    bool holds(size_t off) {
        std::lock_guard<std::mutex> lk(m.mu);
        for (const Range& h : m.holds[std::this_thread::get_id()])
            if (h.lo == at(off)) return true;
        return false;
    }
    void check_own() {  // other threads never unregister under this thread's holds, so this is free of races
        std::lock_guard<std::mutex> lk(m.mu);
        for (const Range& h : m.holds[std::this_thread::get_id()]) {
            int covering = 0;
            for (const auto& e : m.live) covering += h.inside(Range{e.first, e.second});
            CHECK(covering == 1, "the hold [%zu, +%zu) lies inside %d live registrations", (size_t)(h.lo - BASE), h.bytes, covering);
        }
    }
    // single-threaded moments only: the registry's map is the model's, interval by interval, with the model's hold counts
    void check_same() {
        const std::vector<PinInterval> snap = reg.snapshot();
        std::lock_guard<std::mutex> lk(m.mu);
        CHECK(snap.size() == m.live.size(), "the registry has %zu intervals, the runtime %zu registrations", snap.size(), m.live.size());
        for (const PinInterval& iv : snap) {
            auto it = m.live.find(iv.lo);
            CHECK(it != m.live.end() && it->second == iv.bytes, "interval [%zu, +%zu) is not a live registration", (size_t)(iv.lo - BASE), iv.bytes);
            for (const auto& who : iv.holders) {
                unsigned want = 0;
                auto hs = m.holds.find(who.first);
                if (hs != m.holds.end())
                    for (const Range& h : hs->second) want += h.inside(Range{iv.lo, iv.bytes});
                CHECK(who.second == want, "a thread's hold count on [%zu, +%zu) is %u, the model's %u", (size_t)(iv.lo - BASE), iv.bytes, who.second, want);
            }
        }
    }
    void check_quiet(const char* scenario) {
        check_same();
        std::lock_guard<std::mutex> lk(m.mu);
        CHECK(m.live.empty(), "%s: %zu registrations are still live at the end", scenario, m.live.size());
        CHECK(m.registers == m.unregisters, "%s: %llu registrations, %llu unregistrations", scenario, m.registers, m.unregisters);
        for (const auto& t : m.holds) CHECK(t.second.empty(), "%s: a thread still holds %zu ranges", scenario, t.second.size());
    }
    void expect_log(const char* scenario, const std::vector<std::string>& want) {
        std::lock_guard<std::mutex> lk(m.mu);
        if (m.log == want) return;
        std::string got;
        for (const auto& s : m.log) got += "[" + s + "] ";
        violation("%s: the runtime saw %s", scenario, got.c_str());
    }
};

// a thread of its own that runs what it is given: the registry tells threads apart by std::this_thread::get_id()
class Actor {
    std::mutex mu_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool busy_ = false, stop_ = false;
    std::thread th_;

  public:
    Actor() : th_([this] { loop(); }) {}
    ~Actor() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [this] { return stop_ || job_; });
            if (!job_) return;
            std::function<void()> j;
            j.swap(job_);
            lk.unlock();
            j();
            lk.lock();
            busy_ = false;
            cv_.notify_all();
        }
    }
    void post(std::function<void()> j) {
        std::lock_guard<std::mutex> lk(mu_);
        job_ = std::move(j);
        busy_ = true;
        cv_.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !busy_; });
    }
    void run(std::function<void()> j) {
        post(std::move(j));
        wait();
    }
};

template <class P>
static void until_someone_waits(PinRegistry<P>& reg) {  // no sleep: the gauge goes up under the registry's lock, right before the wait
    while (reg.stats().waiting == 0) std::this_thread::yield();
}

static std::string tr(const PinTrace& t) {
    std::string s = pin_branch_name(t.branch);
    if (t.waits) s += "+waited";
    if (t.rechecks) s += "+rechecked" + std::to_string(t.rechecks);
    return s;
}
static void say(const char* scenario, const std::string& what) {
    std::lock_guard<std::mutex> lk(g_out_mu);
    printf("scenario %s: %s\n", scenario, what.c_str());
}

static void s_fresh() {
    Harness h(2000);
    PinTrace a, r;
    CHECK(h.acquire(0, 100, &a), "fresh: refused");
    h.check_same();
    h.release(0, &r);
    h.expect_log("fresh", {"register 0 100", "unregister 0 100"});
    h.check_quiet("fresh");
    say("fresh", tr(a) + " " + tr(r));
}
static void s_same_thread() {
    Harness h(2000);
    PinTrace a, b, r1, r2;
    h.acquire(0, 100, &a);
    h.acquire(0, 100, &b);
    h.check_same();
    h.release(0, &r1);
    h.check_same();
    h.release(0, &r2);
    h.expect_log("same-thread", {"register 0 100", "unregister 0 100"});
    h.check_quiet("same-thread");
    say("same-thread", tr(a) + " " + tr(b) + " " + tr(r1) + " " + tr(r2));
}
static void s_other_thread() {  // shared, released by whoever is last: here the second thread
    Harness h(2000);
    Actor other;
    PinTrace a, b, r1, r2;
    h.acquire(0, 100, &a);
    other.run([&] { h.acquire(0, 100, &b); });
    h.check_same();
    h.release(0, &r1);
    h.expect_log("other-thread", {"register 0 100"});
    h.check_same();
    other.run([&] { h.release(0, &r2); });
    h.expect_log("other-thread", {"register 0 100", "unregister 0 100"});
    h.check_quiet("other-thread");
    say("other-thread", tr(a) + " " + tr(b) + " " + tr(r1) + " " + tr(r2));
}
static void s_nested() {
    Harness h(2000);
    PinTrace a, b, r1, r2;
    h.acquire(0, 1000, &a);
    h.acquire(100, 100, &b);
    h.check_same();
    h.release(100, &r1);
    h.release(0, &r2);
    h.expect_log("nested", {"register 0 1000", "unregister 0 1000"});
    h.check_quiet("nested");
    say("nested", tr(a) + " " + tr(b) + " " + tr(r1) + " " + tr(r2));
}
static void s_adjacent() {
    Harness h(2000);
    PinTrace a, b, r1, r2;
    h.acquire(0, 100, &a);
    h.acquire(100, 100, &b);
    h.check_same();
    CHECK(h.reg.snapshot().size() == 2, "adjacent: not two intervals");
    h.release(0, &r1);
    h.release(100, &r2);
    h.expect_log("adjacent", {"register 0 100", "register 100 100", "unregister 0 100", "unregister 100 100"});
    h.check_quiet("adjacent");
    say("adjacent", tr(a) + " " + tr(b) + " " + tr(r1) + " " + tr(r2));
}
static void s_own_union() {  // [0,100) then [50,150) then [140,300): holds carried over, released with the original addresses in every order
    const size_t addr[3] = {0, 50, 140};
    int order[3] = {0, 1, 2};
    std::string all;
    do {
        Harness h(2000);
        PinTrace a, b, c, r[3];
        h.acquire(0, 100, &a);
        h.acquire(50, 100, &b);
        h.check_same();
        h.acquire(140, 160, &c);
        h.check_same();
        const std::vector<PinInterval> snap = h.reg.snapshot();
        CHECK(snap.size() == 1 && snap[0].lo == at(0) && snap[0].bytes == 300 && snap[0].holders.size() == 1 && snap[0].holders.begin()->second == 3,
              "own-union: not one interval [0, 300) with three holds");
        std::vector<std::string> want = {"register 0 100", "sync", "unregister 0 100", "register 0 150", "sync", "unregister 0 150", "register 0 300"};
        for (int i = 0; i < 3; ++i) {
            h.expect_log("own-union", want);  // not unregistered before the last release
            h.release(addr[order[i]], &r[i]);
            h.check_same();
        }
        want.push_back("unregister 0 300");
        h.expect_log("own-union", want);
        h.check_quiet("own-union");
        const std::string line = tr(a) + " " + tr(b) + " " + tr(c) + " " + tr(r[0]) + " " + tr(r[1]) + " " + tr(r[2]);
        if (all.empty()) all = line;
        CHECK(all == line, "own-union: order %d%d%d took %s", order[0], order[1], order[2], line.c_str());
    } while (std::next_permutation(order, order + 3));
    say("own-union", all + " (6 orders)");
}
// during the union's synchronisation another thread does `meddle`; the request must look again, wait for that thread, and only then
// unregister: [0,100) (and [200,300) when `gap`) are this thread's, the request is [50,150) or [50,250)
static void s_union_recheck(const char* name, bool gap, size_t m_off, size_t m_bytes, int m_branch) {
    Harness h(2000);
    Actor me, other;
    PinTrace a, m, r;
    me.run([&] {
        h.acquire(0, 100);
        if (gap) h.acquire(200, 100);
    });
    h.m.hook = [&] { other.run([&] { h.acquire(m_off, m_bytes, &m); }); };
    me.post([&] { h.acquire(50, gap ? 200 : 100, &a); });
    until_someone_waits(h.reg);  // the request has looked again and found the other thread in its way
    {
        std::lock_guard<std::mutex> lk(h.m.mu);
        CHECK(h.m.unregisters == 0, "%s: unregistered under the other thread's hold", name);
    }
    other.run([&] { h.release(m_off, &r); });
    me.wait();
    CHECK(m.branch == m_branch, "%s: the other thread's request took %s", name, pin_branch_name(m.branch));
    h.check_same();
    const std::vector<PinInterval> snap = h.reg.snapshot();
    const size_t want_bytes = gap ? 300 : 150;
    CHECK(snap.size() == 1 && snap[0].lo == at(0) && snap[0].bytes == want_bytes, "%s: not one interval [0, %zu)", name, want_bytes);
    me.run([&] {
        h.release(0);
        if (gap) h.release(200);
        h.release(50);
    });
    h.check_quiet(name);
    say(name, tr(a) + " other:" + tr(m) + " " + tr(r));
}
static void s_union_fails() {
    Harness h(2000);
    PinTrace a, b, r, again, r2;
    h.acquire(0, 100, &a);
    h.m.fail_next = 1;
    const bool ok = h.acquire(50, 100, &b);
    CHECK(!ok, "union-fails: granted");
    CHECK(h.reg.snapshot().empty() && h.m.live.empty(), "union-fails: something of the union is registered");
    h.release(0, &r);  // the earlier hold is gone: a no-op
    h.expect_log("union-fails", {"register 0 100", "sync", "unregister 0 100", "refuse 0 150"});
    h.acquire(0, 150, &again);
    h.release(0, &r2);
    h.expect_log("union-fails", {"register 0 100", "sync", "unregister 0 100", "refuse 0 150", "register 0 150", "unregister 0 150"});
    h.check_quiet("union-fails");
    say("union-fails", tr(a) + " " + tr(b) + " " + tr(r) + " " + tr(again) + " " + tr(r2));
}
static void s_register_fails() {
    Harness h(2000);
    PinTrace a, again, r;
    h.m.fail_next = 1;
    CHECK(!h.acquire(0, 100, &a), "register-fails: granted");
    CHECK(h.reg.snapshot().empty(), "register-fails: an interval was kept");
    h.acquire(0, 100, &again);
    h.release(0, &r);
    h.check_quiet("register-fails");
    say("register-fails", tr(a) + " " + tr(again) + " " + tr(r));
}
static void s_wait_release() {  // both hold [0,100); this thread asks for [50,150) and sleeps until the other one lets go
    Harness h(2000);
    Actor me, other;
    PinTrace a, r;
    other.run([&] { h.acquire(0, 100); });
    me.run([&] { h.acquire(0, 50); });
    me.post([&] { h.acquire(50, 100, &a); });
    until_someone_waits(h.reg);
    h.expect_log("wait-release", {"register 0 100"});
    other.run([&] { h.release(0, &r); });
    me.wait();
    h.expect_log("wait-release", {"register 0 100", "sync", "unregister 0 100", "register 0 150"});  // once, and before the union
    h.check_same();
    me.run([&] {
        h.release(0);
        h.release(50);
    });
    h.check_quiet("wait-release");
    say("wait-release", tr(a) + " other:" + tr(r));
}
static void s_wait_gives_up() {
    const long limit = 50;
    Harness h(limit);
    Actor other;
    PinTrace a;
    other.run([&] { h.acquire(0, 100); });
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = h.acquire(50, 100, &a);
    const long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    CHECK(!ok, "wait-gives-up: granted");
    CHECK(ms >= limit && ms < 100 * limit, "wait-gives-up: returned after %ld ms with a limit of %ld ms", ms, limit);
    h.check_same();  // the map and the holder's count are what they were
    h.expect_log("wait-gives-up", {"register 0 100"});
    const std::vector<PinInterval> snap = h.reg.snapshot();
    CHECK(snap.size() == 1 && snap[0].bytes == 100 && snap[0].holders.size() == 1 && snap[0].holders.begin()->second == 1, "wait-gives-up: the map changed");
    other.run([&] { h.release(0); });
    h.check_quiet("wait-gives-up");
    say("wait-gives-up", tr(a));
}
static void s_release_not_held() {
    Harness h(2000);
    Actor other;
    PinTrace r, r2;
    h.acquire(0, 100);
    other.run([&] { h.release(0, &r); });
    h.check_same();
    h.expect_log("release-not-held", {"register 0 100"});
    h.release(0, &r2);
    h.check_quiet("release-not-held");
    say("release-not-held", tr(r) + " " + tr(r2));
}
static void s_release_unknown() {
    Harness h(2000);
    PinTrace r0, r1, r2;
    h.release(5000, &r0);  // an empty map
    h.acquire(0, 100);
    h.release(5000, &r1);  // past the interval
    h.release(100, &r2);   // one past its end
    h.check_same();
    h.release(0);
    h.expect_log("release-unknown", {"register 0 100", "unregister 0 100"});
    h.check_quiet("release-unknown");
    say("release-unknown", tr(r0) + " " + tr(r1) + " " + tr(r2));
}
static void s_bridge_gap() {
    Harness h(2000);
    PinTrace a, r[3];
    h.acquire(0, 100);
    h.acquire(200, 100);
    h.acquire(50, 200, &a);
    h.check_same();
    const std::vector<PinInterval> snap = h.reg.snapshot();
    CHECK(snap.size() == 1 && snap[0].bytes == 300 && snap[0].holders.begin()->second == 3, "bridge-gap: not one interval [0, 300) with three holds");
    h.release(0, &r[0]);
    h.release(200, &r[1]);
    h.release(50, &r[2]);
    h.expect_log("bridge-gap", {"register 0 100", "register 200 100", "sync", "unregister 0 100", "unregister 200 100", "register 0 300", "unregister 0 300"});
    h.check_quiet("bridge-gap");
    say("bridge-gap", tr(a) + " " + tr(r[0]) + " " + tr(r[1]) + " " + tr(r[2]));
}

// 8 threads, a fixed-seed sequence each over 40 overlapping ranges, a refused registration now and then, wait limit 20 ms
static void s_stress(unsigned ops) {
    Harness h(20);
    h.m.keep_log = false;
    const int threads = 8, ranges = 40;
    std::atomic<unsigned long long> granted{0}, denied{0};
    std::atomic<int> ready{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1);
            auto rnd = [&] {
                x ^= x << 13;
                x ^= x >> 7;
                x ^= x << 17;
                return x;
            };
            std::vector<size_t> mine;
            for (++ready; ready.load() < threads;) std::this_thread::yield();  // all at once, not one after the other
            for (unsigned i = 0; i < ops; ++i) {
                const uint64_t r = rnd();
                if (i % 8 == 0) std::this_thread::yield();
                if (mine.size() < 3 && (mine.empty() || (r & 1))) {
                    const int k = (int)((r >> 8) % ranges);
                    const size_t off = 64 * (size_t)((k * 7) % ranges), bytes = 64 * (size_t)(1 + (k * 5) % 4);
                    if ((r >> 20) % 64 == 0) {
                        std::lock_guard<std::mutex> lk(h.m.mu);
                        h.m.fail_next = 1;  // whichever registration comes next is refused
                    }
                    if (h.acquire(off, bytes)) {
                        mine.push_back(off);
                        ++granted;
                    } else {
                        ++denied;
                        // a refused union took the thread's holds inside it along: forget them as the library's callers may not (their
                        // releases are no-ops, or land on nothing of theirs), which the model cannot tell from a wrong release
                        mine.erase(std::remove_if(mine.begin(), mine.end(), [&](size_t o) { return !h.holds(o); }), mine.end());
                    }
                } else {
                    const size_t j = (size_t)((r >> 8) % mine.size());
                    h.release(mine[j]);
                    mine.erase(mine.begin() + (long)j);
                }
            }
            for (size_t off : mine) h.release(off);
        });
    for (auto& th : pool) th.join();
    {
        std::lock_guard<std::mutex> lk(h.m.mu);
        h.m.fail_next = 0;
    }
    h.check_quiet("stress");
    const PinStats st = h.reg.stats();
    unsigned long long acquired = st.branch[PIN_FRESH] + st.branch[PIN_SHARED] + st.branch[PIN_UNION];
    unsigned long long released = st.branch[PIN_RELEASED_LAST] + st.branch[PIN_RELEASED_KEPT];
    // holds lost to a refused union are never released: every other hold is, exactly once
    CHECK(acquired == granted && released <= acquired, "stress: %llu granted, %llu counted, %llu released", granted.load(), acquired, released);
    CHECK(st.branch[PIN_UNION] > 0 && st.branch[PIN_SHARED] > 0, "stress: the sequence reached no union or no shared hold");
    {
        std::lock_guard<std::mutex> lk(g_out_mu);
        printf("stress: %llu granted %llu denied; fresh %llu shared %llu union %llu union-failed %llu register-failed %llu gave-up %llu waits %llu rechecks %llu\n",
               granted.load(), denied.load(), st.branch[PIN_FRESH], st.branch[PIN_SHARED], st.branch[PIN_UNION], st.branch[PIN_UNION_FAILED],
               st.branch[PIN_REGISTER_FAILED], st.branch[PIN_GAVE_UP], st.waits, st.rechecks);
    }
    say("stress", "balanced");
}

int main(int argc, char** argv) {
    const unsigned ops = argc > 1 ? (unsigned)atoi(argv[1]) : 3000;
    s_fresh();
    s_same_thread();
    s_other_thread();
    s_nested();
    s_adjacent();
    s_own_union();
    s_union_recheck("union-recheck", false, 10, 10, PIN_SHARED);        // a hold INSIDE the old interval
    s_union_recheck("union-recheck-gap", true, 120, 30, PIN_FRESH);     // a registration of its own in the gap the union bridges
    s_union_recheck("union-recheck-beyond", false, 120, 100, PIN_FRESH);  // ... and past the end the union extends
    s_union_fails();
    s_register_fails();
    s_wait_release();
    s_wait_gives_up();
    s_release_not_held();
    s_release_unknown();
    s_bridge_gap();
    s_stress(ops);
    if (g_violations) {
        printf("FAILED: %d violations\n", g_violations);
        return 1;
    }
    printf("OK\n");
    return 0;
}
