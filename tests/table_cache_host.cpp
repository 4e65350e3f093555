// table_cache_host.cpp -- the cache of device-resident tables (plonky_amd/csrc/table_cache.h) on the host, with a T that counts its
// constructions and destructions in place of device buffers.  Stand-alone: g++ -std=c++17 -pthread, with or without a sanitizer
// (tests/test_table_cache_host.py).  Every scenario prints one line; the Python test compares the lines.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <random>
#include <set>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "table_cache.h"

using namespace plk;

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
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) violation(__VA_ARGS__); \
    } while (0)

constexpr int N_CACHES = 3, N_KEYS = 8;
static std::atomic<long> g_constructed{0}, g_destroyed{0};
static std::atomic<long> g_key_built[N_CACHES][N_KEYS], g_key_destroyed[N_CACHES][N_KEYS];  // tables whose build succeeded

struct Tab {
    int cache = -1, key = -1;  // set by a build that succeeds
    Tab() { ++g_constructed; }
    ~Tab() {
        ++g_destroyed;
        if (cache >= 0) ++g_key_destroyed[cache][key];
    }
    Tab(const Tab&) = delete;
    Tab& operator=(const Tab&) = delete;
};
using Cache = TableCache<int, Tab>;
using Ptr = std::shared_ptr<Tab>;

static long alive() { return g_constructed.load() - g_destroyed.load(); }
static void say(const char* name, const std::string& what) { printf("scenario %s: %s\n", name, what.c_str()); }
static std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}
// a build that succeeds and counts itself
static auto ok_build(int cache, int key, int* builds = nullptr) {
    return [=](Tab& t) {
        t.cache = cache;
        t.key = key;
        ++g_key_built[cache][key];
        if (builds) ++*builds;
        return PLK_OK;
    };
}

static void hit_and_miss() {
    Cache c;
    int builds = 0;
    Ptr a, b, other;
    const int rc1 = c.get(5, a, ok_build(0, 5, &builds));
    const int rc2 = c.get(5, b, ok_build(0, 5, &builds));
    const int rc3 = c.get(6, other, ok_build(0, 6, &builds));
    say("hit-and-miss", fmt("rc %d %d %d builds %d same %d distinct %d alive %ld", rc1, rc2, rc3, builds, a && a == b, other && other != a, alive()));
}

static void failed_build() {
    Cache c;
    const long c0 = g_constructed, d0 = g_destroyed;
    int builds = 0;
    Ptr p;
    const int rc1 = c.get(1, p, [&](Tab&) {
        ++builds;
        return PLK_ERR_OOM;
    });
    const bool empty_after_fail = !p;
    const long c1 = g_constructed - c0, d1 = g_destroyed - d0;  // the half-built one: constructed and destroyed once, before get returned
    const int rc2 = c.get(1, p, ok_build(0, 1, &builds));
    say("failed-build", fmt("rc %d then %d builds %d out-empty %d half-built constructed %ld destroyed %ld got-key %d", rc1, rc2, builds, empty_after_fail, c1, d1,
                            p ? p->key : -1));
}

// is the key in the cache?  A get whose build fails inserts nothing, so it asks without disturbing the cache
static bool present(Cache& c, int key, Ptr* which = nullptr) {
    bool ran = false;
    Ptr p;
    c.get(key, p, [&](Tab&) {
        ran = true;
        return PLK_ERR_INVALID_ARG;
    });
    if (which) *which = p;
    return !ran;
}

static void bound() {
    Cache c(4);
    Ptr held[6];
    for (int k = 0; k < 6; ++k) c.get(k, held[k], ok_build(1, k));
    std::string kept;
    for (int k = 0; k < 6; ++k) {
        Ptr in_cache;
        if (present(c, k, &in_cache) && in_cache == held[k]) kept += (kept.empty() ? "" : " ") + std::to_string(k);
    }
    // keys 0 and 1 were evicted; the test's own pointers keep the objects alive
    const long while_held = g_key_destroyed[1][0] + g_key_destroyed[1][1];
    held[0].reset();
    held[1].reset();
    say("bound", fmt("kept [%s] evicted destroyed while held %ld after release %ld %ld", kept.c_str(), while_held, g_key_destroyed[1][0].load(),
                     g_key_destroyed[1][1].load()));
}

static void clear_under_hold() {
    Cache c;
    Ptr p;
    c.get(3, p, ok_build(0, 3));
    const long d0 = g_key_destroyed[0][3];
    c.clear();
    const bool gone = !present(c, 3);
    const long after_clear = g_key_destroyed[0][3] - d0;
    const int held_key = p->key;  // still alive
    p.reset();
    const long after_release = g_key_destroyed[0][3] - d0;
    c.clear();
    say("clear-under-hold", fmt("absent %d destroyed after clear %ld held-key %d destroyed after release %ld at end %ld", gone, after_clear, held_key,
                                after_release, g_key_destroyed[0][3] - d0));
}

static void nested() {
    Cache a, b;
    int builds_a = 0, builds_b = 0;
    auto get_a = [&](int key, Ptr& out) {
        return a.get(key, out, [&](Tab& t) {
            Ptr inner;  // as the Plonk tables take the NTT plan: cache a's lock, then cache b's
            const int rc = b.get(key + 1, inner, ok_build(1, key + 1, &builds_b));
            if (rc != PLK_OK) return rc;
            return ok_build(0, key, &builds_a)(t);
        });
    };
    Ptr p, q;
    const int rc1 = get_a(2, p);
    b.clear();
    const int rc2 = get_a(2, q);  // a hit: b is not asked again
    table_caches_clear();
    const int rc3 = get_a(2, q);
    say("nested", fmt("rc %d %d %d builds a %d b %d", rc1, rc2, rc3, builds_a, builds_b));
}

// ---- stress: 8 threads, 3 caches (0 nests into 1, 2 is bounded), random get / clear / table_caches_clear ----
static Cache g_c0, g_c1, g_c2(4);
static Cache* const g_caches[N_CACHES] = {&g_c0, &g_c1, &g_c2};
static std::atomic<unsigned long long> g_clock{1};
static std::atomic<bool> g_in_build[N_CACHES];
struct Span {
    unsigned long long begin, end;
};
static std::mutex g_log_mu;
static std::vector<unsigned long long> g_build_at[N_CACHES][N_KEYS];  // stamps taken under the cache's lock
static std::vector<Span> g_clears[N_CACHES];                           // stamps taken around the call
// The bounded cache is followed exactly.  Its gets run side by side (the gate shared) but never beside a clear of it (the gate
// exclusive), so g_shadow - updated by the builds, which the cache's lock orders, and emptied by the clearing thread - is the set of
// keys in the cache at every build: a build of a key that is there is a violation.
static std::shared_mutex g_c2_gate;
static std::set<int> g_shadow;

static int stress_build(int c, int key, bool fail, Tab& t) {
    CHECK(!g_in_build[c].exchange(true), "two builds of cache %d at once", c);
    int rc = PLK_OK;
    if (c == 0) {
        Ptr inner;
        rc = g_c1.get(key, inner, [&](Tab& t1) { return stress_build(1, key, false, t1); });
        CHECK(rc != PLK_OK || (inner && inner->cache == 1 && inner->key == key), "nested get of key %d returned another table", key);
    }
    if (rc == PLK_OK && fail) rc = PLK_ERR_HIP;
    if (rc == PLK_OK) {
        ok_build(c, key)(t);
        if (c == 2) {
            CHECK(!g_shadow.count(key), "bounded cache: key %d built while it was there", key);
            if (g_shadow.size() >= 4) g_shadow.erase(g_shadow.begin());
            g_shadow.insert(key);
        }
        const unsigned long long at = g_clock++;
        std::lock_guard<std::mutex> lk(g_log_mu);
        g_build_at[c][key].push_back(at);
    }
    g_in_build[c] = false;
    return rc;
}
static void note_clear(int first, int last, const std::function<void()>& call) {
    std::unique_lock<std::shared_mutex> gate(g_c2_gate, std::defer_lock);
    if (last == 2) gate.lock();
    const unsigned long long begin = g_clock++;
    call();
    if (last == 2) g_shadow.clear();
    const unsigned long long end = g_clock++;
    std::lock_guard<std::mutex> lk(g_log_mu);
    for (int c = first; c <= last; ++c) g_clears[c].push_back({begin, end});
}

static void stress() {
    const long c0 = g_constructed, d0 = g_destroyed;
    long built0[N_CACHES][N_KEYS], destroyed0[N_CACHES][N_KEYS];
    for (int c = 0; c < N_CACHES; ++c)
        for (int k = 0; k < N_KEYS; ++k) built0[c][k] = g_key_built[c][k], destroyed0[c][k] = g_key_destroyed[c][k];
    std::vector<std::thread> threads;
    for (int th = 0; th < 8; ++th) {
        threads.emplace_back([th] {
            std::mt19937 rng(1234u + (unsigned)th);
            Ptr held;  // a table kept across later calls, as a running call keeps its tables across a clear
            for (int i = 0; i < 400; ++i) {
                const unsigned r = rng() % 100;
                const int c = (int)(rng() % N_CACHES), key = (int)(rng() % N_KEYS);
                if (r < 88) {
                    Ptr p;
                    const bool fail = rng() % 16 == 0;
                    std::shared_lock<std::shared_mutex> gate(g_c2_gate, std::defer_lock);
                    if (c == 2) gate.lock();
                    const int rc = g_caches[c]->get(key, p, [&](Tab& t) { return stress_build(c, key, fail, t); });
                    CHECK(rc == PLK_OK || (rc == PLK_ERR_HIP && fail && !p), "get: rc %d", rc);
                    CHECK(rc != PLK_OK || (p && p->cache == c && p->key == key), "get of cache %d key %d returned another table", c, key);
                    if (rc == PLK_OK && rng() % 4 == 0) held = p;
                } else if (r < 96) {
                    note_clear(c, c, [c] { g_caches[c]->clear(); });
                } else {
                    note_clear(0, N_CACHES - 1, [] { table_caches_clear(); });
                }
            }
        });
    }
    for (auto& t : threads) t.join();
    table_caches_clear();
    // Every successful build put its table into the cache, and the cache has let go of every one of them: a key was built exactly as
    // often as it was absent when asked for iff no get built a key that was there.  The bounded cache's shadow set has checked that at
    // every build.  For the other two, whose clears run beside their gets: builds of one cache are ordered by its lock, and two
    // successive builds of a key need a clear() that overlaps the time between them.
    for (int c = 0; c < N_CACHES; ++c) {
        for (int k = 0; k < N_KEYS; ++k) {
            const long built = g_key_built[c][k] - built0[c][k], destroyed = g_key_destroyed[c][k] - destroyed0[c][k];
            CHECK(built == destroyed, "cache %d key %d: built %ld destroyed %ld", c, k, built, destroyed);
            CHECK(built == (long)g_build_at[c][k].size(), "cache %d key %d: %ld builds, %zu logged", c, k, built, g_build_at[c][k].size());
            const auto& at = g_build_at[c][k];
            for (size_t i = 0; c != 2 && i + 1 < at.size(); ++i) {
                bool absent = false;
                for (const Span& s : g_clears[c]) absent = absent || (s.begin < at[i + 1] && s.end > at[i]);
                CHECK(absent, "cache %d key %d built at %llu and again at %llu with nothing that removed it in between", c, k, at[i], at[i + 1]);
            }
        }
    }
    const long constructed = g_constructed - c0, destroyed = g_destroyed - d0;
    CHECK(constructed == destroyed, "constructed %ld destroyed %ld", constructed, destroyed);
    CHECK(constructed > 100, "only %ld tables built", constructed);
    say("stress", g_violations ? "violations" : "balanced");
}

int main() {
    hit_and_miss();
    failed_build();
    bound();
    clear_under_hold();
    nested();
    stress();
    CHECK(alive() == 0, "%ld tables alive at the end", alive());
    if (g_violations) {
        printf("FAILED: %d violations\n", g_violations);
        return 1;
    }
    printf("OK\n");
    return 0;
}
