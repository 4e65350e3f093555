// Host harness of tests/test_msm_geom_host.py: plonky_amd/csrc/msm_geom.h compiled by g++ (it is plain C++), swept over a grid of
// (curve, n, window, mode, lanes, knobs) for what the MSM's kernels assume of a geometry.  With -DMSM_GEOM_HOST_MAIN it is a program
// that runs the same sweep (the form a sanitizer build takes).
#include <cstdarg>
#include <cstring>
#include <vector>

#include "../plonky_amd/csrc/ec.cuh"
#include "../plonky_amd/csrc/fz.cuh"
#include "../plonky_amd/csrc/msm_geom.h"

using namespace plk;

namespace {

// 32-bit words of a coordinate and uint4 of a raw point (29-bit limbs): what msm.hip passes from the curve structs
int limbs_of(int curve) { return with_curve(curve, [](auto t) { return (int)tag_t<decltype(t)>::FP::NL; }); }
int raw_u4_of(int curve) { return with_curve(curve, [](auto t) { return (int)FzCfg<typename tag_t<decltype(t)>::FP>::NZ; }); }
#define GEOM_BITS_CHECK(C) static_assert(msm_scalar_bits(C::CURVE_ID) == C::SP::BITS, "msm_scalar_bits");
PLK_FOR_EACH_CURVE(GEOM_BITS_CHECK)
#undef GEOM_BITS_CHECK

struct Report {
    long rows = 0, refused = 0, violations = 0;
    char first[256] = {};
    void fail(const char* fmt, ...) {
        if (!violations++) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(first, sizeof first, fmt, ap);
            va_end(ap);
        }
    }
};

struct Case {
    int curve;
    size_t n;
    unsigned window_bits;
    bool table_free;
    size_t slots;
    MsmKnobs knobs;
    const char* knob_name;
};

int geometry(const Case& c, size_t n, unsigned window_bits, MsmGeom* g) {
    return msm_geometry(c.curve, n, window_bits, c.table_free, c.slots, limbs_of(c.curve), raw_u4_of(c.curve), c.knobs, g);
}

void check(const Case& c, Report& r) {
    MsmGeom g;
    ++r.rows;
    const int rc = geometry(c, c.n, c.window_bits, &g);
#define REQUIRE(cond)                                                                                                                        \
    do {                                                                                                                                     \
        if (!(cond))                                                                                                                         \
            r.fail("%s fails: curve %d n %zu window_bits %u table_free %d slots %zu knob %s", #cond, c.curve, c.n, c.window_bits, (int)c.table_free, \
                   c.slots, c.knob_name);                                                                                                    \
    } while (0)
    if (rc != PLK_OK) {
        ++r.refused;
        REQUIRE(rc == PLK_ERR_INVALID_ARG && g.error[0] != 0);
        return;
    }
    const OrdCfg& o = g.ord;
    const TailGeom& t = g.tail;
    const size_t entries = g.n_eff * (size_t)g.windows;
    // the ordering (msm_order.hip)
    REQUIRE(g.c >= 2 && g.c <= MSM_MAX_WINDOW && (!g.table_free || g.c <= MSM_TF_MAX_WINDOW));
    REQUIRE(o.fine_bits >= 0 && o.fine_bits <= ORD_MAX_FINE);
    REQUIRE(o.nbins >= 1 && o.nbins <= ORD_MAX_BINS);
    REQUIRE(g.buckets == (uint32_t)o.nbins << o.fine_bits);
    REQUIRE(g.buckets >= (g.table_free ? g.wbuckets * (uint32_t)g.windows : g.wbuckets));
    REQUIRE(o.spt >= 1 && o.spt <= (uint32_t)ORD_THREADS);
    REQUIRE(o.spt * (uint32_t)g.windows <= (uint32_t)ORD_TILE);
    REQUIRE(entries < ((size_t)1 << 31) && o.entries_cap == entries);
    REQUIRE((size_t)o.nt1 * o.spt * o.sub >= g.n_eff && o.nt1 >= 1);
    REQUIRE(o.bin_lo == 0 && o.bin_hi == (uint32_t)o.nbins && o.ent_first == 0 && o.ent_stride == g.n_eff);
    REQUIRE(o.c == g.c && o.windows == g.windows && o.window_buckets == (g.table_free ? g.wbuckets : 0u) && o.raw_signed == (g.glv ? 1 : 0));
    if (o.perm == 1)
        REQUIRE(!c.knobs.order_v1 && !g.table_free && o.nbins == 512 && o.fine_bits >= 9 && o.sub == 4 && o.spt * o.sub == 1024u && g.windows <= 16 &&
                o.nt1 <= 2048u && (double)g.n_eff * g.windows / (double)o.nbins * 1.15 <= (double)ORD2_BIN_CAP);
    // the reduction (msm_tail.hip)
    REQUIRE(t.buckets == g.buckets && t.heavy_cap == g.heavy_cap && t.table_free == (g.table_free ? 1 : 0) && t.windows == g.windows);
    REQUIRE(t.transposed == o.perm && t.many_heads == 0 && t.two_level == (g.c - 1 >= 12 ? 1 : 0));
    if (t.two_level) {
        REQUIRE(t.L + t.H == g.c - 1);
        REQUIRE(t.g_log >= 0 && t.g_log <= t.L);
        REQUIRE(t.lpl_log >= 0 && t.lpl_log <= 4);
        REQUIRE(t.tail_wbuckets == 1u << t.H && t.planes >= t.H && (t.L < t.H || t.planes == t.H + 1));
        REQUIRE(!t.transposed || t.H == o.fine_bits);
    }
    if (t.plane_blocks > 1) REQUIRE(t.planes * t.plane_blocks * 4 <= FINAL_THREADS);
    REQUIRE(t.plane_blocks >= 1 && t.plane_blocks <= MSM_MAX_PLANE_PARTS);
    // the accumulation's chunking, as msm_geometry defines it
    REQUIRE((c.knobs.slice >= 2 && c.knobs.slice <= 4096) ? g.chunk == (uint32_t)c.knobs.slice : (g.chunk >= 8 && g.chunk <= 96));
    REQUIRE(g.max_lanes == entries / g.chunk + 2);
    REQUIRE(g.heavy_cap == (uint32_t)(g.max_lanes / HEAVY_HEADS + g.max_lanes / HEAVY_CHUNK + 2));
    const double heads = (double)entries / (double)g.buckets / (double)g.chunk;
    REQUIRE(t.lpb_log == (heads > 6.0 ? 3 : heads > 2.0 ? 2 : 0));
    // the workspace: what the kernels index
    const size_t raw_bytes = (size_t)raw_u4_of(c.curve) * 16;
    REQUIRE(g.part_bytes[PART_META] == (size_t)META_WORDS * 4);
    REQUIRE(g.part_bytes[PART_TMP] >= entries * 8 && g.part_bytes[PART_SORTED] >= entries * 4);
    REQUIRE(g.part_bytes[PART_OFF] >= ((size_t)g.buckets + 1) * 4 && g.part_bytes[PART_P_START] == (size_t)g.buckets * raw_bytes);
    REQUIRE(g.part_bytes[PART_P_HEAD] >= g.max_lanes * raw_bytes && g.part_bytes[PART_HEAD_LIVE] == 9 * head_lanes_padded(g.max_lanes));
    REQUIRE(head_lanes_padded(g.max_lanes) % 16 == 0 && head_lanes_padded(g.max_lanes) >= g.max_lanes + ACC_THREADS);
#undef REQUIRE
}

// A context sized for a halving sequence (msm_precompute's also_n) can be rebound to every member: each part of each member's
// workspace is at most the maximum the precomputation reserves.  `plus`: the inner-product argument's lengths are 2^k + 2.
void check_halving(const Case& c, size_t plus, Report& r) {
    size_t cap[MSM_WORK_PARTS] = {}, tab = 0;
    std::vector<size_t> ns;
    for (size_t n = c.n; n >= 2; n /= 2) ns.push_back(n + plus);
    MsmGeom g;
    for (size_t n : ns) {  // what msm_precompute_t does: its own n, then every other count, refused ones skipped
        if (geometry(c, n, 0, &g) != PLK_OK) continue;
        for (int k = 0; k < MSM_WORK_PARTS; ++k)
            if (g.part_bytes[k] > cap[k]) cap[k] = g.part_bytes[k];
        if (g.n_eff > tab) tab = g.n_eff;
    }
    for (size_t n : ns) {  // what msm_rebind_t checks
        ++r.rows;
        if (geometry(c, n, 0, &g) != PLK_OK) {
            ++r.refused;
            continue;
        }
        for (int k = 0; k < MSM_WORK_PARTS; ++k)
            if (g.part_bytes[k] > cap[k]) r.fail("halving from %zu: part %d of n %zu needs %zu bytes, the maximum is %zu (curve %d)", c.n, k, n, g.part_bytes[k], cap[k], c.curve);
        if (g.n_eff > tab) r.fail("halving from %zu: n %zu does not fit the table (curve %d)", c.n, n, c.curve);
    }
}

MsmKnob knob(int v) { return MsmKnob{true, v}; }

}  // namespace

// Sweeps the grid; returns the number of violated requirements (the first one's text in msg), rows / refused: geometries asked for / refused.
extern "C" long msm_geom_check_grid(long* rows, long* refused, char* msg, size_t msg_len) {
    struct Setting { const char* name; MsmKnobs k; };
    std::vector<Setting> settings;
    auto add = [&](const char* name, auto set) {
        MsmKnobs k;
        set(k);
        settings.push_back({name, k});
    };
    add("none", [](MsmKnobs&) {});
    add("SLICE=2", [](MsmKnobs& k) { k.slice = 2; });
    add("SLICE=96", [](MsmKnobs& k) { k.slice = 96; });
    static const char* const glog_names[7] = {"GLOG=0", "GLOG=1", "GLOG=2", "GLOG=3", "GLOG=4", "GLOG=5", "GLOG=6"};
    for (int v = 0; v <= 6; ++v) add(glog_names[v], [v](MsmKnobs& k) { k.glog = knob(v); });
    add("WINDOW_TF=9", [](MsmKnobs& k) { k.window_tf = knob(9); });
    add("NO_GLV", [](MsmKnobs& k) { k.no_glv = true; });
    add("ORDER_V1", [](MsmKnobs& k) { k.order_v1 = true; });
    add("WINDOW_2P14=13", [](MsmKnobs& k) { k.window_2p14 = knob(13); });
    add("WINDOW=13", [](MsmKnobs& k) { k.window = knob(13); });
    std::vector<size_t> ns = {0, 1, 2, 3, 31, 1000, 6000, 349525, 1000003};
    for (int k = 10; k <= 24; ++k)
        for (int d = -1; d <= 1; ++d) ns.push_back(((size_t)1 << k) + d);
    const unsigned windows[] = {0, 2, 3, 11, 12, 13, 16, 17, 19, 20, 21, 22};
    Report r;
    for (const Setting& s : settings)
        for (int curve = 0; curve < 5; ++curve)
            for (int tf = 0; tf < 2; ++tf)
                for (size_t mul : {1, 2, 4}) {
                    Case c{curve, 0, 0, tf != 0, (size_t)128 * 256 * mul, s.k, s.name};
                    for (size_t n : ns)
                        for (unsigned w : windows) {
                            c.n = n;
                            c.window_bits = w;
                            check(c, r);
                        }
                    c.n = (size_t)1 << 20;
                    c.window_bits = 0;
                    check_halving(c, 0, r);
                    check_halving(c, 2, r);
                }
    if (rows) *rows = r.rows;
    if (refused) *refused = r.refused;
    if (msg && msg_len) snprintf(msg, msg_len, "%s", r.first);
    return r.violations;
}

// the window a context over n generators gets when none is asked for (no knobs), or -1
extern "C" int msm_geom_auto_window(int curve, size_t n, int table_free) {
    if (curve < 0 || curve >= 5) return -1;
    MsmGeom g;
    return msm_geometry(curve, n, 0, table_free != 0, (size_t)128 * 256, limbs_of(curve), raw_u4_of(curve), MsmKnobs{}, &g) == PLK_OK ? g.c : -1;
}

#ifdef MSM_GEOM_HOST_MAIN
int main() {
    long rows = 0, refused = 0;
    char msg[256];
    const long bad = msm_geom_check_grid(&rows, &refused, msg, sizeof msg);
    printf("%ld geometries (%ld refused), %ld violations%s%s\n", rows, refused, bad, bad ? ": " : "", msg);
    return bad ? 1 : 0;
}
#endif
