// msm_geom.h -- the geometry of an MSM context as a pure value: window, bucket and partition counts, the reduction's shape, the
// accumulation's chunking and the sizes of the workspace parts, all from (curve, n, window, mode, knobs).  Plain C++ (no HIP type,
// no device call, no getenv, no static state): hipcc compiles it into the library (msm.hip; msm_dev.cuh includes it for the
// kernels' translation units) and g++ into the host test (tests/msm_geom_host.cpp), like the *_step.cuh replays and hostnorm.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/plonky_hip.h"
#include "glv_params.cuh"

namespace plk {

constexpr int ACC_THREADS = 128;

// ---- geometry shared by the host side (msm.hip) and the kernels' translation units (msm_order.hip, msm_tail.hip) ----
constexpr int MSM_MAX_PLANE_PARTS = 16;  // blocks per bit-plane in the reduction (planes * parts quads must fit the final block)
constexpr int MSM_TF_MAX_WINDOW = 16;  // table-free mode: every window has its own 2^(c-1) buckets
constexpr int MSM_MAX_WINDOW = 21;   // c - 1 <= 10 coarse + 11 fine bits in the partition (ORD_MAX_BINS, ORD_MAX_FINE)
constexpr uint32_t CODE_INVALID = 0xFFFFFFFFu;
constexpr int ORD_THREADS = 256;
constexpr int ORD_TILE = 4096;      // entries staged per tile of the level-1 scatter
constexpr int ORD_MAX_BINS = 1024;  // coarse bins
constexpr int ORD_MAX_FINE = 11;    // fine bits: buckets per coarse bin <= 2048
constexpr int ORD_BIN_THREADS = 512;
constexpr uint32_t ORD_SEG = 8192;  // entries per level-2 workgroup
constexpr int ORD_SEG_EPT = (int)(ORD_SEG / ORD_BIN_THREADS);  // ... and per thread of it
// k_ord_bin_scatter stages a whole segment in LDS (3 fine-bit tables + the staged entries): ~74 KB, above the 64 KB a workgroup
// gets on gfx90a / gfx942 - this library is built for gfx950 (160 KB of LDS per CU) only, plk_init refuses other devices
static_assert(3 * (4u << ORD_MAX_FINE) + 4 * ORD_BIN_THREADS + 6 * ORD_SEG <= 160 * 1024, "k_ord_bin_scatter's LDS tile must fit a gfx950 CU");
constexpr uint32_t ORD2_BIN_CAP = 32768;  // round 6 (k_ord_bin_sort): entries of a coarse bin that are ordered inside LDS by one workgroup (128 KiB)
constexpr int PLANE_THREADS = 512;
constexpr int FINAL_FUSE_WINDOWS = 4;  // up to this many tail windows are added by the last block of k_msm_final itself
constexpr int FINAL_THREADS = 512;  // <= 8 waves, so the compiler may use 256 VGPRs: the point arithmetic must not spill
constexpr int COMBINE_THREADS = 512;
constexpr uint32_t HEAD_NONE = 0xFFFFFFFFu;
constexpr uint32_t HEAVY_HEADS = 32;   // more head pieces than this PER LANE of k_msm_assemble (2^lpb_log lanes per bucket): the bucket is summed by workgroups
constexpr uint32_t HEAVY_CHUNK = 2048;

struct OrdCfg {
    int c;                   // window bits
    int windows;             // digits per scalar
    uint32_t window_buckets; // table-free mode: 2^(c-1) (every window has its own bucket range), else 0
    int fine_bits;           // bucket id = [coarse bin | fine]
    int nbins;               // coarse bins in use
    uint32_t spt;            // scalars per sub-tile (<= ORD_THREADS, spt * windows <= ORD_TILE)
    uint32_t sub;            // sub-tiles per tile (one block walks them in turn)
    uint32_t nt1;            // tiles
    int raw_signed;          // 1: the "scalars" are half scalars of a GLV split: canonical magnitude, sign in bit 255 (glv.cuh)
    uint32_t entries_cap;    // n_eff * windows: size of tmp[] / sorted[] and of the table (checked build)
    uint32_t ent_stride;     // entry id of (window j, scalar i) = j * ent_stride + ent_first + i: the table index.  ent_stride = n_eff of the
    uint32_t ent_first;      // context; ent_first > 0 when the scalars belong to generators first .. first + n - 1 only (plk_msm_execute_parts_dev)
    // round 6: 1 = the tile-major level 1 (k_ord_tiles, msm_order.hip) with the coarse bin taken from the LOW bits of the bucket id: the
    // buckets are ordered (and numbered, for everything downstream) by v = [low coarse bits | high fine bits] of the digit's bucket
    // b = |d| - 1, so that a short top window - whose digits are all small - spreads over every bin instead of filling the first few.
    // The reduction reads the weight of v off its two halves (TailGeom::transposed).
    int perm;
    // round 6: only entries whose coarse bin lies in [bin_lo, bin_hi) are kept (0, nbins: all of them).  A rank of a device group that
    // takes a BUCKET range of a sharded vector - every rank reads the whole vector and keeps its N-th of the bins - orders, accumulates
    // and reduces an N-th of the entries over an N-th of the buckets (plk_msm_execute_parts_buckets_dev).
    uint32_t bin_lo, bin_hi;
};

// what the reduction's launches need of a context (msm_tail.hip: msm_launch_reduce_stage)
struct TailGeom {
    uint32_t buckets, heavy_cap, tail_wbuckets;
    int lpb_log;             // lanes per bucket in k_msm_assemble
    int two_level;           // many buckets: row / column sums of the 2^H x 2^L bucket grid first
    int L, H, g_log, lpl_log;
    int table_free, windows;
    int tail_windows;        // windows seen by the plane kernels (two per real window in two-level mode: columns, rows)
    int plane_blocks;        // blocks (parts) per plane
    int planes;
    int tail_shift;          // doublings between consecutive tail windows
    // 1: bucket slot v = lo * 2^H + hi holds the bucket of weight hi * 2^L + lo + 1 (OrdCfg::perm): the grid in memory is 2^L rows of
    // 2^H slots, its ROW sums are the column sums C_lo of the weighting and its column sums the row sums R_hi
    int transposed;
    // 1: some vector of the batch is a BUCKET share (OrdCfg::bin_lo / bin_hi): its entries are spread over all the accumulation lanes in
    // chains shorter than a bucket, so most lanes end inside a bucket and the list of live head pieces is long - k_msm_heads gets a grid of
    // 2048 blocks instead of 512.  A property of the call, not of the context: 0 in MsmGeom::tail, set on the copy a reduction is launched with.
    int many_heads;
};

// ---- the `meta` part of a workspace, in 32-bit words: the ordering's bin tables, then the counters the kernels hand to each other ----
constexpr int META_BIN_TOTAL = 0;                                  // bin_total[ORD_MAX_BINS]
constexpr int META_BIN_BASE = META_BIN_TOTAL + ORD_MAX_BINS;       // bin_base[ORD_MAX_BINS + 1]
constexpr int META_SEG_BASE = META_BIN_BASE + ORD_MAX_BINS + 1;    // seg_base[ORD_MAX_BINS + 1]
constexpr int META_DONE = META_SEG_BASE + ORD_MAX_BINS + 1;        // the "last block" counter of k_ord_scan1
constexpr int META_FINAL_DONE = META_DONE + 1;                     // windows finished by k_msm_final
constexpr int META_DYN_CHUNK = META_DONE + 2;                      // entries per accumulation lane of this execution
constexpr int META_LIVE_COUNT = META_DONE + 3;                     // length of the list of live head pieces
constexpr int META_WORDS = META_DONE + 8;

// the parts of a workspace slab, in the order they are laid out
enum MsmPart {
    PART_TMP,         // uint2 (code, entry id) ordered by coarse bin
    PART_SORTED,      // (entry id << 1 | negative) ordered by bucket
    PART_CNT1,        // [nbins][nt1]
    PART_CNT2,        // [segment][fine]
    PART_META,        // META_* above
    PART_OFF,         // off[buckets + 1]
    PART_P_START,     // raw pieces, one per bucket
    PART_P_HEAD,      // raw pieces, one per accumulation lane
    PART_HEAD_LIVE,   // one flag byte per lane, then the lanes' head buckets (4 bytes each), then the list of live lanes (4 bytes each)
    PART_BUCKET,      // packed points: operands of the plane sums
    PART_HEAVY,       // heavy-bucket work list (see k_msm_heavy_list)
    PART_HEAVY_PART,
    PART_LINE_PART,   // two-level tail: row / column partial sums
    PART_PLANE_PART,
    PART_WIN_PTS,     // the per-window results
    MSM_WORK_PARTS
};

// head_live[] (bytes), head_bucket[] (words, at 1 x this offset) and live_list[] (words, at 5 x) share PART_HEAD_LIVE
inline size_t head_lanes_padded(size_t max_lanes) { return (max_lanes + ACC_THREADS + 15) & ~(size_t)15; }

// The environment's knobs as values (msm.hip: msm_knobs_from_env reads them).  An integer knob is atoi of its variable when that is set.
struct MsmKnob {
    bool set = false;
    int v = 0;
};
struct MsmKnobs {
    MsmKnob window;       // PLK_MSM_WINDOW: the tabled window, whatever the size
    MsmKnob window_2p14;  // PLK_MSM_WINDOW_2P14: ... of 2^14 <= n < 2^15 alone (the IPA's frozen generators)
    MsmKnob window_tf;    // PLK_MSM_WINDOW_TF: the table-free window
    MsmKnob glog;         // PLK_MSM_GLOG: log2 of the lines a row / column partial sum covers
    int slice = 0;        // PLK_MSM_SLICE: entries per accumulation lane when in [2, 4096] (0: not set)
    int comb = -1;        // PLK_MSM_COMB: 0 never a comb, > 0 a comb up to COMB_MAX_N generators, < 0 (not set) by size
    bool no_glv = false;    // PLK_MSM_NO_GLV
    bool order_v1 = false;  // PLK_MSM_ORDER_V1: round 5's ordering kernels everywhere
};

struct MsmGeom {
    int c = 0;          // window bits
    int windows = 0;    // ceil((BITS + 1) / c)
    uint32_t buckets = 0;   // bucket slots: 2^(c-1) with tables; windows * 2^(c-1) (rounded up to whole partition bins) without
    uint32_t wbuckets = 0;  // 2^(c-1): buckets per window
    bool table_free = false;  // no window tables: every window has its own buckets and is doubled into place at the end
    bool glv = false;         // table-free mode on a curve with the endomorphism: 2n points, half-length scalars (glv.cuh)
    size_t n_eff = 0;         // points the kernels see: 2n with glv, else n
    OrdCfg ord{};
    TailGeom tail{};
    uint32_t chunk = 24;      // entries per accumulation lane
    size_t max_lanes = 0;     // upper bound of the accumulation lanes of an execution
    uint32_t heavy_cap = 0;
    size_t part_bytes[MSM_WORK_PARTS] = {};  // what every part of a workspace needs
    char error[192] = {};     // msm_geometry's refusal, for the caller's set_error
};

constexpr int msm_scalar_bits(int curve) {  // bits of the scalar field's modulus (msm.hip checks them against the curve structs)
    return curve == PLK_CURVE_BLS12_377 ? 253 : (curve >= PLK_CURVE_TWEEDLEDEE && curve <= PLK_CURVE_VESTA) ? 255 : -1;
}

inline int ilog2_ceil(uint64_t v) {
    int b = 0;
    while (((uint64_t)1 << b) < v) ++b;
    return b;
}

inline int choose_window(size_t n, int curve, const MsmKnobs& knobs) {
    int lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) ++lg;
    const int bits = msm_scalar_bits(curve) + 1;
    auto digits = [&](int c) { return (bits + c - 1) / c; };
    auto top_bits = [&](int c) { return bits - (digits(c) - 1) * c; };
    int c;
    if (lg >= 14) {
        // From 2^14 generators on the window minimises a count of field multiplications: digits(c) mixed additions per scalar
        // (10 each) + two full additions per bucket in the reduction (14 each) + a tenth on top of the accumulation when the TOP
        // WINDOW IS SHORT (fewer than c / 2 bits: every scalar's top digit lands in a handful of buckets, which go through the
        // heavy-bucket path - ~120 us of workgroup-wide sums whatever the size; 24 windows of 11 leave the top one 3 bits, 18
        // of 15 one bit).  Measured in round 3 (profiles/r03_commit9_scaling.txt, r03_window_sweeps.txt): 2^14: 13 (0.41 ms
        // against 0.52 at 11), 2^16 / 2^17 / 2^18: 16 (0.53 against 0.68 at 14; 0.88 against 1.01 at 18), 2^19 (BLS12-377): 17,
        // 2^20 and up: 20 (13 additions per scalar, 2^19 buckets: round 2).  Round 6 (the list-driven assembly, tools/gpu/r06_small_msm2.sh,
        // profiles/r06_small_msm_windows.txt): at 2^14 the count is no longer the measure - every stage is a chain of a few point operations -
        // and 16 wins (two vectors: 0.442 ms against 0.481 at 13; one bucket piece per lane, so no k_msm_assemble tree), with a smaller table.
        double best = 0;
        c = 0;
        for (int t = 10; t <= MSM_MAX_WINDOW - 1; ++t) {
            const double acc = 10.0 * (double)n * digits(t);
            const double cost = acc + 28.0 * (double)((size_t)1 << (t - 1)) + (2 * top_bits(t) < t ? 0.1 * acc : 0.0);
            if (c == 0 || cost < best) {
                best = cost;
                c = t;
            }
        }
        if (lg == 14) {
            c = 16;
            if (knobs.window_2p14.set) c = knobs.window_2p14.v;  // A/B of this size alone (the IPA's frozen generators)
        }
    } else {
        c = lg - 4;
        if (c < 3) c = 3;
        // the smallest window with the same number of digits (fewer buckets for the same additions) ...
        while (c > 3 && digits(c - 1) == digits(c)) --c;
        // ... unless that leaves the top window short: then the next width whose top window holds at least half a window
        for (int t = c; t <= c + 4 && t <= 16; ++t)
            if (2 * top_bits(t) >= t) {
                c = t;
                break;
            }
    }
    if (knobs.window.set) c = knobs.window.v;
    if (c < 3) c = 3;
    if (c > MSM_MAX_WINDOW) c = MSM_MAX_WINDOW;
    return c;
}

// table-free window: windows * 2^(c-1) bucket slots, long chunks wanted.  A top window of one or two bits (131 = 13 * 10 + 1)
// would put every scalar's top digit into a handful of buckets: a neighbouring width is taken instead.
inline int choose_window_table_free(size_t n, int bits, const MsmKnobs& knobs) {
    int lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) ++lg;
    int c = lg - 5;
    if (c < 3) c = 3;
    if (c > MSM_TF_MAX_WINDOW) c = MSM_TF_MAX_WINDOW;
    auto top = [&](int w) { return bits - ((bits + w - 1) / w - 1) * w; };
    if (top(c) < 3) {
        if (c + 1 <= MSM_TF_MAX_WINDOW && top(c + 1) >= 3) c = c + 1;
        else if (c - 1 >= 3 && top(c - 1) >= 3) c = c - 1;
    }
    if (knobs.window_tf.set) c = knobs.window_tf.v;
    if (c < 3) c = 3;
    if (c > MSM_TF_MAX_WINDOW) c = MSM_TF_MAX_WINDOW;
    return c;
}

// The geometry of a context over n generators of `curve`: window (window_bits, or chosen when that is 0), ordering configuration,
// tail geometry, the accumulation's chunking for `slots` lanes running at once, and the bytes of every workspace part for
// coordinates of `limbs` 32-bit words and raw points of `raw_u4` uint4.  PLK_OK, or PLK_ERR_INVALID_ARG with the reason in out->error.
inline int msm_geometry(int curve, size_t n, unsigned window_bits, bool table_free, size_t slots, int limbs, int raw_u4, const MsmKnobs& knobs,
                        MsmGeom* out) {
    MsmGeom g;
    auto refuse = [&](const char* fmt, auto... args) {
        snprintf(g.error, sizeof g.error, fmt, args...);
        *out = g;
        return PLK_ERR_INVALID_ARG;
    };
    const int scalar_bits = msm_scalar_bits(curve);
    if (scalar_bits < 0) return refuse("bad curve id %d", curve);
    // table-free mode on the prime-order curves: split every scalar along the endomorphism (glv.cuh) - 2n points, half the windows
    const bool glv = table_free && n > 0 && curve != PLK_CURVE_BLS12_377 && !knobs.no_glv;
    const size_t n_eff = glv ? 2 * n : n;
    const int bits = (glv ? GLV_BITS : scalar_bits) + 1;
    const int c = window_bits ? (int)window_bits : (table_free ? choose_window_table_free(n_eff ? n_eff : 1, bits, knobs) : choose_window(n ? n : 1, curve, knobs));
    if (c < 2 || c > MSM_MAX_WINDOW) return refuse("window_bits %d outside [2, %d]", c, MSM_MAX_WINDOW);
    const int windows = (bits + c - 1) / c;
    if (table_free && c > MSM_TF_MAX_WINDOW)
        return refuse("table-free mode: window_bits %d above %d", c, MSM_TF_MAX_WINDOW);
    if (table_free) {
        // bit-plane reduction over the buckets themselves up to 12 bits, the two-level reduction per window above
        const size_t slot_limit = c - 1 >= 12 ? (size_t)ORD_MAX_BINS << ORD_MAX_FINE : 65536;
        const int window_limit = c - 1 >= 12 ? COMBINE_THREADS / 8 : COMBINE_THREADS / 4;
        if (((size_t)windows << (c - 1)) > slot_limit || windows > window_limit)
            return refuse("table-free mode: window_bits %d gives %d windows x %d buckets (limits: %zu slots, %d windows)", c, windows, 1 << (c - 1),
                          slot_limit, window_limit);
    }
    if (n_eff * (size_t)windows >= ((size_t)1 << 31))
        return refuse("n * windows = %zu entries exceeds 2^31", n_eff * (size_t)windows);
    g.table_free = table_free;
    g.glv = glv;
    g.n_eff = n_eff;
    g.c = c;
    g.windows = windows;
    g.wbuckets = 1u << (c - 1);
    OrdCfg& o = g.ord;
    {
        // partition geometry from the number of bucket slots: <= 512 coarse bins (one workgroup each at level 2), the rest fine
        const uint32_t want = table_free ? g.wbuckets * (uint32_t)windows : g.wbuckets;
        const int slot_bits = ilog2_ceil(want);
        // up to 2^10 bucket slots: ONE level - the coarse bins are the buckets, the first level's output is the bucket order
        int coarse = slot_bits <= 10 ? slot_bits : 9;
        if (slot_bits - coarse > ORD_MAX_FINE) coarse = slot_bits - ORD_MAX_FINE;
        o.c = c;
        o.windows = windows;
        o.window_buckets = table_free ? g.wbuckets : 0u;
        o.fine_bits = slot_bits - coarse;
        o.nbins = (int)((want + (1u << o.fine_bits) - 1) >> o.fine_bits);
        g.buckets = (uint32_t)o.nbins << o.fine_bits;
        o.spt = (uint32_t)(ORD_TILE / windows);
        if (o.spt > (uint32_t)ORD_THREADS) o.spt = ORD_THREADS;
        o.sub = n_eff >= ((size_t)1 << 16) ? 4 : 1;
        o.nt1 = (uint32_t)((n_eff + (size_t)o.spt * o.sub - 1) / ((size_t)o.spt * o.sub));
        if (o.nt1 == 0) o.nt1 = 1;
        o.raw_signed = glv ? 1 : 0;
        o.entries_cap = (uint32_t)(n_eff * (size_t)windows);
        o.ent_stride = (uint32_t)n_eff;
        o.ent_first = 0;
        // round 6: the tile-major level 1 with the bins taken from the LOW bits of the bucket number (OrdCfg::perm) - tabled contexts whose
        // buckets split into at least as many fine as coarse bits (c = 19 .. 21: the 2^19 generators and up that get such windows), tiles
        // of 1024 scalars, records of at most 16 windows.  PLK_MSM_ORDER_V1 keeps round 5's kernels (A/B, tests/test_gpu_knobs.py).
        // ... and a bin's expected share of the entries fits the LDS of k_ord_bin_sort with 15 % to spare (2^20 scalars of 13 windows over 512
        // bins: 26.6 k of 32 k; larger problems keep round 5's kernels, hot bins of a skewed vector take the segmented ones).
        const bool bins_fit = (double)n_eff * windows / (double)o.nbins * 1.15 <= (double)ORD2_BIN_CAP;
        o.bin_lo = 0;
        o.bin_hi = (uint32_t)o.nbins;
        o.perm = (!knobs.order_v1 && !table_free && coarse == 9 && o.fine_bits >= coarse && o.nbins == (1 << coarse) && o.sub == 4 && o.spt * o.sub == 1024u &&
                  windows <= 16 && o.nt1 <= 2048u && bins_fit)
                     ? 1
                     : 0;
    }
    // tail geometry
    TailGeom& t = g.tail;
    t.buckets = g.buckets;
    t.table_free = table_free ? 1 : 0;
    t.windows = windows;
    t.transposed = o.perm;
    t.two_level = c - 1 >= 12 ? 1 : 0;
    t.L = t.H = t.g_log = t.lpl_log = 0;
    if (t.two_level) {
        t.L = (c - 1) / 2;
        t.H = c - 1 - t.L;
        if (o.perm) {
            // the bucket slots are numbered [coarse bin = LOW bits of the bucket | fine = its high bits]: the weighting splits where the
            // ordering does (TailGeom::transposed)
            t.L = c - 1 - o.fine_bits;
            t.H = o.fine_bits;
        }
        t.g_log = c - 1 >= 17 ? 3 : 2;
        if (knobs.glog.set) t.g_log = knobs.glog.v;
        if (t.g_log > t.L) t.g_log = t.L;
        if (t.g_log < 0) t.g_log = 0;
        const int longest = t.H - t.g_log;  // log2 of the partials per column (rows have L - g_log <= that)
        t.lpl_log = longest < 4 ? longest : 4;  // quads per line
        t.tail_windows = table_free ? 2 * windows : 2;  // per real window: its column sums, then its row sums
        t.tail_wbuckets = 1u << t.H;
        t.tail_shift = c;  // between real windows (table-free mode); the row sums of a window weigh 2^L more (k_msm_final)
        t.planes = t.H;  // weights up to 2^H - 1 (rows) / 2^L (columns): plane H - 1 is the top one for rows; columns need bit L <= H - 1 or L == H
        if (t.L == t.H) t.planes = t.H + 1;  // column weight 2^L = 2^H needs plane H
    } else {
        t.tail_windows = table_free ? windows : 1;
        t.tail_wbuckets = g.wbuckets;
        t.tail_shift = c;
        t.planes = c;
    }
    t.plane_blocks = 1;
    while (t.plane_blocks < MSM_MAX_PLANE_PARTS && (uint32_t)t.plane_blocks * 512u < t.tail_wbuckets &&
           t.planes * t.plane_blocks * 4 <= FINAL_THREADS)  // after doubling: planes * parts / 2 quads in the final block
        t.plane_blocks *= 2;
    // entries per accumulation lane and what follows from it (lanes, heavy-bucket capacity, lanes per bucket in k_msm_assemble)
    const size_t entries = n_eff * windows;
    {
        // whole rounds of the lanes the GPU holds, at most 72 entries each (longer chunks: fewer pieces)
        const double per_slot = (double)entries / (double)slots;
        size_t rounds = (size_t)(per_slot / 72.0 + 0.999);
        if (rounds < 1) rounds = 1;
        size_t ch = (size_t)(per_slot / (double)rounds + 0.999);
        if (ch < 8) ch = 8;
        if (ch > 96) ch = 96;
        g.chunk = (uint32_t)ch;
        if (knobs.slice >= 2 && knobs.slice <= 4096) g.chunk = (uint32_t)knobs.slice;
    }
    g.max_lanes = entries / g.chunk + 2;
    // at most max_lanes / HEAVY_HEADS heavy buckets, max_lanes / HEAVY_CHUNK + that many chunk items
    g.heavy_cap = t.heavy_cap = (uint32_t)(g.max_lanes / HEAVY_HEADS + g.max_lanes / HEAVY_CHUNK + 2);
    {
        // lanes per bucket in k_msm_assemble: from the expected number of head pieces per bucket
        const double heads = (double)entries / (double)g.buckets / (double)g.chunk;
        t.lpb_log = heads > 6.0 ? 3 : heads > 2.0 ? 2 : 0;
    }
    // the workspace
    const size_t packed_bytes = (size_t)4 * limbs * 4;
    const size_t raw_bytes = (size_t)raw_u4 * 16;
    // packed operands of the plane sums: the buckets themselves, or (two-level tail) the column and row sums
    const size_t tail_slots = t.two_level ? (size_t)t.tail_windows * t.tail_wbuckets : (size_t)g.buckets;
    size_t* p = g.part_bytes;
    p[PART_TMP] = entries * 8 + 16;
    p[PART_SORTED] = entries * 4 + 16;
    p[PART_CNT1] = (size_t)o.nbins * o.nt1 * 4;
    p[PART_CNT2] = ((entries / ORD_SEG + o.nbins + 1) << o.fine_bits) * 4;
    p[PART_META] = (size_t)META_WORDS * 4;
    p[PART_OFF] = ((size_t)g.buckets + 2) * 4;
    p[PART_P_START] = (size_t)g.buckets * raw_bytes;
    p[PART_P_HEAD] = (g.max_lanes + 1) * raw_bytes;
    p[PART_HEAD_LIVE] = 9 * head_lanes_padded(g.max_lanes);
    p[PART_BUCKET] = tail_slots * packed_bytes;
    p[PART_HEAVY] = (size_t)(2 + 3 * g.heavy_cap) * 4;
    p[PART_HEAVY_PART] = (size_t)g.heavy_cap * raw_bytes;
    p[PART_LINE_PART] = t.two_level ? (size_t)2 * (g.buckets >> t.g_log) * raw_bytes : 0;
    p[PART_PLANE_PART] = (size_t)t.tail_windows * t.planes * t.plane_blocks * packed_bytes;
    p[PART_WIN_PTS] = t.tail_windows > 1 ? (size_t)t.tail_windows * packed_bytes : 0;
    *out = g;
    return PLK_OK;
}

}  // namespace plk
