// msm.hip -- multi-scalar multiplication sum_i s_i * G_i on gfx950 (bucket method on window tables).
//
// Replaces the reference's src/curve/curve_msm.rs (+ curve_summations.rs, curve_adds.rs):
//   msm_precompute / precompute_single_generator  curve_msm.rs:27-52  -> k_msm_table (device tables)
//   to_digits                                     curve_msm.rs:159-180 -> ord_digit (signed, carry based; recomputed where used)
//   digit_occurrences scatter (serial in the ref) curve_msm.rs:117-126 -> two-level LDS partition (k_ord_*)
//   per-digit affine multi-summation              curve_msm.rs:131-145 -> k_msm_accumulate (XYZZ mixed adds, equal chunks)
//   serial Yao tail  u += acc[d]; y += u          curve_msm.rs:149-154 -> k_msm_assemble + k_msm_gsum/lsum + k_msm_planes + k_msm_final
//   msm_execute / msm_execute_parallel            curve_msm.rs:63-157  -> msm_execute_dev_impl
//   msm_parallel (precompute + execute, one use)  curve_msm.rs:54-61   -> the table-free mode (PLK_MSM_TABLE_FREE)
// Same mathematical structure as the reference (Yao's method over per-generator power tables
// [2^(c j)] G_i, one bucket per digit value, result = sum_d d * bucket_d) with two MI355X-first
// changes: (1) digits are signed (carry-based integer recoding, never s -> r - s, so it is valid
// on BLS12-377 G1 whose cofactor is even): half the buckets for the same window; (2) the serial
// running sum is replaced by a two-level weighting (row / column sums of the bucket grid) followed by
// bit-plane tree sums (sum_d d B_d = sum_p 2^p sum_{d: bit p} B_d), so the tail is O(log) deep instead of
// 2 * 2^w sequential additions and costs 2 additions per bucket - which is what makes windows of 18-20 bits
// (13 additions per scalar at 2^20) affordable.  The result is returned as
// the unique affine point (to_affine, curve.rs:206-214), on which parity is defined.
//
// Work decomposition: every (scalar i, window j) with a non-zero digit is one *entry* that adds
// +-table[j*n + i] into bucket |d|-1.  Entries are counting-sorted by bucket; the sorted list is cut
// into equal chunks and one lane accumulates one chunk (storing a piece at every bucket boundary), so the
// load per lane is the same whatever the digit distribution (a skewed witness cannot serialise the kernel).
//
// Table-free mode (generators used once): only the generators themselves are stored; window j gets its own
// bucket range [j 2^(c-1), (j+1) 2^(c-1)), the same kernels run over all windows at once, every window's
// sum (plane sums over its buckets up to 12 bits, over its row / column sums above) is doubled into place (2^(c j)) by a
// quad and k_msm_combine adds the windows.  On the prime-order curves the scalars are split along the endomorphism first
// (glv.cuh): 2n points [G.., phi(G)..], half-length scalars, half the windows - half of that doubling chain.
// Batches: every MSM of a group has its own workspace and the group shares one reduction (msm_execute_dev_impl).
// The reduction kernels run on quads of lanes (ecz_coop.cuh): they are chains of point operations, i.e. latency.
// This file: the table kernels and the host side (contexts, workspaces, precompute / rebind / execute).  Everything a context's shape
// follows from - window, partition, reduction geometry, chunking, workspace sizes - is one pure function, msm_geometry (msm_geom.h).
#include <mutex>
#include <type_traits>
#include <vector>

#include "msm_dev.cuh"  // msm_geom.h: the constants, OrdCfg / TailGeom, MsmGeom and msm_geometry
#include "glv.cuh"
#include "ecz_coop.cuh"
#include "tables.cuh"

namespace plk {

constexpr size_t COMB_MAX_N = (size_t)1 << 15;  // generators up to which a tabled context with an automatic window is a comb (1 GB of table at 2^15)
constexpr size_t COMB_AUTO_MAX_N = (size_t)1 << 12;  // ... and up to which it is chosen without being asked for (measured faster than the bucket method)
constexpr int COMB_WINDOW = 4, COMB_WINDOWS = 64;



// ---------------------------------------------------------------------------------------------
// table construction: tab[j*n + i] = [2^(c j)] G_i, affine  (curve_msm.rs:40-52)
// ---------------------------------------------------------------------------------------------
// The table is what the accumulation kernel multiplies with, so it is stored in the working form of
// that kernel (ecz.cuh / fz.cuh): coordinates in R'-form (x 2^(29 NZ)), canonical, packed in the
// same 32-bit words.  The generators arrive in the reference's R-form.
// One lane per generator, on the lazy arithmetic of the accumulation kernel (ecz.cuh): c doublings per window,
// then back to affine with the division-step inversion (about a quarter of a window's work).
// glv != 0 (table-free mode on the curves with the endomorphism, glv.cuh): tab[n + i] = phi(G_i) = (beta x, y).
// The generators may come in two pieces: n_main points at `bases` (+ optional identity flags) followed by n - n_main points at
// `extra` (an IPA round appends H and U' to the half of G it multiplies, halo.rs:86-93).
template <class C>
__global__ void __launch_bounds__(128) k_msm_table(const uint4* __restrict__ bases, const uint8_t* __restrict__ base_zero, uint4* __restrict__ tab,
                                                   size_t n, int c, int windows, int glv, size_t n_main, const uint4* __restrict__ extra) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // R-form (the reference's) -> canonical R'-form, the form the table is stored and consumed in
    const uint4* src = i < n_main ? bases + i * 2 * W : extra + (i - n_main) * 2 * W;
    const Fe<FP> x_in = fe_load<FP>(src);
    Fe<FP> xr = to_rprime<FP>(x_in), yr = to_rprime<FP>(fe_load<FP>(src + W));
    bool ident = (base_zero && i < n_main) ? base_zero[i] != 0 : false;
    affine_store<FP>(tab + i * 2 * W, xr, yr, ident);
    if constexpr (C::Glv::ENABLED) {
        if (glv) {
            Fe<FP> beta;
#pragma unroll
            for (int k = 0; k < FP::NL; ++k) beta.v[k] = C::Glv::BETA[k];
            const Fe<FP> xphi = to_rprime<FP>(fe_mul<FP>(x_in, fe_from_canonical<FP>(beta)));
            affine_store<FP>(tab + (n + i) * 2 * W, xphi, yr, ident);
        }
    }
    const Fz<FP> one = fz_one_rprime<FP>();
    for (int j = 1; j < windows; ++j) {
        if (!ident) {
            XyzzZ<FP> p;
            p.x = fz_from_fe<FP>(xr);
            p.y = fz_from_fe<FP>(yr);
            p.zz = one;
            p.zzz = one;
            p.inf = false;
            for (int k = 0; k < c; ++k) p = xyzzz_dbl<FP>(p);
            ident = p.inf;
            if (!ident) {
                // x = X / ZZ, y = Y / ZZZ with 1 / Z = ZZ / ZZZ (xyzz_to_affine, ec.cuh), all in R'-form
                const Fe<FP> zzz_r = fz_to_fe_canonical<FP>(fz_mul<FP>(p.zzz, fz_const_rprime_to_r<FP>()));
                const Fz<FP> i3 = fz_from_fe<FP>(to_rprime<FP>(fe_inv_safegcd<FP>(zzz_r)));
                const Fz<FP> iz = fz_mul<FP>(p.zz, i3);
                const Fz<FP> izz = fz_sqr<FP>(iz);
                xr = fz_to_fe_canonical<FP>(fz_mul<FP>(p.x, izz));
                yr = fz_to_fe_canonical<FP>(fz_mul<FP>(p.y, i3));
            }
        }
        affine_store<FP>(tab + ((size_t)j * n + i) * 2 * W, xr, yr, ident);
    }
}

// The reference's own table (MsmPrecomputation::powers_per_generator, curve_msm.rs:16-52): the device table
// [j][i] in R'-form becomes [i][j] in the reference's Montgomery form, with AffinePoint::zero flags.
template <class C>
__global__ void __launch_bounds__(256) k_msm_table_export(const uint4* __restrict__ tab, size_t n, int digits, uint4* __restrict__ out_xy,
                                                          uint8_t* __restrict__ out_zero) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // output slot i * digits + j
    if (e >= n * (size_t)digits) return;
    const size_t i = e / digits, j = e % digits;
    Fe<FP> x, y;
    const bool ident = affine_load<FP>(tab + (j * n + i) * 2 * W, x, y);
    const Fz<FP> back = fz_const_rprime_to_r<FP>();
    x = ident ? fe_zero<FP>() : fz_to_fe_canonical<FP>(fz_mul<FP>(fz_from_fe<FP>(x), back));
    y = ident ? fe_zero<FP>() : fz_to_fe_canonical<FP>(fz_mul<FP>(fz_from_fe<FP>(y), back));
    fe_store<FP>(out_xy + e * 2 * W, x);
    fe_store<FP>(out_xy + e * 2 * W + W, y);
    out_zero[e] = ident ? 1 : 0;
}

// Short generator lists (the frozen generators of an inner-product argument: 2^14 + 2 points): one lane per generator is a
// dependency chain, and in k_msm_table a quarter of it is the inversion that brings every window back to affine before the next
// c doublings.  Here the chain only doubles - c (windows - 1) doublings without a normalisation in between, every window's
// XYZZ point parked in scratch memory - and a second kernel normalises all (window, generator) pairs side by side:
// 1.75 -> 1.2 ms for 2^14 + 2 generators at c = 13 with a lane per generator, 0.65 ms on quads in one-wave workgroups (a chain of quad
// doublings takes 3.6 us per step in two-wave workgroups at this occupancy, 2.2 us in one-wave ones: tools/lab/mul_latency.hip).  Same points, so the same (unique) affine table entries.
template <class C>
__global__ void __launch_bounds__(64) k_msm_table_chain(const uint4* __restrict__ bases, const uint8_t* __restrict__ base_zero, uint4* __restrict__ tab,
                                                         uint4* __restrict__ raw, size_t n, int c, int windows, size_t n_main, const uint4* __restrict__ extra) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    constexpr int RU = raw_u4<FP>();
    // a quad per generator (ecz_coop.cuh): a doubling is 3 multiplications deep instead of 9
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const int ql = threadIdx.x & 3;
    if (i >= n) return;
    const uint4* src = i < n_main ? bases + i * 2 * W : extra + (i - n_main) * 2 * W;
    const Fe<FP> xr = to_rprime<FP>(fe_load<FP>(src)), yr = to_rprime<FP>(fe_load<FP>(src + W));
    const bool ident = (base_zero && i < n_main) ? base_zero[i] != 0 : false;
    if (ql == 0) affine_store<FP>(tab + i * 2 * W, xr, yr, ident);
    XyzzZ<FP> p = xyzzz_identity<FP>();
    if (!ident) {
        p.x = fz_from_fe<FP>(xr);
        p.y = fz_from_fe<FP>(yr);
        p.zz = fz_one_rprime<FP>();
        p.zzz = p.zz;
        p.inf = false;
    }
    for (int j = 1; j < windows; ++j) {
        for (int k = 0; k < c; ++k) p = xyzzz_dbl_q<FP>(p, ql);
        if (ql == 0) xyzzz_store_raw<FP>(raw + ((size_t)(j - 1) * n + i) * RU, p);
    }
}
template <class C>
__global__ void __launch_bounds__(64) k_msm_table_norm(const uint4* __restrict__ raw, uint4* __restrict__ tab, size_t n, int windows) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    constexpr int RU = raw_u4<FP>();
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)(windows - 1) * n) return;
    const XyzzZ<FP> p = xyzzz_load_raw<FP>(raw + t * RU);
    Fe<FP> xr = fe_zero<FP>(), yr = fe_zero<FP>();
    if (!p.inf) {
        // x = X / ZZ, y = Y / ZZZ with 1 / Z = ZZ / ZZZ (xyzz_to_affine, ec.cuh), all in R'-form
        const Fe<FP> zzz_r = fz_to_fe_canonical<FP>(fz_mul<FP>(p.zzz, fz_const_rprime_to_r<FP>()));
        const Fz<FP> i3 = fz_from_fe<FP>(to_rprime<FP>(fe_inv_safegcd<FP>(zzz_r)));
        const Fz<FP> iz = fz_mul<FP>(p.zz, i3);
        const Fz<FP> izz = fz_sqr<FP>(iz);
        xr = fz_to_fe_canonical<FP>(fz_mul<FP>(p.x, izz));
        yr = fz_to_fe_canonical<FP>(fz_mul<FP>(p.y, i3));
    }
    affine_store<FP>(tab + (n + t) * 2 * W, xr, yr, p.inf);   // entry (j, i) of the table sits at j n + i = n + t
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
}  // namespace plk

// per-execution device workspace; a batched execution owns one per MSM of a group
struct MsmWork {
    void* part[plk::MSM_WORK_PARTS] = {};  // the parts (MsmPart, msm_geom.h): pointers into the slab
    size_t cap[plk::MSM_WORK_PARTS] = {};  // bytes of each part (a context that is rebound to fewer points keeps its layout)
    void* slab = nullptr;      // the one allocation the parts point into
    bool pooled = false;       // slab comes from the library's scratch pool (table-free contexts: built and dropped per call)
    bool ready = false;
    // executions on different streams share the workspace: the next user waits for the previous one's last kernel
    hipEvent_t ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool used = false;
    uint32_t* meta(int word) const { return (uint32_t*)part[plk::PART_META] + word; }  // META_* (msm_geom.h)
    void release() {
        if (slab && pooled) plk::scratch_release(slab, last_stream);  // stream-ordered: the next taker waits for our last kernel
        else if (slab) (void)hipFree(slab);
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
        slab = nullptr;
        for (void*& p : part) p = nullptr;
        ready = false;
        used = false;
    }
};

struct plk_msm_ctx {
    int curve = 0;
    int device = 0;
    size_t n = 0;
    plk::MsmGeom geom;  // window, buckets, ordering and tail geometry, workspace sizes: everything that follows from (curve, n, mode)
    // device memory
    void* tab = nullptr;
    size_t tab_cap = 0;      // bytes allocated for the table
    hipStream_t tab_stream = nullptr;  // table-free: the stream the (pooled) table was built on
    std::vector<MsmWork> ws;   // ws[0] at precompute; a batched execution allocates one per MSM of a group (<= TAIL_MAX)
    size_t ws_bytes = 0;       // size of one workspace slab
    std::mutex mu;             // one enqueue at a time per context
    hipStream_t tail_stream = nullptr;  // batched executions: the reduction of vector k runs here, under the accumulation of vector k + 1
    hipEvent_t ev_tail = nullptr;
    std::vector<hipEvent_t> ev_acc;
    std::vector<hipStream_t> fork_streams;  // small batched executions: the ordering + accumulation of vector k >= 1 runs on fork_streams[k - 1]
    // optional per-kernel timing (HIP events on the launch stream) for bench.py's roofline
    bool profiling = false;
    static constexpr int N_STAGES = 7;  // order: count + scan | scatter | bins; accumulate; heavy + assemble + lines; planes; final
    std::vector<std::vector<hipEvent_t>> prof_sets;  // each N_STAGES + 1 events, recorded
    std::vector<std::vector<hipEvent_t>> prof_free;
    // A context built while the library runs over several devices (plk_init_devices; multi.hip) owns one context with the full
    // tables on every other logical device (peers[d - 1]) and, on every device d including this one, a context over that device's
    // contiguous share of the generators with the window such a share deserves (shards[d]): whole vectors of a batch run on the
    // full tables, a single MSM runs sharded by base range.
    std::vector<plk_msm_ctx*> peers, shards;
    // A tabled context over few generators (automatic window; <= COMB_AUTO_MAX_N by default, PLK_MSM_COMB) is a COMB (comb.hip): no window tables,
    // no workspaces, no bucket method - executions are mixed additions of table entries and a tree over the lanes' sums.
    plk::CombPlan* comb = nullptr;
    bool auto_window = false;
    ~plk_msm_ctx() {
        if (comb) plk::comb_free(comb);
        for (auto* v : {&peers, &shards})
            for (plk_msm_ctx* sub : *v)
                if (sub) {
                    (void)hipSetDevice(sub->device);
                    delete sub;
                }
        (void)hipSetDevice(device);
        if (tab && geom.table_free) {
            // pooled: hand it back ordered after the last kernel that read it (several user streams: wait for them here)
            hipStream_t last = tab_stream;
            int users = 0;
            for (MsmWork& w : ws)
                if (w.used) {
                    if (users++ && w.last_stream != last) (void)hipStreamSynchronize(last);
                    last = w.last_stream;
                }
            plk::scratch_release(tab, last);
        } else if (tab) {
            (void)hipFree(tab);
        }
        for (MsmWork& w : ws) w.release();
        if (tail_stream) {
            (void)hipStreamSynchronize(tail_stream);
            plk::stream_pool_release(tail_stream);
        }
        if (ev_tail) (void)hipEventDestroy(ev_tail);
        for (hipEvent_t e : ev_acc) (void)hipEventDestroy(e);
        for (hipStream_t st : fork_streams) {
            (void)hipStreamSynchronize(st);
            plk::stream_pool_release(st);
        }
        for (auto* v : {&prof_sets, &prof_free})
            for (auto& set : *v)
                for (hipEvent_t e : set) (void)hipEventDestroy(e);
    }
};

namespace plk {

// accumulation lanes the GPU runs at once (for the chunk size: whole rounds of lanes, no ragged last round)
template <class C> static size_t accumulate_slots() {
    static std::mutex mu;
    static size_t slots[64] = {};  // per device
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    size_t& s = slots[dev & 63];
    if (s == 0) {
        int per_cu = 0, cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        per_cu = msm_accumulate_blocks_per_cu<C>();
        s = (size_t)per_cu * ACC_THREADS * (size_t)cus;
    }
    return s;
}

// the scalar-field widths msm_geom.h carries are those of the curve structs
#define PLK_GEOM_BITS_CHECK(C) static_assert(msm_scalar_bits(C::CURVE_ID) == C::SP::BITS, "msm_scalar_bits");
PLK_FOR_EACH_CURVE(PLK_GEOM_BITS_CHECK)
#undef PLK_GEOM_BITS_CHECK

// The environment's knobs, read in one place: at every precompute and rebind, PLK_MSM_ORDER_V1 once per process.
static MsmKnobs msm_knobs_from_env() {
    auto knob = [](const char* name) {
        const char* e = getenv(name);
        return MsmKnob{e != nullptr, e ? atoi(e) : 0};
    };
    MsmKnobs k;
    k.window = knob("PLK_MSM_WINDOW");
    k.window_2p14 = knob("PLK_MSM_WINDOW_2P14");
    k.window_tf = knob("PLK_MSM_WINDOW_TF");
    k.glog = knob("PLK_MSM_GLOG");
    k.slice = knob("PLK_MSM_SLICE").v;
    if (const char* e = getenv("PLK_MSM_COMB")) k.comb = atoi(e);
    k.no_glv = getenv("PLK_MSM_NO_GLV") != nullptr;
    static const bool order_v1 = getenv("PLK_MSM_ORDER_V1") != nullptr;
    k.order_v1 = order_v1;
    return k;
}

// msm_geometry (msm_geom.h) for n generators of `curve` on the calling thread's device; a refusal becomes the thread's error text
static int msm_geometry_of(int curve, size_t n, unsigned window_bits, bool table_free, const MsmKnobs& knobs, MsmGeom* out) {
    const int rc = or_bad_curve(with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        return msm_geometry(curve, n, window_bits, table_free, accumulate_slots<C>(), C::FP::NL, raw_u4<typename C::FP>(), knobs, out);
    }), curve);
    return rc != PLK_OK && out->error[0] ? set_error(rc, "%s", out->error) : rc;
}

// One slab per workspace: a single hipMalloc / hipFree instead of a dozen (they dominate a one-shot msm_parallel).  Every part gets
// what the geometry asks for (MsmGeom::part_bytes), or what w.cap reserves for the other generator counts of a rebound context.
static int msm_alloc_work(plk_msm_ctx* ctx, MsmWork& w, hipStream_t stream) {
    size_t total = 0;
    for (int k = 0; k < MSM_WORK_PARTS; ++k) {
        if (w.cap[k] < ctx->geom.part_bytes[k]) w.cap[k] = ctx->geom.part_bytes[k];
        total += (w.cap[k] + 255) & ~(size_t)255;
    }
    ctx->ws_bytes = total + 256;
    // A table-free context lives for one call (msm_parallel, an IPA round): its memory comes from the scratch pool, because
    // hipMalloc + hipFree of a few hundred MB cost as much as a tenth of the MSM itself (0.4 ms of 3.8 at 2^20).
    w.pooled = ctx->geom.table_free;
    if (w.pooled) {
        w.slab = scratch_acquire(total + 256, stream);
        if (!w.slab) return PLK_ERR_OOM;
        w.last_stream = stream;
    } else {
        PLK_HIP_TRY(hipMalloc(&w.slab, total + 256));
    }
    uint8_t* cur = (uint8_t*)w.slab;
    for (int k = 0; k < MSM_WORK_PARTS; ++k) {
        w.part[k] = w.cap[k] ? cur : nullptr;
        cur += (w.cap[k] + 255) & ~(size_t)255;
    }
    // the "last block" counter of k_ord_scan1 and the heavy-list counters start at zero and are left at zero by their users
    // (on the caller's stream: a non-blocking stream is not ordered after the null stream)
    PLK_HIP_TRY(hipMemsetAsync(w.part[PART_META], 0, (size_t)META_WORDS * 4, stream));
    PLK_HIP_TRY(hipMemsetAsync(w.part[PART_HEAVY], 0, 8, stream));
    PLK_HIP_TRY(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    w.ready = true;
    return PLK_OK;
}

template <class C> static void msm_launch_table(plk_msm_ctx* ctx, const void* d_bases, const void* d_zero, const void* d_extra, size_t n_extra,
                                                hipStream_t stream) {
    const size_t n = ctx->n;
    const MsmGeom& g = ctx->geom;
    if (!n) return;
    static const bool no_split = getenv("PLK_MSM_TABLE_FUSED") != nullptr;
    if (!g.table_free && g.windows > 1 && n <= ((size_t)1 << 15) && !no_split) {
        constexpr size_t RAW = (size_t)raw_u4<typename C::FP>() * 16;
        const size_t entries = (size_t)(g.windows - 1) * n;
        if (uint4* raw = (uint4*)scratch_acquire(entries * RAW, stream)) {
            k_msm_table_chain<C><<<(unsigned)((4 * n + 63) / 64), 64, 0, stream>>>((const uint4*)d_bases, (const uint8_t*)d_zero, (uint4*)ctx->tab, raw, n,
                                                                                 g.c, g.windows, n - n_extra, (const uint4*)d_extra);
            k_msm_table_norm<C><<<(unsigned)((entries + 63) / 64), 64, 0, stream>>>(raw, (uint4*)ctx->tab, n, g.windows);
            scratch_release(raw, stream);
            return;
        }
        (void)hipGetLastError();  // no scratch memory: the fused kernel needs none
    }
    k_msm_table<C><<<(unsigned)((n + 127) / 128), 128, 0, stream>>>((const uint4*)d_bases, (const uint8_t*)d_zero, (uint4*)ctx->tab, n, g.c,
                                                                   g.table_free ? 1 : g.windows, g.glv ? 1 : 0, n - n_extra, (const uint4*)d_extra);
}

template <class C>
static int msm_precompute_t(plk_msm_ctx* ctx, const MsmKnobs& knobs, const void* d_bases, const void* d_zero, const void* d_extra, size_t n_extra,
                            hipStream_t stream, const size_t* also_n, int also_count) {
    using FP = typename C::FP;
    const size_t pt_bytes = (size_t)2 * FP::NL * 4;
    // Few generators with an automatic window are a COMB (comb.hip) - chosen BY SIZE since round 5: measured in round 4
    // (profiles/r04_comb_small_msm.txt) an execution takes 0.19 / 0.25 ms against 0.30 / 0.33 for the bucket method at 2^10 / 2^12
    // generators, the same at 2^14 and more at 2^15 (eight dependent gathers + additions per lane and two trees of full additions are
    // latency too), and its table costs 2-4 x the window tables to build: up to COMB_AUTO_MAX_N = 2^12 generators it is the default.
    // PLK_MSM_COMB=0 turns it off, PLK_MSM_COMB=1 forces it up to COMB_MAX_N (the parity suites run through it that way too).  The frozen
    // generators of an opening argument (2^14 + 2, explicit window) stay on the bucket method.
    const int comb_mode = knobs.comb;
    const bool want_comb = comb_mode > 0 || (comb_mode < 0 && ctx->n <= COMB_AUTO_MAX_N);
    if (!ctx->geom.table_free && ctx->auto_window && ctx->n >= 1 && ctx->n <= COMB_MAX_N && want_comb) {
        // the doubling chain [2^(4 j)] G_i on quads (window 0 affine in `base0`, the others raw in `raw`), then comb.hip turns every
        // window's point into its multiples 1 .. 8
        const size_t n = ctx->n;
        constexpr size_t RAW = (size_t)raw_u4<FP>() * 16;
        uint4* base0 = (uint4*)scratch_acquire(n * pt_bytes + 16, stream);
        uint4* raw = (uint4*)scratch_acquire((size_t)(COMB_WINDOWS - 1) * n * RAW + 16, stream);
        int rc = (base0 && raw) ? PLK_OK : PLK_ERR_OOM;
        if (rc == PLK_OK) {
            k_msm_table_chain<C><<<(unsigned)((4 * n + 63) / 64), 64, 0, stream>>>((const uint4*)d_bases, (const uint8_t*)d_zero, base0, raw, n, COMB_WINDOW,
                                                                                 COMB_WINDOWS, n - n_extra, (const uint4*)d_extra);
            if (hipGetLastError() != hipSuccess) rc = set_error(PLK_ERR_HIP, "comb chain launch failed");
        }
        if (rc == PLK_OK) rc = comb_build(ctx->curve, n, base0, raw, stream, &ctx->comb);
        if (raw) scratch_release(raw, stream);
        if (base0) scratch_release(base0, stream);
        // The comb's table is ~20 x the window tables it replaces (32 KiB per generator, 48 for BLS12-377: 128-192 MiB at 2^12).  A host
        // that holds many small contexts can run out of HBM on it: when the comb was the library's own choice and its
        // table cannot be had, the context falls back to the bucket method below instead of failing.
        if (rc == PLK_ERR_OOM && comb_mode < 0) {
            (void)hipGetLastError();
            ctx->comb = nullptr;
        } else {
            PLK_TRY(rc);
            ctx->geom.c = COMB_WINDOW;
            ctx->geom.windows = COMB_WINDOWS;
            PLK_HIP_TRY(hipStreamSynchronize(stream));
            return PLK_OK;
        }
    }
    ctx->ws.resize(1);
    size_t tab_min = 0;
    if (also_count > 0) {
        // the context will be rebound to these generator counts (msm_rebind_dev_impl): every part of the workspace is
        // sized for the largest need over all of them - the parts are not monotonic in n (the window, hence the bucket and
        // tile counts, changes with it)
        for (int a = 0; a < also_count; ++a) {
            MsmGeom other;
            if (msm_geometry_of(ctx->curve, also_n[a], 0, ctx->geom.table_free, knobs, &other) != PLK_OK) continue;
            for (int k = 0; k < MSM_WORK_PARTS; ++k)
                if (other.part_bytes[k] > ctx->ws[0].cap[k]) ctx->ws[0].cap[k] = other.part_bytes[k];
            if (other.n_eff * pt_bytes + 16 > tab_min) tab_min = other.n_eff * pt_bytes + 16;
        }
    }
    const MsmGeom& g = ctx->geom;
    if (g.table_free) {
        ctx->tab_cap = g.n_eff * pt_bytes + 16;
        if (ctx->tab_cap < tab_min) ctx->tab_cap = tab_min;
        ctx->tab = scratch_acquire(ctx->tab_cap, stream);
        if (!ctx->tab) return PLK_ERR_OOM;
        ctx->tab_stream = stream;
    } else {
        ctx->tab_cap = g.n_eff * g.windows * pt_bytes + 16;
        PLK_HIP_TRY(hipMalloc(&ctx->tab, ctx->tab_cap));
    }
    PLK_TRY(msm_alloc_work(ctx, ctx->ws[0], stream));
    msm_launch_table<C>(ctx, d_bases, d_zero, d_extra, n_extra, stream);
    PLK_HIP_TRY(hipGetLastError());
    PLK_HIP_TRY(hipStreamSynchronize(stream));
    return PLK_OK;
}

// A table-free context re-used for another (smaller or equal) generator set: new geometry, same memory, no allocation, no
// synchronisation - the rounds of an inner-product argument halve their generators every time (halo.rs:63-124).
template <class C>
static int msm_rebind_t(plk_msm_ctx* ctx, size_t n, const MsmGeom& g, const void* d_bases, const void* d_zero, const void* d_extra, size_t n_extra,
                        hipStream_t stream) {
    using FP = typename C::FP;
    const size_t pt_bytes = (size_t)2 * FP::NL * 4;
    if (g.n_eff * pt_bytes + 16 > ctx->tab_cap) return set_error(PLK_ERR_INVALID_ARG, "rebind: %zu points do not fit the context's table", g.n_eff);
    MsmWork& w = ctx->ws[0];
    for (int k = 0; k < MSM_WORK_PARTS; ++k)
        if (g.part_bytes[k] > w.cap[k])
            return set_error(PLK_ERR_INVALID_ARG, "rebind: workspace part %d needs %zu bytes, the context holds %zu", k, g.part_bytes[k], w.cap[k]);
    ctx->n = n;
    ctx->geom = g;
    if (w.used && w.last_stream != stream) PLK_HIP_TRY(hipStreamWaitEvent(stream, w.ev, 0));
    msm_launch_table<C>(ctx, d_bases, d_zero, d_extra, n_extra, stream);
    PLK_HIP_TRY(hipGetLastError());
    ctx->tab_stream = stream;
    w.last_stream = stream;
    return PLK_OK;
}

int msm_precompute_dev_impl(int curve, size_t n, const void* d_bases, const void* d_zero, unsigned window_bits, unsigned flags, hipStream_t stream,
                            plk_msm_ctx** out_ctx, const void* d_extra, size_t n_extra, const size_t* also_n, int also_count) {
    if (!out_ctx) return set_error(PLK_ERR_INVALID_ARG, "null out_ctx");
    *out_ctx = nullptr;
    if (curve_limbs(curve) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (n > n_extra && !d_bases) return set_error(PLK_ERR_INVALID_ARG, "null bases");
    if (n_extra > n || (n_extra && !d_extra)) return set_error(PLK_ERR_INVALID_ARG, "bad extra generators");
    PLK_TRY(ensure_device());
    int dev = 0;
    PLK_HIP_TRY(hipGetDevice(&dev));
    auto* ctx = new plk_msm_ctx();
    ctx->device = dev;
    ctx->curve = curve;
    ctx->n = n;
    ctx->auto_window = window_bits == 0 && also_count == 0;
    const MsmKnobs knobs = msm_knobs_from_env();
    int rc = msm_geometry_of(curve, n, window_bits, (flags & PLK_MSM_TABLE_FREE) != 0, knobs, &ctx->geom);
    if (rc == PLK_OK)
        rc = or_bad_curve(with_curve(curve, [&](auto t) {
            return msm_precompute_t<tag_t<decltype(t)>>(ctx, knobs, d_bases, d_zero, d_extra, n_extra, stream, also_n, also_count);
        }), curve);
    if (rc != PLK_OK) {
        delete ctx;
        return rc;
    }
    *out_ctx = ctx;
    return PLK_OK;
}

// see msm_rebind_t.  n counts the extra generators (the last n_extra of the n points come from d_extra).
int msm_rebind_dev_impl(plk_msm_ctx* ctx, size_t n, const void* d_bases, const void* d_zero, const void* d_extra, size_t n_extra, hipStream_t stream) {
    if (!ctx || !ctx->geom.table_free || ctx->ws.empty()) return set_error(PLK_ERR_INVALID_ARG, "rebind needs a table-free context");
    if (n_extra > n || (n > n_extra && !d_bases) || (n_extra && !d_extra)) return set_error(PLK_ERR_INVALID_ARG, "bad generators");
    PLK_TRY(ensure_device());
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int curve = ctx->curve;
    MsmGeom g;
    PLK_TRY(msm_geometry_of(curve, n, 0, true, msm_knobs_from_env(), &g));
    return or_bad_curve(with_curve(curve, [&](auto t) { return msm_rebind_t<tag_t<decltype(t)>>(ctx, n, g, d_bases, d_zero, d_extra, n_extra, stream); }), curve);
}

// what one execution asks for beyond its scalars: the form of the result, and whether some vector of the batch is a bucket share
struct MsmCall {
    bool projective;  // results as the reference's un-normalised ProjectivePoint, not the affine point
    bool many_heads;  // TailGeom::many_heads
};

static uint32_t* head_bucket_of(const plk_msm_ctx* ctx, const MsmWork& w) {
    return (uint32_t*)((uint8_t*)w.part[PART_HEAD_LIVE] + head_lanes_padded(ctx->geom.max_lanes));
}
static uint32_t* live_list_of(const plk_msm_ctx* ctx, const MsmWork& w) {
    return (uint32_t*)((uint8_t*)w.part[PART_HEAD_LIVE] + 5 * head_lanes_padded(ctx->geom.max_lanes));
}
static TailSlot tail_slot(const plk_msm_ctx* ctx, const MsmWork& w, const MsmCall& call, void* d_out_xy, void* d_out_zero) {
    TailSlot t;
    t.off = (const uint32_t*)w.part[PART_OFF];
    t.p_start = (uint4*)w.part[PART_P_START];
    t.p_head = (const uint4*)w.part[PART_P_HEAD];
    t.head_live = (const uint8_t*)w.part[PART_HEAD_LIVE];
    t.head_bucket = head_bucket_of(ctx, w);
    t.live_list = live_list_of(ctx, w);
    t.live_count = w.meta(META_LIVE_COUNT);
    t.bucket = (uint4*)w.part[PART_BUCKET];
    t.heavy = (uint32_t*)w.part[PART_HEAVY];
    t.heavy_part = (uint4*)w.part[PART_HEAVY_PART];
    t.line_part = (uint4*)w.part[PART_LINE_PART];
    t.plane_part = (uint4*)w.part[PART_PLANE_PART];
    t.win_pts = (uint4*)w.part[PART_WIN_PTS];
    t.final_done = w.meta(META_FINAL_DONE);
    t.dyn_chunk = w.meta(META_DYN_CHUNK);
    t.out_xy = (uint4*)d_out_xy;
    t.out_zero = (uint8_t*)d_out_zero;
    t.projective = call.projective ? 1 : 0;
    return t;
}

// pieces -> buckets -> (row / column sums ->) bit-plane sums -> result, for the tb.count MSMs of a batch at once (msm_tail.hip)
template <class C, class Mark>
static int msm_reduce_t(const plk_msm_ctx* ctx, const MsmCall& call, const TailBatch& tb, hipStream_t stream, Mark&& mark) {
    TailGeom g = ctx->geom.tail;
    g.many_heads = call.many_heads ? 1 : 0;
    for (int stage = 0; stage < 3; ++stage) {
        PLK_TRY(msm_launch_reduce_stage<C>(stage, g, tb, stream));
        mark();
    }
    return PLK_OK;
}

// phases: 1 = bucket ordering, 2 = accumulation, 4 = reduction; 7 = the whole MSM on one stream
constexpr int PH_ORDER = 1, PH_ACC = 2, PH_REDUCE = 4, PH_ALL = 7;
template <class C>
static int msm_execute_t(plk_msm_ctx* ctx, MsmWork& w, const MsmCall& call, const void* d_scalars, void* d_out_xy, void* d_out_zero, hipStream_t stream,
                         int phases = PH_ALL, size_t first = 0, size_t count = (size_t)-1, uint32_t bucket_part = 0, uint32_t bucket_parts = 1) {
    // count != -1: the scalars belong to generators first .. first + count - 1 (tabled contexts: the table index of an entry is its id)
    const bool ranged = count != (size_t)-1;
    const MsmGeom& g = ctx->geom;
    const size_t n = ranged ? count : g.n_eff;
    OrdCfg o = g.ord;
    if (ranged) {
        o.nt1 = (uint32_t)((n + (size_t)o.spt * o.sub - 1) / ((size_t)o.spt * o.sub));
        if (o.nt1 == 0) o.nt1 = 1;
        o.ent_first = (uint32_t)first;
    }
    if (bucket_parts > 1) {  // this execution's range of the coarse bins (the larger ranges first, like shard_bounds)
        const uint32_t nb = (uint32_t)o.nbins, base = nb / bucket_parts, rem = nb % bucket_parts;
        o.bin_lo = bucket_part * base + (bucket_part < rem ? bucket_part : rem);
        o.bin_hi = o.bin_lo + base + (bucket_part < rem ? 1u : 0u);
    }
    // the workspace may still be in use by an execution enqueued on another stream
    if (w.used && w.last_stream != stream) PLK_HIP_TRY(hipStreamWaitEvent(stream, w.ev, 0));
    std::vector<hipEvent_t> ev;
    if (ctx->profiling && phases == PH_ALL) {
        if (!ctx->prof_free.empty()) {
            ev = ctx->prof_free.back();
            ctx->prof_free.pop_back();
        } else {
            ev.resize(plk_msm_ctx::N_STAGES + 1);
            for (auto& e : ev) PLK_HIP_TRY(hipEventCreate(&e));
        }
    }
    int stage = 0;
    auto mark = [&]() {
        if (!ev.empty()) (void)hipEventRecord(ev[stage], stream);
        ++stage;
    };
    mark();
    if (phases & PH_ORDER) {
        void* halves = nullptr;
        if (g.glv) {
            // the two half scalars of every scalar (stream-ordered scratch: handed back once the ordering kernels are enqueued)
            halves = scratch_acquire(n * 32, stream);
            if (!halves) return PLK_ERR_OOM;
            PLK_TRY(msm_launch_glv_split<C>(d_scalars, ctx->n, halves, stream));
            d_scalars = halves;
        }
        // the pooled buffers of this call go back on every path out of it
        struct Guard {
            void*& halves;
            std::vector<hipEvent_t>& ev;
            plk_msm_ctx* ctx;
            hipStream_t stream;
            bool armed = true;
            ~Guard() {
                if (!armed) return;
                if (halves) scratch_release(halves, stream);
                if (!ev.empty()) ctx->prof_free.push_back(ev);
            }
        } guard{halves, ev, ctx, stream};
        OrdBuffers ob;
        ob.scalars = d_scalars; ob.n = n; ob.cnt1 = w.part[PART_CNT1]; ob.tmp = w.part[PART_TMP]; ob.sorted = w.part[PART_SORTED]; ob.cnt2 = w.part[PART_CNT2];
        ob.off = w.part[PART_OFF]; ob.meta = w.meta(0);
        ob.chunk = g.chunk; ob.lanes = (uint32_t)(g.max_lanes > 2 ? g.max_lanes - 2 : 1); ob.buckets = g.buckets;
        PLK_TRY(msm_launch_order_stage<C>(0, o, ob, stream));
        mark();
        PLK_TRY(msm_launch_order_stage<C>(1, o, ob, stream));
        mark();
        PLK_TRY(msm_launch_order_stage<C>(2, o, ob, stream));
        PLK_HIP_TRY(hipGetLastError());
        guard.armed = false;
        if (halves) scratch_release(halves, stream);
        mark();
    } else {
        stage += 3;
    }
    if (phases & PH_ACC) {
        // the entry count is only known on the device: launch for the upper bound, lanes past it exit
        const unsigned ablocks = (unsigned)((g.max_lanes + ACC_THREADS - 1) / ACC_THREADS);
        msm_launch_accumulate<C>(ablocks, stream, ctx->tab, w.part[PART_SORTED], w.part[PART_OFF], w.part[PART_P_START], w.part[PART_P_HEAD], w.part[PART_HEAD_LIVE],
                                 head_bucket_of(ctx, w), live_list_of(ctx, w), w.meta(META_LIVE_COUNT), g.buckets, w.meta(META_DYN_CHUNK),
                                 g.table_free ? g.c - 1 : 31, g.table_free ? (uint32_t)n : 0u,
                                 // tabled: sorted[] entries index the table; table-free: the table holds the n_eff points, sorted[] the entries
                                 g.table_free ? (uint32_t)g.n_eff : o.entries_cap);
        PLK_HIP_TRY(hipGetLastError());
    }
    mark();
    if (phases & PH_REDUCE) {
        TailBatch tb;
        tb.count = 1;
        tb.s[0] = tail_slot(ctx, w, call, d_out_xy, d_out_zero);
        PLK_TRY(msm_reduce_t<C>(ctx, call, tb, stream, mark));
        if (!ev.empty()) ctx->prof_sets.push_back(ev);
    }
    return PLK_OK;
}

// the events, and the pooled streams asked for, that a batched execution over groups of `group` vectors synchronises through
static int ensure_batch_sync(plk_msm_ctx* ctx, unsigned group, bool want_fork_streams, bool want_tail_stream) {
    if (want_tail_stream && !ctx->tail_stream && !(ctx->tail_stream = stream_pool_acquire())) return PLK_ERR_HIP;
    if (!ctx->ev_tail) PLK_HIP_TRY(hipEventCreateWithFlags(&ctx->ev_tail, hipEventDisableTiming));
    while (ctx->ev_acc.size() < group) {
        hipEvent_t e = nullptr;
        PLK_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ev_acc.push_back(e);
    }
    while (want_fork_streams && ctx->fork_streams.size() + 1 < group) {
        hipStream_t st = stream_pool_acquire();
        if (!st) return PLK_ERR_HIP;
        ctx->fork_streams.push_back(st);
    }
    return PLK_OK;
}

static void work_done(MsmWork& w, hipStream_t stream) {
    (void)hipEventRecord(w.ev, stream);
    w.last_stream = stream;
    w.used = true;
}

// ready (optional): one event per scalar vector; vector b is not touched before ready[b] has completed (the host-pointer entry
// point copies vector b + 1 through PCIe while vector b is being reduced)
int msm_execute_dev_impl(plk_msm_ctx* ctx, unsigned batch, const void* d_scalars, size_t n_scalars, void* d_out_xy, void* d_out_zero, hipStream_t stream,
                         hipEvent_t* ready, const MsmParts* parts, unsigned out_flags) {
    // out_flags bit 0: results as the reference's un-normalised ProjectivePoint, x | y | z (3 L limbs per vector), not the affine point
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    if (parts) {
        // vector b: parts->count[b] scalars at parts->scalars[b] for the generators parts->first[b] .. (plk_msm_execute_parts_dev)
        if (ctx->geom.table_free) return set_error(PLK_ERR_INVALID_ARG, "a sub-range of the generators needs a tabled context");
        if (!parts->first || !parts->count || !parts->scalars) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
        if ((parts->bucket_part == nullptr) != (parts->bucket_parts == nullptr)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
        for (unsigned b = 0; b < batch && parts->bucket_parts; ++b) {
            if (parts->bucket_parts[b] > 1 && (ctx->comb || parts->bucket_part[b] >= parts->bucket_parts[b] || parts->bucket_parts[b] > (uint32_t)ctx->geom.ord.nbins))
                return set_error(PLK_ERR_INVALID_ARG, "vector %u: bucket range %u of %u over %d coarse bins%s", b, parts->bucket_part[b], parts->bucket_parts[b],
                                 ctx->geom.ord.nbins, ctx->comb ? " (a comb context has no buckets)" : "");
        }
        for (unsigned b = 0; b < batch; ++b) {
            if (parts->first[b] > ctx->n || parts->count[b] > ctx->n - parts->first[b])
                return set_error(PLK_ERR_SIZE_MISMATCH, "vector %u covers generators %llu .. +%llu but the precomputation holds %zu", b,
                                 (unsigned long long)parts->first[b], (unsigned long long)parts->count[b], ctx->n);
            if (parts->count[b] && !parts->scalars[b]) return set_error(PLK_ERR_INVALID_ARG, "null scalars in batch slot %u", b);
        }
    } else if (n_scalars != ctx->n) {
        return set_error(PLK_ERR_SIZE_MISMATCH, "scalars.len() = %zu but the precomputation holds %zu generators (curve_msm.rs:67)", n_scalars, ctx->n);
    }
    if (batch == 0) return PLK_OK;
    if ((!parts && ctx->n && !d_scalars) || !d_out_xy || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    PLK_HIP_TRY(hipSetDevice(ctx->device));  // a context works on the device it was built on, whichever device the thread last used
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t L = (size_t)curve_limbs(ctx->curve);
    MsmCall call{(out_flags & 1u) != 0, false};
    for (unsigned b = 0; b < batch && parts && parts->bucket_parts; ++b) call.many_heads = call.many_heads || parts->bucket_parts[b] > 1;
    const size_t out_stride = (call.projective ? 3 : 2) * L * 8;
    if (ctx->comb) {
        if (call.projective) return set_error(PLK_ERR_INVALID_ARG, "a comb context returns affine points (the caller expands them)");
        // few generators: additions of table entries and a tree, two launches for the whole batch (comb.hip)
        std::vector<const void*> ptr(batch);
        std::vector<uint64_t> first(batch), count(batch);
        for (unsigned b = 0; b < batch; ++b) {
            if (ready) PLK_HIP_TRY(hipStreamWaitEvent(stream, ready[b], 0));
            ptr[b] = parts ? parts->scalars[b] : (const void*)((const uint8_t*)d_scalars + (size_t)b * ctx->n * 32);
            first[b] = parts ? parts->first[b] : 0;
            count[b] = parts ? parts->count[b] : ctx->n;
        }
        return comb_execute(ctx->comb, batch, ptr.data(), first.data(), count.data(), d_out_xy, d_out_zero, stream);
    }
    auto run_one = [&](unsigned b, MsmWork& w, hipStream_t st, int phases) -> int {
        if (ready && (phases & PH_ORDER)) PLK_HIP_TRY(hipStreamWaitEvent(st, ready[b], 0));
        const uint8_t* sc = parts ? (const uint8_t*)parts->scalars[b] : (const uint8_t*)d_scalars + (size_t)b * ctx->n * 32;
        const size_t first = parts ? (size_t)parts->first[b] : 0, count = parts ? (size_t)parts->count[b] : (size_t)-1;
        const uint32_t bp = (parts && parts->bucket_parts) ? parts->bucket_part[b] : 0u, bps = (parts && parts->bucket_parts) ? parts->bucket_parts[b] : 1u;
        uint8_t* oxy = (uint8_t*)d_out_xy + (size_t)b * out_stride;
        uint8_t* oz = (uint8_t*)d_out_zero + b;
        return or_bad_curve(with_curve(ctx->curve, [&](auto t) { return msm_execute_t<tag_t<decltype(t)>>(ctx, w, call, sc, oxy, oz, st, phases, first, count, bp, bps); }),
                            ctx->curve);
    };
    static const bool no_batching = getenv("PLK_MSM_NO_OVERLAP") != nullptr;  // every MSM of a batch start to end, one by one
    if (batch == 1 || ctx->profiling || no_batching) {
        for (unsigned b = 0; b < batch; ++b) PLK_TRY(run_one(b, ctx->ws[0], stream, PH_ALL));
        work_done(ctx->ws[0], stream);
        return PLK_OK;
    }
    // Several scalar vectors against the same generators (commit_polynomials, plonk_util.rs:215-231), in groups of up
    // to TAIL_MAX: every MSM of a group has its own workspace, ordering and accumulation run one MSM after the other,
    // and the latency-bound reduction runs ONCE for the whole group - it is a chain of point operations on few points,
    // so nine of them cost little more than one.
    unsigned group = batch < (unsigned)TAIL_MAX ? batch : (unsigned)TAIL_MAX;
    const size_t budget = (size_t)16 << 30;  // bytes of workspace a batch may hold
    while (group > 2 && ctx->ws_bytes * group > budget) --group;
    while (ctx->ws.size() < group) {
        ctx->ws.emplace_back();
        if (msm_alloc_work(ctx, ctx->ws.back(), stream) != PLK_OK) {
            ctx->ws.back().release();
            ctx->ws.pop_back();
            (void)hipGetLastError();
            group = (unsigned)ctx->ws.size();  // make do with what fits (at least the workspace of the precomputation)
            break;
        }
    }
    auto reduce = [&](const TailBatch& tb, hipStream_t st) -> int {
        auto nomark = [] {};
        return or_bad_curve(with_curve(ctx->curve, [&](auto t) { return msm_reduce_t<tag_t<decltype(t)>>(ctx, call, tb, st, nomark); }), ctx->curve);
    };
    // Pipelined reductions: the reduction of a vector is mostly latency (chains on few points) plus
    // 0.1 ms of full-width row / column sums; on a second stream it runs under the ordering and accumulation of the NEXT vector
    // instead of after the last one.  The caller's stream waits for the second stream before the call returns.
    // Measured (profiles/r03_commit9_scaling.txt): SLOWER than one shared reduction at the end - 12.85 against 12.38 ms for nine
    // 2^20 vectors, 2.52 against 2.21 ms for a rank's share of them at eight ranks: the accumulation is sized as exactly one round
    // of lanes, and every slot a reduction workgroup takes sends part of that round into a second one.  Off unless asked for.
    static const bool pipeline_tails = getenv("PLK_MSM_TAIL_PIPELINE") != nullptr;
    if (pipeline_tails) {
        PLK_TRY(ensure_batch_sync(ctx, group, false, true));
        for (unsigned g0 = 0; g0 < batch; g0 += group) {
            const unsigned cnt = batch - g0 < group ? batch - g0 : group;
            // the workspaces of the previous group are free again when its reductions are done
            if (g0) {
                PLK_HIP_TRY(hipEventRecord(ctx->ev_tail, ctx->tail_stream));
                PLK_HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_tail, 0));
            }
            for (unsigned k = 0; k < cnt; ++k) {
                const unsigned b = g0 + k;
                PLK_TRY(run_one(b, ctx->ws[k], stream, PH_ORDER | PH_ACC));
                PLK_HIP_TRY(hipEventRecord(ctx->ev_acc[k], stream));
                PLK_HIP_TRY(hipStreamWaitEvent(ctx->tail_stream, ctx->ev_acc[k], 0));
                TailBatch tb;
                tb.count = 1;
                tb.s[0] = tail_slot(ctx, ctx->ws[k], call, (uint8_t*)d_out_xy + (size_t)b * out_stride, (uint8_t*)d_out_zero + b);
                PLK_TRY(reduce(tb, ctx->tail_stream));
            }
        }
        PLK_HIP_TRY(hipEventRecord(ctx->ev_tail, ctx->tail_stream));
        PLK_HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_tail, 0));
        for (unsigned k = 0; k < group && k < ctx->ws.size(); ++k) work_done(ctx->ws[k], stream);
        return PLK_OK;
    }
    // Small MSMs (the rounds of an inner-product argument over frozen generators: 2^14 points, two vectors): ordering and
    // accumulation are six short kernels per vector that leave most of the GPU idle - the vectors of a group run them side by side
    // on streams of their own and meet again for the shared reduction (0.52 -> 0.42 ms for such a round).
    static const bool no_fork = getenv("PLK_MSM_NO_FORK") != nullptr;
    const bool fork = !no_fork && group > 1 && ctx->geom.n_eff * (size_t)ctx->geom.windows <= ((size_t)1 << 21);
    if (fork) PLK_TRY(ensure_batch_sync(ctx, group, true, false));
    for (unsigned g0 = 0; g0 < batch; g0 += group) {
        const unsigned cnt = batch - g0 < group ? batch - g0 : group;
        TailBatch tb;
        tb.count = (int)cnt;
        if (fork && cnt > 1) PLK_HIP_TRY(hipEventRecord(ctx->ev_tail, stream));  // the scalars (and the previous group's reduction) are ready
        for (unsigned k = 0; k < cnt; ++k) {
            const unsigned b = g0 + k;
            hipStream_t st = stream;
            if (fork && k > 0) {
                st = ctx->fork_streams[k - 1];
                PLK_HIP_TRY(hipStreamWaitEvent(st, ctx->ev_tail, 0));
            }
            PLK_TRY(run_one(b, ctx->ws[k], st, PH_ORDER | PH_ACC));
            if (st != stream) {
                PLK_HIP_TRY(hipEventRecord(ctx->ev_acc[k], st));
                PLK_HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_acc[k], 0));
            }
            tb.s[k] = tail_slot(ctx, ctx->ws[k], call, (uint8_t*)d_out_xy + (size_t)b * out_stride, (uint8_t*)d_out_zero + b);
        }
        PLK_TRY(reduce(tb, stream));
        for (unsigned k = 0; k < cnt; ++k) work_done(ctx->ws[k], stream);
    }
    return PLK_OK;
}

int msm_ctx_is_comb(const plk_msm_ctx* ctx) { return ctx && ctx->comb ? 1 : 0; }

int msm_set_profiling_impl(plk_msm_ctx* ctx, int enable) {
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->profiling = enable != 0 && !ctx->comb;
    // a comb (few generators, automatic window: comb.hip) has no stages to time - two launches - and says so instead of staying silently off
    if (enable && ctx->comb) return set_error(PLK_ERR_INVALID_ARG, "per-stage timings: this context over %zu generators is a comb (no bucket stages)", ctx->n);
    return PLK_OK;
}
// sum_ms[7]: digits, partition (counts), bucket scan + final scatter, accumulate, bucket sums, planes, final -- summed over `calls` executions since the last read
int msm_get_timings_impl(plk_msm_ctx* ctx, double* sum_ms, unsigned* calls) {
    if (!ctx || !sum_ms) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int k = 0; k < plk_msm_ctx::N_STAGES; ++k) sum_ms[k] = 0;
    unsigned cnt = 0;
    for (auto& set : ctx->prof_sets) {
        if (hipEventSynchronize(set.back()) != hipSuccess) continue;
        for (int k = 0; k < plk_msm_ctx::N_STAGES; ++k) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, set[k], set[k + 1]);
            sum_ms[k] += ms;
        }
        ++cnt;
        ctx->prof_free.push_back(set);
    }
    ctx->prof_sets.clear();
    if (calls) *calls = cnt;
    return PLK_OK;
}

size_t msm_ctx_len(const plk_msm_ctx* ctx) { return ctx->n; }
unsigned msm_ctx_window(const plk_msm_ctx* ctx) { return (unsigned)ctx->geom.c; }
int msm_ctx_curve(const plk_msm_ctx* ctx) { return ctx->curve; }
int msm_ctx_table_free(const plk_msm_ctx* ctx) { return ctx->geom.table_free ? 1 : 0; }
void msm_ctx_delete(plk_msm_ctx* ctx) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    delete ctx;  // frees on the devices its parts live on
    if (cur >= 0) (void)hipSetDevice(cur);
}
int msm_ctx_device(const plk_msm_ctx* ctx) { return ctx->device; }
std::vector<plk_msm_ctx*>& msm_ctx_peers(plk_msm_ctx* ctx) { return ctx->peers; }
std::vector<plk_msm_ctx*>& msm_ctx_shards(plk_msm_ctx* ctx) { return ctx->shards; }

// msm_precompute with the reference's output (curve_msm.rs:27-52): powers_per_generator[i][j] = [2^(w j)] G_i, j < ceil(BITS / w)
int msm_table_digits(int curve, unsigned w) { return w ? (curve_scalar_bits(curve) + (int)w - 1) / (int)w : -1; }

template <class C>
static int msm_reference_table_t(size_t n, const void* d_bases, const void* d_zero, int w, int digits, void* d_out_xy, void* d_out_zero,
                                 hipStream_t stream) {
    using FP = typename C::FP;
    const size_t pt_bytes = (size_t)2 * FP::NL * 4;
    void* tab = scratch_acquire(n * digits * pt_bytes + 16, stream);
    if (!tab) return PLK_ERR_OOM;
    k_msm_table<C><<<(unsigned)((n + 127) / 128), 128, 0, stream>>>((const uint4*)d_bases, (const uint8_t*)d_zero, (uint4*)tab, n, w, digits, 0, n, nullptr);
    const size_t total = n * (size_t)digits;
    k_msm_table_export<C><<<(unsigned)((total + 255) / 256), 256, 0, stream>>>((const uint4*)tab, n, digits, (uint4*)d_out_xy, (uint8_t*)d_out_zero);
    hipError_t e = hipGetLastError();
    scratch_release(tab, stream);
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "table launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

int msm_reference_table_dev_impl(int curve, size_t n, const void* d_bases, const void* d_zero, unsigned w, void* d_out_xy, void* d_out_zero,
                                 hipStream_t stream) {
    if (curve_limbs(curve) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (w < 1 || w > 64) return set_error(PLK_ERR_INVALID_ARG, "window size %u outside [1, 64]", w);
    if (n == 0) return PLK_OK;
    if (!d_bases || !d_out_xy || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    const int digits = msm_table_digits(curve, w);
    return or_bad_curve(with_curve(curve, [&](auto t) { return msm_reference_table_t<tag_t<decltype(t)>>(n, d_bases, d_zero, (int)w, digits, d_out_xy, d_out_zero, stream); }),
                        curve);
}

// the device's digit recoding on its own (plk_msm_debug_digits): d_digits = n * windows int32, windows = ceil((BITS + 1) / window_bits)
int msm_debug_digits_impl(int curve, unsigned window_bits, size_t n, const void* d_scalars, void* d_digits, hipStream_t stream) {
    if (window_bits < 2 || window_bits > (unsigned)MSM_MAX_WINDOW) return set_error(PLK_ERR_INVALID_ARG, "window of %u bits (2..%d)", window_bits, MSM_MAX_WINDOW);
    if (curve < 0 || curve > PLK_CURVE_VESTA) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (!n) return PLK_OK;
    if (!d_scalars || !d_digits) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    OrdCfg o{};
    o.c = (int)window_bits;
    o.windows = (curve_scalar_bits(curve) + 1 + o.c - 1) / o.c;
    return or_bad_curve(with_curve(curve, [&](auto t) { return msm_launch_digits<tag_t<decltype(t)>>(d_scalars, n, o, d_digits, stream); }), curve);
}
int msm_debug_digit_count(int curve, unsigned window_bits) {
    if (curve < 0 || curve > PLK_CURVE_VESTA || window_bits < 2 || window_bits > (unsigned)MSM_MAX_WINDOW) return -1;
    return (curve_scalar_bits(curve) + 1 + (int)window_bits - 1) / (int)window_bits;
}

// workspaces for batches of up to `count` vectors, allocated ahead of the first batched execution
int msm_reserve_workspaces_impl(plk_msm_ctx* ctx, unsigned count, hipStream_t stream) {
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    PLK_TRY(ensure_device());
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->comb) return PLK_OK;  // nothing to reserve
    if (count > (unsigned)TAIL_MAX) count = TAIL_MAX;
    while (ctx->ws.size() < count) {
        ctx->ws.emplace_back();
        const int rc = msm_alloc_work(ctx, ctx->ws.back(), stream);
        if (rc != PLK_OK) {
            ctx->ws.back().release();
            ctx->ws.pop_back();
            return rc;
        }
    }
    return PLK_OK;
}

}  // namespace plk
