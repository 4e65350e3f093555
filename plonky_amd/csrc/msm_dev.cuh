// msm_dev.cuh -- device-side definitions shared by the translation units of the MSM (msm.hip: tables and the host side;
// msm_order.hip: digits and the bucket ordering; msm_acc.hip: the bucket accumulation; msm_tail.hip: the reduction).  The kernels
// are split over several files so that a change to one of them rebuilds in a minute instead of five; device code is not relocatable
// here (no -fgpu-rdc), so anything both sides need lives in this header.  The constants and the geometry structs (OrdCfg, TailGeom)
// are plain C++ and live in msm_geom.h, with the function that computes them.
#pragma once
#include "common.h"
#include "ec.cuh"
#include "ecz.cuh"
#include "msm_geom.h"

namespace plk {

// -DPLK_CHECKED (make checked -> libplonky_hip_checked.so; SURVEY.md section 5: the reference's debug assertions and overflow
// checks have no equivalent in a release kernel): every index the ordering and accumulation kernels compute into sorted[],
// tmp[], the tables and the bucket arrays is compared with its bound; a violation is counted per site and the access is
// skipped.  plk_checked_failures() reads the counters.  In the normal build the guards compile to nothing.
#ifdef PLK_CHECKED
static __device__ unsigned g_plk_chk[8];  // one copy per translation unit; checked_failures_impl adds them up
#define PLK_CHK(cond, site) (!(cond) ? (atomicAdd(&g_plk_chk[site], 1u), false) : true)
#else
#define PLK_CHK(cond, site) (true)
#endif
enum { CHK_TMP_INDEX = 0, CHK_TILE_STAGE = 1, CHK_SORTED_INDEX = 2, CHK_SEG_STAGE = 3, CHK_TABLE_INDEX = 4, CHK_BUCKET = 5, CHK_ENTRY_RANGE = 6 };

// accumulation pieces as they travel between the kernels (lazy 29-bit limbs, accumulator invariant of ecz.cuh; the identity is ZZ = 0)
template <class FP> constexpr int raw_u4() { return FzCfg<FP>::NZ; }  // uint4 per raw point: 4 NZ words

template <class FP> PLK_DI void xyzzz_store_raw(uint4* dst, const XyzzZ<FP>& a) {
    constexpr int NZ = FzCfg<FP>::NZ;
    uint32_t w[4 * NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        // the identity is ZZ = 0 (xyzzz_load_raw); its other coordinates are never looked at, so only ZZ pays for a select - the
        // store sits on the path that some lane of an accumulation wave takes almost every round
        w[i] = a.x.l[i];
        w[NZ + i] = a.y.l[i];
        w[2 * NZ + i] = a.inf ? 0u : a.zz.l[i];
        w[3 * NZ + i] = a.zzz.l[i];
    }
#pragma unroll
    for (int i = 0; i < NZ; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
template <class FP> PLK_DI XyzzZ<FP> xyzzz_load_raw(const uint4* src) {
    constexpr int NZ = FzCfg<FP>::NZ;
    uint32_t w[4 * NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const uint4 v = src[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    XyzzZ<FP> r;
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        r.x.l[i] = w[i];
        r.y.l[i] = w[NZ + i];
        r.zz.l[i] = w[2 * NZ + i];
        r.zzz.l[i] = w[3 * NZ + i];
        any |= w[2 * NZ + i];
    }
    r.inf = any == 0;  // a live accumulator never has ZZ = 0 (that case is caught as the identity in ecz.cuh)
    // a piece closed inside the accumulation's loop is stored with its Y UNCARRIED (limbs <= 3 * 2^29 - 3, ecz.cuh: the carry pass
    // would sit on the path some lane of a wave takes almost every round); the carries are moved here, where the piece is read
    fz_carry<FP>(r.y);
    return r;
}

constexpr int TAIL_MAX = 16;
struct TailSlot {
    const uint32_t* off;  // bucket offsets off[buckets + 1]
    uint4* p_start;       // raw, one per bucket (becomes the assembled bucket)
    const uint4* p_head;  // raw, one per accumulation lane
    const uint8_t* head_live;  // 1: p_head[lane] holds a piece that is not part of a start piece yet
    const uint32_t* head_bucket;  // the bucket lane's head piece belongs to (HEAD_NONE: the lane starts at a bucket boundary)
    const uint32_t* live_list;    // the lanes whose head piece is live, in no particular order (k_msm_accumulate appends)
    uint32_t* live_count;         // how many; zero between executions (reset by the reduction)
    uint4* bucket;        // packed points: the operands of the plane sums
    uint32_t* heavy;
    uint4* heavy_part;    // raw
    uint4* line_part;     // raw: row partials then column partials
    uint4* plane_part;
    uint4* win_pts;
    uint32_t* final_done;  // windows finished by k_msm_final (the last one adds them up); zero between executions
    const uint32_t* dyn_chunk;  // entries per accumulation lane of this execution (k_ord_scan1)
    uint4* out_xy;        // the result: x | y affine, or (projective) x | y | z
    uint8_t* out_zero;
    int projective;       // 1: the reference's ProjectivePoint, not normalised (emit_projective, ecz.cuh)
};
struct TailBatch {
    int count;
    TailSlot s[TAIL_MAX];
};

// the buffers of one ordering (msm_order.hip: msm_launch_order_stage)
struct OrdBuffers {
    const void* scalars;
    size_t n;
    void *cnt1, *tmp, *sorted, *cnt2, *off;
    uint32_t* meta;  // META_* (msm_geom.h)
    uint32_t chunk, lanes, buckets;
};

// the launchers msm.hip calls, instantiated per curve by the unit that holds the kernels
// msm_acc.hip: the bucket accumulation kernel
template <class C> int msm_accumulate_blocks_per_cu();
template <class C>
void msm_launch_accumulate(unsigned blocks, hipStream_t stream, const void* tab, const void* sorted, const void* off, void* p_start, void* p_head,
                           void* head_live, void* head_bucket, void* live_list, uint32_t* live_count, uint32_t buckets, const uint32_t* dyn_chunk, int wshift,
                           uint32_t n_sub, uint32_t tab_entries);
// msm_order.hip: digits + the two-level bucket ordering; msm_tail.hip: the reduction
template <class C> int msm_launch_glv_split(const void* d_scalars, size_t n, void* halves, hipStream_t stream);
template <class C> int msm_launch_order_stage(int stage, const OrdCfg& o, const OrdBuffers& b, hipStream_t stream);
template <class C> int msm_launch_digits(const void* d_scalars, size_t n, const OrdCfg& o, void* d_digits, hipStream_t stream);
template <class C> int msm_launch_reduce_stage(int stage, const TailGeom& g, const TailBatch& tb, hipStream_t stream);

// the guard counters of a translation unit (-DPLK_CHECKED), read back for plk_checked_failures
#ifdef PLK_CHECKED
#define PLK_CHK_READER(fn)                                                                        \
    int fn(unsigned* counts) {                                                                    \
        PLK_HIP_TRY(hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_plk_chk), 8 * sizeof(unsigned)));    \
        return PLK_OK;                                                                            \
    }
#else
#define PLK_CHK_READER(fn)                       \
    int fn(unsigned* counts) {                   \
        for (int k = 0; k < 8; ++k) counts[k] = 0; \
        return PLK_OK;                           \
    }
#endif

}  // namespace plk
