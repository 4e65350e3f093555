// curve_ops.hip -- point utilities above the group law that are no part of the MSM: the sum of k affine points, the combination of a
// device group's partial results, synthetic generators G0 + (first + i) D, affine -> projective, and the two test surfaces of the point
// arithmetic (the quad self-test and plk_curve_op).  Split from msm.hip (build time; nothing here touches an MSM context).
#include "common.h"
#include "ec.cuh"
#include "ecz.cuh"
#include "ecz_coop.cuh"

namespace plk {

template <class FP> PLK_DI Xyzz<FP> block_sum(Xyzz<FP> v, uint4* s_pts) {
    constexpr int W = FP::NL / 4;
    const int tid = threadIdx.x;
    xyzz_store<FP>(s_pts + tid * 4 * W, v);
    __syncthreads();
    for (int d = blockDim.x >> 1; d >= 1; d >>= 1) {
        if (tid < d) {
            v = xyzz_add<FP>(v, xyzz_load<FP>(s_pts + (tid + d) * 4 * W));
            xyzz_store<FP>(s_pts + tid * 4 * W, v);
        }
        __syncthreads();
    }
    return v;
}

// ---------------------------------------------------------------------------------------------
// small utilities: sum of k affine points; synthetic generators G0 + (first + i) D
// ---------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(64) k_sum_affine(const uint4* __restrict__ pts, const uint8_t* __restrict__ zero, size_t k, uint4* __restrict__ out_xy,
                                                   uint8_t* __restrict__ out_zero) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    extern __shared__ __attribute__((aligned(16))) uint4 s_pts[];
    Xyzz<FP> acc = xyzz_identity<FP>();
    for (size_t i = threadIdx.x; i < k; i += blockDim.x) {
        if (zero && zero[i]) continue;
        Fe<FP> x = fe_load<FP>(pts + i * 2 * W), y = fe_load<FP>(pts + i * 2 * W + W);
        xyzz_madd<FP>(acc, x, y);
    }
    acc = block_sum<FP>(acc, s_pts);
    if (threadIdx.x == 0) {
        Fe<FP> x, y;
        bool ident = xyzz_to_affine<FP, true>(acc, x, y);
        fe_store<FP>(out_xy, x);
        fe_store<FP>(out_xy + W, y);
        *out_zero = ident ? 1 : 0;
    }
}

// Multi-GPU exchange (plonky_hip.h): every rank's results travel as one packed record of `slots` points then
// `slots` identity flags.  Block v produces vector v: a whole vector (v < whole * world) is rank v % world's slot v / world,
// a sharded one is the sum over the ranks of slot whole + (v - whole * world).
template <class C>
__global__ void __launch_bounds__(64) k_combine_partials(const uint8_t* __restrict__ gathered, size_t rec_bytes, unsigned world, unsigned slots,
                                                         unsigned whole, uint4* __restrict__ out_xy, uint8_t* __restrict__ out_zero) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    extern __shared__ __attribute__((aligned(16))) uint4 s_pts[];
    const unsigned v = blockIdx.x;
    const bool is_whole = v < whole * world;
    const unsigned slot = is_whole ? v / world : whole + (v - whole * world);
    const unsigned r0 = is_whole ? v % world : 0, r1 = is_whole ? r0 + 1 : world;
    Xyzz<FP> acc = xyzz_identity<FP>();
    // The records were written by OTHER devices (peer copies over xGMI, multi.hip), by RCCL or through the host, into a buffer this
    // device may have read before (the scratch pool hands it out again): every word is read at SYSTEM scope, past this device's
    // caches - a few hundred bytes per rank, so the price is nothing, and the hand-over does not depend on what a kernel boundary
    // invalidates (each XCD has its own L2; MI355X_MICROARCH.md).  Records are 16-byte aligned (msm_partials_bytes).
    auto word = [](const uint8_t* p) { return __hip_atomic_load((const uint32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    for (unsigned r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
        const uint8_t* rec = gathered + (size_t)r * rec_bytes;
        const size_t flag_at = (size_t)slots * 2 * W * 16 + slot;
        if ((word(rec + (flag_at & ~(size_t)3)) >> (8 * (flag_at & 3))) & 0xffu) continue;
        const uint8_t* pt = rec + (size_t)slot * 2 * W * 16;
        Fe<FP> x, y;
#pragma unroll
        for (int i = 0; i < FP::NL; ++i) {
            x.v[i] = word(pt + 4 * i);
            y.v[i] = word(pt + 4 * (FP::NL + i));
        }
        xyzz_madd<FP>(acc, x, y);
    }
    acc = block_sum<FP>(acc, s_pts);
    if (threadIdx.x == 0) {
        Fe<FP> x, y;
        const bool ident = xyzz_to_affine<FP, true>(acc, x, y);
        fe_store<FP>(out_xy + (size_t)v * 2 * W, x);
        fe_store<FP>(out_xy + (size_t)v * 2 * W + W, y);
        out_zero[v] = ident ? 1 : 0;
    }
}

template <class C>
__global__ void __launch_bounds__(128) k_gen_bases(const uint4* __restrict__ g0d, uint4* __restrict__ out, size_t n, uint64_t first) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<FP> gx = fe_load<FP>(g0d), gy = fe_load<FP>(g0d + W), dx = fe_load<FP>(g0d + 2 * W), dy = fe_load<FP>(g0d + 3 * W);
    // (first + i) * D by double-and-add from the top bit, then + G0
    uint64_t m = first + i;
    Xyzz<FP> acc = xyzz_identity<FP>();
    for (int b = 63; b >= 0; --b) {
        acc = xyzz_dbl<FP>(acc);
        if ((m >> b) & 1) xyzz_madd<FP>(acc, dx, dy);
    }
    xyzz_madd<FP>(acc, gx, gy);
    Fe<FP> x, y;
    bool ident = xyzz_to_affine<FP>(acc, x, y);
    (void)ident;  // G0 + m D is the identity only for one m in the whole group; callers use small m
    fe_store<FP>(out + i * 2 * W, x);
    fe_store<FP>(out + i * 2 * W + W, y);
}

// ---------------------------------------------------------------------------------------------
// self-test: the quad arithmetic (ecz_coop.cuh) against the one-lane arithmetic (ecz.cuh) on the same operands
// ---------------------------------------------------------------------------------------------
// same group element: x1 zz2 == x2 zz1 and y1 zzz2 == y2 zzz1 (the projective equality of curve.rs:280-302)
template <class FP> PLK_DI bool xyzzz_same(const XyzzZ<FP>& a, const XyzzZ<FP>& b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    const Fe<FP> l1 = fz_to_fe_canonical<FP>(fz_mul<FP>(a.x, b.zz)), r1 = fz_to_fe_canonical<FP>(fz_mul<FP>(b.x, a.zz));
    const Fe<FP> l2 = fz_to_fe_canonical<FP>(fz_mul<FP>(a.y, b.zzz)), r2 = fz_to_fe_canonical<FP>(fz_mul<FP>(b.y, a.zzz));
    bool ok = true;
    for (int i = 0; i < FP::NL; ++i) ok = ok && (l1.v[i] == r1.v[i]) && (l2.v[i] == r2.v[i]);
    return ok;
}
template <class C>
__global__ void __launch_bounds__(256) k_selftest_quad(const uint4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ mismatches) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    const uint32_t quad = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const int ql = threadIdx.x & 3;
    const uint32_t i = quad % n, j = (quad * 7u + 3u) % n;
    const Fz<FP> k = fz_const_r_to_rprime<FP>();
    auto load_pt = [&](uint32_t idx, Fz<FP>& x, Fz<FP>& y) {
        x = fz_from_fe<FP>(fz_to_fe_canonical<FP>(fz_mul<FP>(fz_from_fe<FP>(fe_load<FP>(pts + (size_t)idx * 2 * W)), k)));
        y = fz_from_fe<FP>(fz_to_fe_canonical<FP>(fz_mul<FP>(fz_from_fe<FP>(fe_load<FP>(pts + (size_t)idx * 2 * W + W)), k)));
    };
    Fz<FP> xi, yi, xj, yj;
    load_pt(i, xi, yi);
    load_pt(j, xj, yj);
    XyzzZ<FP> a = xyzzz_identity<FP>(), b = xyzzz_identity<FP>();
    xyzzz_madd<FP>(a, xi, yi);
    a = xyzzz_dbl<FP>(a);           // 2 P_i, zz != 1
    xyzzz_madd<FP>(b, xj, yj);
    xyzzz_madd<FP>(b, xi, yi);      // P_j + P_i (or 2 P_i / identity when the indices collide)
    XyzzZ<FP> na = a;
    na.y = fz_sub<FP, 2>(fz_zero<FP>(), a.y);  // -a, y < 4p
    bool ok = true;
    // sum over the 16 quads of the wave against a serial sum of the same 16 points (whole wave active)
    bool wave_ok;
    {
        XyzzZ<FP> tot = wave_sum_q<FP>(a, 16, ql);
        XyzzZ<FP> ser = xyzzz_identity<FP>();
        for (int q = 0; q < 16; ++q) {
            XyzzZ<FP> t = a;  // lane 4q of this wave holds that quad's a
            const int src = 4 * q;
#pragma unroll
            for (int l = 0; l < FzCfg<FP>::NZ; ++l) {
                t.x.l[l] = __shfl(a.x.l[l], src);
                t.y.l[l] = __shfl(a.y.l[l], src);
                t.zz.l[l] = __shfl(a.zz.l[l], src);
                t.zzz.l[l] = __shfl(a.zzz.l[l], src);
            }
            t.inf = __shfl((int)a.inf, src) != 0;
            ser = xyzzz_add<FP>(ser, t);
        }
        wave_ok = xyzzz_same<FP>(tot, ser);
    }
    switch (quad & 7u) {
        case 0: ok = xyzzz_same<FP>(xyzzz_add_q<FP>(a, b, ql), xyzzz_add<FP>(a, b)); break;
        case 1: ok = xyzzz_same<FP>(xyzzz_dbl_q<FP>(a, ql), xyzzz_dbl<FP>(a)); break;
        case 2: ok = xyzzz_same<FP>(xyzzz_add_q<FP>(a, a, ql), xyzzz_dbl<FP>(a)); break;          // doubling inside the addition
        case 3: ok = xyzzz_add_q<FP>(a, na, ql).inf; break;                                          // opposite points
        case 4: ok = xyzzz_same<FP>(xyzzz_add_q<FP>(xyzzz_identity<FP>(), b, ql), b); break;
        case 5: ok = xyzzz_same<FP>(xyzzz_add_q<FP>(b, xyzzz_identity<FP>(), ql), b); break;
        case 6: ok = xyzzz_same<FP>(xyzzz_dbl_q<FP>(xyzzz_dbl_q<FP>(b, ql), ql), xyzzz_dbl<FP>(xyzzz_dbl<FP>(b))); break;
        default: ok = wave_ok;
    }
    if (!ok) atomicAdd(mismatches + (quad & 7u), 1u);
}

// ---------------------------------------------------------------------------------------------
// plk_curve_op: one point operation of ecz.cuh / ecz_coop.cuh per element, on operands the caller chooses, result in affine form.
// The parity tests compare it with big integers (tests/test_gpu_group_law.py): unlike the self-test above nothing here compares
// one law of this library with another.
// ---------------------------------------------------------------------------------------------
constexpr int CURVE_OP_ADD = 0, CURVE_OP_DBL = 1, CURVE_OP_ADD_Q = 2, CURVE_OP_DBL_Q = 3, CURVE_OP_MADD = 4, CURVE_OP_MADD_ENTRY = 5,
              CURVE_OP_DBL_Q_TIMES = 6, CURVE_OP_WAVE_SUM_Q = 7, CURVE_OP_CHAIN_Q = 8, CURVE_OP_COUNT = 9;
constexpr uint8_t CURVE_OP_INFLATE = 1, CURVE_OP_NEGATE = 2;
constexpr bool curve_op_is_quad(int op) { return op == CURVE_OP_ADD_Q || op == CURVE_OP_DBL_Q || op >= CURVE_OP_DBL_Q_TIMES; }

struct CurveOpArgs {
    const uint4 *a_xy, *a_lam, *b_xy, *b_lam;   // affine points (2L limbs) and lambda (L limbs), Montgomery form
    const uint8_t *a_zero, *b_zero;             // identity flags, nullable
    const uint8_t* flags;
    uint4* out_xy;
    uint8_t* out_zero;
    uint32_t* mismatch;
    uint32_t count, param;
    int op;
};

// R-form words of the interface -> R'-form working limbs, value < 2p, exactly normalised
template <class FP> PLK_DI Fz<FP> curve_op_load(const uint4* src) { return fz_mul<FP>(fz_from_fe<FP>(fe_load<FP>(src)), fz_const_r_to_rprime<FP>()); }
// the representative (x l^2, y l^3, l^2, l^3) of the affine point e; inflated: X + 6p, Y + 2p with carried limbs (X < 8p, Y < 4p)
template <class FP> PLK_DI XyzzZ<FP> curve_op_operand(const uint4* xy, const uint8_t* zero, const uint4* lam, uint32_t e, bool inflate) {
    constexpr int W = FP::NL / 4;
    if (zero && zero[e]) return xyzzz_identity<FP>();
    const Fz<FP> l = curve_op_load<FP>(lam + (size_t)e * W);
    XyzzZ<FP> r;
    r.zz = fz_sqr<FP>(l);
    r.zzz = fz_mul<FP>(r.zz, l);
    r.x = fz_mul<FP>(curve_op_load<FP>(xy + (size_t)e * 2 * W), r.zz);
    r.y = fz_mul<FP>(curve_op_load<FP>(xy + (size_t)e * 2 * W + W), r.zzz);
    r.inf = false;
    if (inflate) {
        const Fz<FP> z = fz_zero<FP>();
        r.x = fz_sub<FP, 2>(fz_sub<FP, 1>(r.x, z), z);  // + 2p + 4p
        r.y = fz_sub<FP, 1>(r.y, z);                    // + 2p
    }
    return r;
}

// ops 0, 1, 4, 5: one lane per element
template <class C>
__global__ void __launch_bounds__(256) k_curve_op_lane(CurveOpArgs g) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.count) return;
    const uint8_t fl = g.flags[e];
    XyzzZ<FP> a = curve_op_operand<FP>(g.a_xy, g.a_zero, g.a_lam, e, fl & CURVE_OP_INFLATE);
    const bool b_ident = g.b_zero && g.b_zero[e];
    switch (g.op) {
        case CURVE_OP_ADD: a = xyzzz_add<FP>(a, curve_op_operand<FP>(g.b_xy, g.b_zero, g.b_lam, e, fl & CURVE_OP_INFLATE)); break;
        case CURVE_OP_DBL: a = xyzzz_dbl<FP>(a); break;
        case CURVE_OP_MADD:
            if (!b_ident) {  // a table entry is never the identity: the accumulation has no branch for it
                const Fz<FP> x2 = fz_from_fe<FP>(fz_to_fe_canonical<FP>(curve_op_load<FP>(g.b_xy + (size_t)e * 2 * W)));
                const Fz<FP> y2 = fz_from_fe<FP>(fz_to_fe_canonical<FP>(curve_op_load<FP>(g.b_xy + (size_t)e * 2 * W + W)));
                xyzzz_madd<FP>(a, x2, y2);
            }
            break;
        case CURVE_OP_MADD_ENTRY:
            if (!b_ident) {
                const Fe<FP> x2 = fz_to_fe_canonical<FP>(curve_op_load<FP>(g.b_xy + (size_t)e * 2 * W));
                const Fe<FP> y2 = fz_to_fe_canonical<FP>(curve_op_load<FP>(g.b_xy + (size_t)e * 2 * W + W));
                xyzzz_madd_entry<FP>(a, x2, y2, (fl & CURVE_OP_NEGATE) != 0);
                xyzzz_settle<FP>(a);
            }
            break;
        default: break;
    }
    emit_affine<FP>(a, g.out_xy + (size_t)e * 2 * W, g.out_zero + e);
}

// ops 2, 3, 6, 7, 8: one quad per element, whole waves active (elements past the end are the identity and are not stored).
// Every lane of a quad - of a group of quads for the wave sum - must hold the same affine result: lanes that differ from the
// first lane of theirs are counted into *mismatch.
template <class C>
__global__ void __launch_bounds__(256) k_curve_op_quad(CurveOpArgs g) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    const uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const int ql = threadIdx.x & 3;
    const bool live = e < g.count;
    const uint8_t fl = live ? g.flags[e] : 0;
    XyzzZ<FP> a = xyzzz_identity<FP>(), b = xyzzz_identity<FP>();
    if (live) a = curve_op_operand<FP>(g.a_xy, g.a_zero, g.a_lam, e, fl & CURVE_OP_INFLATE);
    if (live && (g.op == CURVE_OP_ADD_Q || g.op == CURVE_OP_CHAIN_Q)) b = curve_op_operand<FP>(g.b_xy, g.b_zero, g.b_lam, e, fl & CURVE_OP_INFLATE);
    uint32_t group = 1;  // quads that share one result
    switch (g.op) {
        case CURVE_OP_ADD_Q: a = xyzzz_add_q<FP>(a, b, ql); break;
        case CURVE_OP_DBL_Q: a = xyzzz_dbl_q<FP>(a, ql); break;
        case CURVE_OP_DBL_Q_TIMES:
            for (uint32_t i = 0; i < g.param; ++i) a = xyzzz_dbl_q<FP>(a, ql);
            break;
        case CURVE_OP_WAVE_SUM_Q:
            group = g.param;
            a = wave_sum_q<FP>(a, (int)group, ql);
            break;
        default:  // CURVE_OP_CHAIN_Q: results of the quad law fed back into it
            a = xyzzz_dbl_q<FP>(xyzzz_add_q<FP>(xyzzz_add_q<FP>(a, b, ql), a, ql), ql);
    }
    uint4 xy[2 * W];
    uint8_t zero;
    emit_affine<FP>(a, xy, &zero);
    const int first = (int)((threadIdx.x & 63u) & ~(4u * group - 1u));  // first lane of the quad / of the group, inside the wave
    bool same = __shfl((int)zero, first) == (int)zero;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(xy);
#pragma unroll
    for (int i = 0; i < 2 * FP::NL; ++i) same = same && __shfl(w[i], first) == w[i];
    const uint32_t head = e & ~(group - 1u);  // first element of the group
    if (head >= g.count) return;
    if (!same) atomicAdd(g.mismatch, 1u);
    if (e == head && ql == 0) {
#pragma unroll
        for (int i = 0; i < 2 * W; ++i) g.out_xy[(size_t)(e / group) * 2 * W + i] = xy[i];
        g.out_zero[e / group] = zero;
    }
}
// ---- host side ----
// affine results as ProjectivePoints with z = 1 (contexts and paths that normalise anyway: combs, device groups)
template <class FP> __global__ void k_affine_to_projective(const uint4* __restrict__ xy, const uint8_t* __restrict__ zero, uint4* __restrict__ xyz, unsigned batch) {
    constexpr int W = FP::NL / 4;
    const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const bool ident = zero[b] != 0;
    fe_store<FP>(xyz + (size_t)b * 3 * W, ident ? fe_zero<FP>() : fe_load<FP>(xy + (size_t)b * 2 * W));
    fe_store<FP>(xyz + (size_t)b * 3 * W + W, ident ? fe_zero<FP>() : fe_load<FP>(xy + (size_t)b * 2 * W + W));
    fe_store<FP>(xyz + (size_t)b * 3 * W + 2 * W, ident ? fe_zero<FP>() : fe_one<FP>());
}
int msm_affine_to_projective_impl(int curve, unsigned batch, const void* d_xy, const void* d_zero, void* d_xyz, hipStream_t stream) {
    if (batch == 0) return PLK_OK;
    const unsigned blocks = (batch + 63) / 64;
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using FP = typename tag_t<decltype(t)>::FP;
        k_affine_to_projective<FP><<<blocks, 64, 0, stream>>>((const uint4*)d_xy, (const uint8_t*)d_zero, (uint4*)d_xyz, batch);
        return PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

int curve_sum_affine_dev_impl(int curve, size_t k, const void* d_pts, const void* d_zero, void* d_out_xy, void* d_out_zero, hipStream_t stream) {
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        k_sum_affine<C><<<1, 64, 64 * 4 * C::FP::NL * 4, stream>>>((const uint4*)d_pts, (const uint8_t*)d_zero, k, (uint4*)d_out_xy, (uint8_t*)d_out_zero);
        return PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

size_t msm_partials_bytes(int curve, unsigned slots) {
    const int L = curve_limbs(curve);
    if (L < 0) return 0;
    return ((size_t)slots * 2 * L * 8 + slots + 15) & ~(size_t)15;
}
int msm_combine_partials_dev_impl(int curve, unsigned world, unsigned batch, unsigned whole_per_rank, const void* d_gathered, void* d_out_xy, void* d_out_zero,
                                  hipStream_t stream) {
    if (curve_limbs(curve) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (batch == 0) return PLK_OK;
    if (world == 0 || !d_gathered || !d_out_xy || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer or world = 0");
    if ((size_t)whole_per_rank * world > batch) return set_error(PLK_ERR_INVALID_ARG, "whole_per_rank %u x world %u exceeds the batch %u", whole_per_rank, world, batch);
    PLK_TRY(ensure_device());
    const unsigned slots = whole_per_rank + (batch - whole_per_rank * world);
    const size_t rec = msm_partials_bytes(curve, slots);
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        k_combine_partials<C><<<batch, 64, 64 * 4 * C::FP::NL * 4, stream>>>((const uint8_t*)d_gathered, rec, world, slots, whole_per_rank, (uint4*)d_out_xy,
                                                                             (uint8_t*)d_out_zero);
        return PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

// counts[8]: mismatches per case of k_selftest_quad over `quads` quads on the n points d_pts
int selftest_quad_dev_impl(int curve, const void* d_pts, uint32_t n, uint32_t quads, uint32_t* counts) {
    if (!d_pts || !counts || n == 0 || quads == 0) return set_error(PLK_ERR_INVALID_ARG, "bad argument");
    PLK_TRY(ensure_device());
    uint32_t* d_cnt = (uint32_t*)scratch_acquire(32, nullptr);
    if (!d_cnt) return PLK_ERR_OOM;
    (void)hipMemsetAsync(d_cnt, 0, 32, nullptr);
    const unsigned blocks = (quads * 4 + 255) / 256;
    const int rc = with_curve(curve, [&](auto t) {
        k_selftest_quad<tag_t<decltype(t)>><<<blocks, 256>>>((const uint4*)d_pts, n, d_cnt);
        return PLK_OK;
    });
    if (rc != PLK_OK) {
        scratch_release(d_cnt, nullptr);
        return or_bad_curve(rc, curve);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(counts, d_cnt, 32, hipMemcpyDeviceToHost);
    scratch_release(d_cnt, nullptr);
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "selftest failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

// plk_curve_op on device arrays (capi.hip has checked the ranges): d_mismatch is one zeroed word; waits for the kernel
int curve_op_dev_impl(int curve, int op, unsigned param, uint32_t count, const void* d_a_xy, const void* d_a_zero, const void* d_a_lambda, const void* d_b_xy,
                      const void* d_b_zero, const void* d_b_lambda, const void* d_flags, void* d_out_xy, void* d_out_zero, void* d_mismatch) {
    if (op < 0 || op >= CURVE_OP_COUNT || count == 0) return set_error(PLK_ERR_INVALID_ARG, "bad argument");
    CurveOpArgs g{(const uint4*)d_a_xy, (const uint4*)d_a_lambda, (const uint4*)d_b_xy, (const uint4*)d_b_lambda, (const uint8_t*)d_a_zero, (const uint8_t*)d_b_zero,
                  (const uint8_t*)d_flags, (uint4*)d_out_xy, (uint8_t*)d_out_zero, (uint32_t*)d_mismatch, count, param, op};
    const bool quad = curve_op_is_quad(op);
    const unsigned blocks = (unsigned)(((size_t)count * (quad ? 4 : 1) + 255) / 256);
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        if (quad) k_curve_op_quad<C><<<blocks, 256>>>(g);
        else k_curve_op_lane<C><<<blocks, 256>>>(g);
        return PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    PLK_HIP_TRY(hipDeviceSynchronize());
    return PLK_OK;
}

int curve_gen_bases_dev_impl(int curve, size_t n, uint64_t first, const void* d_g0d, void* d_out, hipStream_t stream) {
    if (n == 0) return PLK_OK;
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        k_gen_bases<tag_t<decltype(t)>><<<(unsigned)((n + 127) / 128), 128, 0, stream>>>((const uint4*)d_g0d, (uint4*)d_out, n, first);
        return PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
