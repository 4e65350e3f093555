// polydiv.hip -- Polynomial::polynomial_division (polynomial.rs:299-327) for a divisor of low degree, on device-resident coefficients:
// the public-input quotient of the prover (plonk.rs:199-235), whose divisor prod (X - s_i) has degree ceil(num_public_inputs / 9).
// The reference inverts rev(b) mod X^n by Newton's iteration (inv_mod_xn: log n rounds of three transforms); for a divisor of degree
// k <= 32 long division is a k-th order linear recurrence over the coefficients of a, and a recurrence scans.  The field is exact and
// quotient and remainder are unique, so the words are the reference's whatever the order of operations.
//
// Reduce-then-scan, like the grand product Z (plonk.hip), from the top coefficient down with the running remainder R[0..k) as state
// (polydiv_step.cuh).  a is cut into segments of S = 256 coefficients; a group of k' = next power of two >= k lanes owns a segment,
// lane i holds R[i] and -b'[i] (b' = b / lead, monic), t = R[k-1] is broadcast inside the group and R[i-1] comes from the neighbour
// lane: one product per lane and coefficient, 64 / k' segments per wave.
//   1. k_pdiv_table (one workgroup of k' x k' lanes): -b' and the exit factor in R'-form, and by repeated squaring of the companion
//      matrix the transition T_S (column i = X^(S + i) mod b') and T_SB of a block of B = 64 segments.
//   2. k_pdiv_local: every segment from the zero state -> its local remainder rho_g.
//   3. k_pdiv_scan: state_in(g) = rho_(g+1) + T_S state_in(g+1), a group of k' lanes per block of 64 segments (lane i: row i, six
//      products per reduction); with more than one block: block totals from zero, one sequential pass over them with T_SB, then the
//      blocks again from their true incoming states.
//   4. k_pdiv_apply: every segment again from state_in(g): writes q (times 1 / lead when b is not monic: the product that settles the
//      lazy value anyway) and the zeros up to q_len; segment 0 writes the remainder.
// No workgroup waits for another inside a launch.  a is read twice, q written once; 2 la k' products plus the scan.
// Segments cover [g S, (g + 1) S): the top one is filled with zeros above la - leading zeros leave the state alone - so every group
// runs the same S steps.  Quotient words of a group are kept by the lane whose index is the step (mod k') and stored k' at a time.
#include <vector>

#include "common.h"
#include "fp.cuh"
#include "fz.cuh"
#include "polydiv_step.cuh"
#include "tables.cuh"

namespace plk {

constexpr int PDIV_LANES = 256;   // workgroup of the per-coefficient kernels
constexpr int PDIV_AHEAD = 4;     // coefficients loaded ahead of the steps that use them
static_assert(PDIV_S % PDIV_AHEAD == 0 && PDIV_S % PDIV_MAX_K == 0 && 64 % PDIV_MAX_K == 0, "segment, load-ahead and group geometry");
static_assert(PDIV_MAX_K == PLK_POLY_DIV_MAX_DEGREE, "the header's limit");

struct PdivArg {  // host words of the call: -b' (R-form, zeros above k) and the exit factor (1 or 1 / lead, R-form)
    uint32_t negb[PDIV_MAX_K][8];
    uint32_t factor[8];
};

template <class P> PLK_DI Fz<P> pdiv_shfl(const Fz<P>& v, int src) {
    Fz<P> r;
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.l[i] = (uint32_t)__shfl((int)v.l[i], src, 64);
    return r;
}

// tid = column * kp + row.  negb_tab[i], factor_tab[0]: limb form, R'-form; t_s / t_sb: entry (row i, column j) at j * kp + i, limb form
template <class P>
__global__ void __launch_bounds__(PDIV_MAX_K* PDIV_MAX_K) k_pdiv_table(PdivArg arg, int k, int kp, int levels, uint32_t* __restrict__ negb_tab,
                                                                        uint32_t* __restrict__ factor_tab, uint32_t* __restrict__ t_s, uint32_t* __restrict__ t_sb) {
    constexpr int W = P::NL / 4;
    extern __shared__ uint4 s_m[];  // kp * kp entries, sized by the launch
    const int tid = threadIdx.x, i = tid & (kp - 1), j = tid / kp;
    const Fe<P> nb = i < k ? to_rprime<P>(fe_from_words<P>(arg.negb[i])) : fe_zero<P>();
    if (j == 0) limbs_store<P>(negb_tab, i, fz_from_fe<P>(nb));
    if (tid == 0) limbs_store<P>(factor_tab, 0, fz_from_fe<P>(to_rprime<P>(fe_from_words<P>(arg.factor))));
    Fe<P> e = pdiv_companion_entry<P>(i, j, k, nb);
    fe_store<P>(s_m + tid * W, e);
    __syncthreads();
    const int squarings = PDIV_S_LOG + (levels > 1 ? PDIV_B_LOG : 0);
    for (int s = 0; s < squarings; ++s) {
        e = pdiv_row<P>(fe_zero<P>(), kp, [&](int l) { return fz_from_fe<P>(fe_load<P>(s_m + (j * kp + l) * W)); },
                        [&](int l) { return fz_from_fe<P>(fe_load<P>(s_m + (l * kp + i) * W)); });
        __syncthreads();
        fe_store<P>(s_m + tid * W, e);
        __syncthreads();
        if (s == PDIV_S_LOG - 1) limbs_store<P>(t_s, tid, fz_from_fe<P>(e));
    }
    if (levels > 1) limbs_store<P>(t_sb, tid, fz_from_fe<P>(e));
}

// The S steps of a segment on one lane of its group.  top: index of the segment's first (highest) coefficient; coefficients at or
// above la read as zero.  emit(s, t): the quotient coefficient of index top - s.
template <class P, bool REDUCE, class EMIT>
PLK_DI Fz<P> pdiv_run_segment(const uint4* __restrict__ a, size_t la, size_t top, Fz<P> R, const Fz<P>& negb, int i, int src_prev, int src_t, EMIT emit) {
    constexpr int W = P::NL / 4;
    Fe<P> cur[PDIV_AHEAD], nxt[PDIV_AHEAD];
#pragma unroll
    for (int u = 0; u < PDIV_AHEAD; ++u) cur[u] = top - u < la ? fe_load<P>(a + (top - u) * W) : fe_zero<P>();
#pragma unroll 1
    for (int s0 = 0; s0 < PDIV_S; s0 += PDIV_AHEAD) {
        if (s0 + PDIV_AHEAD < PDIV_S) {
#pragma unroll
            for (int u = 0; u < PDIV_AHEAD; ++u) {
                const size_t jn = top - (size_t)(s0 + PDIV_AHEAD + u);
                nxt[u] = jn < la ? fe_load<P>(a + jn * W) : fe_zero<P>();
            }
        }
#pragma unroll
        for (int u = 0; u < PDIV_AHEAD; ++u) {
            const Fz<P> t = pdiv_shfl<P>(R, src_t);
            Fz<P> prev = pdiv_shfl<P>(R, src_prev);
            if (i == 0) prev = fz_from_fe<P>(cur[u]);
            emit(s0 + u, t);
            R = pdiv_lane_step<P, REDUCE>(prev, t, negb);
        }
#pragma unroll
        for (int u = 0; u < PDIV_AHEAD; ++u) cur[u] = nxt[u];
    }
    return R;
}

// rho[seg * kp + i] = R[i] after the segment from the zero state (zero for i >= k).  At most 2 waves per SIMD are asked for, so that the
// register allocator keeps the load-ahead buffers without spilling; a launch never has more: 2^20 coefficients are 4096 segments, 2 waves per
// SIMD at k' = 32 and only 64 / 128 / 256 waves in all at k' = 1 / 2 / 4 (latency-bound there: profiles/r09_poly_division.txt).
template <class P, bool REDUCE>
__global__ void __launch_bounds__(PDIV_LANES) __attribute__((amdgpu_waves_per_eu(1, 2))) k_pdiv_local(const uint4* __restrict__ a, size_t la, size_t nseg, const uint32_t* __restrict__ negb_tab, int k,
                                                            int kp, uint4* __restrict__ rho) {
    constexpr int W = P::NL / 4;
    const size_t gl = (size_t)blockIdx.x * PDIV_LANES + threadIdx.x, seg = gl / (unsigned)kp;
    const int i = (int)(gl & (size_t)(kp - 1)), lane = threadIdx.x & 63;
    const Fz<P> negb = limbs_load<P>(negb_tab, i);
    const Fz<P> R = pdiv_run_segment<P, REDUCE>(a, la, (seg + 1) * PDIV_S - 1, fz_zero<P>(), negb, i, (lane + 63) & 63, lane - i + k - 1, [](int, const Fz<P>&) {});
    if (seg < nseg) fe_store<P>(rho + gl * W, i < k ? pdiv_settle<P>(R, fz_one_rprime<P>()) : fe_zero<P>());
}

// q[j] = factor * t_j for j < q_len (the segments cover [0, nseg S)); rem[i] = R[i] after segment 0
template <class P, bool REDUCE>
__global__ void __launch_bounds__(PDIV_LANES) __attribute__((amdgpu_waves_per_eu(1, 2))) k_pdiv_apply(const uint4* __restrict__ a, size_t la, size_t nseg, const uint32_t* __restrict__ negb_tab,
                                                            const uint32_t* __restrict__ factor_tab, const uint4* __restrict__ states, int k, int kp,
                                                            uint4* __restrict__ q, size_t q_len, uint4* __restrict__ rem) {
    constexpr int W = P::NL / 4;
    const size_t gl = (size_t)blockIdx.x * PDIV_LANES + threadIdx.x, seg = gl / (unsigned)kp;
    const int i = (int)(gl & (size_t)(kp - 1)), lane = threadIdx.x & 63;
    const bool live = seg < nseg;
    const Fz<P> negb = limbs_load<P>(negb_tab, i), factor = limbs_load<P>(factor_tab, 0);
    const Fz<P> R0 = live ? fz_from_fe<P>(fe_load<P>(states + gl * W)) : fz_zero<P>();
    const size_t top = (seg + 1) * PDIV_S - 1;
    Fz<P> keep = fz_zero<P>();
    const Fz<P> R = pdiv_run_segment<P, REDUCE>(a, la, top, R0, negb, i, (lane + 63) & 63, lane - i + k - 1, [&](int s, const Fz<P>& t) {
        const int slot = s & (kp - 1);
        if (slot == i) keep = t;
        if (slot == kp - 1) {  // the same for every lane of the wave: the group's kp words, consecutive
            const size_t j = top - (size_t)(s - (kp - 1) + i);
            if (live && j < q_len) fe_store<P>(q + j * W, pdiv_settle<P>(keep, factor));
        }
    });
    if (seg == 0 && i < k && rem) fe_store<P>(rem + i * W, pdiv_settle<P>(R, fz_one_rprime<P>()));
}

// Items (segments, or blocks of them) in blocks of bsize, a group of kp lanes per block, from the block's top item down:
//   cur = in_states[block] (zero without);  per item g: out_states[g] = cur;  cur = rho[g] + T cur;  out_totals[block] = cur.
template <class P>
__global__ void __launch_bounds__(64) k_pdiv_scan(const uint4* __restrict__ rho, size_t n, size_t bsize, const uint32_t* __restrict__ tab,
                                                  const uint4* __restrict__ in_states, uint4* __restrict__ out_states, uint4* __restrict__ out_totals, int kp) {
    constexpr int W = P::NL / 4;
    const int lane = threadIdx.x, i = lane & (kp - 1), base = lane - i;
    const size_t blk = ((size_t)blockIdx.x * 64 + lane) / (unsigned)kp, nblk = (n + bsize - 1) / bsize;
    const bool valid = blk < nblk;
    const size_t first = blk * bsize, count = valid ? (n - first < bsize ? n - first : bsize) : 0;
    Fe<P> cur = valid && in_states ? fe_load<P>(in_states + (blk * kp + i) * W) : fe_zero<P>();
    for (size_t it = 0; it < bsize; ++it) {  // every group the same number of rounds: the lanes of a wave stay together
        const bool active = it < count;
        const size_t g = active ? first + count - 1 - it : 0;
        if (active && out_states) fe_store<P>(out_states + (g * kp + i) * W, cur);
        const Fe<P> r = active ? fe_load<P>(rho + (g * kp + i) * W) : fe_zero<P>();
        const Fz<P> cz = fz_from_fe<P>(cur);
        const Fe<P> nw = pdiv_row<P>(r, kp, [&](int j) { return pdiv_shfl<P>(cz, base + j); }, [&](int j) { return limbs_load<P>(tab, (size_t)j * kp + i); });
        if (active) cur = nw;
    }
    if (valid && out_totals) fe_store<P>(out_totals + (blk * kp + i) * W, cur);
}

// ---- host side ----
template <class P, bool REDUCE>
static void pdiv_launch(const PdivArg& arg, int k, int kp, const void* d_a, size_t la, void* d_q, size_t q_len, void* d_rem, uint32_t* negb_tab, uint32_t* factor_tab,
                        uint32_t* t_s, uint32_t* t_sb, uint4* rho, uint4* states, uint4* totals, uint4* block_in, hipStream_t stream) {
    const size_t nseg = (la + PDIV_S - 1) / PDIV_S, nblk = (nseg + PDIV_B - 1) / PDIV_B;
    const unsigned seg_grid = (unsigned)((nseg * kp + PDIV_LANES - 1) / PDIV_LANES), blk_grid = (unsigned)((nblk * kp + 63) / 64);
    k_pdiv_table<P><<<1, kp * kp, (size_t)kp * kp * 32, stream>>>(arg, k, kp, nblk > 1 ? 2 : 1, negb_tab, factor_tab, t_s, t_sb);
    k_pdiv_local<P, REDUCE><<<seg_grid, PDIV_LANES, 0, stream>>>((const uint4*)d_a, la, nseg, negb_tab, k, kp, rho);
    if (nblk > 1) {
        k_pdiv_scan<P><<<blk_grid, 64, 0, stream>>>(rho, nseg, (size_t)PDIV_B, t_s, nullptr, nullptr, totals, kp);
        k_pdiv_scan<P><<<1, 64, 0, stream>>>(totals, nblk, nblk, t_sb, nullptr, block_in, nullptr, kp);
    }
    k_pdiv_scan<P><<<blk_grid, 64, 0, stream>>>(rho, nseg, (size_t)PDIV_B, t_s, nblk > 1 ? block_in : nullptr, states, nullptr, kp);
    k_pdiv_apply<P, REDUCE><<<seg_grid, PDIV_LANES, 0, stream>>>((const uint4*)d_a, la, nseg, negb_tab, factor_tab, states, k, kp, (uint4*)d_q, q_len, (uint4*)d_rem);
}

template <class P>
static int poly_division_t(const uint64_t* negb, const uint64_t* factor, int k, const void* d_a, size_t la, void* d_q, size_t q_len, void* d_rem, hipStream_t stream) {
    int kp = 1;
    while (kp < k) kp <<= 1;
    const size_t nseg = (la + PDIV_S - 1) / PDIV_S, nblk = (nseg + PDIV_B - 1) / PDIV_B;
    ScratchSet ss(stream);
    constexpr int NZ = FzCfg<P>::NZ;
    uint32_t* negb_tab = (uint32_t*)ss.get(limb_bytes(PDIV_MAX_K, NZ));
    uint32_t* factor_tab = (uint32_t*)ss.get(limb_bytes(1, NZ));
    uint32_t* t_s = (uint32_t*)ss.get(limb_bytes((size_t)kp * kp, NZ));
    uint32_t* t_sb = (uint32_t*)ss.get(limb_bytes((size_t)kp * kp, NZ));
    uint4* rho = (uint4*)ss.get(nseg * kp * 32);
    uint4* states = (uint4*)ss.get(nseg * kp * 32);
    uint4* totals = (uint4*)ss.get(nblk * kp * 32);
    uint4* block_in = (uint4*)ss.get(nblk * kp * 32);
    if (!negb_tab || !factor_tab || !t_s || !t_sb || !rho || !states || !totals || !block_in) return PLK_ERR_OOM;  // scratch_acquire has set the error text
    PdivArg arg = {};
    for (int i = 0; i < k; ++i) limbs_to_words(arg.negb[i], negb + 4 * i);
    limbs_to_words(arg.factor, factor);
    if (k > PDIV_LAZY_MAX_K) pdiv_launch<P, true>(arg, k, kp, d_a, la, d_q, q_len, d_rem, negb_tab, factor_tab, t_s, t_sb, rho, states, totals, block_in, stream);
    else pdiv_launch<P, false>(arg, k, kp, d_a, la, d_q, q_len, d_rem, negb_tab, factor_tab, t_s, t_sb, rho, states, totals, block_in, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "polynomial division launch (table, local, scan or apply) failed: %s", hipGetErrorString(e));
    if (q_len > nseg * PDIV_S) PLK_HIP_TRY(hipMemsetAsync((char*)d_q + nseg * PDIV_S * 32, 0, (q_len - nseg * PDIV_S) * 32, stream));
    return PLK_OK;
}

static bool ranges_overlap(const void* x, size_t xb, const void* y, size_t yb) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + yb && b < a + xb;
}

int poly_division_check(int field, size_t la, const uint64_t* b, size_t lb, size_t q_len) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (!b) return set_error(PLK_ERR_INVALID_ARG, "null pointer: b");
    if (lb < 2 || lb - 1 > (size_t)PDIV_MAX_K)
        return set_error(PLK_ERR_INVALID_ARG, "divisor of degree %lld: the degree must be in 1..%d (PLK_POLY_DIV_MAX_DEGREE)", (long long)lb - 1, PDIV_MAX_K);
    const uint64_t* lead = b + 4 * (lb - 1);
    if (!(lead[0] | lead[1] | lead[2] | lead[3])) return set_error(PLK_ERR_INVALID_ARG, "the leading coefficient b[%zu] is zero", lb - 1);
    if (la <= lb - 1) return set_error(PLK_ERR_INVALID_ARG, "a has %zu coefficients: more than the divisor's degree %zu are required", la, lb - 1);
    if (q_len < la - (lb - 1)) return set_error(PLK_ERR_INVALID_ARG, "q_len %zu is below la - k = %zu", q_len, la - (lb - 1));
    return PLK_OK;
}

int poly_division_dev_impl(int field, const void* d_a, size_t la, const uint64_t* b, size_t lb, void* d_q, size_t q_len, void* d_rem, hipStream_t stream) {
    PLK_TRY(poly_division_check(field, la, b, lb, q_len));
    if (!d_a || !d_q) return set_error(PLK_ERR_INVALID_ARG, "null pointer: a / q");
    const int k = (int)(lb - 1);
    if (ranges_overlap(d_q, q_len * 32, d_a, la * 32)) return set_error(PLK_ERR_INVALID_ARG, "q must not alias a (a is read twice)");
    if (d_rem && (ranges_overlap(d_rem, (size_t)k * 32, d_a, la * 32) || ranges_overlap(d_rem, (size_t)k * 32, d_q, q_len * 32)))
        return set_error(PLK_ERR_INVALID_ARG, "the remainder must not alias a or q");
    uint64_t negb[PDIV_MAX_K * 4] = {}, factor[4];
    if (host_pdiv_prepare(field, b, lb, negb, factor) != 0) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    PLK_TRY(ensure_device());
    return or_invalid(with_field4(field, [&](auto t) { return poly_division_t<tag_t<decltype(t)>>(negb, factor, k, d_a, la, d_q, q_len, d_rem, stream); }),
                      "field %d is not a 4-limb field", field);
}

int poly_from_roots_impl(int field, unsigned k, const uint64_t* roots, uint64_t* out) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (k > (unsigned)PDIV_MAX_K) return set_error(PLK_ERR_INVALID_ARG, "%u roots: at most %d (PLK_POLY_DIV_MAX_DEGREE)", k, PDIV_MAX_K);
    if ((k && !roots) || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    if (host_poly_from_roots(field, k, roots, out) != 0) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    return PLK_OK;
}

}  // namespace plk
