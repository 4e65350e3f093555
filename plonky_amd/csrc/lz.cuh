// lz.cuh -- the working form of the Plonk and Plookup kernels (plonk.hip, plookup.hip): lazily reduced 29-bit limbs whose value
// bounds are part of the types, the conversions from / to the reference's form, the tables of powers every circuit-size cache
// starts from, and the workgroup / tile product scans of the two grand products.
#pragma once
#include "common.h"
#include "fp.cuh"
#include "tables.cuh"

namespace plk {

constexpr int XS_LO_LOG = 10;

// Working form of the kernels: lazily reduced 29-bit limbs in R'-form (fz.cuh) with the value bound carried in the TYPE, in
// eighths of p: Lz<P, B> holds a value below (B / 8) p with limbs below 2^29 + 8.  The operators pick the multiple of p a
// subtraction needs, give every result its bound, and refuse at compile time a product whose operand could exceed 15p or a
// sum that could leave the 261 bits of the representation - so the gate formulas below read like the reference's and cannot
// overflow silently.  A product of values below a p and b p comes back below (a b / 127.9 + 1) p (p / R' < 2^-7 (1 + 2^-22)).
constexpr int LZ_MUL_MAX = 120, LZ_VAL_MAX = 1000;
constexpr int lz_sub_k(int b) {
    int k = 0;
    while ((8 << k) - 1 < b) ++k;  // 2^k p must exceed the subtrahend's bound
    return k;
}
constexpr int lz_mul_bound(int a, int b) { return a * b / 1023 + 9; }
template <class P, int B> struct Lz {
    static_assert(FzCfg<P>::NZ == 9 && Mod29<P>::limb(8) <= (1u << 22), "bounds are derived for p < 2^254 (1 + 2^-22), R' = 2^261");
    Fz<P> v;
    template <int B2> PLK_DI Lz<P, B2> widen() const {
        static_assert(B2 >= B, "a bound can only be relaxed");
        return Lz<P, B2>{v};
    }
    PLK_DI Lz<P, lz_mul_bound(B, B)> sq() const {
        static_assert(B <= LZ_MUL_MAX, "operand of a product above 15p");
        return {fz_sqr<P>(v)};
    }
    PLK_DI Lz<P, 2 * B> dbl() const {  // field.rs:181-183 multiplies by TWO: the same value
        static_assert(2 * B <= LZ_VAL_MAX, "value could leave the representation");
        return {fz_add<P>(v, v)};
    }
    PLK_DI auto quad() const { return dbl().dbl(); }  // field.rs:191-193
    PLK_DI Lz<P, 16> rs() const {                      // any value of the representation -> below 2p, no multiplication
        static_assert(B <= 1023, "value could leave the representation");
        return {fz_reduce_small<P>(v)};
    }
    PLK_DI auto pow5() const {  // exp_usize(5), rescue_a.rs:58, rescue_b.rs:44
        const auto x2 = sq();
        return x2.sq() * *this;
    }
};
template <class P, int A, int B> PLK_DI Lz<P, A + B> operator+(const Lz<P, A>& a, const Lz<P, B>& b) {
    static_assert(A + B <= LZ_VAL_MAX, "value could leave the representation");
    return {fz_add<P>(a.v, b.v)};
}
template <class P, int A, int B> PLK_DI Lz<P, A + (8 << lz_sub_k(B))> operator-(const Lz<P, A>& a, const Lz<P, B>& b) {
    static_assert(A + (8 << lz_sub_k(B)) <= LZ_VAL_MAX, "value could leave the representation");
    return {fz_sub<P, lz_sub_k(B)>(a.v, b.v)};
}
template <class P, int A, int B> PLK_DI Lz<P, lz_mul_bound(A, B)> operator*(const Lz<P, A>& a, const Lz<P, B>& b) {
    static_assert(A <= LZ_MUL_MAX && B <= LZ_MUL_MAX, "operand of a product above 15p");
    return {fz_mul<P>(a.v, b.v)};
}
// A sum of products (and plain values) through ONE reduction (fz.cuh: FzWide; round 5).  B: bound of the accumulated value in eighths of p
// (a product of values below a p and b p adds a b / 1023; the reduction's own + p is added when it is taken), U: the column budget used
// (FZ_WIDE_UNITS).  RAW_A / RAW_B: the operand may have limbs up to 2^30 (a row as lz_load returns it) instead of carried / normalised ones.
template <class P, int B, int U> struct LzWide {
    FzWide<P> w;
};
template <class P> PLK_DI LzWide<P, 0, 0> lz_wide() {
    LzWide<P, 0, 0> r;
    fz_wide_clear<P>(r.w);
    return r;
}
template <bool RAW_A = false, bool RAW_B = false, class P, int B, int U, int A1, int A2>
PLK_DI LzWide<P, B + A1 * A2 / 1023 + 1, U + (RAW_A ? 2 : 1) * (RAW_B ? 2 : 1)> lz_mac(const LzWide<P, B, U>& acc, const Lz<P, A1>& a, const Lz<P, A2>& b) {
    static_assert(A1 <= LZ_MUL_MAX && A2 <= LZ_MUL_MAX, "operand of a product above 15p");
    static_assert(U + (RAW_A ? 2 : 1) * (RAW_B ? 2 : 1) <= FZ_WIDE_UNITS, "the column sums have no room for another product");
    static_assert(B + A1 * A2 / 1023 + 1 <= LZ_VAL_MAX, "value could leave the representation");
    LzWide<P, B + A1 * A2 / 1023 + 1, U + (RAW_A ? 2 : 1) * (RAW_B ? 2 : 1)> r{acc.w};
    fz_wide_mac<P>(r.w, a.v, b.v);
    return r;
}
template <class P, int B, int U, int A> PLK_DI LzWide<P, B + A, U> lz_wide_add(const LzWide<P, B, U>& acc, const Lz<P, A>& v) {
    static_assert(B + A <= LZ_VAL_MAX, "value could leave the representation");
    LzWide<P, B + A, U> r{acc.w};
    fz_wide_add<P>(r.w, v.v);
    return r;
}
template <class P, int B, int U> PLK_DI Lz<P, B + 9> lz_reduce(const LzWide<P, B, U>& acc) { return {fz_wide_reduce<P>(acc.w)}; }
// keeps a running value small: past 30p it is brought back below 2p
template <class P, int B> PLK_DI auto lz_tame(const Lz<P, B>& a) {
    if constexpr (B > 240) return a.rs();
    else return a;
}
// The caller's data is in the reference's R-form (x 2^256, canonical).  R' = 2^261 = 32 R: the R'-form of the same element is
// 32 x, i.e. the words re-sliced into 29-bit limbs five bits lower, then reduced below 2p without a multiplication.
template <class P> PLK_DI Lz<P, 16> lz_from_rform(const Fe<P>& x) {
    constexpr int NZ = FzCfg<P>::NZ, S = 29 * NZ - 32 * P::NL;
    static_assert(S > 0 && S < 29, "R' / R must be a shift by less than a limb");
    Fz<P> r;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const int off = 29 * i - S;
        uint32_t v;
        if (off < 0) v = x.v[0] << (-off);
        else {
            const int w = off >> 5, sh = off & 31;
            if (sh == 0) v = x.v[w];
            else if (sh + 29 <= 32 || w + 1 >= P::NL) v = x.v[w] >> sh;
            else v = (x.v[w] >> sh) | (x.v[w + 1] << (32 - sh));
        }
        r.l[i] = v & FzCfg<P>::M;
    }
    return {fz_reduce_small<P>(r)};
}
// The same conversion for the rows a point reads (~110 loads per point of the quotient numerator), without the reduction: cut the
// word X < p at bit s = floor(log2 p) - 5, X = t 2^s + X_low.  Then 32 X = 32 X_low + t 2^(s + 5) with 32 X_low < 2^(s + 5) <= p, and
// (t 2^(s + 5)) mod p is a table of p / 2^s + 1 <= 38 plain integers in 29-bit limbs (LZ_TOP_ROWS rows, staged in LDS by
// the kernels; built with the circuit-size tables): nine limb additions instead of a quotient estimate and a multiply-subtract per
// limb.  Value below 2p; limbs below 2^30 - 1 (two exact limbs added, no carry pass) - what fz_sub accepts of a subtrahend
// (fz.cuh) and what a product accepts of BOTH operands: 9 (2^30)^2 + 9 2^58 + 2^36 < 2^64.
constexpr int LZ_TOP_ROWS = 64, LZ_TOP_STRIDE = 12;
template <class P> struct LzSplit {
    static constexpr int top_bit() {
        for (int b = 32 * P::NL - 1; b >= 0; --b)
            if ((P::MOD[b >> 5] >> (b & 31)) & 1u) return b;
        return 0;
    }
    // R' / R = 2^SH: the re-slicing of lz_from_rform shifts by SH, so the cut and the table's exponent must use the same SH (5 for the
    // 256-bit fields on nine 29-bit limbs - the only instantiation today; a field with another SH gets the right table, not a wrong residue)
    static constexpr int SH = 29 * FzCfg<P>::NZ - 32 * P::NL;
    static constexpr int S = top_bit() - SH;  // X_low = X mod 2^S
    static constexpr int E = S + SH;          // table row t = (t 2^E) mod p, 2^E <= p
    static_assert(SH > 0 && SH < 29, "R' / R must be a shift by less than a limb");
    static_assert(S >= 29 * (FzCfg<P>::NZ - 1) - SH && S >= 32 * (P::NL - 1), "the cut must lie in the top limb and the top word");
    static_assert((P::MOD[P::NL - 1] >> (S - 32 * (P::NL - 1))) < 64u, "the top part of a canonical word must index the table (LZ_TOP_ROWS)");
};
// LDS copy of the table: a row is read with three 16-byte accesses (a limb-major copy read word by word - no two rows in one bank -
// was measured too: 10.44-10.51 ms against 10.27-10.28 for this layout, profiles/r04_quotient_diet.txt)
template <class P> using LzTop = uint32_t[LZ_TOP_ROWS][LZ_TOP_STRIDE];
template <class P> PLK_DI Lz<P, 16> lz_from_rform(const Fe<P>& x, const LzTop<P>& top) {
    constexpr int NZ = FzCfg<P>::NZ, SH = 29 * NZ - 32 * P::NL, S = LzSplit<P>::S;
    static_assert(SH > 0 && SH < 29 && NZ <= LZ_TOP_STRIDE, "R' / R must be a shift by less than a limb");
    // t <= (p - 1) >> S for a canonical word.  Words >= p violate the boundary's contract (include/plonky_hip.h: elements are fully reduced,
    // as every element of the reference is - monty.rs:41-45,103-106); the clamp only keeps such a word's load inside the table
    const uint32_t t = min(x.v[P::NL - 1] >> (S - 32 * (P::NL - 1)), (uint32_t)LZ_TOP_ROWS - 1u);
    const uint4 t0 = *reinterpret_cast<const uint4*>(&top[t][0]), t1 = *reinterpret_cast<const uint4*>(&top[t][4]),
                t2 = *reinterpret_cast<const uint4*>(&top[t][8]);
    const uint32_t tl[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
    Fz<P> r;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const int off = 29 * i - SH;
        uint32_t v;
        if (off < 0) v = x.v[0] << (-off);
        else {
            const int w = off >> 5, sh = off & 31;
            if (sh == 0) v = x.v[w];
            else if (sh + 29 <= 32 || w + 1 >= P::NL) v = x.v[w] >> sh;
            else v = (x.v[w] >> sh) | (x.v[w + 1] << (32 - sh));
        }
        // the top limb ends at the cut: bits 29 (NZ - 1) - SH .. S - 1 of X
        const uint32_t mask = i == NZ - 1 ? (1u << (S - (29 * (NZ - 1) - SH))) - 1u : FzCfg<P>::M;
        r.l[i] = (v & mask) + tl[i];
    }
    return {r};
}
template <class P> PLK_DI Lz<P, 16> lz_load(const uint4* p, size_t i) { return lz_from_rform<P>(fe_load<P>(p + i * 2)); }  // k_all_constraints: no table staged
template <class P> PLK_DI Lz<P, 16> lz_load(const uint4* p, size_t i, const LzTop<P>& top) { return lz_from_rform<P>(fe_load<P>(p + i * 2), top); }
// the table (LZ_TOP_ROWS rows of LZ_TOP_STRIDE words) into LDS; the caller's next barrier publishes it
template <class P> PLK_DI void stage_top_table(const uint32_t* __restrict__ top_global, LzTop<P>& s_top) {
    for (int k = threadIdx.x; k < LZ_TOP_ROWS * LZ_TOP_STRIDE / 4; k += blockDim.x)
        reinterpret_cast<uint4*>(&s_top[0][0])[k] = reinterpret_cast<const uint4*>(top_global)[k];
}
// table entries are stored in R'-form, canonical
template <class P> PLK_DI Lz<P, 8> lz_table(const uint4* p, size_t i) { return {fz_from_fe<P>(fe_load<P>(p + i * 2))}; }
template <class P> PLK_DI Lz<P, 8> lz_one() { return {fz_one_rprime<P>()}; }
// back to the reference's form: x R' * R / R' = x R, below 2p, then the unique representative
template <class P, int B> PLK_DI Fe<P> lz_to_rform(const Lz<P, B>& a) {
    static_assert(B <= LZ_MUL_MAX, "operand of a product above 15p");
    return fz_to_fe_canonical<P>(fz_mul<P>(a.v, fz_const_rprime_to_r<P>()));
}

// the powers of the domain's root in both forms, the small inverses and the table of lz_from_rform: one launch when a size's tables are built
template <class P> __global__ void k_plonk_xs(const uint4* __restrict__ pw, int log_t, int log_n8, uint4* __restrict__ lo, uint4* __restrict__ hi,
                                              uint4* __restrict__ lo_z, uint4* __restrict__ hi_z, uint4* __restrict__ small, uint32_t* __restrict__ top) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n_lo = (size_t)1 << XS_LO_LOG;
    const size_t n_hi = log_n8 > XS_LO_LOG ? (size_t)1 << (log_n8 - XS_LO_LOG) : 1;
    if (idx < n_lo) {
        const uint64_t e = (idx & (((uint64_t)1 << log_n8) - 1)) << (log_t - log_n8);
        const Fe<P> v = pow_from_table<P>(pw, 0, e, log_t);
        fe_store<P>(lo + idx * 2, v);
        fe_store<P>(lo_z + idx * 2, to_rprime<P>(v));
    } else if (idx < n_lo + n_hi) {
        const uint64_t e = (((idx - n_lo) << XS_LO_LOG) & (((uint64_t)1 << log_n8) - 1)) << (log_t - log_n8);
        const Fe<P> v = pow_from_table<P>(pw, 0, e, log_t);
        fe_store<P>(hi + (idx - n_lo) * 2, v);
        fe_store<P>(hi_z + (idx - n_lo) * 2, to_rprime<P>(v));
    } else if (idx < n_lo + n_hi + 7) {
        // 1 / v for v = 1 .. 7
        const uint32_t v = (uint32_t)(idx - n_lo - n_hi) + 1;
        Fe<P> c = fe_zero<P>();
        c.v[0] = v;
        fe_store<P>(small + (v - 1) * 2, to_rprime<P>(fe_inv_safegcd<P>(fe_from_canonical<P>(c))));
    } else if (idx < n_lo + n_hi + 7 + LZ_TOP_ROWS) {
        // (t 2^(S + 5)) mod p as a plain integer: the product of the two numbers in Montgomery form, brought back
        const uint32_t tt = (uint32_t)(idx - n_lo - n_hi - 7);
        constexpr int E = LzSplit<P>::E;  // 2^E <= p
        Fe<P> a = fe_zero<P>(), b = fe_zero<P>();
        a.v[0] = tt;
        b.v[E >> 5] = 1u << (E & 31);
        const Fe<P> prod = fe_to_canonical<P>(fe_mul<P>(fe_from_canonical<P>(a), fe_from_canonical<P>(b)));
        const Fz<P> z = fz_from_fe<P>(prod);
#pragma unroll
        for (int i = 0; i < LZ_TOP_STRIDE; ++i) top[tt * LZ_TOP_STRIDE + i] = i < FzCfg<P>::NZ ? z.l[i] : 0u;
    }
}
// what k_plonk_xs fills for a domain of 2^log_domain points (g its primitive root): the start of the Plonk tables (8n points) and
// of the Plookup ones (4N points)
struct DomainTables {
    DevBuf xs_lo;    // g^j, j < 1024, R-form: feeds the Lagrange table of the family
    DevBuf xs_hi;    // g^(1024 j)
    DevBuf xs_lo_z;  // the same two tables in R'-form: the point x of a lane is one product of them
    DevBuf xs_hi_z;
    DevBuf small;    // [0..7]: 1/1 .. 1/7 then unused, R'-form; MDS entry (r, c) = 1 / (4 + r - c)  (mds.rs:63-77)
    DevBuf top;      // (t 2^(S + 5)) mod p, t < LZ_TOP_ROWS, plain integers in 29-bit limbs (lz_from_rform)
};
// Allocates and fills them on `stream`, asynchronously.  The power table of the NTT plan is only borrowed for the launch: the caller
// keeps plan_hold until it has synchronised the stream.
template <class P> int build_domain_tables(int log_domain, hipStream_t stream, DomainTables& t, std::shared_ptr<const void>& plan_hold) {
    const void* pw = nullptr;
    int log_t = 0;
    PLK_TRY(ntt_plan_pow_table(P::FIELD_ID, (unsigned)log_domain, &pw, &log_t, &plan_hold));
    const size_t n_lo = (size_t)1 << XS_LO_LOG, n_hi = log_domain > XS_LO_LOG ? (size_t)1 << (log_domain - XS_LO_LOG) : 1;
    PLK_TRY(t.xs_lo.alloc(n_lo * 32));
    PLK_TRY(t.xs_hi.alloc(n_hi * 32));
    PLK_TRY(t.xs_lo_z.alloc(n_lo * 32));
    PLK_TRY(t.xs_hi_z.alloc(n_hi * 32));
    PLK_TRY(t.small.alloc(8 * 32));
    PLK_TRY(t.top.alloc((size_t)LZ_TOP_ROWS * LZ_TOP_STRIDE * 4));
    const size_t cnt = n_lo + n_hi + 7 + LZ_TOP_ROWS;
    k_plonk_xs<P><<<(unsigned)((cnt + 127) / 128), 128, 0, stream>>>((const uint4*)pw, log_t, log_domain, (uint4*)t.xs_lo.p, (uint4*)t.xs_hi.p, (uint4*)t.xs_lo_z.p,
                                                                     (uint4*)t.xs_hi_z.p, (uint4*)t.small.p, (uint32_t*)t.top.p);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

template <class P> PLK_DI Fe<P> plonk_x(const uint4* lo, const uint4* hi, size_t i) {
    const Fe<P> a = fe_load<P>(lo + (i & (((size_t)1 << XS_LO_LOG) - 1)) * 2);
    if ((i >> XS_LO_LOG) == 0) return a;
    return fe_mul<P>(a, fe_load<P>(hi + (i >> XS_LO_LOG) * 2));
}

// ---- product scans of the grand products (permutation Z, plonk.hip; Plookup Z, plookup.hip) ----
constexpr int PERM_SCAN_LANES = 1024;
template <class P> using LzP = Lz<P, 9>;  // every product: below (9 / 8) p with exact limbs
template <class P> PLK_DI LzP<P> lz_shfl_up(const LzP<P>& a, int d) {
    LzP<P> r;
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.v.l[i] = __shfl_up(a.v.l[i], d);
    return r;
}
// exclusive product scan of v over the workgroup (NW waves): wave shuffles, then the wave totals through LDS
template <class P, int NW> PLK_DI LzP<P> wg_exclusive_product(LzP<P> v, uint32_t (*s_wave)[FzCfg<P>::NZ]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const LzP<P> one = lz_one<P>().template widen<9>();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const LzP<P> o = lz_shfl_up<P>(v, d);
        if (lane >= d) v = v * o;
    }
    LzP<P> ex = lz_shfl_up<P>(v, 1);
    if (lane == 0) ex = one;
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < FzCfg<P>::NZ; ++i) s_wave[w][i] = v.v.l[i];
    }
    __syncthreads();
    for (int k = 0; k < w && k < NW; ++k) {
        LzP<P> t;
#pragma unroll
        for (int i = 0; i < FzCfg<P>::NZ; ++i) t.v.l[i] = s_wave[k][i];
        ex = ex * t;
    }
    return ex;
}

// the tile totals -> exclusive tile prefixes (times R, so that k_perm_fix's one product lands in the reference's form); one workgroup
template <class P>
__global__ void __launch_bounds__(PERM_SCAN_LANES) k_perm_tiles(uint32_t* __restrict__ tile_tot, size_t tiles, const unsigned* __restrict__ zeros,
                                                                uint32_t* __restrict__ status) {
    __shared__ uint32_t s_wave[PERM_SCAN_LANES / 64][FzCfg<P>::NZ];
    const LzP<P> one = lz_one<P>().template widen<9>();
    const size_t per = (tiles + PERM_SCAN_LANES - 1) / PERM_SCAN_LANES;
    const size_t b = (size_t)threadIdx.x * per, e = b + per < tiles ? b + per : tiles;
    LzP<P> run = one;
    for (size_t k = b; k < e; ++k) {
        const LzP<P> v{limbs_load<P>(tile_tot, k)};
        limbs_store<P>(tile_tot, k, run.v);
        run = run * v;
    }
    const LzP<P> ex = wg_exclusive_product<P, PERM_SCAN_LANES / 64>(run, s_wave);
    const LzP<P> c = ex * Lz<P, 8>{fz_const_rprime_to_r<P>()};
    for (size_t k = b; k < e; ++k) limbs_store<P>(tile_tot, k, (LzP<P>{limbs_load<P>(tile_tot, k)} * c).v);
    if (threadIdx.x == PERM_SCAN_LANES - 1 && status) {
        const Fe<P> total = lz_to_rform<P>(ex * run), one_r = fe_one<P>();
        bool is_one = true;
#pragma unroll
        for (int i = 0; i < P::NL; ++i) is_one = is_one && total.v[i] == one_r.v[i];
        status[0] = zeros[0];
        status[1] = zeros[0] == 0 && zeros[1] == 0 && is_one ? 1u : 0u;
    }
}

}  // namespace plk
