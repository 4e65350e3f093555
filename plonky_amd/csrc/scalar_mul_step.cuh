// scalar_mul_step.cuh -- the per-element steps of scalar_mul.hip, kept apart from the kernels so that tests/scalar_mul_host_replay.cpp
// walks the same code on the host.  Plain C++17 outside hipcc.
//
//   halo_chunk / halo_n_value     the bits of n(s) (plonk_util.rs:50-75) and its value a ZETA_SCALAR + b
//   halo_addend / halo_chain_step Algorithm 1 (plonk_util.rs:79-110): Acc = 2 Acc + S, S one of +-P, +-phi(P), picked by value
//   sm_recode_w2 / sm_digit_w2    carry-based signed base-4 digits of a 256-bit integer, digits in {-1, 0, 1, 2}
//   sm_glv_code / sm_glv_addend   the joint walk over the two halves of glv_split: P, phi P, P +- phi P, picked by value
//
// The reference's (ZETA, ZETA_SCALAR) is one of the two pairs of primitive cube roots; the lattice of glv_params.cuh was generated
// over (BETA, LAMBDA), which is the reference's pair on Tweedledee, Tweedledum and Pallas and the OTHER pair on Vesta (its ZETA is
// Pallas's ZETA_SCALAR and the other way round, vesta_curve.rs:22-33, while the generator took the smaller root on either side).
// The split k = k1 + k2 LAMBDA works with either pair; n(s) does not: halo_zeta / halo_zeta_scalar square BETA and LAMBDA there.
#pragma once
#include <stdint.h>

#include "ecz.cuh"
#include "glv.cuh"

namespace plk {

template <class Glv> struct HaloZeta { static constexpr bool SQUARED = false; };
template <> struct HaloZeta<VestaGlv> { static constexpr bool SQUARED = true; };

// HaloCurve::ZETA (base field) and ZETA_SCALAR (scalar field), Montgomery form
template <class C> PLK_DI Fe<typename C::FP> halo_zeta() {
    using FP = typename C::FP;
    Fe<FP> b;
#pragma unroll
    for (int k = 0; k < FP::NL; ++k) b.v[k] = C::Glv::BETA[k];
    b = fe_from_canonical<FP>(b);
    return HaloZeta<typename C::Glv>::SQUARED ? fe_sqr<FP>(b) : b;
}
template <class C> PLK_DI Fe<typename C::SP> halo_zeta_scalar() {
    using SP = typename C::SP;
    Fe<SP> l;
#pragma unroll
    for (int k = 0; k < SP::NL; ++k) l.v[k] = C::Glv::LAMBDA[k];
    l = fe_from_canonical<SP>(l);
    return HaloZeta<typename C::Glv>::SQUARED ? fe_sqr<SP>(l) : l;
}

// bit j of a little-endian word array
PLK_DI uint32_t sm_bit(const uint32_t* k, int j) { return (k[j >> 5] >> (j & 31)) & 1u; }

// chunk c of to_canonical_bool_vec() (field.rs:104-112: least significant bit first): bit_lo | bit_hi << 1
PLK_DI uint32_t halo_chunk(const uint32_t* k, int c) { return (k[c >> 4] >> ((2 * c) & 31)) & 3u; }

// n(s) over the low `bits` bits of the canonical k (bits even): chunks from index 0, so the lowest chunk ends up most significant
template <class C> PLK_DI Fe<typename C::SP> halo_n_value(const uint32_t* k, unsigned bits) {
    using SP = typename C::SP;
    const Fe<SP> one = fe_one<SP>(), minus_one = fe_neg<SP>(one);
    Fe<SP> a = fe_zero<SP>(), b = fe_zero<SP>();
    for (unsigned c = 0; c < bits / 2; ++c) {
        const uint32_t ch = halo_chunk(k, (int)c);
        const Fe<SP> sign = (ch & 1u) ? one : minus_one;
        a = fe_dbl<SP>(a);
        b = fe_dbl<SP>(b);
        const Fe<SP> a1 = fe_add<SP>(a, sign), b1 = fe_add<SP>(b, sign);
#pragma unroll
        for (int i = 0; i < SP::NL; ++i) {
            a.v[i] = (ch & 2u) ? a1.v[i] : a.v[i];
            b.v[i] = (ch & 2u) ? b.v[i] : b1.v[i];
        }
    }
    return fe_add<SP>(fe_mul<SP>(a, halo_zeta_scalar<C>()), b);
}

// R-form words of the interface -> canonical R'-form working limbs (what xyzzz_madd takes as an affine operand)
template <class FP> PLK_DI Fz<FP> sm_enter(const Fe<FP>& v) {
    return fz_from_fe<FP>(fz_to_fe_canonical<FP>(fz_mul<FP>(fz_from_fe<FP>(v), fz_const_r_to_rprime<FP>())));
}

// the addend of one chunk: (x or ZETA x, y or -y).  x, y canonical; zx = ZETA x (< 2p, exactly normalised); ny = 2p - y
template <class FP> PLK_DI void halo_addend(uint32_t ch, const Fz<FP>& x, const Fz<FP>& zx, const Fz<FP>& y, const Fz<FP>& ny, Fz<FP>& tx, Fz<FP>& ty) {
#pragma unroll
    for (int i = 0; i < FzCfg<FP>::NZ; ++i) {
        tx.l[i] = (ch & 2u) ? zx.l[i] : x.l[i];
        ty.l[i] = (ch & 1u) ? y.l[i] : ny.l[i];
    }
}
// Acc = 2 Acc + S (plonk_util.rs:106): the complete forms of ecz.cuh take Acc = O, Acc = S and Acc = -S
template <class FP> PLK_DI void halo_chain_step(XyzzZ<FP>& acc, uint32_t ch, const Fz<FP>& x, const Fz<FP>& zx, const Fz<FP>& y, const Fz<FP>& ny) {
    Fz<FP> tx, ty;
    halo_addend<FP>(ch, x, zx, y, ny, tx, ty);
    acc = xyzzz_dbl<FP>(acc);
    xyzzz_madd<FP>(acc, tx, ty);
}

// ---- signed base-4 digits (curves without the endomorphism) ----
// k + 0x5555...55 carries exactly where a base-4 digit of k (plus the carry from below) reaches 3: digit j of the sum, minus 1, is
// the signed digit d_j in {-1, 0, 1, 2}, and  sum_j d_j 4^j + carry 4^128 = k.  The table of a walk over them is {P, 2P}.
constexpr int SM_W2_DIGITS = 128;
PLK_DI uint32_t sm_recode_w2(const uint32_t* k, uint32_t (&e)[8]) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)k[i] + 0x55555555u;
        e[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;  // the digit of weight 4^128: 0 for every k < 2^255 (k + (2^256 - 1) / 3 < 2^256), so for every scalar field here
}
PLK_DI int sm_digit_w2(const uint32_t (&e)[8], int j) { return (int)((e[j >> 4] >> ((2 * j) & 31)) & 3u) - 1; }

// the addend of one signed digit over {P, 2P}: d = 0 adds nothing (`skip`), d = -1 negates
template <class FP> PLK_DI void sm_w2_addend(int d, const Fz<FP>& x1, const Fz<FP>& y1, const Fz<FP>& x2, const Fz<FP>& y2, Fz<FP>& tx, Fz<FP>& ty, bool& two) {
    two = d == 2;
    Fz<FP> y;
#pragma unroll
    for (int i = 0; i < FzCfg<FP>::NZ; ++i) {
        tx.l[i] = two ? x2.l[i] : x1.l[i];
        y.l[i] = two ? y2.l[i] : y1.l[i];
    }
    const Fz<FP> ny = fz_neg_canonical<FP>(y);
#pragma unroll
    for (int i = 0; i < FzCfg<FP>::NZ; ++i) ty.l[i] = d < 0 ? ny.l[i] : y.l[i];
}

// ---- the joint walk over the two halves of glv_split ----
// k1, k2: magnitudes below 2^GLV_BITS (sign bit cleared).  Column j: 0 nothing, 1 P, 2 phi P, 3 both
PLK_DI uint32_t sm_glv_code(const uint32_t* k1, const uint32_t* k2, int j) { return sm_bit(k1, j) | (sm_bit(k2, j) << 1); }
// n1, n2: the halves are negative.  The addend of column code c:
//   1: +-P = (x, +-y)      2: +-phi P = (beta x, +-y)
//   3: signs agree: +-(P + phi P) = -+phi^2 P = (beta^2 x, -+y) [1 + lambda + lambda^2 = 0];  signs differ: +-(P - phi P) = +-(dx, dy)
// x3 / y3: (beta^2 x, y) when the signs agree, (dx, dy) when they differ - chosen once per element by the caller.
template <class FP>
PLK_DI void sm_glv_addend(uint32_t c, bool n1, bool n2, const Fz<FP>& x, const Fz<FP>& bx, const Fz<FP>& x3, const Fz<FP>& y, const Fz<FP>& y3, Fz<FP>& tx, Fz<FP>& ty) {
    const bool both = c == 3u;
    const bool neg = c == 2u ? n2 : (both && n1 == n2) ? !n1 : n1;
    Fz<FP> yy;
#pragma unroll
    for (int i = 0; i < FzCfg<FP>::NZ; ++i) {
        tx.l[i] = both ? x3.l[i] : c == 2u ? bx.l[i] : x.l[i];
        yy.l[i] = both ? y3.l[i] : y.l[i];
    }
    const Fz<FP> ny = fz_neg_canonical<FP>(yy);
#pragma unroll
    for (int i = 0; i < FzCfg<FP>::NZ; ++i) ty.l[i] = neg ? ny.l[i] : yy.l[i];
}

// P - phi(P) for an affine P = (x, y), R-form; inv = 1 / ((beta - 1) x).  Slope (-y - y) / (beta x - x)
template <class FP> PLK_DI void sm_diff_with_phi(const Fe<FP>& x, const Fe<FP>& y, const Fe<FP>& beta_x, const Fe<FP>& inv, Fe<FP>& dx, Fe<FP>& dy) {
    const Fe<FP> lam = fe_mul<FP>(fe_neg<FP>(fe_dbl<FP>(y)), inv);
    dx = fe_sub<FP>(fe_sub<FP>(fe_sqr<FP>(lam), x), beta_x);
    dy = fe_sub<FP>(fe_mul<FP>(lam, fe_sub<FP>(x, dx)), y);
}
// the denominator of P - phi(P), and the five coordinates a lane walks with: x, y, beta x and the addend of a column with both bits
// set - (beta^2 x, y) [negated by the selection] when the halves' signs agree, P - phi(P) when they differ.  inv = 1 / sm_glv_den
template <class C> PLK_DI Fe<typename C::FP> sm_glv_beta() {
    using FP = typename C::FP;
    Fe<FP> bc;
#pragma unroll
    for (int k = 0; k < FP::NL; ++k) bc.v[k] = C::Glv::BETA[k];
    return fe_from_canonical<FP>(bc);
}
template <class C> PLK_DI Fe<typename C::FP> sm_glv_den(const Fe<typename C::FP>& px) {
    using FP = typename C::FP;
    return fe_mul<FP>(fe_sub<FP>(sm_glv_beta<C>(), fe_one<FP>()), px);
}
template <class C>
PLK_DI void sm_glv_table(const Fe<typename C::FP>& px, const Fe<typename C::FP>& py, const Fe<typename C::FP>& inv, bool n1, bool n2, Fz<typename C::FP>& x,
                         Fz<typename C::FP>& y, Fz<typename C::FP>& bx, Fz<typename C::FP>& x3, Fz<typename C::FP>& y3) {
    using FP = typename C::FP;
    const Fe<FP> beta_r = sm_glv_beta<C>();
    const Fe<FP> bx_r = fe_mul<FP>(beta_r, px);
    Fe<FP> x3_r = fe_mul<FP>(beta_r, bx_r), y3_r = py;
    if (n1 != n2) sm_diff_with_phi<FP>(px, py, bx_r, inv, x3_r, y3_r);
    x = sm_enter<FP>(px);
    y = sm_enter<FP>(py);
    bx = sm_enter<FP>(bx_r);
    x3 = sm_enter<FP>(x3_r);
    y3 = sm_enter<FP>(y3_r);
}
// working limbs -> R-form words, canonical (the way back from sm_enter)
template <class FP> PLK_DI Fe<FP> sm_leave(const Fz<FP>& v) { return fz_to_fe_canonical<FP>(fz_mul<FP>(v, fz_const_rprime_to_r<FP>())); }

// 2P for an affine P with y != 0, R-form; inv = 1 / (2y).  Slope 3 x^2 / 2y (a = 0)
template <class FP> PLK_DI void sm_affine_double(const Fe<FP>& x, const Fe<FP>& y, const Fe<FP>& inv, Fe<FP>& x2, Fe<FP>& y2) {
    const Fe<FP> xx = fe_sqr<FP>(x);
    const Fe<FP> lam = fe_mul<FP>(fe_add<FP>(fe_dbl<FP>(xx), xx), inv);
    x2 = fe_sub<FP>(fe_sqr<FP>(lam), fe_dbl<FP>(x));
    y2 = fe_sub<FP>(fe_mul<FP>(lam, fe_sub<FP>(x, x2)), y);
}

// ---- one chain step on the working limbs, and the chains the kernels run (one lane = one element) ----
// column j of the joint walk: Acc = 2 Acc, then + the column's addend unless both bits are clear
template <class FP>
PLK_DI void sm_glv_chain_step(XyzzZ<FP>& acc, uint32_t c, bool n1, bool n2, const Fz<FP>& x, const Fz<FP>& bx, const Fz<FP>& x3, const Fz<FP>& y, const Fz<FP>& y3) {
    acc = xyzzz_dbl<FP>(acc);
    if (c != 0u) {
        Fz<FP> tx, ty;
        sm_glv_addend<FP>(c, n1, n2, x, bx, x3, y, y3, tx, ty);
        xyzzz_madd<FP>(acc, tx, ty);
    }
}
// signed digit d of the base-4 walk: Acc = 4 Acc, then + d P unless d = 0 or the addend is 2P = O (two_ident: P is a 2-torsion point)
template <class FP>
PLK_DI void sm_w2_chain_step(XyzzZ<FP>& acc, int d, bool two_ident, const Fz<FP>& x1, const Fz<FP>& y1, const Fz<FP>& x2, const Fz<FP>& y2) {
    acc = xyzzz_dbl<FP>(xyzzz_dbl<FP>(acc));
    if (d != 0 && !(d == 2 && two_ident)) {
        Fz<FP> tx, ty;
        bool two;
        sm_w2_addend<FP>(d, x1, y1, x2, y2, tx, ty, two);
        xyzzz_madd<FP>(acc, tx, ty);
    }
}
// the denominator the batched inversion takes for the second table point: (beta - 1) x, or 2y without the endomorphism
template <class C> PLK_DI Fe<typename C::FP> sm_table_den(const Fe<typename C::FP>& px, const Fe<typename C::FP>& py) {
    using FP = typename C::FP;
    if constexpr (C::Glv::ENABLED) return sm_glv_den<C>(px);
    else return fe_dbl<FP>(py);
}
// [s] (px, py) for a canonical s and a point that is not the identity; inv = 1 / sm_table_den (0 where that is 0)
template <class C> PLK_DI XyzzZ<typename C::FP> sm_scalar_mul_chain(const uint32_t (&s)[8], const Fe<typename C::FP>& px, const Fe<typename C::FP>& py, const Fe<typename C::FP>& inv) {
    using FP = typename C::FP;
    XyzzZ<FP> acc = xyzzz_identity<FP>();
    if constexpr (C::Glv::ENABLED) {
        uint32_t k1[8], k2[8];
        glv_split<typename C::Glv>(s, k1, k2);
        const bool n1 = (k1[7] >> 31) != 0, n2 = (k2[7] >> 31) != 0;
        k1[7] &= 0x7fffffffu;
        k2[7] &= 0x7fffffffu;
        Fz<FP> x, y, bx, x3, y3;
        sm_glv_table<C>(px, py, inv, n1, n2, x, y, bx, x3, y3);
        for (int j = GLV_BITS - 1; j >= 0; --j) sm_glv_chain_step<FP>(acc, sm_glv_code(k1, k2, j), n1, n2, x, bx, x3, y, y3);
    } else {
        uint32_t e[8];
        (void)sm_recode_w2(s, e);
        const bool two_ident = fe_is_zero<FP>(py);  // a 2-torsion point: 2P = O
        Fe<FP> x2_r = px, y2_r = py;
        if (!two_ident) sm_affine_double<FP>(px, py, inv, x2_r, y2_r);
        const Fz<FP> x1 = sm_enter<FP>(px), y1 = sm_enter<FP>(py), x2 = sm_enter<FP>(x2_r), y2 = sm_enter<FP>(y2_r);
        for (int j = SM_W2_DIGITS - 1; j >= 0; --j) sm_w2_chain_step<FP>(acc, sm_digit_w2(e, j), two_ident, x1, y1, x2, y2);
    }
    return acc;
}
// [n(s)] (px, py) by Algorithm 1 over the low `bits` bits of the canonical s; the point is not the identity
template <class C> PLK_DI XyzzZ<typename C::FP> halo_n_mul_chain(const uint32_t (&s)[8], unsigned bits, const Fe<typename C::FP>& px, const Fe<typename C::FP>& py) {
    using FP = typename C::FP;
    const Fz<FP> x = sm_enter<FP>(px), y = sm_enter<FP>(py), zx = sm_enter<FP>(fe_mul<FP>(halo_zeta<C>(), px)), ny = fz_neg_canonical<FP>(y);
    XyzzZ<FP> acc = xyzzz_identity<FP>();
    for (unsigned c = 0; c < bits / 2; ++c) halo_chain_step<FP>(acc, halo_chunk(s, (int)c), x, zx, y, ny);
    return acc;
}

}  // namespace plk
