// rescue_step.cuh -- the pieces of the Rescue permutation (src/rescue.rs:70-88, src/mds.rs:43-77, Field::kth_root field.rs:346-375) that
// the kernels of rescue.hip and tests/rescue_host_replay.cpp share.  Plain C++17: under hipcc the field code is device code, under g++
// it is the host's.
//
//   rescue_kth_root_exponent   the exponent d of x^(1/k) = x^d, from P::MOD and a 32-bit k (integers only; host and device)
//   rescue_alpha               F::ALPHA: 5, or 11 where 5 does not permute the field (Bls12377Scalar)
//   rescue_mds_entry           the Cauchy matrix M[r][c] = 1 / ((W + r) - c)
//   rescue_pow                 x^d on lazy 29-bit limbs: fixed 4-bit windows over a table of the odd powers
//   rescue_pow_alpha           x^5 / x^11 as a fixed chain
//   rescue_mds_row             sum_c M[r][c] x_c + constant: four products under one reduction
//   rescue_permutation_step    one round of a whole state, the way a quad of lanes walks it (the host replay's loop)
//
// Forms.  A state element lives in R'-form (x 2^(29 NZ), fz.cuh) as a lazy value: below 4p, limbs carried.  The matrix entries and the
// round constants are R'-form too, fully reduced and cut into 29-bit limbs (one 32-bit word per limb, NZ words per element): a product
// of a state element with an entry, and a sum with a constant, stay in the state's form, and nothing is converted inside a round.
#pragma once
#include <stdint.h>

#include <utility>

#include "fp.cuh"
#include "fz.cuh"

#ifdef __HIPCC__
#define RESCUE_HD __host__ __device__ inline
#else
#define RESCUE_HD inline
#endif

namespace plk {

constexpr int RESCUE_WIDTH = 4;  // RESCUE_SPONGE_WIDTH: the one supported width
constexpr int RESCUE_RATE = 3;   // RESCUE_SPONGE_RATE
constexpr int RESCUE_WINDOW = 4;

// ---- the exponent of a k-th root ------------------------------------------------------------------------------------------------
// field.rs:346-375 takes the first n in 1 ..= k with k | p + n (p - 1) and returns x^(((p + n (p - 1)) / k) mod (p - 1)).  With
// m = n + 1 the numerator is m (p - 1) + 1, so the condition is m a = -1 (mod k) for a = (p - 1) mod k: solvable exactly when
// gcd(a, k) = gcd(p - 1, k) = 1, and then by one m in every run of k integers - the first n is m - 1 for the m in 2 ..= k + 1.
// Finding m through the inverse of a replaces the reference's walk over n (up to k steps); tests/rescue_ref.py walks.
// Returns false, and d = 0, when x^k does not permute the field (or k = 0).
template <class P> RESCUE_HD bool rescue_kth_root_exponent(uint32_t k, uint32_t (&d)[P::NL]) {
    constexpr int NL = P::NL;
    for (int i = 0; i < NL; ++i) d[i] = 0;
    if (k == 0) return false;
    uint32_t pm1[NL];
    for (int i = 0; i < NL; ++i) pm1[i] = P::MOD[i];
    pm1[0] -= 1u;  // p is odd
    uint64_t a = 0;
    for (int i = NL - 1; i >= 0; --i) a = ((a << 32) | pm1[i]) % k;
    // inverse of a mod k (extended Euclid on 64-bit integers)
    int64_t r0 = (int64_t)k, r1 = (int64_t)a, t0 = 0, t1 = 1;
    while (r1 != 0) {
        const int64_t q = r0 / r1, r2 = r0 - q * r1, t2 = t0 - q * t1;
        r0 = r1; r1 = r2; t0 = t1; t1 = t2;
    }
    if (r0 != 1) return false;  // gcd(k, p - 1) != 1
    const int64_t inv = ((t0 % (int64_t)k) + (int64_t)k) % (int64_t)k;
    uint64_t m = ((uint64_t)k - (uint64_t)inv) % k;  // -1 / a mod k
    while (m < 2) m += k;
    // numerator = m (p - 1) + 1, m < 2^33: NL + 2 words
    uint32_t num[NL + 2];
    {
        const uint64_t m_lo = m & 0xFFFFFFFFull, m_hi = m >> 32;  // m_hi is 0 or 1
        uint64_t carry = 1;
        for (int i = 0; i < NL + 2; ++i) {
            uint64_t acc = carry;
            carry = 0;
            if (i < NL) acc += (uint64_t)pm1[i] * m_lo;  // < 2^64 - 2^33 + 1 + carry: cannot wrap for carry < 2^33
            if (m_hi && i >= 1 && i - 1 < NL) {
                const uint64_t s = acc + pm1[i - 1];
                if (s < acc) carry += (uint64_t)1 << 32;
                acc = s;
            }
            num[i] = (uint32_t)acc;
            carry += acc >> 32;
        }
    }
    // divide by k (exact)
    uint64_t rem = 0;
    for (int i = NL + 1; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | num[i];
        num[i] = (uint32_t)(cur / k);
        rem = cur % k;
    }
    // reduce mod p - 1: the quotient is below 2 (p - 1) + 1, but loop rather than count
    for (;;) {
        bool ge = true;
        for (int i = NL + 1; i >= 0; --i) {
            const uint32_t b = i < NL ? pm1[i] : 0u;
            if (num[i] != b) {
                ge = num[i] > b;
                break;
            }
        }
        if (!ge) break;
        uint64_t borrow = 0;
        for (int i = 0; i < NL + 2; ++i) {
            const uint64_t b = (i < NL ? (uint64_t)pm1[i] : 0u) + borrow;
            borrow = (uint64_t)num[i] < b ? 1u : 0u;
            num[i] = (uint32_t)((uint64_t)num[i] - b);
        }
    }
    for (int i = 0; i < NL; ++i) d[i] = num[i];
    return true;
}

// bits of the exponent, and its 4-bit windows
template <int NL> RESCUE_HD int rescue_exponent_bits(const uint32_t (&d)[NL]) {
    for (int i = NL - 1; i >= 0; --i)
        if (d[i])
            for (int b = 31; b >= 0; --b)
                if ((d[i] >> b) & 1u) return 32 * i + b + 1;
    return 0;
}
RESCUE_HD int rescue_windows(int bits) { return (bits + RESCUE_WINDOW - 1) / RESCUE_WINDOW; }

// F::ALPHA: the smallest of 5 and 11 that permutes the field; 0 when neither does (none of the six fields)
template <class P> constexpr uint32_t rescue_alpha() {
    uint64_t m5 = 0, m11 = 0;
    for (int i = P::NL - 1; i >= 0; --i) {
        const uint32_t w = i == 0 ? P::MOD[0] - 1u : P::MOD[i];
        m5 = ((m5 << 32) | w) % 5u;
        m11 = ((m11 << 32) | w) % 11u;
    }
    return m5 != 0 ? 5u : m11 != 0 ? 11u : 0u;
}

// recommended_rounds (rescue.rs:123-125)
RESCUE_HD size_t rescue_rounds(size_t width, size_t security_bits) {
    const size_t r = (security_bits + 2 * width - 1) / (2 * width);
    return r < 10 ? 10 : r;
}

// ---- field side -------------------------------------------------------------------------------------------------------------------
// an R-form element (the reference's limbs) as a lazy R'-form value, and back as the one fully reduced R-form representative
template <class P> PLK_DI Fz<P> rescue_enter(const Fe<P>& v) { return fz_mul<P>(fz_from_fe<P>(v), fz_const_r_to_rprime<P>()); }
template <class P> PLK_DI Fe<P> rescue_leave(const Fz<P>& v) { return fz_to_fe_canonical<P>(fz_mul<P>(v, fz_const_rprime_to_r<P>())); }
// the table form: R'-form, fully reduced, exact 29-bit limbs
template <class P> PLK_DI Fz<P> rescue_table_form(const Fe<P>& v) { return fz_from_fe<P>(fz_to_fe_canonical<P>(rescue_enter<P>(v))); }

// M[r][c] = 1 / ((W + r) - c) (mds.rs:68-71), R-form
template <class P> PLK_DI Fe<P> rescue_mds_entry(int width, int r, int c) {
    Fe<P> s = fe_zero<P>();
    s.v[0] = (uint32_t)(width + r - c);  // 1 .. 2 W - 1
    return fe_inv<P>(fe_from_canonical<P>(s));
}

template <class P> PLK_DI Fz<P> rescue_words(const uint32_t* w) {
    Fz<P> r;
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.l[i] = w[i];
    return r;
}

// t[i] for a uniform i, every index a constant: the table stays in registers
template <class F, int... I> PLK_DI void rescue_static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> PLK_DI void rescue_static_for(F&& f) { rescue_static_for_impl(f, std::make_integer_sequence<int, N>{}); }
template <class P> PLK_DI Fz<P> rescue_pick(const Fz<P> (&t)[8], uint32_t i) {
    Fz<P> r = t[0];
    rescue_static_for<8>([&](auto K) {  // an unrolled loop is unrolled too late: the table would live in scratch memory
        constexpr int k = K.value;
        if constexpr (k != 0) {
            const bool hit = i == (uint32_t)k;
#pragma unroll
            for (int l = 0; l < FzCfg<P>::NZ; ++l) r.l[l] = hit ? t[k].l[l] : r.l[l];  // word by word: a copy of the struct goes through memory
        }
    });
    return r;
}

// x^d for the `windows` 4-bit digits of d (d != 0: the top digit is not zero), most significant first.  A digit o 2^s with o odd is
// 4 - s squarings, a product with x^o and s squarings, so the table holds the eight odd powers only.  The digits are the same for
// every lane (plk_uniform_u32 keeps them in scalar registers): no lane diverges.  Input below 4p with carried limbs; every
// intermediate value is what fz_mul / fz_sqr return (below 2p, exact limbs), never reduced further.
template <class P> PLK_DI Fz<P> rescue_pow(const Fz<P>& x, const uint32_t* d, int windows) {
    Fz<P> t[8];
    t[0] = x;
    const Fz<P> x2 = fz_sqr<P>(x);
    t[1] = fz_mul<P>(t[0], x2);
    t[2] = fz_mul<P>(t[1], x2);
    t[3] = fz_mul<P>(t[2], x2);
    t[4] = fz_mul<P>(t[3], x2);
    t[5] = fz_mul<P>(t[4], x2);
    t[6] = fz_mul<P>(t[5], x2);
    t[7] = fz_mul<P>(t[6], x2);
    Fz<P> r = fz_one_rprime<P>();  // windows == 0: x^0
    for (int w = windows - 1; w >= 0; --w) {
        const uint32_t dg = plk_uniform_u32((d[w >> 3] >> (RESCUE_WINDOW * (w & 7))) & 15u);
        int s = 0;
        while (dg != 0 && ((dg >> s) & 1u) == 0) ++s;
        if (w == windows - 1) {
            r = rescue_pick<P>(t, dg >> (s + 1));
        } else {
            const int before = dg ? RESCUE_WINDOW - s : RESCUE_WINDOW;
            for (int i = 0; i < before; ++i) r = fz_sqr<P>(r);
            if (dg) r = fz_mul<P>(r, rescue_pick<P>(t, dg >> (s + 1)));
        }
        if (dg)
            for (int i = 0; i < s; ++i) r = fz_sqr<P>(r);
    }
    return r;
}

// x^ALPHA: 3 products for 5, 5 for 11
template <class P> PLK_DI Fz<P> rescue_pow_alpha(const Fz<P>& x) {
    static_assert(rescue_alpha<P>() == 5u || rescue_alpha<P>() == 11u, "a field with no permuting alpha");
    const Fz<P> x2 = fz_sqr<P>(x), x4 = fz_sqr<P>(x2);
    if constexpr (rescue_alpha<P>() == 5u) {
        return fz_mul<P>(x4, x);
    } else {
        return fz_mul<P>(fz_mul<P>(fz_sqr<P>(x4), x2), x);
    }
}

// Column bound of the row sum below, in units of 2^29: four products of a carried limb (below 2^29 + 16: what fz_mul, fz_sqr and
// fz_add return) with an entry's exact limb, the quotient digits times the modulus, the carry, the constant.  A fully reduced value has no limb above bit BITS, so an entry of
// Bls12377Base (377 = 13 * 29 bits) has an empty fourteenth limb, which is what lets four products of 14 limbs share a column.
template <class P> struct RescueRowBound {
    static constexpr int NZ = FzCfg<P>::NZ;
    static constexpr int ENTRY_LIMBS = (P::BITS + 28) / 29;
    static constexpr bool holds() {
        for (int k = 0; k <= 2 * NZ - 2; ++k) {
            uint64_t units = 0;  // column / 2^29
            for (int i = 0; i < NZ; ++i) {
                const int j = k - i;
                if (j >= 0 && j < ENTRY_LIMBS) units += (uint64_t)RESCUE_WIDTH * ((1u << 29) + 16u);
                if (i < k && j >= 1 && j < NZ) units += FzCfg<P>::plimb(j);
            }
            units += 512;  // carry in (< 2^36), the 2^29 - 1 of the digit trick, a constant's limb
            if (units >= ((uint64_t)1 << 35)) return false;
        }
        return true;
    }
};

// row r of apply_mds plus the round constant: sum_c M[r][c] x_c + k_r (mds.rs:47-51, rescue.rs:78-79 / 83-84).  x_c: what fz_mul /
// fz_sqr return; m: the row's W entries, k: the constant, both in the table form.  Value below 4 (2p)(p) / R' + 2p < 3p.
template <class P> PLK_DI Fz<P> rescue_mds_row(const Fz<P> (&x)[RESCUE_WIDTH], const uint32_t* m, const uint32_t* k) {
    static_assert(RescueRowBound<P>::holds(), "four products and a constant overflow a 64-bit column");
    constexpr int NZ = FzCfg<P>::NZ;
    FzWide<P> w;
    fz_wide_clear<P>(w);
#pragma unroll
    for (int c = 0; c < RESCUE_WIDTH; ++c) fz_wide_mac<P>(w, x[c], rescue_words<P>(m + c * NZ));
    fz_wide_add<P>(w, rescue_words<P>(k));
    Fz<P> r = fz_wide_reduce<P>(w);
    return r;
}

// One round of a whole state (rescue.rs:75-85): step A with the root, step B with the power.  d / windows: the exponent of 1 / ALPHA;
// mds: W x W entries, row-major; ka / kb: the W constants of the two steps.  The kernels run the same calls with one element per
// lane and the x_c of a row fetched from the neighbouring lanes.
template <class P>
PLK_DI void rescue_permutation_step(Fz<P> (&state)[RESCUE_WIDTH], const uint32_t* d, int windows, const uint32_t* mds, const uint32_t* ka, const uint32_t* kb) {
    constexpr int NZ = FzCfg<P>::NZ;
    Fz<P> y[RESCUE_WIDTH];
    for (int e = 0; e < RESCUE_WIDTH; ++e) y[e] = rescue_pow<P>(state[e], d, windows);
    for (int e = 0; e < RESCUE_WIDTH; ++e) state[e] = rescue_mds_row<P>(y, mds + e * RESCUE_WIDTH * NZ, ka + e * NZ);
    for (int e = 0; e < RESCUE_WIDTH; ++e) y[e] = rescue_pow_alpha<P>(state[e]);
    for (int e = 0; e < RESCUE_WIDTH; ++e) state[e] = rescue_mds_row<P>(y, mds + e * RESCUE_WIDTH * NZ, kb + e * NZ);
}

}  // namespace plk
