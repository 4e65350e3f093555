// fe_sqrt.cuh -- Field::square_root (field.rs:440-472) on the arithmetic of fp.cuh, shared by the point decompression (serial.hip)
// and the two hashes to the curve (hash_to_curve.hip, rescue_h2c.hip).  Device code; fe_sqrt_with also serves the host replay of
// rescue_h2c_step.cuh.
#pragma once
#include "fp.cuh"
#include "tables.cuh"

namespace plk {

// x^e for a multi-limb exponent (little-endian 32-bit words)
template <class P> PLK_DI Fe<P> fe_pow_limbs(const Fe<P>& x, const uint32_t (&e)[P::NL]) {
    Fe<P> r = fe_one<P>();
    bool started = false;
    for (int i = P::NL - 1; i >= 0; --i)
        for (int b = 31; b >= 0; --b) {
            if (started) r = fe_sqr<P>(r);
            if ((e[i] >> b) & 1u) {
                r = started ? fe_mul<P>(r, x) : x;
                started = true;
            }
        }
    return r;
}

// Through the whole loop z = ROOT_2ADIC^(2^(TWO_ADICITY - v)), so the w of a step, z^(2^j) with j = v - k - 1, is
// ROOT_2ADIC^(2^(TWO_ADICITY - k - 1)) whatever the steps before it were.  The two ways to get it return the same element - every
// value is the one fully reduced representative - so the root, and with it its sign, is the same bit for bit.
template <class P> struct SqrtRootBySquaring {  // the reference's way: j squarings of z
    PLK_DI Fe<P> operator()(const Fe<P>& z, int j, int /*m*/) const {
        Fe<P> w = z;
        for (int s = 0; s < j; ++s) w = fe_sqr<P>(w);
        return w;
    }
};
#ifdef __HIPCC__
template <class P> struct SqrtRootFromTable {  // tab[m] = ROOT_2ADIC^(2^m), m < TWO_ADICITY, as fe_store leaves them
    const uint4* tab;
    PLK_DI Fe<P> operator()(const Fe<P>& /*z*/, int /*j*/, int m) const { return fe_load<P>(tab + (size_t)m * (P::NL / 4)); }
};
#endif

// Tonelli-Shanks with z = g^T, T = (p - 1) / 2^TWO_ADICITY.  Returns false for a non-residue (the reference tests Euler's
// criterion first; here the same fact falls out of the loop: b = a^T has order dividing 2^(adicity - 1) exactly when a is a square).
template <class P, class RootPow> PLK_DI bool fe_sqrt_with(const Fe<P>& a, Fe<P>& root, const RootPow& root_pow) {
    if (fe_is_zero<P>(a)) {
        root = a;
        return true;
    }
    // (T - 1) / 2 from the modulus: T = (p - 1) >> adicity is odd
    uint32_t e[P::NL];
    {
        uint32_t t[P::NL];
        for (int i = 0; i < P::NL; ++i) t[i] = P::MOD[i];
        t[0] -= 1u;  // p is odd
        constexpr int sh = P::TWO_ADICITY + 1;  // (T - 1) / 2 = (p - 1) >> (adicity + 1), T odd
        for (int i = 0; i < P::NL; ++i) {
            const int src = i + sh / 32, bit = sh % 32;
            uint32_t lo = src < P::NL ? t[src] : 0u, hi = src + 1 < P::NL ? t[src + 1] : 0u;
            e[i] = bit ? (lo >> bit) | (hi << (32 - bit)) : lo;
        }
    }
    Fe<P> z = fe_const<P>(P::ROOT_2ADIC);
    Fe<P> w = fe_pow_limbs<P>(a, e);
    Fe<P> x = fe_mul<P>(w, a);
    Fe<P> b = fe_mul<P>(x, w);
    const Fe<P> one = fe_one<P>();
    int v = P::TWO_ADICITY;
    while (!fe_eq<P>(b, one)) {
        int k = 0;
        Fe<P> b2k = b;
        while (!fe_eq<P>(b2k, one)) {
            b2k = fe_sqr<P>(b2k);
            ++k;
            if (k >= v) return false;  // not a square
        }
        w = root_pow(z, v - k - 1, P::TWO_ADICITY - k - 1);
        z = fe_sqr<P>(w);
        b = fe_mul<P>(b, z);
        x = fe_mul<P>(x, w);
        v = k;
    }
    root = x;
    return true;
}
template <class P> PLK_DNI bool fe_sqrt(const Fe<P>& a, Fe<P>& root) { return fe_sqrt_with<P>(a, root, SqrtRootBySquaring<P>{}); }
#ifdef __HIPCC__
// the same root with the table of powers in place of the squarings (k_h2c_root_table below builds the table)
template <class P> PLK_DNI bool fe_sqrt_tabled(const Fe<P>& a, Fe<P>& root, const uint4* tab) {
    return fe_sqrt_with<P>(a, root, SqrtRootFromTable<P>{tab});
}

// tab[m] = ROOT_2ADIC^(2^m), m < TWO_ADICITY: the w of every Tonelli-Shanks step, for fe_sqrt_tabled (one lane, once per call)
template <class P> __global__ void k_h2c_root_table(uint4* __restrict__ tab) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Fe<P> w = fe_const<P>(P::ROOT_2ADIC);
    for (int m = 0; m < P::TWO_ADICITY; ++m) {
        fe_store<P>(tab + (size_t)m * (P::NL / 4), w);
        w = fe_sqr<P>(w);
    }
}
#endif

}  // namespace plk
