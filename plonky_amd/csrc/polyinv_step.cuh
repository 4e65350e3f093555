// polyinv_step.cuh -- the per-lane steps of the power-series inverse and of the general polynomial division (polydiv_newton.hip), kept
// apart from the kernels so that tests/polyinv_host_replay.cpp can walk the same code on the host (fp.cuh / fz.cuh are plain C++
// outside hipcc): the seed recurrence, the pointwise steps on the evaluations, the index maps and the subtraction of the remainder.
//
// The reference reverses coefficient arrays (Polynomial::rev, polynomial.rs:299-327).  Here no reversed array exists: on a cyclic
// domain of N points the reversal of x is x read at index -k mod N, up to a rotation, and both are index arithmetic:
//   * evaluations: FFT(x)[(N - k) mod N] are the evaluations of x(1 / X)               -> pinv_neg_index
//   * coefficients: a product with x(1 / X) X^s in place of x comes out rotated by s   -> pinv_shift_index
// polydiv_newton.hip says which product uses which.
//
// Forms: coefficients and evaluations are the reference's words (R-form, canonical).  The evaluations of ONE factor of every product
// are stored in canonical R'-form (the transform's store hook multiplies by R' / R, as poly.hip does for Polynomial::mul), so that a
// product on 29-bit limbs (fz.cuh) of an R'-form and an R-form value is an R-form value again: x R' * y R / R' = x y R.
// Bounds (fz.cuh): an operand loaded from canonical words has exact limbs and a value below p; fz_sqr / fz_mul return exact limbs and a
// value below a b / R' + p, so g^2 is below 1.01 p and g^2 h below 1.01 p p / R' + p < 2 p: one conditional subtraction settles it.
#pragma once
#include <stddef.h>

#include "fp.cuh"
#include "fz.cuh"

namespace plk {

constexpr int PINV_SEED_LOG = 6;               // g mod X^SEED comes from the triangular recurrence (one workgroup); the first
constexpr int PINV_SEED = 1 << PINV_SEED_LOG;  // Newton level then runs transforms of 4 SEED = 256 points
constexpr uint32_t PINV_STATUS_NO_INVERSE = 1u;  // bit 0 of the status word: h[0] == 0
constexpr uint32_t PINV_STATUS_ZERO_LEAD = 2u;   // bit 1: b[k] == 0

// ---- index maps ----
// coefficient j of the series to invert: h[j], or rev(b)[j] = b[len - 1 - j]; false: it reads as zero (j >= len)
PLK_DI bool pinv_series_index(bool reversed, size_t len, size_t j, size_t& src) {
    if (j >= len) return false;
    src = reversed ? len - 1 - j : j;
    return true;
}
// -k mod N, N a power of two
PLK_DI size_t pinv_neg_index(size_t k, size_t n) { return (n - k) & (n - 1); }
// t - shift mod N, N a power of two (the difference may wrap around 2^64: N divides it)
PLK_DI size_t pinv_shift_index(size_t t, size_t shift, size_t n) { return (t - shift) & (n - 1); }
// the quotient's output: q[s] = product[s] below m, zero from m to q_len; false: zero
PLK_DI bool pinv_quotient_index(size_t s, size_t m, size_t& src) {
    src = s;
    return s < m;
}

// ---- the seed: g_0 = 1 / h_0,  g_i = -(1 / h_0) sum_{j = 1..i} h_j g_(i - j) ----
// lane t keeps acc_t = sum_{j >= 1} h_j g_(t - j) over the g known so far; step i: lane i finishes g_i, lanes t > i take it in
template <class P> PLK_DI Fe<P> pinv_seed_coeff(size_t i, const Fe<P>& acc, const Fe<P>& inv, const Fe<P>& neg_inv) { return i == 0 ? inv : fe_mul<P>(neg_inv, acc); }
template <class P> PLK_DI Fe<P> pinv_seed_accumulate(const Fe<P>& acc, const Fe<P>& h_t_minus_i, const Fe<P>& g_i) { return fe_add<P>(acc, fe_mul<P>(h_t_minus_i, g_i)); }

// ---- pointwise steps: gp an evaluation in R'-form, y in R-form, both canonical ----
// Newton level l -> 2 l:  g (2 - h g) = 2 g - g^2 h, and below X^l the new g is the old one: only g^2 h is transformed back
template <class P> PLK_DI Fe<P> pinv_newton_point(const Fe<P>& gp, const Fe<P>& h) {
    return fz_to_fe_canonical<P>(fz_mul<P>(fz_sqr<P>(fz_from_fe<P>(gp)), fz_from_fe<P>(h)));
}
template <class P> PLK_DI Fe<P> pinv_product_point(const Fe<P>& xp, const Fe<P>& y) { return fz_to_fe_canonical<P>(fz_mul<P>(fz_from_fe<P>(xp), fz_from_fe<P>(y))); }

// ---- coefficient steps ----
// g_t = -(g^2 h)_t for l <= t < 2 l
template <class P> PLK_DI Fe<P> pinv_update_coeff(const Fe<P>& g2h_t) { return fe_neg<P>(g2h_t); }
// rem_i = a_i - (q b)_i
template <class P> PLK_DI Fe<P> pinv_rem_coeff(const Fe<P>& a_i, const Fe<P>& qb_i) { return fe_sub<P>(a_i, qb_i); }

}  // namespace plk
