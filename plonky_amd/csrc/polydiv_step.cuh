// polydiv_step.cuh -- the lane-level arithmetic of the low-degree polynomial division (polydiv.hip), kept apart from the kernels so that
// tests/poly_division_host_replay.cpp can walk the same code on the host (fp.cuh / fz.cuh are plain C++ outside hipcc).
//
// Division of a by a MONIC b' of degree k, from the top coefficient down, with the running remainder R[0..k) as state.  One step
// with the next coefficient c:  t = R[k-1] (the quotient coefficient of that position),  R[i] <- R[i-1] - t b'[i],  R[0] <- c - t b'[0].
// Lane i of a group holds R[i] and -b'[i]; the table holds -b' in canonical R'-form, so a product with it is a stored word again.
//
// Bounds (fz.cuh: a multiplicand below R'/8 >= 16 p with carried limbs, the other operand exactly normalised):
//   * lazy form, k <= PDIV_LAZY_MAX_K = 8: a product is below t p / R' + p <= 1.125 p for t < 16 p; a value gains one product per
//     lane it passes, so t = R[k-1] < p + 8 * 1.125 p = 10 p.  No reduction inside the step.
//   * reduced form, k > 8: every step ends in fz_reduce_small (below 2 p): t < 2 p, the sum below 3.02 p < R'/4.
#pragma once
#include "fp.cuh"
#include "fz.cuh"

namespace plk {

constexpr int PDIV_S_LOG = 8;                 // a segment: S = 256 consecutive coefficients, one group of lanes
constexpr int PDIV_S = 1 << PDIV_S_LOG;
constexpr int PDIV_B_LOG = 6;                 // a scan block: B = 64 segments; more than one block takes the second scan level
constexpr int PDIV_B = 1 << PDIV_B_LOG;
constexpr int PDIV_MAX_K = 32;                // PLK_POLY_DIV_MAX_DEGREE
constexpr int PDIV_LAZY_MAX_K = 8;
constexpr int PDIV_GROUP = 6;                 // products per shared reduction (FZ_WIDE_UNITS)
static_assert(PDIV_GROUP <= FZ_WIDE_UNITS, "column bound of the shared reduction");

// R[i] <- prev + t * (-b'[i]);  prev = R[i-1], or the next coefficient on lane 0
template <class P, bool REDUCE> PLK_DI Fz<P> pdiv_lane_step(const Fz<P>& prev, const Fz<P>& t, const Fz<P>& negb) {
    const Fz<P> r = fz_add<P>(prev, fz_mul<P>(t, negb));
    if constexpr (REDUCE) return fz_reduce_small<P>(r);
    else return r;
}

// a lazy value (below 16 p) times an R'-form factor -> the stored word; the factor is 1 (fz_one_rprime) or 1 / lead
template <class P> PLK_DI Fe<P> pdiv_settle(const Fz<P>& v, const Fz<P>& factor) { return fz_to_fe_canonical<P>(fz_mul<P>(v, factor)); }

// rho + sum_{j < kp} x(j) m(j): a row of the k x k transition times a state (the scan), or an entry of a matrix square (the table).
// x(j): carried limbs, value below 2 p; m(j): exactly normalised, canonical.  Six products share a reduction (below 1.05 p each
// time), at most six groups for kp = 32: the total stays below 7.3 p + rho and leaves through one product with 1.
template <class P, class X, class M> PLK_DI Fe<P> pdiv_row(const Fe<P>& rho, int kp, X x, M m) {
    Fz<P> total = fz_from_fe<P>(rho);
    for (int j0 = 0; j0 < kp; j0 += PDIV_GROUP) {
        FzWide<P> w;
        fz_wide_clear<P>(w);
#pragma unroll
        for (int t = 0; t < PDIV_GROUP; ++t)
            if (j0 + t < kp) fz_wide_mac<P>(w, x(j0 + t), m(j0 + t));
        total = fz_add<P>(total, fz_wide_reduce<P>(w));
    }
    return pdiv_settle<P>(total, fz_one_rprime<P>());
}

// entry (row i, column j) of the companion matrix of b' padded to kp x kp, canonical R'-form: column j < k - 1 is e_(j+1), column
// k - 1 is -b', everything else zero.  Its 2^e-th power has X^(2^e + j) mod b' in column j.
template <class P> PLK_DI Fe<P> pdiv_companion_entry(int i, int j, int k, const Fe<P>& negb_i_rprime) {
    if (j < k - 1 && i == j + 1) return fz_to_fe_canonical<P>(fz_one_rprime<P>());
    if (j == k - 1 && i < k) return negb_i_rprime;
    return fe_zero<P>();
}

}  // namespace plk
