// rescue_h2c_step.cuh -- hash_base_field_to_curve (src/hash_to_curve.rs:78-104) for one seed, kept apart from the kernel
// (rescue_h2c.hip) so that tests/rescue_h2c_host_replay.cpp walks the same code on the host.  Plain C++17: under hipcc the field code
// is device code, under g++ it is the host's.
//
//   rescue_h2c_from_u64   from_canonical_u32 / from_canonical_usize (field.rs:124-132): the seed of the integer form, the counter i
//   rescue_h2c_y_neg      outputs[1].to_canonical_bool_vec()[0] (field.rs:104-112): bit 0 of limb 0 of the canonical form
//   rescue_h2c_point      the curve half of a try: x^3 + B, Field::square_root, the sign
//   rescue_h2c_tries      tries i_first ..= i_last of one seed; the sponge and the root come from the caller: the kernel hands in the
//                         permutation over a quad of lanes and the tabled root, the host replay rescue_h2c_sponge_state and fe_sqrt
//   rescue_h2c_sponge_state   rescue_sponge([seed, i], 2): one chunk, one block, one permutation of a whole state
#pragma once
#include "fe_sqrt.cuh"
#include "h2c_step.cuh"
#include "rescue_step.cuh"

namespace plk {

// an integer below 2^64 is below every modulus: its canonical words are the integer
template <class P> PLK_DI Fe<P> rescue_h2c_from_u64(uint64_t n) {
    Fe<P> c = fe_zero<P>();
    c.v[0] = (uint32_t)n;
    c.v[1] = (uint32_t)(n >> 32);
    return fe_from_canonical<P>(c);
}

template <class P> PLK_DI uint32_t rescue_h2c_y_neg(const Fe<P>& o1) { return fe_to_canonical<P>(o1).v[0] & 1u; }

// o0, o1: the sponge's two outputs, R-form.  false when x^3 + B is no square (x and y are then unset).
template <class P, class Sqrt> PLK_DI bool rescue_h2c_point(const Fe<P>& o0, const Fe<P>& o1, const Fe<P>& b_mont, const Sqrt& square_root, Fe<P>& x, Fe<P>& y) {
    const Fe<P> rhs = fe_add<P>(fe_mul<P>(fe_sqr<P>(o0), o0), b_mont);  // x^3 + A x + B, A = 0 on every in-scope curve
    Fe<P> r;
    if (!square_root(rhs, r)) return false;
    x = o0;
    y = rescue_h2c_y_neg<P>(o1) ? fe_neg<P>(r) : r;
    return true;
}

// Tries i_first ..= i_last of `seed` (R-form).  sponge(seed, i, o0, o1) squeezes the two outputs of [seed, from_canonical_u32(i)].
// true: (x, y) is the point of the first try whose x^3 + B has a root; false: none of these tries settled the seed.  Every lane of a
// quad calls this with the same values, so the loop leaves on quad-uniform data.
template <class P, class Sponge, class Sqrt>
PLK_DI bool rescue_h2c_tries(const Fe<P>& seed, int i_first, int i_last, const Fe<P>& b_mont, const Sponge& sponge, const Sqrt& square_root, Fe<P>& x, Fe<P>& y) {
    for (int i = i_first; i <= i_last; ++i) {
        Fe<P> o0, o1;
        sponge(seed, (uint32_t)i, o0, o1);
        if (rescue_h2c_point<P>(o0, o1, b_mont, square_root, x, y)) return true;
    }
    return false;
}

// rescue_sponge([seed, i], 2) (rescue.rs:40-68) on a whole state: the zero state plus the chunk, one permutation, state[0] and
// state[1].  d / windows / mds / consts as rescue_permutation_step takes them.
template <class P>
PLK_DI void rescue_h2c_sponge_state(const Fe<P>& seed, uint32_t i, uint32_t rounds, const uint32_t* d, int windows, const uint32_t* mds, const uint32_t* consts,
                                    Fe<P>& o0, Fe<P>& o1) {
    constexpr int NZ = FzCfg<P>::NZ;
    Fz<P> state[RESCUE_WIDTH] = {rescue_enter<P>(seed), rescue_enter<P>(rescue_h2c_from_u64<P>(i)), fz_zero<P>(), fz_zero<P>()};
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t* ka = consts + (size_t)r * 2 * RESCUE_WIDTH * NZ;
        rescue_permutation_step<P>(state, d, windows, mds, ka, ka + RESCUE_WIDTH * NZ);
    }
    o0 = rescue_leave<P>(state[0]);
    o1 = rescue_leave<P>(state[1]);
}

}  // namespace plk
