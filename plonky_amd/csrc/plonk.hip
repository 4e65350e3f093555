// plonk.hip -- the Plonk quotient numerator on the device.
//
// Reference path                                                              here
//   Prover::vanishing_poly, the 8n-point loop      plonk.rs:392-453      ->  k_vanishing_points
//   evaluate_all_constraints                       gates/mod.rs:46-125   ->  all_constraints()
//   Gate::evaluate_filtered / evaluate_prefix_filter  gates/mod.rs:262-300 -> the shared prefix products below
//   the ten gates' evaluate_unfiltered             gates/*.rs            ->  gate by gate below (file:line at each)
//   eval_l_1                                       plonk_util.rs:14-24   ->  a cached table of L_1 over the 8n domain
//   mds_matrix                                     mds.rs:56-77          ->  seven inverses 1/1 .. 1/7 (Cauchy entries 1/(4 + r - c))
//   reduce_with_powers                             plonk_util.rs:27-33   ->  per gate (ReducedSink), closed in the last launch
// The reference evaluates the 8n points with Rayon, one full field inversion per point for L_1(x) and a freshly
// cloned MDS matrix per gate; here a point is one lane, everything that depends only on the circuit size (the powers
// of the 8n-th root, L_1 over the domain, the MDS entries) is a cached table, and the inversions behind L_1 are
// batched eight to a lane when that table is built.  The closing Polynomial::from_evaluations (plonk.rs:455) is the
// inverse NTT of ntt.hip.  The arithmetic runs on lazily reduced limbs whose value bounds are part of the types (Lz, lz.cuh);
// every operation is exact modulo p and the result is reduced to the unique representative at the end, so it is
// bit-identical to the reference's (field arithmetic is exact and associative; only the grouping differs).
// get_subgroup_shift (partition.rs:140-153) draws its k_i from ChaCha8: they are inputs here.
#include <cstdlib>
#include <memory>
#include <tuple>

#include "common.h"
#include "fp.cuh"
#include "tables.cuh"
#include "lz.cuh"
#include "witness_step.cuh"

namespace plk {

constexpr int NUM_WIRES = 9;         // plonk.rs:21
constexpr int NUM_ROUTED_WIRES = 6;  // plonk.rs:22
constexpr int NUM_CONSTANTS = 6;     // plonk.rs:24
constexpr int GRID_WIDTH = 65;       // plonk.rs:25
constexpr int NUM_TERMS = 8;         // the longest gate constraint list (base_4_sum: 1 + 7, rescue_a: 8)

// circuit-size tables (device, field, log_degree): everything the loop needs that does not depend on the proof
struct PlonkTables : DomainTables {  // the domain of the primitive 8n-th root g (circuit_builder.rs:1122)
    DevBuf l1;                       // L_1(g^i), i < 8n  (plonk_util.rs:14-24), R'-form
};
static TableCache<std::tuple<int, int, int>, PlonkTables> g_plonk;

// L_1(x) = (x^n - 1) / (n (x - 1)), L_1(1) = 1; eight points per lane share one inversion (Montgomery's trick)
constexpr int L1_PER_LANE = 8;
template <class P> __global__ void __launch_bounds__(64) k_plonk_l1(const uint4* __restrict__ lo, const uint4* __restrict__ hi, int log_degree,
                                                                    uint4* __restrict__ l1) {
    const size_t n8 = (size_t)8 << log_degree;
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * L1_PER_LANE;
    if (i0 >= n8) return;
    Fe<P> nf = fe_zero<P>();
    nf.v[log_degree >> 5] = 1u << (log_degree & 31);
    nf = fe_from_canonical<P>(nf);  // from_canonical_usize(n)
    const Fe<P> one = fe_one<P>();
    Fe<P> den[L1_PER_LANE], pre[L1_PER_LANE];
    Fe<P> run = one;
#pragma unroll
    for (int m = 0; m < L1_PER_LANE; ++m) {
        const Fe<P> x = plonk_x<P>(lo, hi, i0 + m);
        den[m] = i0 + m == 0 ? one : fe_mul<P>(nf, fe_sub<P>(x, one));
        pre[m] = run;
        run = fe_mul<P>(run, den[m]);
    }
    Fe<P> inv = fe_inv_safegcd<P>(run);
    // x^n = (g^n)^i with g^n a primitive 8th root of unity: g^(n i) = g^(n (i mod 8))
#pragma unroll
    for (int m = L1_PER_LANE - 1; m >= 0; --m) {
        const Fe<P> dinv = fe_mul<P>(inv, pre[m]);
        inv = fe_mul<P>(inv, den[m]);
        const size_t i = i0 + m;
        const Fe<P> xn = plonk_x<P>(lo, hi, ((i & 7) << log_degree));
        Fe<P> r = fe_mul<P>(fe_sub<P>(xn, one), dinv);
        if (i == 0) r = one;
        fe_store<P>(l1 + i * 2, to_rprime<P>(r));
    }
}

template <class P> static int get_plonk_tables(int log_degree, hipStream_t stream, std::shared_ptr<PlonkTables>& out) {
    int dev = 0;
    PLK_HIP_TRY(hipGetDevice(&dev));
    return g_plonk.get(std::make_tuple(dev, (int)P::FIELD_ID, log_degree), out, [&](PlonkTables& t) {
        const int log_n8 = log_degree + 3;
        const size_t n8 = (size_t)1 << log_n8;
        std::shared_ptr<const void> plan_hold;  // keeps the plan (and its power table) alive across the two launches
        PLK_TRY(build_domain_tables<P>(log_n8, stream, t, plan_hold));
        PLK_TRY(t.l1.alloc(n8 * 32));
        const size_t lanes = (n8 + L1_PER_LANE - 1) / L1_PER_LANE;
        k_plonk_l1<P><<<(unsigned)((lanes + 63) / 64), 64, 0, stream>>>((const uint4*)t.xs_lo.p, (const uint4*)t.xs_hi.p, log_degree, (uint4*)t.l1.p);
        PLK_HIP_TRY(hipGetLastError());
        PLK_HIP_TRY(hipStreamSynchronize(stream));  // the power table of the plan is only borrowed for these two launches
        return PLK_OK;
    });
}

// the R-form powers of the 8n-th root for sigma.hip: g_n^r = plonk_x(xs_lo, xs_hi, 8 r); *hold shares ownership of the tables
int plonk_domain_powers(int field, unsigned log_degree, hipStream_t stream, const void** xs_lo, const void** xs_hi, std::shared_ptr<const void>* hold) {
    return with_field4(field, [&](auto tag) {
        std::shared_ptr<PlonkTables> t;
        PLK_TRY(get_plonk_tables<tag_t<decltype(tag)>>((int)log_degree, stream, t));
        *xs_lo = t->xs_lo.p;
        *xs_hi = t->xs_hi.p;
        *hold = t;
        return (int)PLK_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// evaluate_all_constraints (gates/mod.rs:46-125): the unified constraint set at one point
// ---------------------------------------------------------------------------------------------
// The gates hand their filter and their constraint list to a sink.  Two sinks:
//  * TermSink: term t of the unified set += filter * constraint t (what evaluate_all_constraints returns, gates/mod.rs:100-124);
//  * ReducedSink: total += filter * (c_0 + alpha c_1 + alpha^2 c_2 + ..), the gate's share of reduce_with_powers over the unified
//    terms (plonk_util.rs:27-33; the sum over the gates and the powers of alpha commute) - one running value instead of eight,
//    and one product by the filter per gate instead of one per constraint.
// Ten gates, each adds at most once to a term / to the total, every summand a product (below LZ_SUMMAND_MAX / 8 p = 2p - a filter that is
// a difference of two prefix products and a sum of constraints can both be a few p): the sums stay below 20p.
constexpr int LZ_SUMMAND_MAX = 16;
template <class P> using Term = Lz<P, 10 * LZ_SUMMAND_MAX>;
// Between two gates: the instruction scheduler must not interleave them (left alone it overlaps all ten gates for
// instruction-level parallelism and the kernel needs several times the register file).
PLK_DI void gate_fence() {
#ifdef __HIPCC__
    __builtin_amdgcn_sched_barrier(0);
#endif
}
template <int GATE, class P, int B> PLK_DI void add_product(Term<P>& u, const Lz<P, B>& product) {
    static_assert(GATE >= 0 && GATE < 10, "ten gates");
    static_assert(B <= LZ_SUMMAND_MAX, "a summand must be a product");
    u.v = fz_add<P>(u.v, product.v);
}
template <class P> struct TermSink {
    static constexpr bool kReduced = false;
    Term<P> (&u)[NUM_TERMS];
    template <int GATE, int T, class F> PLK_DI void put(const F&) {}
    template <int GATE, int T, class F, class C0, class... Cs> PLK_DI void put(const F& f, const C0& c0, const Cs&... cs) {
        add_product<GATE>(u[T], f * c0);
        put<GATE, T + 1>(f, cs...);
    }
    template <int GATE, class F, class... Cs> PLK_DI void gate(const F& f, const Cs&... cs) {
        gate_fence();
        put<GATE, 0>(f, cs...);
        gate_fence();
    }
};
template <class A, class C0> PLK_DI auto lz_horner(const A&, const C0& c0) { return c0; }
template <class A, class C0, class... Cs> PLK_DI auto lz_horner(const A& alpha, const C0& c0, const Cs&... cs) { return c0 + lz_horner(alpha, cs...) * alpha; }
// The weights of a launch (k_plonk_weights): what depends on alpha / beta / k_is only, so that a point does not recompute it.
//   [0..3]  W_c  = sum_i alpha^(2 i + 1) / (4 + i - c): RescueStepA's share of reduce_with_powers that is linear in its state wire 4 + c
//           (its constraints 2 i + 1 are rows of the MDS matrix, mds.rs:63-77 - sixteen products by matrix entries become four by W_c);
//   [4..7]  W'_c = sum_i alpha^i / (4 + i - c): the same for RescueStepB (constraint i is MDS row i over the fifth powers);
//   [8..13] beta k_is[j] (plonk.rs:431: beta * k_i * x is one product per wire instead of two).
//   [14..21] alpha^1 .. alpha^8: a gate's share of reduce_with_powers is the DOT product of its constraints with them - one reduction for up
//           to six constraints instead of one per Horner step, no sums in between (round 5).
constexpr int WEIGHT_ALPHA = 8 + NUM_ROUTED_WIRES, NUM_ALPHA_POWERS = 8;
constexpr int NUM_WEIGHTS = 8 + NUM_ROUTED_WIRES + NUM_ALPHA_POWERS;
template <class P> struct ReducedSink {
    static constexpr bool kReduced = true;
    Lz<P, 16> alpha;
    Term<P> total;
    const uint32_t (*weights)[FzCfg<P>::NZ];  // staged in LDS, read where a gate uses them
    PLK_DI Lz<P, 16> weight(int w) const {
        Lz<P, 16> r;
#pragma unroll
        for (int i = 0; i < FzCfg<P>::NZ; ++i) r.v.l[i] = weights[w][i];
        return r;
    }
    // c_I alpha^I + ... into the accumulator; when its columns are full the partial sum is reduced and re-enters as a value
    template <int I, class W> PLK_DI auto dot(const W& w) const { return lz_reduce(w); }
    template <int I, int B, int U, class C, class... Cs> PLK_DI auto dot(const LzWide<P, B, U>& w, const C& c, const Cs&... cs) const {
        static_assert(I >= 1 && I <= NUM_ALPHA_POWERS, "alpha^I is not staged");
        if constexpr (U + 1 > FZ_WIDE_UNITS) {
            return dot<I>(lz_wide_add(lz_wide<P>(), lz_reduce(w)), c, cs...);
        } else {
            return dot<I + 1>(lz_mac(w, c, weight(WEIGHT_ALPHA + I - 1)), cs...);
        }
    }
    // value below 15p for the product by the filter
    template <int B> PLK_DI static auto tamed(const Lz<P, B>& h) {
        if constexpr (B > LZ_MUL_MAX) return h.rs();
        else return h;
    }
    template <int GATE, class F, class C0, class... Cs> PLK_DI void gate(const F& f, const C0& c0, const Cs&... cs) {
        gate_fence();
        if constexpr (sizeof...(cs) == 0) add_product<GATE>(total, f * tamed(c0));
        else add_product<GATE>(total, f * tamed(dot<1>(lz_wide_add(lz_wide<P>(), c0), cs...)));
        gate_fence();
    }
    // filter * (c_0 + alpha c_1 + ... + extra): `extra` is the part of the gate's sum that was folded into the launch's weights
    template <int GATE, class F, class E, class C0, class... Cs> PLK_DI void gate_extra(const F& f, const E& extra, const C0& c0, const Cs&... cs) {
        gate_fence();
        add_product<GATE>(total, f * tamed(dot<1>(lz_wide_add(lz_wide_add(lz_wide<P>(), c0), extra), cs...)));
        gate_fence();
    }
};
// Base4SumGate's running sum, computed = 4 computed + limb over the seven limbs (base_4_sum.rs:44-48)
template <int I, class P, int B, class LW> PLK_DI auto base4_chain(const Lz<P, B>& computed, const LW& l) {
    if constexpr (I == NUM_WIRES - 2) return computed;
    else return base4_chain<I + 1>(lz_tame(computed.quad() + l[2 + I]), l);
}

// k: local constants [6]; l: local wires [9]; r: right wires (only indices 0..3 are read by any gate); b2, b3: below wires 2, 3
// (only CurveEndoGate reads below, curve_endo.rs:115-117); small: 1/1 .. 1/7 (R'-form table).
// Prefix filters (gates/mod.rs:289-300) are formed where they are used, along the prefix tree of gates/mod.rs:1-16 (BufferGate,
// PREFIX 101000 in the code - buffer.rs:27; the doc comment of gates/mod.rs says 101010 -, has no constraints: buffer.rs:26-33): a filter kept alive for the whole kernel costs nine registers.
// gate groups (a kernel evaluates a subset: the live set of all ten gates is several register files wide)
constexpr int GATES_RESCUE_A = 1, GATES_ENDO = 2, GATES_BASE4_ARITH = 4, GATES_ADD_PUBLIC = 8, GATES_DBL_CONST = 16, GATES_RESCUE_B = 32, GATES_ALL = 63;
constexpr int GATES_RESCUE = GATES_RESCUE_A | GATES_RESCUE_B;
// The inputs of a point are READ WHERE A GATE USES THEM: k / l / r are rows of the prover's tables (or plain arrays, in
// k_all_constraints) indexed through operator[], every mention a load and a re-slicing into the working form (~80
// instructions against ~220 for a product).  An input held from the top of the kernel costs nine registers for its whole
// length; 21 of them are 189 - with the working set of a gate that is a whole register file and one wave per SIMD.
template <class P> struct LazyRow {
    const uint4* base;
    size_t stride, i;
    const LzTop<P>& top;
    PLK_DI Lz<P, 16> operator[](int j) const { return lz_load<P>(base, (size_t)j * stride + i, top); }
};
template <class P, class D, int MASK, class K, class LW, class RW, class Sink>
PLK_DI void all_constraints(const K& k, const LW& l, const RW& r, const D& b2, const D& b3, const D& zeta, const D& a_coeff,
                            const uint4* __restrict__ small, Sink& sink) {
    const auto one = lz_one<P>();
    if constexpr ((MASK & GATES_RESCUE) != 0) {  // RescueStepAGate 00, rescue_a.rs:38-69, and RescueStepBGate 01, rescue_b.rs:30-58
        const auto nk0 = one - k[0];
        const D k1 = k[1];
        // both steps in one launch: (1 - k0) (1 - k1) = (1 - k0) - (1 - k0) k1, one product for the two filters
        constexpr bool BOTH_STEPS = (MASK & GATES_RESCUE) == GATES_RESCUE;
        const auto f_step_b = nk0 * k1;
        auto filter_a = [&] {
            if constexpr (BOTH_STEPS) return nk0 - f_step_b;
            else return nk0 * (one - k1);
        };
        Lz<P, 8> mds[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) mds[i] = lz_table<P>(small, i);  // mds[v - 1] = 1 / v; entry (r, c) = 1 / (4 + r - c), mds.rs:63-77
        // row i of the MDS matrix times (v0 .. v3), plus the round constant, against the right gate's wire i
#define PLK_MDS_ROW(i, v0, v1, v2, v3) (k[2 + i] + (mds[3 + i] * v0 + mds[2 + i] * v1 + mds[1 + i] * v2 + mds[i] * v3) - r[i])
        if constexpr ((MASK & GATES_RESCUE_A) != 0) {
            const D l4 = l[4], l5 = l[5], l6 = l[6], l7 = l[7];
            if constexpr (Sink::kReduced) {
                // sum_t alpha^t c_t with the matrix part of the odd constraints taken out: sum_c l_(4 + c) W_c (weights 0..3)
                // four products, one reduction; the rows as loaded have limbs up to 2^30 (two column units each: carried copies go in)
                auto carried = [](D v) {
                    fz_carry<P>(v.v);
                    return v;
                };
                const auto folded = lz_reduce(lz_mac(lz_mac(lz_mac(lz_mac(lz_wide<P>(), carried(l4), sink.weight(0)), carried(l5), sink.weight(1)),
                                                            carried(l6), sink.weight(2)), carried(l7), sink.weight(3)));
                sink.template gate_extra<7>(filter_a(), folded,                      //
                                            l4.pow5() - l[0], k[2] - r[0],            //
                                            l5.pow5() - l[1], k[3] - r[1],            //
                                            l6.pow5() - l[2], k[4] - r[2],            //
                                            l7.pow5() - l[3], k[5] - r[3]);
            } else {
                sink.template gate<7>(filter_a(),                                                //
                                      l4.pow5() - l[0], PLK_MDS_ROW(0, l4, l5, l6, l7),           //
                                      l5.pow5() - l[1], PLK_MDS_ROW(1, l4, l5, l6, l7),           //
                                      l6.pow5() - l[2], PLK_MDS_ROW(2, l4, l5, l6, l7),           //
                                      l7.pow5() - l[3], PLK_MDS_ROW(3, l4, l5, l6, l7));
            }
        }
        if constexpr ((MASK & GATES_RESCUE_B) != 0) {
            const auto e0 = l[0].pow5(), e1 = l[1].pow5(), e2 = l[2].pow5(), e3 = l[3].pow5();
            if constexpr (Sink::kReduced) {
                const auto folded = lz_reduce(lz_mac(lz_mac(lz_mac(lz_mac(lz_wide<P>(), e0, sink.weight(4)), e1, sink.weight(5)), e2, sink.weight(6)),
                                                     e3, sink.weight(7)));
                sink.template gate_extra<8>(f_step_b, folded, k[2] - r[0], k[3] - r[1], k[4] - r[2], k[5] - r[3]);
            } else {
                sink.template gate<8>(f_step_b, PLK_MDS_ROW(0, e0, e1, e2, e3), PLK_MDS_ROW(1, e0, e1, e2, e3), PLK_MDS_ROW(2, e0, e1, e2, e3),
                                      PLK_MDS_ROW(3, e0, e1, e2, e3));
            }
        }
#undef PLK_MDS_ROW
    }
    [[maybe_unused]] Lz<P, lz_mul_bound(16, 16)> f_endo{fz_zero<P>()};  // k0 k1; the prefix 10 below is k0 - k0 k1 when both are evaluated here
    if constexpr ((MASK & GATES_ENDO) != 0) {  // CurveEndoGate 11, curve_endo.rs:96-141
        const D &x1 = l[0], &y1 = l[1], &x_in = l[4], &y_in = l[5], &x3 = r[0], &y3 = r[1];
        const D &unsigned_old = l[2], &unsigned_new = b2, &signed_old = l[3], &signed_new = b3, &bit0 = l[6], &bit1 = l[7], &inverse = l[8];
        const auto mult = (zeta - one) * bit1 + one;  // x2's factor and signed_limb_multiplier are the same expression
        const auto x2 = mult * x_in;
        const auto sgn = bit0.dbl() - one;
        const auto y2 = sgn * y_in;
        const auto lambda = (y1 - y2) * inverse;
        const auto computed_x3 = lambda.sq() - x1 - x2;
        const auto computed_y3 = lambda * (x1 - x3) - y1;
        const auto signed_limb = sgn * mult;
        f_endo = k[0] * k[1];
        sink.template gate<2>(f_endo, computed_x3 - x3, computed_y3 - y3, unsigned_new - (unsigned_old.quad() + bit1.dbl() + bit0).rs(),
                              signed_new - (signed_old.dbl() + signed_limb), bit0 * (bit0 - one), bit1 * (bit1 - one), inverse * (x1 - x2) - one);
    }
    if constexpr ((MASK & (GATES_BASE4_ARITH | GATES_ADD_PUBLIC | GATES_DBL_CONST)) == 0) return;
    const auto p10 = [&] {
        if constexpr ((MASK & GATES_ENDO) != 0) return k[0] - f_endo;
        else return k[0] * (one - k[1]);
    }();
    if constexpr ((MASK & GATES_BASE4_ARITH) != 0) {
        const auto p100 = p10 * (one - k[2]);
        // the two filters below p100 share one product: p100 (1 - k3) = p100 - p100 k3
        const auto f_arith = p100 * k[3];
        const auto f_base4 = p100 - f_arith;
        // ArithmeticGate 1001, arithmetic.rs:30-46
        // k4 l0 l1 + k5 l2 - l3: the two outer products through one reduction (rows as loaded: two column units per raw operand)
        sink.template gate<6>(f_arith, lz_reduce(lz_mac<true, true>(lz_mac<false, true>(lz_wide<P>(), k[4] * l[0], l[1]), k[5], l[2])) - l[3]);
        {  // Base4SumGate 1000, base_4_sum.rs:34-63: 7 limbs in wires 2..8
            const auto two = one.dbl();
            // (limb - 0) (limb - 1) (limb - 2) (limb - 3), times ONE in the reference: with t = limb^2 - 3 limb = limb (limb - 3) it is
            // t (t + 2) - a squaring and a product instead of three products
            auto b4 = [&](const D& limb) {
                const auto t = limb.sq() - (limb.dbl() + limb);
                return t * (t + two);
            };
#define PLK_B4(i) b4(l[2 + i])
            sink.template gate<3>(f_base4, (base4_chain<0>(l[0], l) - l[1]).rs(), PLK_B4(0), PLK_B4(1), PLK_B4(2), PLK_B4(3), PLK_B4(4), PLK_B4(5), PLK_B4(6));
#undef PLK_B4
        }
    }
    if constexpr ((MASK & (GATES_ADD_PUBLIC | GATES_DBL_CONST)) == 0) return;
    const auto p101 = p10 * k[2];
    if constexpr ((MASK & GATES_ADD_PUBLIC) != 0) {
        const auto p1010 = p101 * (one - k[3]);
        const auto f_add = p1010 * k[4];        // p1010 (1 - k4) = p1010 - p1010 k4: the two filters below p1010 share one product
        const auto f_not_add = p1010 - f_add;
        {  // CurveAddGate 10101, curve_add.rs:60-101
            const D &x1 = l[0], &y1 = l[1], &x4 = r[0], &y4 = r[1], &acc_old = l[2], &acc_new = l[3], &x2 = l[4], &y2 = l[5], &bit = l[6], &inverse = l[7],
                    &lambda = l[8];
            const auto computed_lambda = (y1 - y2) * inverse;
            const auto x3 = lambda.sq() - x1 - x2;
            const auto y3 = lambda * (x1 - x4) - y1;
            const auto not_bit = one - bit;
            // bit x3 + (1 - bit) x1 = x1 + bit (x3 - x1): one product each instead of two
            const auto computed_x4 = x1 + bit * (x3 - x1);
            const auto computed_y4 = y1 + bit * (y3 - y1);
            sink.template gate<0>(f_add, computed_lambda - lambda, computed_x4 - x4, computed_y4 - y4, acc_new - (acc_old.dbl() + bit), bit * not_bit,
                                  inverse * (x1 - x2) - one);
        }
        // PublicInputGate 101001, public_input.rs:26-37: advice wires 6..8 against the right gate's wires 0..2
        sink.template gate<4>(f_not_add * k[5], l[6] - r[0], l[7] - r[1], l[8] - r[2]);
    }
    if constexpr ((MASK & GATES_DBL_CONST) != 0) {
        const auto p1011 = p101 * k[3];
        const auto f_dbl = p1011 * k[4];
        const auto f_const = p1011 - f_dbl;
        // ConstantGate 10110, constant.rs:28-39
        sink.template gate<5>(f_const, k[5] - l[0]);
        {  // CurveDblGate 10111, curve_dbl.rs:42-68
            const D &x_old = l[0], &y_old = l[1], &x_new = l[2], &y_new = l[3], &inverse = l[4], &lambda = l[5];
            const auto xx = x_old.sq();
            const auto numerator = xx.dbl() + xx + a_coeff;  // square().triple() + A
            const auto computed_lambda = numerator * inverse;
            const auto computed_x_new = lambda.sq() - x_old.dbl();
            const auto computed_y_new = lambda * (x_old - x_new) - y_old;
            sink.template gate<1>(f_dbl, computed_lambda - lambda, computed_x_new - x_new, computed_y_new - y_new, y_old.dbl() * inverse - one);
        }
    }
}

struct PlonkScalars {
    uint32_t k_is[NUM_ROUTED_WIRES][8];
    uint32_t alpha[8], beta[8], gamma[8], zeta[8], a[8];
};
// the scalars of a launch in the working form, converted once per workgroup: [0..5] k_is, 6 alpha, 7 beta, 8 gamma, 9 zeta, 10 a
constexpr int NUM_SCALARS = NUM_ROUTED_WIRES + 5;
// rows NUM_SCALARS .. NUM_SCALARS + NUM_WEIGHTS - 1: the weights of the launch (k_plonk_weights; limb form already), when there are any
template <class P> PLK_DI void stage_scalars(const PlonkScalars& sc, uint32_t (*s_sc)[FzCfg<P>::NZ], const uint32_t* __restrict__ weights = nullptr) {
    const int t = threadIdx.x;
    if (weights && t >= NUM_SCALARS && t < NUM_SCALARS + NUM_WEIGHTS) {
#pragma unroll
        for (int i = 0; i < FzCfg<P>::NZ; ++i) s_sc[t][i] = weights[(t - NUM_SCALARS) * FzCfg<P>::NZ + i];
    }
    if (t < NUM_SCALARS) {
        const uint32_t* w = t < NUM_ROUTED_WIRES ? sc.k_is[t] : t == 6 ? sc.alpha : t == 7 ? sc.beta : t == 8 ? sc.gamma : t == 9 ? sc.zeta : sc.a;
        Fe<P> x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = w[i];
        const Lz<P, 16> z = lz_from_rform<P>(x);
#pragma unroll
        for (int i = 0; i < FzCfg<P>::NZ; ++i) s_sc[t][i] = z.v.l[i];
    }
    __syncthreads();
}
template <class P> PLK_DI Lz<P, 16> scalar_at(const uint32_t (*s_sc)[FzCfg<P>::NZ], int t) {
    Lz<P, 16> r;
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.v.l[i] = s_sc[t][i];
    return r;
}

// The weights of a call (ReducedSink), one lane each; alpha^e by repeated products - fourteen lanes, once per call.
template <class P> __global__ void __launch_bounds__(64) k_plonk_weights(const uint4* __restrict__ small, PlonkScalars sc, uint32_t* __restrict__ out) {
    using D = Lz<P, 16>;
    const int t = threadIdx.x;
    if (t >= NUM_WEIGHTS) return;
    auto load = [](const uint32_t (&w)[8]) {
        Fe<P> x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = w[i];
        return lz_from_rform<P>(x);
    };
    D res;
    if (t < 8) {
        const D alpha = load(sc.alpha);
        const int c = t & 3;
        const bool step_b = t >= 4;
        // RescueStepA: exponents 1, 3, 5, 7 (its matrix rows are the odd constraints); RescueStepB: 0, 1, 2, 3
        D pw = step_b ? lz_one<P>().template widen<16>() : alpha;
        const D step = step_b ? alpha : (alpha * alpha).template widen<16>();
        D acc{fz_zero<P>()};
        for (int i = 0; i < 4; ++i) {
            acc = (acc + pw * lz_table<P>(small, 3 + i - c)).rs();  // MDS entry (i, c) = 1 / (4 + i - c), mds.rs:63-77
            pw = (pw * step).template widen<16>();
        }
        res = acc;
    } else if (t < WEIGHT_ALPHA) {
        res = (load(sc.beta) * load(sc.k_is[t - 8])).template widen<16>();
    } else {
        const D alpha = load(sc.alpha);
        res = alpha.rs();  // exactly normalised limbs, like the products below
        for (int e = 1; e < t - WEIGHT_ALPHA + 1; ++e) res = (res * alpha).template widen<16>();
    }
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) out[t * FzCfg<P>::NZ + i] = res.v.l[i];
}

// plonk.rs:392-453, one lane per point of the 8n domain, in FOUR launches.  The ten gates, the permutation argument and their
// inputs (21 + 10 elements per point) are several register files wide; evaluated in one piece the kernel spills to scratch
// and, at one wave per SIMD, waits out every reload.  A launch evaluates a group of gates and hands the running sum on (limb
// form, 48 B per point, in `part`); its inputs are read where a gate uses them (LazyRow), so a launch fits the 256
// registers of two waves per SIMD:
//   PASS 0: RescueStepA + RescueStepB (PASS 1 is RescueStepB alone when PLK_VANISH_MERGE_RESCUE is 0)   PASS 2: CurveEndo, Base4Sum,
//   Arithmetic   PASS 3: CurveAdd, PublicInput, CurveDbl, Constant   PASS 4: the permutation argument, L_1 and reduce_with_powers -> out
// The sum over the gates and the powers of alpha commute (ReducedSink), every value is exact: same result as one loop.
#ifndef PLK_VANISH_MERGE_RESCUE
#define PLK_VANISH_MERGE_RESCUE 1  // 1: the two Rescue gates in one launch (PASS 1 is not launched); 0: a launch each (measured 3 % slower, round 4)
#endif
#ifndef PLK_VANISH_WAVES
#define PLK_VANISH_WAVES 2  // waves per SIMD the register allocation is held to (3 was measured in round 4: tools/gpu/r04_vanish_waves.sh)
#endif
template <class P, int PASS>
__global__ void __launch_bounds__(128, PLK_VANISH_WAVES) k_vanishing_points(const uint4* __restrict__ constants, const uint4* __restrict__ wires, const uint4* __restrict__ s_sigma,
                                                             const uint4* __restrict__ z, const uint4* __restrict__ xs_lo_z, const uint4* __restrict__ xs_hi_z,
                                                             const uint4* __restrict__ l1, const uint4* __restrict__ small, PlonkScalars sc, int log_degree,
                                                             uint32_t* __restrict__ part, uint4* __restrict__ out, size_t first, size_t count,
                                                             const uint32_t* __restrict__ weights, const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    using D = Lz<P, 16>;
    constexpr int MASK = PASS == 0 ? (PLK_VANISH_MERGE_RESCUE ? GATES_RESCUE : GATES_RESCUE_A) : PASS == 1 ? GATES_RESCUE_B
                         : PASS == 2 ? (GATES_ENDO | GATES_BASE4_ARITH) : PASS == 3 ? (GATES_ADD_PUBLIC | GATES_DBL_CONST) : 0;
    static_assert(NUM_SCALARS + NUM_WEIGHTS <= 128, "one lane of the workgroup stages one row");
    __shared__ uint32_t s_sc[NUM_SCALARS + NUM_WEIGHTS][FzCfg<P>::NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    stage_scalars<P>(sc, s_sc, weights);  // ends with the barrier that publishes both
    const size_t n8 = (size_t)8 << log_degree;
    const size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // this launch covers the points first .. first + count - 1
    if (i >= first + count || i >= n8) return;
    const size_t i_right = (i + 8) & (n8 - 1), i_below = (i + 8 * GRID_WIDTH) & (n8 - 1);
    // the rows a gate reads from: local constants, local wires, the right gate's wires (loaded where they are used)
    const LazyRow<P> k{constants, n8, i, s_top}, l{wires, n8, i, s_top}, r{wires, n8, i_right, s_top};
    const D alpha = scalar_at<P>(s_sc, 6);
    if constexpr (PASS < 4) {
        D b2{fz_zero<P>()}, b3{fz_zero<P>()};
        if constexpr ((MASK & GATES_ENDO) != 0) {
            b2 = lz_load<P>(wires, (size_t)2 * n8 + i_below, s_top);
            b3 = lz_load<P>(wires, (size_t)3 * n8 + i_below, s_top);
        }
        ReducedSink<P> sink{alpha, Term<P>{fz_zero<P>()}, s_sc + NUM_SCALARS};
        all_constraints<P, D, MASK>(k, l, r, b2, b3, scalar_at<P>(s_sc, 9), scalar_at<P>(s_sc, 10), small, sink);
        if constexpr (PASS == 0) {
            limbs_store<P>(part, i, sink.total.v);  // one or two gates, below 2p each
        } else {
            // gates so far: 1 (PASS 1), 2 (PASS 2), 5 (PASS 3), each below 2p
            const Lz<P, LZ_SUMMAND_MAX * (PASS == 1 ? 1 : PASS == 2 ? 2 : 5)> before{limbs_load<P>(part, i)};
            limbs_store<P>(part, i, (before + sink.total).v);
        }
    } else {
        const Lz<P, 9 * LZ_SUMMAND_MAX> total{limbs_load<P>(part, i)};  // nine gates with constraints: < 18p
        const auto one = lz_one<P>();
        const auto x = lz_table<P>(xs_lo_z, i & (((size_t)1 << XS_LO_LOG) - 1)) * lz_table<P>(xs_hi_z, i >> XS_LO_LOG);  // hi[0] = 1
        const D z_x = lz_load<P>(z, i, s_top), z_gz = lz_load<P>(z, i_right, s_top);
        // (z_1_term = L_1(x) (Z(x) - 1), plonk.rs:425, joins the last reduction below)
        const D beta = scalar_at<P>(s_sc, 7), gamma = scalar_at<P>(s_sc, 8);
        Lz<P, 9> f_prime = one.template widen<9>(), g_prime = f_prime;
#pragma unroll
        for (int j = 0; j < NUM_ROUTED_WIRES; ++j) {  // plonk.rs:428-437
            const auto beta_s_id = scalar_at<P>(s_sc, NUM_SCALARS + 8 + j) * x;  // beta * (k_is[j] * x), plonk.rs:430-431: beta k_is[j] is a weight of the call
            const D s_sig = lz_load<P>(s_sigma, (size_t)j * n8 + i, s_top);
            const D lj = l[j];
            f_prime = f_prime * (lj + beta_s_id + gamma);
            g_prime = g_prime * (lj + beta * s_sig + gamma);
        }
        // Z(x) f'(x) - g'(x) Z(g x), plonk.rs:438: two products, one reduction (z_x / z_gz are rows as loaded: two column units each)
        const auto zero = Lz<P, 0>{fz_zero<P>()};
        const auto v_shift_term = lz_reduce(lz_mac<false, true>(lz_mac<false, true>(lz_wide<P>(), f_prime, z_x), zero - g_prime, z_gz));
        // reduce_with_powers over [z_1_term, v_shift_term, constraint terms] (plonk.rs:440-447, plonk_util.rs:27-33):
        // total alpha^2 + v_shift alpha + L_1 (Z - 1), three products through one reduction
        const auto res = lz_reduce(lz_mac(lz_mac(lz_mac(lz_wide<P>(), total.rs(), scalar_at<P>(s_sc, NUM_SCALARS + WEIGHT_ALPHA + 1)), v_shift_term, alpha),
                                          lz_table<P>(l1, i), z_x - one));
        fe_store<P>(out + i * 2, lz_to_rform<P>(res));
    }
}

// evaluate_all_constraints at `count` independent points (constants [count][6], local / right / below [count][9], out [count][8])
template <class P>
__global__ void __launch_bounds__(128) k_all_constraints(const uint4* __restrict__ constants, const uint4* __restrict__ local, const uint4* __restrict__ right,
                                                         const uint4* __restrict__ below, const uint4* __restrict__ small, PlonkScalars sc, size_t count,
                                                         uint4* __restrict__ out) {
    using D = Lz<P, 16>;
    __shared__ uint32_t s_sc[NUM_SCALARS][FzCfg<P>::NZ];
    stage_scalars<P>(sc, s_sc);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    D k[NUM_CONSTANTS], l[NUM_WIRES], r[4];
#pragma unroll
    for (int j = 0; j < NUM_CONSTANTS; ++j) k[j] = lz_load<P>(constants, i * NUM_CONSTANTS + j);
#pragma unroll
    for (int j = 0; j < NUM_WIRES; ++j) l[j] = lz_load<P>(local, i * NUM_WIRES + j);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = lz_load<P>(right, i * NUM_WIRES + j);
    Term<P> u[NUM_TERMS];
#pragma unroll
    for (int t = 0; t < NUM_TERMS; ++t) u[t] = Term<P>{fz_zero<P>()};
    TermSink<P> sink{u};
    all_constraints<P, D, GATES_ALL>(k, l, r, lz_load<P>(below, i * NUM_WIRES + 2), lz_load<P>(below, i * NUM_WIRES + 3), scalar_at<P>(s_sc, 9),
                                     scalar_at<P>(s_sc, 10), small, sink);
#pragma unroll
    for (int t = 0; t < NUM_TERMS; ++t) fe_store<P>(out + (i * NUM_TERMS + t) * 2, lz_to_rform<P>(u[t].rs()));
}

template <class P>
static int vanishing_points_t(unsigned log_degree, const void* d_constants, const void* d_wires, const void* d_s_sigma, const void* d_z, const PlonkScalars& sc,
                              void* d_out, hipStream_t stream) {
    std::shared_ptr<PlonkTables> t;
    PLK_TRY(get_plonk_tables<P>((int)log_degree, stream, t));
    const size_t n8 = (size_t)8 << log_degree;
    void* part = scratch_acquire(limb_bytes(n8, FzCfg<P>::NZ), stream);
    if (!part) return PLK_ERR_OOM;
    uint32_t* weights = (uint32_t*)scratch_acquire((size_t)NUM_WEIGHTS * FzCfg<P>::NZ * 4, stream);
    if (!weights) {
        scratch_release(part, stream);
        return PLK_ERR_OOM;
    }
    k_plonk_weights<P><<<1, 64, 0, stream>>>((const uint4*)t->small.p, sc, weights);
    // PLK_VANISH_SLAB_LOG=k: the launches walk the domain in slabs of 2^k points, so that the rows a slab reads (29 x 32 B per
    // point) are still in the 256 MiB Infinity Cache when the next launch of the slab re-reads them (round-3 review item 5;
    // measured in DESIGN.md section 4c).  Default: the whole domain per launch.
    static const int slab_log = [] {
        const char* e = getenv("PLK_VANISH_SLAB_LOG");
        const int v = e ? atoi(e) : 0;
        return v >= 10 && v <= 40 ? v : 0;
    }();
    const size_t slab = slab_log ? ((size_t)1 << slab_log) : n8;
#define PLK_VANISH(PASS)                                                                                                                                  \
    k_vanishing_points<P, PASS><<<blocks, 128, 0, stream>>>((const uint4*)d_constants, (const uint4*)d_wires, (const uint4*)d_s_sigma, (const uint4*)d_z, \
                                                            (const uint4*)t->xs_lo_z.p, (const uint4*)t->xs_hi_z.p, (const uint4*)t->l1.p, (const uint4*)t->small.p, sc, \
                                                            (int)log_degree, (uint32_t*)part, (uint4*)d_out, first, cnt, weights, (const uint32_t*)t->top.p)
    for (size_t first = 0; first < n8; first += slab) {
        const size_t cnt = n8 - first < slab ? n8 - first : slab;
        const unsigned blocks = (unsigned)((cnt + 127) / 128);
        PLK_VANISH(0);
        if (!PLK_VANISH_MERGE_RESCUE) PLK_VANISH(1);
        PLK_VANISH(2);
        PLK_VANISH(3);
        PLK_VANISH(4);
    }
#undef PLK_VANISH
    const hipError_t e = hipGetLastError();
    scratch_release(weights, stream);
    scratch_release(part, stream);
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "vanishing points launch failed: %s", hipGetErrorString(e));
    // the tables stay alive in the cache (plk_ntt_clear_cache / plk_shutdown drop them after a device synchronisation)
    return PLK_OK;
}

static int fill_scalars(PlonkScalars& sc, const uint64_t* k_is, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* zeta,
                        const uint64_t* a) {
    if (!zeta || !a) return set_error(PLK_ERR_INVALID_ARG, "null InnerC constant");
    static const uint64_t zero4[4] = {0, 0, 0, 0};
    for (int j = 0; j < NUM_ROUTED_WIRES; ++j) limbs_to_words(sc.k_is[j], k_is ? k_is + 4 * j : zero4);
    limbs_to_words(sc.alpha, alpha ? alpha : zero4);
    limbs_to_words(sc.beta, beta ? beta : zero4);
    limbs_to_words(sc.gamma, gamma ? gamma : zero4);
    limbs_to_words(sc.zeta, zeta);
    limbs_to_words(sc.a, a);
    return PLK_OK;
}

int plonk_vanishing_points_dev_impl(int field, unsigned log_degree, const void* d_constants, const void* d_wires, const void* d_s_sigma, const void* d_z,
                                    const uint64_t* k_is, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* inner_zeta,
                                    const uint64_t* inner_a, void* d_out, hipStream_t stream) {
    if (!d_constants || !d_wires || !d_s_sigma || !d_z || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    if (!k_is || !alpha || !beta || !gamma) return set_error(PLK_ERR_INVALID_ARG, "null challenge / shift pointer");
    if (log_degree + 3 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_degree %u too large", log_degree);
    PLK_TRY(ensure_device());
    PlonkScalars sc;
    PLK_TRY(fill_scalars(sc, k_is, alpha, beta, gamma, inner_zeta, inner_a));
    return or_invalid(with_field4(field, [&](auto t) { return vanishing_points_t<tag_t<decltype(t)>>(log_degree, d_constants, d_wires, d_s_sigma, d_z, sc, d_out, stream); }),
                      "field %d is not a circuit scalar field", field);
}

template <class P>
static int all_constraints_t(size_t count, const void* d_constants, const void* d_local, const void* d_right, const void* d_below, const PlonkScalars& sc,
                             void* d_out, hipStream_t stream) {
    std::shared_ptr<PlonkTables> t;
    PLK_TRY(get_plonk_tables<P>(7, stream, t));  // only the small inverses are used: any circuit size serves
    k_all_constraints<P><<<(unsigned)((count + 127) / 128), 128, 0, stream>>>((const uint4*)d_constants, (const uint4*)d_local, (const uint4*)d_right,
                                                                             (const uint4*)d_below, (const uint4*)t->small.p, sc, count, (uint4*)d_out);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

int plonk_all_constraints_dev_impl(int field, size_t count, const void* d_constants, const void* d_local, const void* d_right, const void* d_below,
                                   const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_out, hipStream_t stream) {
    if (count == 0) return PLK_OK;
    if (!d_constants || !d_local || !d_right || !d_below || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    PlonkScalars sc;
    PLK_TRY(fill_scalars(sc, nullptr, nullptr, nullptr, nullptr, inner_zeta, inner_a));
    return or_invalid(with_field4(field, [&](auto t) { return all_constraints_t<tag_t<decltype(t)>>(count, d_constants, d_local, d_right, d_below, sc, d_out, stream); }),
                      "field %d is not a circuit scalar field", field);
}

// ---------------------------------------------------------------------------------------------
// the witness check: which gate a witness does not satisfy, which routed wire differs from its copy
// ---------------------------------------------------------------------------------------------
// What the reference answers in debug builds only (plonk.rs:158-167: the degree-8n vanishing polynomial evaluated at each of the n
// subgroup points, O(n^2), then "{}-th gate constraints are not satisfied").  On the subgroup the L_1 and Z terms aside, the vanishing
// polynomial is the unified constraint set: all_constraints() above at the n rows themselves, no LDE, straight off the n-point tables
// (or the 8n ones, one element in eight).  The copy constraints are one comparison per routed wire with its neighbour under sigma.
//   k_check_init    the report before anything is counted
//   k_check_rows    a lane per gate row: the eight terms SUMMED over the ten gates (TermSink - with selectors that are not 0 / 1 the
//                   shares of two gates can cancel, so masks per gate group OR-ed together would differ from the reference), reduced to
//                   the unique representative, bit t of the row's mask set iff term t is nonzero; count and smallest failing row by wave
//   k_check_first   one lane evaluates the first failing row again and writes its mask and its eight terms
//   k_check_copies  a lane per routed wire: 32 bytes at w against 32 bytes at sigma[w] (canonical elements: equal values are equal words)
// A wave merges its lanes with a ballot (witness_step.cuh) and issues one integer atomicAdd and one atomicMin: the report does not
// depend on the order of the waves.
constexpr int CHECK_LANES = 128, CHECK_COPY_LANES = 256;

// the unified constraint set of gate row i of the tables, in the reference's form; the row's mask.  terms (nullable): 8 elements.
template <class P>
PLK_DI uint32_t check_row(const uint4* __restrict__ constants, unsigned constants_stride, const uint4* __restrict__ wires, int log_degree, uint32_t i,
                          const LzTop<P>& s_top, const uint32_t (*s_sc)[FzCfg<P>::NZ], const uint4* __restrict__ small, uint4* __restrict__ terms) {
    using D = Lz<P, 16>;
    const size_t n = (size_t)1 << log_degree;
    const uint32_t i_right = witness_right(i, (unsigned)log_degree), i_below = witness_below(i, (unsigned)log_degree);
    // constant j of row i is element (j n + i) constants_stride: stride 8 walks constants_8n, one point in eight
    const LazyRow<P> k{constants, n * constants_stride, (size_t)i * constants_stride, s_top}, l{wires, n, i, s_top}, r{wires, n, i_right, s_top};
    const D b2 = lz_load<P>(wires, (size_t)2 * n + i_below, s_top), b3 = lz_load<P>(wires, (size_t)3 * n + i_below, s_top);
    Term<P> u[NUM_TERMS];
#pragma unroll
    for (int t = 0; t < NUM_TERMS; ++t) u[t] = Term<P>{fz_zero<P>()};
    TermSink<P> sink{u};
    all_constraints<P, D, GATES_ALL>(k, l, r, b2, b3, scalar_at<P>(s_sc, 9), scalar_at<P>(s_sc, 10), small, sink);
    uint32_t mask = 0;
#pragma unroll
    for (int t = 0; t < NUM_TERMS; ++t) {
        const Fe<P> c = lz_to_rform<P>(u[t].rs());  // the unique representative: zero is eight zero words
        uint32_t any = 0;
#pragma unroll
        for (int w = 0; w < P::NL; ++w) any |= c.v[w];
        if (any) mask |= 1u << t;
        if (terms) fe_store<P>(terms + t * 2, c);
    }
    return mask;
}

__global__ void __launch_bounds__(64) k_check_init(uint32_t* __restrict__ report) {
    if (threadIdx.x < WITNESS_REPORT_WORDS) report[threadIdx.x] = witness_report_init((int)threadIdx.x);
}

template <class P>
__global__ void __launch_bounds__(CHECK_LANES) k_check_rows(const uint4* __restrict__ constants, unsigned constants_stride, const uint4* __restrict__ wires,
                                                           const uint4* __restrict__ small, PlonkScalars sc, int log_degree, uint8_t* __restrict__ row_masks,
                                                           uint32_t* __restrict__ report, const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    __shared__ uint32_t s_sc[NUM_SCALARS][FzCfg<P>::NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    stage_scalars<P>(sc, s_sc);  // ends with the barrier that publishes both
    const uint32_t n = 1u << log_degree;
    const uint32_t i = blockIdx.x * CHECK_LANES + threadIdx.x;  // n <= 2^27
    uint32_t mask = 0;
    if (i < n) {
        mask = check_row<P>(constants, constants_stride, wires, log_degree, i, s_top, s_sc, small, nullptr);
        if (row_masks) row_masks[i] = (uint8_t)mask;
    }
    // every lane of the wave is back here; the wave's lanes hold consecutive rows
    const WitnessWave w = witness_wave_merge(__ballot(mask != 0), i - (threadIdx.x & 63));
    if ((threadIdx.x & 63) == 0 && w.count) {
        atomicAdd(&report[WITNESS_BAD_ROWS], w.count);
        atomicMin(&report[WITNESS_FIRST_ROW], w.first);
    }
}

// after k_check_rows, one workgroup: what plk_plonk_evaluate_all_constraints returns for the first failing row, zeros when there is none
template <class P>
__global__ void __launch_bounds__(64) k_check_first(const uint4* __restrict__ constants, unsigned constants_stride, const uint4* __restrict__ wires,
                                                    const uint4* __restrict__ small, PlonkScalars sc, int log_degree, uint32_t* __restrict__ report,
                                                    uint4* __restrict__ first_terms, const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    __shared__ uint32_t s_sc[NUM_SCALARS][FzCfg<P>::NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    stage_scalars<P>(sc, s_sc);
    if (threadIdx.x != 0) return;
    const uint32_t first = report[WITNESS_FIRST_ROW];
    uint32_t mask = 0;
    if (first < (1u << log_degree)) {
        mask = check_row<P>(constants, constants_stride, wires, log_degree, first, s_top, s_sc, small, first_terms);
    } else if (first_terms) {
        const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 2 * NUM_TERMS; ++t) first_terms[t] = z;
    }
    report[WITNESS_FIRST_MASK] = mask;
}

// wire id w = input * n + gate is the flat index into wire_values_by_wire_index; rows 0..5 are the routed wires
__global__ void __launch_bounds__(CHECK_COPY_LANES) k_check_copies(const uint4* __restrict__ wires, const uint32_t* __restrict__ sigma, int log_degree,
                                                                  uint32_t* __restrict__ report) {
    const uint32_t n6 = WITNESS_ROUTED << log_degree;
    const uint32_t w = blockIdx.x * CHECK_COPY_LANES + threadIdx.x;  // 6n < 2^30
    bool differs = false, out_of_range = false;
    if (w < n6) {
        const uint32_t s = sigma[w];
        const WitnessCopy c = witness_copy_class(w, s, (unsigned)log_degree);
        out_of_range = c == WITNESS_COPY_OUT_OF_RANGE;
        if (c == WITNESS_COPY_COMPARE) {
            const uint4 a0 = wires[(size_t)w * 2], a1 = wires[(size_t)w * 2 + 1], b0 = wires[(size_t)s * 2], b1 = wires[(size_t)s * 2 + 1];
            differs = ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) != 0;
        }
    }
    const uint32_t base = w - (threadIdx.x & 63);
    const WitnessWave bad = witness_wave_merge(__ballot(differs), base), far = witness_wave_merge(__ballot(out_of_range), base);
    if ((threadIdx.x & 63) == 0) {
        if (bad.count) {
            atomicAdd(&report[WITNESS_BAD_COPIES], bad.count);
            atomicMin(&report[WITNESS_FIRST_COPY], bad.first);
        }
        if (far.count) atomicAdd(&report[WITNESS_SIGMA_RANGE], far.count);
    }
}

template <class P>
static int check_witness_t(unsigned log_degree, const void* d_constants, unsigned constants_stride, const void* d_wires, const void* d_sigma, const PlonkScalars& sc,
                           void* d_report, void* d_row_masks, void* d_first_terms, hipStream_t stream) {
    std::shared_ptr<PlonkTables> t;
    PLK_TRY(get_plonk_tables<P>(7, stream, t));  // the small inverses and the table of lz_from_rform: any circuit size serves
    const uint32_t n = 1u << log_degree, n6 = WITNESS_ROUTED << log_degree;
    k_check_init<<<1, 64, 0, stream>>>((uint32_t*)d_report);
    k_check_rows<P><<<(n + CHECK_LANES - 1) / CHECK_LANES, CHECK_LANES, 0, stream>>>((const uint4*)d_constants, constants_stride, (const uint4*)d_wires,
                                                                                      (const uint4*)t->small.p, sc, (int)log_degree, (uint8_t*)d_row_masks,
                                                                                      (uint32_t*)d_report, (const uint32_t*)t->top.p);
    k_check_first<P><<<1, 64, 0, stream>>>((const uint4*)d_constants, constants_stride, (const uint4*)d_wires, (const uint4*)t->small.p, sc, (int)log_degree,
                                           (uint32_t*)d_report, (uint4*)d_first_terms, (const uint32_t*)t->top.p);
    if (d_sigma)
        k_check_copies<<<(n6 + CHECK_COPY_LANES - 1) / CHECK_COPY_LANES, CHECK_COPY_LANES, 0, stream>>>((const uint4*)d_wires, (const uint32_t*)d_sigma,
                                                                                                         (int)log_degree, (uint32_t*)d_report);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "witness check launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

// the refusals both entries share, each with its own text: nothing is launched or copied before they pass
int plonk_check_witness_check(unsigned log_degree, int field, const void* constants, unsigned constants_stride, const void* wires, const uint64_t* inner_zeta,
                              const uint64_t* inner_a, const void* report) {
    const int limbs = field_limbs(field);
    if (limbs < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (limbs != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d has %d limbs: not a circuit scalar field", field, limbs);
    if (log_degree > 27) return set_error(PLK_ERR_INVALID_ARG, "log_degree %u: the witness check takes log_degree <= 27", log_degree);
    if (constants_stride != 1 && constants_stride != 8) return set_error(PLK_ERR_INVALID_ARG, "constants_stride %u is neither 1 nor 8", constants_stride);
    if (!constants) return set_error(PLK_ERR_INVALID_ARG, "null pointer: constants");
    if (!wires) return set_error(PLK_ERR_INVALID_ARG, "null pointer: wires");
    if (!report) return set_error(PLK_ERR_INVALID_ARG, "null pointer: report");
    if (!inner_zeta) return set_error(PLK_ERR_INVALID_ARG, "null pointer: inner_zeta");
    if (!inner_a) return set_error(PLK_ERR_INVALID_ARG, "null pointer: inner_a");
    return PLK_OK;
}

int plonk_check_witness_dev_impl(unsigned log_degree, int field, const void* d_constants, unsigned constants_stride, const void* d_wires, const void* d_sigma,
                                 const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_report, void* d_row_masks, void* d_first_terms, hipStream_t stream) {
    PLK_TRY(plonk_check_witness_check(log_degree, field, d_constants, constants_stride, d_wires, inner_zeta, inner_a, d_report));
    PLK_TRY(ensure_device());
    PlonkScalars sc;
    PLK_TRY(fill_scalars(sc, nullptr, nullptr, nullptr, nullptr, inner_zeta, inner_a));
    return or_invalid(with_field4(field,
                                  [&](auto t) {
                                      return check_witness_t<tag_t<decltype(t)>>(log_degree, d_constants, constants_stride, d_wires, d_sigma, sc, d_report, d_row_masks,
                                                                                 d_first_terms, stream);
                                  }),
                      "field %d is not a circuit scalar field", field);
}

// ---------------------------------------------------------------------------------------------
// permutation_polynomial (plonk_util.rs:234-262): the grand product Z of the copy-constraint argument
// ---------------------------------------------------------------------------------------------
// Z[0] = 1, Z[i] = Z[i - 1] num_(i-1) / den_(i-1) with num_r = prod_j (w_j[r] + beta k_j g^r + gamma) and
// den_r = prod_j (w_j[r] + beta sigma_j[r] + gamma): Z is the EXCLUSIVE product scan of f_r = num_r / den_r over the n rows, and the
// inclusive total (row n - 1 included) is 1 exactly when Z closes the cycle.  The reference walks the rows serially, one full
// inversion per row; here it is a reduce-then-scan in three launches (no hand-off between workgroups inside a launch):
//   k_perm_rows   a lane owns PERM_ROWS consecutive rows: their num / den, ONE inversion for the lane (Montgomery's trick on the
//                 prefix products: f's exclusive prefixes are N_m / D_m), then a workgroup scan of the lane totals; writes the
//                 tile-local exclusive prefixes (R'-form words) into the output and one total per tile;
//   k_perm_tiles  one workgroup scans the tile totals (a run of consecutive tiles per lane, then the lanes) and writes the status;
//   k_perm_fix    Z[i] = tile prefix x local prefix, in the reference's form.
// A zero den_r is replaced by 1 and counted (as k_batch_inverse does); rows 0..n-2 are the reference's panic, row n - 1 never
// enters Z and only spoils the wrap check.
constexpr int PERM_ROWS = 8, PERM_LANES = 256, PERM_TILE = PERM_ROWS * PERM_LANES;

template <class P>
__global__ void __launch_bounds__(PERM_LANES) k_perm_rows(const uint4* __restrict__ wires, const uint4* __restrict__ s_sigma, unsigned sigma_stride,
                                                          const uint4* __restrict__ xs_lo_z, const uint4* __restrict__ xs_hi_z, PlonkScalars sc, int log_degree,
                                                          uint4* __restrict__ out, uint32_t* __restrict__ tile_tot, unsigned* __restrict__ zeros,
                                                          const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    constexpr int NZ = FzCfg<P>::NZ;
    using D = Lz<P, 16>;
    __shared__ uint32_t s_sc[NUM_SCALARS][NZ];
    __shared__ uint32_t s_bk[NUM_ROUTED_WIRES][NZ];
    __shared__ uint32_t s_wave[PERM_LANES / 64][NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    stage_scalars<P>(sc, s_sc);  // ends with the barrier that publishes both
    if (threadIdx.x < NUM_ROUTED_WIRES) {  // beta k_j: one product per wire and row instead of two (plonk_util.rs:245)
        const LzP<P> bk = scalar_at<P>(s_sc, 7) * scalar_at<P>(s_sc, threadIdx.x);
#pragma unroll
        for (int i = 0; i < NZ; ++i) s_bk[threadIdx.x][i] = bk.v.l[i];
    }
    __syncthreads();
    const size_t n = (size_t)1 << log_degree, n8 = n << 3;
    const size_t r0 = ((size_t)blockIdx.x * PERM_LANES + threadIdx.x) * PERM_ROWS;
    const D beta = scalar_at<P>(s_sc, 7), gamma = scalar_at<P>(s_sc, 8);
    const LzP<P> one = lz_one<P>().template widen<9>();
    // x = g_n^r = g_8n^(8 r) from the cached powers of the 8n-th root (hi[0] = 1), then one product by g_n = g_8n^8 per row
    const size_t i8 = (r0 << 3) & (n8 - 1);
    LzP<P> x = lz_table<P>(xs_lo_z, i8 & (((size_t)1 << XS_LO_LOG) - 1)) * lz_table<P>(xs_hi_z, i8 >> XS_LO_LOG);
    const Lz<P, 8> g = lz_table<P>(xs_lo_z, 8);  // lo[j] = g_8n^(j mod 8n): 1 when n = 1
    LzP<P> num_pre[PERM_ROWS], den[PERM_ROWS];  // num_pre[m] = N_(m+1) = prod_(k <= m) num_k
    LzP<P> n_run = one, d_run = one;
    unsigned z_head = 0, z_last = 0;
#pragma unroll
    for (int m = 0; m < PERM_ROWS; ++m) {
        const size_t r = r0 + m;
        LzP<P> num = one, de = one;
        if (r < n) {
#pragma unroll
            for (int j = 0; j < NUM_ROUTED_WIRES; ++j) {
                LzP<P> bk;
#pragma unroll
                for (int i = 0; i < NZ; ++i) bk.v.l[i] = s_bk[j][i];
                const D w = lz_load<P>(wires, (size_t)j * n + r, s_top);
                const D s = lz_load<P>(s_sigma, ((size_t)j * n + r) * sigma_stride, s_top);
                num = num * (w + bk * x + gamma);
                de = de * (w + beta * s + gamma);
            }
            if (fz_is_zero_mod_p<P>(de.v)) {  // field.rs "No inverse" for rows 0..n-2
                de = one;
                if (r + 1 < n) ++z_head;
                else ++z_last;
            }
        }
        x = x * g;
        n_run = n_run * num;
        num_pre[m] = n_run;
        den[m] = de;
        d_run = d_run * de;
    }
    // 1 / D_8 through the reference's form (the inversion works on the integer), back to R'-form limbs
    LzP<P> inv = Lz<P, 8>{fz_from_fe<P>(fe_inv_safegcd<P>(lz_to_rform<P>(d_run)))} * Lz<P, 8>{fz_const_r_to_rprime<P>()};
    const LzP<P> lane_total = num_pre[PERM_ROWS - 1] * inv;
    LzP<P> e[PERM_ROWS];  // e[m] = N_m / D_m: the product of f over the lane's rows before m
    e[0] = one;
#pragma unroll
    for (int m = PERM_ROWS - 1; m >= 1; --m) {
        inv = inv * den[m];  // 1 / D_m
        e[m] = num_pre[m - 1] * inv;
    }
    if (z_head) atomicAdd(&zeros[0], z_head);
    if (z_last) atomicAdd(&zeros[1], z_last);
    const LzP<P> ex = wg_exclusive_product<P, PERM_LANES / 64>(lane_total, s_wave);
    if (threadIdx.x == PERM_LANES - 1) limbs_store<P>(tile_tot, blockIdx.x, (ex * lane_total).v);
#pragma unroll
    for (int m = 0; m < PERM_ROWS; ++m) {
        if (r0 + m >= n) break;
        const LzP<P> v = m == 0 ? ex : ex * e[m];
        fe_store<P>(out + (r0 + m) * 2, fz_to_fe_canonical<P>(v.v));  // R'-form words, canonical (k_perm_fix reads them back)
    }
}


template <class P> __global__ void __launch_bounds__(256) k_perm_fix(uint4* __restrict__ out, const uint32_t* __restrict__ tile_pre, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LzP<P> z = lz_table<P>(out, i) * LzP<P>{limbs_load<P>(tile_pre, i / PERM_TILE)};
    fe_store<P>(out + i * 2, fz_to_fe_canonical<P>(z.v));
}

template <class P>
static int permutation_z_t(unsigned log_degree, const void* d_wires, const void* d_s_sigma, unsigned sigma_stride, const PlonkScalars& sc, void* d_out,
                           void* d_status, hipStream_t stream) {
    std::shared_ptr<PlonkTables> t;
    PLK_TRY(get_plonk_tables<P>((int)log_degree, stream, t));
    const size_t n = (size_t)1 << log_degree, tiles = (n + PERM_TILE - 1) / PERM_TILE;
    unsigned* zeros = (unsigned*)scratch_acquire(2 * sizeof(unsigned), stream);
    if (!zeros) return PLK_ERR_OOM;
    uint32_t* tile_tot = (uint32_t*)scratch_acquire(limb_bytes(tiles, FzCfg<P>::NZ), stream);
    if (!tile_tot) {
        scratch_release(zeros, stream);
        return PLK_ERR_OOM;
    }
    hipError_t e = hipMemsetAsync(zeros, 0, 2 * sizeof(unsigned), stream);
    if (e == hipSuccess) {
        k_perm_rows<P><<<(unsigned)tiles, PERM_LANES, 0, stream>>>((const uint4*)d_wires, (const uint4*)d_s_sigma, sigma_stride, (const uint4*)t->xs_lo_z.p,
                                                                   (const uint4*)t->xs_hi_z.p, sc, (int)log_degree, (uint4*)d_out, tile_tot, zeros,
                                                                   (const uint32_t*)t->top.p);
        k_perm_tiles<P><<<1, PERM_SCAN_LANES, 0, stream>>>(tile_tot, tiles, zeros, (uint32_t*)d_status);
        k_perm_fix<P><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>((uint4*)d_out, tile_tot, n);
        e = hipGetLastError();
    }
    scratch_release(tile_tot, stream);
    scratch_release(zeros, stream);
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "permutation Z launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

int plonk_permutation_z_dev_impl(int field, unsigned log_degree, const void* d_wires, const void* d_s_sigma, unsigned sigma_stride, const uint64_t* k_is,
                                 const uint64_t* beta, const uint64_t* gamma, void* d_out, void* d_status, hipStream_t stream) {
    if (!d_wires || !d_s_sigma || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    if (!k_is || !beta || !gamma) return set_error(PLK_ERR_INVALID_ARG, "null challenge / shift pointer");
    if (sigma_stride != 1 && sigma_stride != 8) return set_error(PLK_ERR_INVALID_ARG, "sigma_stride %u is neither 1 nor 8", sigma_stride);
    if (log_degree + 3 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_degree %u too large", log_degree);
    PLK_TRY(ensure_device());
    static const uint64_t zero4[4] = {0, 0, 0, 0};
    PlonkScalars sc;
    PLK_TRY(fill_scalars(sc, k_is, nullptr, beta, gamma, zero4, zero4));
    return or_invalid(with_field4(field, [&](auto t) { return permutation_z_t<tag_t<decltype(t)>>(log_degree, d_wires, d_s_sigma, sigma_stride, sc, d_out, d_status, stream); }),
                      "field %d is not a circuit scalar field", field);
}

}  // namespace plk
