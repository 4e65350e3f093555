// gate_trace_step.cuh -- what the kernels of gate_trace.hip and tests/gate_trace_host_replay.cpp share: where a wire of a row lives in
// the prover's wire table, the rows of a gadget's block, the gate prefixes, one Rescue round emitting its two rows
// (circuit_builder.rs:931-970, rescue_a.rs:116-155, rescue_b.rs) and one CurveAddGate / CurveDblGate row (circuit_curve.rs:287-410,
// curve_add.rs:173-262, curve_dbl.rs) with the chain of a whole curve_msm instance over them.  Plain C++17: under hipcc the field code
// is device code, under g++ it is the host's.
//
// A Sink takes what a step emits: sink.wire(j, row, v) is wire j of gate row `row`, sink.constant(j, row, v) constant column j of it
// (the kernels' sink drops the constants when the caller gave no table).  Elements are R-form (the reference's limbs), fully reduced.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.cuh"
#include "rescue_step.cuh"

#ifdef __HIPCC__
#define TRACE_HD __host__ __device__ __forceinline__
#else
#define TRACE_HD inline
#endif

namespace plk {

constexpr uint32_t TRACE_WIRES = 9;               // NUM_WIRES (plonk.rs:21)
constexpr uint32_t TRACE_CONSTANTS = 6;           // NUM_CONSTANTS (plonk.rs:24)
constexpr uint32_t TRACE_NONE = 0xFFFFFFFFu;      // status word [2] when no instance met an exceptional case
constexpr unsigned TRACE_MAX_LOG_ROWS = 27;       // the witness check's bound on n
constexpr uint32_t TRACE_MSM_MAX_PARTS = 8;
constexpr int TRACE_STATUS_WORDS = 4;
// the status: [0] instances whose block would pass n_rows (nothing of them is written), [1] instances that met an exceptional case,
// [2] the smallest such instance, [3] zero
enum TraceWord : int { TRACE_OVERRUN = 0, TRACE_EXCEPTIONAL, TRACE_FIRST_EXCEPTIONAL };
TRACE_HD uint32_t trace_status_init(int word) { return word == TRACE_FIRST_EXCEPTIONAL ? TRACE_NONE : 0u; }

// ---- addressing -------------------------------------------------------------------------------------------------------------------
// column j of row i of a [columns][n_rows] table (wire_values_by_wire_index, the n-point constants): what plk_plonk_check_witness_dev
// and the NTT batch read
TRACE_HD size_t trace_at(uint32_t column, uint32_t row, uint32_t n_rows) { return (size_t)column * n_rows + row; }
// rows of a block: 2 rounds + 1 (an A and a B row per round, the row that receives the final state); n_bits groups of `parts` add rows
// and one doubling row
TRACE_HD uint64_t trace_rescue_block_rows(uint64_t rounds) { return 2 * rounds + 1; }
TRACE_HD uint64_t trace_msm_block_rows(uint32_t parts, uint32_t n_bits) { return (uint64_t)n_bits * (parts + 1u); }
// compared in 64 bits before any row is formed: a first row near 2^32 cannot wrap into the table
TRACE_HD bool trace_block_fits(uint32_t first_row, uint64_t block_rows, uint32_t n_rows) { return (uint64_t)first_row + block_rows <= (uint64_t)n_rows; }

// ---- gate prefixes: bit i is constant column i (the PREFIX of each gate file as the code has them; buffer.rs:24 is 101000) ---------------------
enum TraceGate : int { TRACE_RESCUE_A = 0, TRACE_RESCUE_B, TRACE_BUFFER, TRACE_CURVE_ADD, TRACE_CURVE_DBL };
TRACE_HD uint32_t trace_prefix_len(int gate) { return gate <= TRACE_RESCUE_B ? 2u : gate == TRACE_BUFFER ? 6u : 5u; }
TRACE_HD uint32_t trace_prefix_bits(int gate) {
    return gate == TRACE_RESCUE_A ? 0x00u    // 00
         : gate == TRACE_RESCUE_B ? 0x02u    // 01
         : gate == TRACE_BUFFER ? 0x05u      // 101000
         : gate == TRACE_CURVE_ADD ? 0x15u   // 10101
                                   : 0x1Du;  // 10111
}
template <class P> PLK_DI Fe<P> trace_prefix_value(int gate, uint32_t column) { return ((trace_prefix_bits(gate) >> column) & 1u) ? fe_one<P>() : fe_zero<P>(); }
template <class P, class Sink> PLK_DI void trace_emit_prefix(int gate, uint32_t row, Sink& sink) {
    for (uint32_t j = 0; j < trace_prefix_len(gate); ++j) sink.constant(j, row, trace_prefix_value<P>(gate, j));
}

// ---- Rescue -------------------------------------------------------------------------------------------------------------------------
// One round of a whole state and its two rows.  Row row_a, the A gate: wires 0..3 the state entering the round, wires 4..7 its roots
// (rescue_a.rs:132), columns 2..5 the step-A constants; row row_a + 1, the B gate: wires 0..3 MDS roots + A constants, columns 2..5
// the step-B constants.  On return `state` is MDS state^5 + B constants: wires 0..3 of row row_a + 2, which the next round, or
// trace_rescue_receive, writes.  d / windows / mds / ka / kb as rescue_permutation_step takes them; ka_r / kb_r: the same constants in
// R-form, as the gates' constant columns hold them.  The kernel runs the same calls with one element per lane.
template <class P, class Sink>
PLK_DI void trace_rescue_round(Fz<P> (&state)[RESCUE_WIDTH], uint32_t row_a, const uint32_t* d, int windows, const uint32_t* mds, const uint32_t* ka,
                               const uint32_t* kb, const Fe<P>* ka_r, const Fe<P>* kb_r, Sink& sink) {
    constexpr int NZ = FzCfg<P>::NZ;
    Fz<P> y[RESCUE_WIDTH];
    for (int e = 0; e < RESCUE_WIDTH; ++e) {
        sink.wire(e, row_a, rescue_leave<P>(state[e]));
        y[e] = rescue_pow<P>(state[e], d, windows);
        sink.wire(RESCUE_WIDTH + e, row_a, rescue_leave<P>(y[e]));
        sink.constant(2 + e, row_a, ka_r[e]);
        sink.constant(2 + e, row_a + 1, kb_r[e]);
    }
    trace_emit_prefix<P>(TRACE_RESCUE_A, row_a, sink);
    trace_emit_prefix<P>(TRACE_RESCUE_B, row_a + 1, sink);
    for (int e = 0; e < RESCUE_WIDTH; ++e) state[e] = rescue_mds_row<P>(y, mds + e * RESCUE_WIDTH * NZ, ka + e * NZ);
    for (int e = 0; e < RESCUE_WIDTH; ++e) {
        sink.wire(e, row_a + 1, rescue_leave<P>(state[e]));
        y[e] = rescue_pow_alpha<P>(state[e]);
    }
    for (int e = 0; e < RESCUE_WIDTH; ++e) state[e] = rescue_mds_row<P>(y, mds + e * RESCUE_WIDTH * NZ, kb + e * NZ);
}
// the row after the last round: a BufferGate that receives the final state (circuit_builder.rs:962-968)
template <class P, class Sink> PLK_DI void trace_rescue_receive(const Fz<P> (&state)[RESCUE_WIDTH], uint32_t row, Sink& sink) {
    for (int e = 0; e < RESCUE_WIDTH; ++e) sink.wire(e, row, rescue_leave<P>(state[e]));
    trace_emit_prefix<P>(TRACE_BUFFER, row, sink);
}

// ---- curve_msm --------------------------------------------------------------------------------------------------------------------
// CurveAddGate::generate (curve_add.rs:229-260): p1 the accumulator, p2 the addend, p4 = bit ? p1 + p2 : p1; the inverse of x1 - x2 and
// lambda are wires, computed whether or not the bit is set.  false where the reference panics "x_1 = x_2".
template <class P>
PLK_DI bool trace_add_step(const Fe<P>& x1, const Fe<P>& y1, const Fe<P>& x2, const Fe<P>& y2, bool bit, Fe<P>& x4, Fe<P>& y4, Fe<P>& inverse, Fe<P>& lambda) {
    const Fe<P> dx = fe_sub<P>(x1, x2);
    if (fe_is_zero<P>(dx)) return false;
    inverse = fe_inv_safegcd<P>(dx);
    lambda = fe_mul<P>(fe_sub<P>(y1, y2), inverse);
    const Fe<P> x3 = fe_sub<P>(fe_sub<P>(fe_sqr<P>(lambda), x1), x2);
    const Fe<P> y3 = fe_sub<P>(fe_mul<P>(lambda, fe_sub<P>(x1, x3)), y1);
    x4 = bit ? x3 : x1;
    y4 = bit ? y3 : y1;
    return true;
}
// CurveDblGate::generate (curve_dbl.rs:150-175): the inverse of 2 y and lambda = (3 x^2 + InnerC::A) / (2 y) are wires; InnerC::A is 0
// on every in-scope curve (ec.cuh).  false where the reference panics "y = 0".
template <class P> PLK_DI bool trace_dbl_step(const Fe<P>& x, const Fe<P>& y, Fe<P>& x_new, Fe<P>& y_new, Fe<P>& inverse, Fe<P>& lambda) {
    if (fe_is_zero<P>(y)) return false;
    inverse = fe_inv_safegcd<P>(fe_dbl<P>(y));
    const Fe<P> xx = fe_sqr<P>(x);
    lambda = fe_mul<P>(fe_add<P>(fe_dbl<P>(xx), xx), inverse);
    x_new = fe_sub<P>(fe_sqr<P>(lambda), fe_dbl<P>(x));
    y_new = fe_sub<P>(fe_mul<P>(lambda, fe_sub<P>(x, x_new)), y);
    return true;
}

// the canonical words of a scalar shifted right by `s` bits (s <= 32 NL), as an R-form element: the scalar accumulator of a part once
// the bits from s up have gone in (scalar_acc_new = 2 scalar_acc_old + bit from zero, curve_add.rs:240)
template <class P> PLK_DI Fe<P> trace_scalar_top(const Fe<P>& canonical, uint32_t s) {
    Fe<P> r;
    const uint32_t w = s >> 5, b = s & 31u;
    for (int i = 0; i < P::NL; ++i) {
        const uint32_t lo = i + w < (uint32_t)P::NL ? canonical.v[i + w] : 0u, hi = i + w + 1 < (uint32_t)P::NL ? canonical.v[i + w + 1] : 0u;
        r.v[i] = b ? (lo >> b) | (hi << (32u - b)) : lo;
    }
    return fe_from_canonical<P>(r);
}

// One curve_msm instance (circuit_curve.rs:287-410), n_bits (parts + 1) rows from first_row: for bit i from n_bits - 1 down to 0 one
// CurveAddGate row per part - wires 0/1 the accumulator, 2/3 the part's scalar accumulator before and after, 4/5 the addend, 6 the
// bit, 7 the inverse, 8 lambda - and one CurveDblGate row - 0/1 the accumulator after the last add, 2/3 its double, 4 the inverse, 5
// lambda.  The doubled point of the last group is still written; the result is that row's wires 0/1.  in.point(j, x, y) /
// in.scalar(j): part j's addend and its scalar (R-form; read through its canonical form).  Every row is written by its own step, all
// its defined wires at once, so nothing of a row depends on the step before it having run.
// Exceptional cases: a scalar with a bit at or above n_bits (found before the first row), x1 = x2 in an add row, y = 0 in a doubling:
// the rows from that one on are written as zero.  Returns true for such an instance.
template <class P, class In, class Sink>
PLK_DI bool trace_msm_instance(uint32_t parts, uint32_t n_bits, uint32_t first_row, const Fe<P>& start_x, const Fe<P>& start_y, In& in, Sink& sink) {
    bool dead = false;
    for (uint32_t j = 0; j < parts; ++j) {
        const Fe<P> top = trace_scalar_top<P>(fe_to_canonical<P>(in.scalar(j)), n_bits);
        dead = dead || !fe_is_zero<P>(top);
    }
    Fe<P> ax = start_x, ay = start_y;
    const Fe<P> zero = fe_zero<P>();
    uint32_t row = first_row;
    for (uint32_t i = n_bits; i-- > 0;) {
        for (uint32_t j = 0; j < parts; ++j, ++row) {
            trace_emit_prefix<P>(TRACE_CURVE_ADD, row, sink);
            Fe<P> x2, y2, x4, y4, inverse, lambda;
            if (!dead) {
                in.point(j, x2, y2);
                const Fe<P> c = fe_to_canonical<P>(in.scalar(j));
                const bool bit = (c.v[i >> 5] >> (i & 31u)) & 1u;
                if (trace_add_step<P>(ax, ay, x2, y2, bit, x4, y4, inverse, lambda)) {
                    const Fe<P> acc_old = trace_scalar_top<P>(c, i + 1);
                    sink.wire(0, row, ax);
                    sink.wire(1, row, ay);
                    sink.wire(2, row, acc_old);
                    sink.wire(3, row, bit ? fe_add<P>(fe_dbl<P>(acc_old), fe_one<P>()) : fe_dbl<P>(acc_old));
                    sink.wire(4, row, x2);
                    sink.wire(5, row, y2);
                    sink.wire(6, row, bit ? fe_one<P>() : zero);
                    sink.wire(7, row, inverse);
                    sink.wire(8, row, lambda);
                    ax = x4;
                    ay = y4;
                    continue;
                }
                dead = true;
            }
            for (uint32_t w = 0; w < TRACE_WIRES; ++w) sink.wire(w, row, zero);
        }
        trace_emit_prefix<P>(TRACE_CURVE_DBL, row, sink);
        Fe<P> x_new, y_new, inverse, lambda;
        if (!dead && trace_dbl_step<P>(ax, ay, x_new, y_new, inverse, lambda)) {
            sink.wire(0, row, ax);
            sink.wire(1, row, ay);
            sink.wire(2, row, x_new);
            sink.wire(3, row, y_new);
            sink.wire(4, row, inverse);
            sink.wire(5, row, lambda);
            ax = x_new;
            ay = y_new;
        } else {
            dead = true;
            for (uint32_t w = 0; w < 6; ++w) sink.wire(w, row, zero);
        }
        ++row;
    }
    return dead;
}

}  // namespace plk
