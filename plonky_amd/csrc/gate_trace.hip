// gate_trace.hip -- gate witness rows on the device: the blocks of rows the in-circuit Rescue permutation and the in-circuit MSM lay
// down, written where the prover's wire table wants them (include/plonky_hip_trace.h).
//
// Reference path                                                              here
//   CircuitBuilder::rescue_permutation        circuit_builder.rs:931-970   ->  k_trace_rescue   (the rows of a block)
//   RescueStepAGate / BGate ::generate        rescue_a.rs:116-155          ->  the round of rescue_step.cuh, one element per lane
//   CircuitBuilder::curve_msm                 circuit_curve.rs:287-410     ->  k_trace_msm      (trace_msm_instance, one instance per lane)
//   CurveAddGate / CurveDblGate ::generate    curve_add.rs:173-262         ->  trace_add_step / trace_dbl_step (gate_trace_step.cuh)
//   generate_partial_witness                  witness.rs                   ->  NOT here: the fixed point over the copy constraints
//
// Rescue: the quad-per-state form of rescue.hip.  A lane holds one element of a state and so owns one column of wires 0..3 and one of
// wires 4..7: it stores the element entering the round, its root, the element after step A, and hands the element after step B to the
// next round.  A store is one 32-byte element, a whole sector of its own, so the sectors written are the same whichever lanes sit
// side by side; the quad layout stays because the matrix rows come over DPP quad broadcasts.
// curve_msm: one instance per lane.  The chain is sequential within an instance and every row needs an inversion that is itself a
// wire; each lane runs the division-step inversion of fp.cuh (fe_inv_safegcd, branch-free in its fixed form: no lane diverges).
#include "ec.cuh"
#include "gate_trace_step.cuh"
#include "rescue_lane.cuh"

namespace plk {

constexpr int TRACE_RESCUE_LANES = 256;  // 64 states per workgroup, as rescue.hip
constexpr int TRACE_RESCUE_STATES = TRACE_RESCUE_LANES / RESCUE_WIDTH;
constexpr int TRACE_MSM_LANES = 64;      // one wave: the chains are long and the batches small

// the caller's tables; constants may be null
template <class P> struct TraceSink {
    uint4* wires;
    uint4* constants;
    uint32_t n_rows;
    PLK_DI void wire(uint32_t j, uint32_t row, const Fe<P>& v) const { fe_store<P>(wires + trace_at(j, row, n_rows) * (P::NL / 4), v); }
    PLK_DI void constant(uint32_t j, uint32_t row, const Fe<P>& v) const {
        if (constants) fe_store<P>(constants + trace_at(j, row, n_rows) * (P::NL / 4), v);
    }
};

__global__ void __launch_bounds__(64) k_trace_status_init(uint32_t* status) {
    if (threadIdx.x < TRACE_STATUS_WORDS) status[threadIdx.x] = trace_status_init((int)threadIdx.x);
}

// consts_r: the context's constants as they came (R-form), rounds x 2 x W elements
template <class P>
__global__ void __launch_bounds__(TRACE_RESCUE_LANES) k_trace_rescue(const uint4* __restrict__ inputs, const uint32_t* __restrict__ first_rows, uint32_t count,
                                                                     RescueTables t, const uint4* __restrict__ consts_r, TraceSink<P> sink, uint32_t* status) {
    constexpr int NZ = FzCfg<P>::NZ, W4 = P::NL / 4;
    const uint32_t s = blockIdx.x * TRACE_RESCUE_STATES + threadIdx.x / RESCUE_WIDTH;
    const uint32_t e = threadIdx.x % RESCUE_WIDTH;
    if (s >= count) return;  // a whole quad leaves together
    const uint32_t first = first_rows[s];
    if (!trace_block_fits(first, trace_rescue_block_rows(t.rounds), sink.n_rows)) {  // the quad's four lanes agree
        if (e == 0 && status) atomicAdd(&status[TRACE_OVERRUN], 1u);
        return;
    }
    const uint32_t* mrow = t.mds + e * RESCUE_WIDTH * NZ;
    Fz<P> x = rescue_enter<P>(fe_load<P>(inputs + ((size_t)s * RESCUE_WIDTH + e) * W4));
#pragma unroll 1
    for (uint32_t r = 0; r < t.rounds; ++r) {
        const uint32_t row = first + 2 * r;
        const size_t at = (size_t)r * 2 * RESCUE_WIDTH + e;
        const uint32_t* k = t.consts + at * NZ;
        sink.wire(e, row, rescue_leave<P>(x));
        const Fz<P> y = rescue_pow<P>(x, t.exp, t.windows);
        sink.wire(RESCUE_WIDTH + e, row, rescue_leave<P>(y));
        x = rescue_lane_row<P>(y, mrow, k);
        sink.wire(e, row + 1, rescue_leave<P>(x));
        x = rescue_lane_row<P>(rescue_pow_alpha<P>(x), mrow, k + RESCUE_WIDTH * NZ);
        if (sink.constants) {  // uniform: a kernel argument
            sink.constant(2 + e, row, fe_load<P>(consts_r + at * W4));
            sink.constant(2 + e, row + 1, fe_load<P>(consts_r + (at + RESCUE_WIDTH) * W4));
            if (e < trace_prefix_len(TRACE_RESCUE_A)) {
                sink.constant(e, row, trace_prefix_value<P>(TRACE_RESCUE_A, e));
                sink.constant(e, row + 1, trace_prefix_value<P>(TRACE_RESCUE_B, e));
            }
        }
    }
    const uint32_t last = first + 2 * t.rounds;
    sink.wire(e, last, rescue_leave<P>(x));
    for (uint32_t j = e; j < trace_prefix_len(TRACE_BUFFER); j += RESCUE_WIDTH) sink.constant(j, last, trace_prefix_value<P>(TRACE_BUFFER, j));
}

// part j of an instance: its addend and its scalar, straight from the caller's arrays (they stay in L2 over the chain)
template <class P> struct TraceMsmIn {
    const uint4* points;   // the instance's `parts` points
    const uint4* scalars;  // the instance's `parts` scalars
    PLK_DI void point(uint32_t j, Fe<P>& x, Fe<P>& y) const {
        x = fe_load<P>(points + (size_t)j * 2 * (P::NL / 4));
        y = fe_load<P>(points + ((size_t)j * 2 + 1) * (P::NL / 4));
    }
    PLK_DI Fe<P> scalar(uint32_t j) const { return fe_load<P>(scalars + (size_t)j * (P::NL / 4)); }
};

struct TraceStart {  // the starting accumulator as a kernel argument: x then y, 8 words each
    uint32_t w[16];
};

template <class P>
__global__ void __launch_bounds__(TRACE_MSM_LANES) k_trace_msm(const uint4* __restrict__ points, const uint4* __restrict__ scalars,
                                                               const uint32_t* __restrict__ first_rows, uint32_t count, uint32_t parts, uint32_t n_bits,
                                                               TraceStart start, TraceSink<P> sink, uint32_t* status) {
    constexpr int W4 = P::NL / 4;
    const uint32_t c = blockIdx.x * TRACE_MSM_LANES + threadIdx.x;
    if (c >= count) return;
    const uint32_t first = first_rows[c];
    if (!trace_block_fits(first, trace_msm_block_rows(parts, n_bits), sink.n_rows)) {
        if (status) atomicAdd(&status[TRACE_OVERRUN], 1u);
        return;
    }
    TraceMsmIn<P> in{points + (size_t)c * parts * 2 * W4, scalars + (size_t)c * parts * W4};
    const bool exceptional = trace_msm_instance<P>(parts, n_bits, first, fe_from_words<P>(start.w), fe_from_words<P>(start.w + P::NL), in, sink);
    if (exceptional && status) {
        atomicAdd(&status[TRACE_EXCEPTIONAL], 1u);
        atomicMin(&status[TRACE_FIRST_EXCEPTIONAL], c);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int trace_rows_check(size_t n_rows) {
    if (n_rows == 0 || n_rows > ((size_t)1 << TRACE_MAX_LOG_ROWS)) return set_error(PLK_ERR_INVALID_ARG, "n_rows %zu: a table has 1 .. 2^%u rows", n_rows, TRACE_MAX_LOG_ROWS);
    return PLK_OK;
}
static int trace_count_check(size_t count) {
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call takes at most 2^32 - 1 instances", count);
    return PLK_OK;
}
static void trace_status_begin(void* d_status, hipStream_t stream) {
    if (d_status) k_trace_status_init<<<1, 64, 0, stream>>>((uint32_t*)d_status);
}

// the refusals the host and device entries share: nothing is launched or copied before they pass
int trace_rescue_check(size_t count, const plk_rescue_ctx* ctx, size_t n_rows) {
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    PLK_TRY(trace_count_check(count));
    PLK_TRY(or_bad_field(with_field(ctx->field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        if (P::NL != 8) return set_error(PLK_ERR_INVALID_ARG, "field %d has %d limbs: the wire table holds 4-limb elements", ctx->field, P::NL / 2);
        if (rescue_alpha<P>() != 5u)
            return set_error(PLK_ERR_INVALID_ARG, "field %d: Rescue exponent %u, the gates hard-code exp_usize(5) (rescue_a.rs:54)", ctx->field, rescue_alpha<P>());
        return (int)PLK_OK;
    }), ctx->field));
    return trace_rows_check(n_rows);
}

int trace_rescue_dev_impl(size_t count, const plk_rescue_ctx* ctx, const void* d_inputs, size_t n_rows, void* d_wires, const void* d_first_rows,
                          void* d_constants, void* d_status, hipStream_t stream) {
    PLK_TRY(trace_rescue_check(count, ctx, n_rows));
    if (count == 0) return PLK_OK;
    if (!d_inputs) return set_error(PLK_ERR_INVALID_ARG, "null pointer: inputs");
    if (!d_wires) return set_error(PLK_ERR_INVALID_ARG, "null pointer: wires");
    if (!d_first_rows) return set_error(PLK_ERR_INVALID_ARG, "null pointer: first_rows");
    PLK_TRY(rescue_on_ctx_device(ctx));
    trace_status_begin(d_status, stream);
    PLK_TRY(or_bad_field(with_field4(ctx->field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        if constexpr (rescue_alpha<P>() == 5u) {
            k_trace_rescue<P><<<(unsigned)((count + TRACE_RESCUE_STATES - 1) / TRACE_RESCUE_STATES), TRACE_RESCUE_LANES, 0, stream>>>(
                (const uint4*)d_inputs, (const uint32_t*)d_first_rows, (uint32_t)count, rescue_tables(ctx), (const uint4*)ctx->d_consts_r,
                TraceSink<P>{(uint4*)d_wires, (uint4*)d_constants, (uint32_t)n_rows}, (uint32_t*)d_status);
        }
        return (int)PLK_OK;
    }), ctx->field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

int trace_msm_check(size_t count, unsigned parts, unsigned n_bits, int curve, const uint64_t* start_xy, size_t n_rows) {
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using FP = typename tag_t<decltype(t)>::FP;
        if (FP::NL != 8) return set_error(PLK_ERR_INVALID_ARG, "curve %d has a %d-limb base field: the wire table holds 4-limb elements", curve, FP::NL / 2);
        PLK_TRY(trace_count_check(count));
        if (parts < 1 || parts > TRACE_MSM_MAX_PARTS) return set_error(PLK_ERR_INVALID_ARG, "parts %u: a curve_msm block takes 1 .. %u parts", parts, TRACE_MSM_MAX_PARTS);
        if (n_bits < 1 || n_bits > (unsigned)FP::BITS - 1)
            return set_error(PLK_ERR_INVALID_ARG, "n_bits %u: 1 .. %d on curve %d (f_bits = BITS - 1, circuit_curve.rs:292)", n_bits, FP::BITS - 1, curve);
        return (int)PLK_OK;
    }), curve));
    PLK_TRY(trace_rows_check(n_rows));
    if (!start_xy) return set_error(PLK_ERR_INVALID_ARG, "null pointer: start_xy");
    return PLK_OK;
}

int trace_msm_dev_impl(size_t count, unsigned parts, unsigned n_bits, int curve, const void* d_points, const void* d_scalars, const uint64_t* start_xy, size_t n_rows,
                       void* d_wires, const void* d_first_rows, void* d_constants, void* d_status, hipStream_t stream) {
    PLK_TRY(trace_msm_check(count, parts, n_bits, curve, start_xy, n_rows));
    if (count == 0) return PLK_OK;
    if (!d_points) return set_error(PLK_ERR_INVALID_ARG, "null pointer: points");
    if (!d_scalars) return set_error(PLK_ERR_INVALID_ARG, "null pointer: scalars");
    if (!d_wires) return set_error(PLK_ERR_INVALID_ARG, "null pointer: wires");
    if (!d_first_rows) return set_error(PLK_ERR_INVALID_ARG, "null pointer: first_rows");
    PLK_TRY(ensure_device());
    TraceStart start;
    limbs_to_words(start.w, start_xy, 8);
    trace_status_begin(d_status, stream);
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        using FP = typename tag_t<decltype(t)>::FP;
        if constexpr (FP::NL == 8) {
            k_trace_msm<FP><<<(unsigned)((count + TRACE_MSM_LANES - 1) / TRACE_MSM_LANES), TRACE_MSM_LANES, 0, stream>>>(
                (const uint4*)d_points, (const uint4*)d_scalars, (const uint32_t*)d_first_rows, (uint32_t)count, parts, n_bits, start,
                TraceSink<FP>{(uint4*)d_wires, (uint4*)d_constants, (uint32_t)n_rows}, (uint32_t*)d_status);
        }
        return (int)PLK_OK;
    }), curve));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
