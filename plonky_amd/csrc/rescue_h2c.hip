// rescue_h2c.hip -- the reference's Rescue hash to the curve on the device.
//
// Reference path                                                            here
//   hash_base_field_to_curve(seed, security_bits)   hash_to_curve.rs:78-104  ->  k_rescue_h2c_tries (rescue_h2c_step.cuh: one try)
//   hash_u32_to_curve / hash_usize_to_curve         hash_to_curve.rs:3-11    ->  the same with seed = from_canonical(seed_start + k)
//   rescue_sponge([seed, i], 2, security_bits)      rescue.rs:40-68          ->  one permutation of the quad's state (rescue_lane.cuh)
//   Field::square_root                              field.rs:440-472         ->  fe_sqrt.cuh, with the table of ROOT_2ADIC^(2^m)
//
// security_bits is the context's number of rounds (plk_rescue_rounds); the constants are the caller's.  A try is one full permutation
// and one square root, and succeeds with probability ~1/2.  One QUAD of adjacent lanes per open seed, as in k_rescue_sponge: lane e
// holds state element e, lanes 0 and 1 absorb the seed and the counter, and the state stays in registers from the absorb to the
// squeeze.  The two outputs are then broadcast over the quad; all four lanes run the same root on the same values and lane 0 stores.
// Every branch and every loop exit of a quad is taken on the broadcast values (or on the quad's index), never on a lane's own
// element: the DPP broadcasts of the permutation read the neighbouring lanes, so a quad must stay whole.
// The tries run in the rounds of hash_to_curve.hip: round r runs try i = r over the list of seeds still open, a seed that succeeds
// writes its point at its own index, one that does not is appended to the next list (lane 0 of each quad votes, one atomic per wave,
// the counts stay on the device).  After bit_length(count) + 2 rounds one last launch loops what is left up to try H2C_TRIES - 1; a
// seed that runs out of i gets status 2 and zero coordinates.  PLK_H2C_NAIVE=1 runs the loop form alone from try 0: same bytes.
#include "rescue_h2c_step.cuh"
#include "rescue_lane.cuh"

namespace plk {

constexpr int RESCUE_H2C_LANES = 64;  // one wave per workgroup: the compaction is wave-wide, and short lists spread over the CUs
constexpr int RESCUE_H2C_SEEDS = RESCUE_H2C_LANES / RESCUE_WIDTH;

// Tries i_first ..= i_last of the seeds of a list (list == nullptr: the seeds 0 .. count-1 themselves); the arguments are those of
// k_h2c_tries.  seeds == nullptr: seed k is from_canonical_usize(seed_start + k); else L limbs in Montgomery form.
template <class P>
__global__ void __launch_bounds__(RESCUE_H2C_LANES) k_rescue_h2c_tries(const uint4* __restrict__ seeds, uint64_t seed_start, uint32_t count, uint32_t b_coeff,
                                                                       const uint4* __restrict__ root_tab, const uint32_t* __restrict__ list,
                                                                       const uint32_t* __restrict__ open_count, int i_first, int i_last,
                                                                       uint32_t* __restrict__ next, uint32_t* __restrict__ next_count,
                                                                       uint4* __restrict__ out_xy, uint8_t* __restrict__ status, RescueTables t) {
    constexpr int W = P::NL / 4;
    const uint32_t g = blockIdx.x * RESCUE_H2C_SEEDS + threadIdx.x / RESCUE_WIDTH;  // the quad's place in the list
    const int e = threadIdx.x % RESCUE_WIDTH;
    uint32_t open = count;
    if (open_count) open = min(*open_count, count);
    uint32_t k = 0;
    bool settled = true;
    if (g < open) {
        k = list ? list[g] : g;
        settled = k >= count;  // never with a sound list: such an entry is dropped, not followed
    }
    if (!settled) {  // the whole quad or none of it
        const Fe<P> seed = seeds ? fe_load<P>(seeds + (size_t)k * W) : rescue_h2c_from_u64<P>(seed_start + k);
        const Fe<P> b_mont = rescue_h2c_from_u64<P>(b_coeff);
        const auto sponge = [&](const Fe<P>& s, uint32_t i, Fe<P>& o0, Fe<P>& o1) {
            const Fe<P> c = rescue_h2c_from_u64<P>(i);
            Fe<P> in;  // the zero state plus the chunk [seed, i]: lane 0 the seed, lane 1 the counter
#pragma unroll
            for (int q = 0; q < P::NL; ++q) in.v[q] = e == 0 ? s.v[q] : e == 1 ? c.v[q] : 0u;
            const Fz<P> st = rescue_lane_permute<P>(rescue_enter<P>(in), t, e);
            o0 = rescue_leave<P>(quad_bcast<P, 0>(st));
            o1 = rescue_leave<P>(quad_bcast<P, 1>(st));
        };
        const auto square_root = [&](const Fe<P>& a, Fe<P>& r) { return fe_sqrt_tabled<P>(a, r, root_tab); };
        Fe<P> x = fe_zero<P>(), y = fe_zero<P>();
        settled = rescue_h2c_tries<P>(seed, i_first, i_last, b_mont, sponge, square_root, x, y);
        if (!settled && !next) {  // i ran out
            settled = true;
            x = fe_zero<P>();
            y = fe_zero<P>();
            if (status && e == 0) status[k] = 2;
        }
        if (settled && e == 0) {
            fe_store<P>(out_xy + (size_t)k * 2 * W, x);
            fe_store<P>(out_xy + (size_t)k * 2 * W + W, y);
        }
    }
    if (!next) return;
    // the seeds of this wave that stay open take consecutive places of the next list: lane 0 of a quad votes, one atomic per wave
    const unsigned long long m = __ballot(!settled && e == 0);
    if (m == 0) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(next_count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (!settled && e == 0) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (at < count) next[at] = k;  // at most `open` <= count seeds stay open
    }
}

template <class C>
static int rescue_h2c_t(int curve, const plk_rescue_ctx* ctx, const void* d_seeds, uint64_t seed_start, size_t count, void* d_out_xy, void* d_status,
                        hipStream_t stream) {
    using P = typename C::FP;
    static const bool naive = getenv("PLK_H2C_NAIVE") != nullptr;
    const uint32_t n = (uint32_t)count, blocks = (uint32_t)(((uint64_t)n + RESCUE_H2C_SEEDS - 1) / RESCUE_H2C_SEEDS), b = curve_b(curve);
    const int rounds = naive ? 0 : h2c_rounds(count);
    const RescueTables t = rescue_tables(ctx);
    ScratchSet ss(stream);
    uint4* tab = (uint4*)ss.get((size_t)P::TWO_ADICITY * P::NL * 4);
    uint32_t* lists = naive ? nullptr : (uint32_t*)ss.get((size_t)2 * n * 4);  // the lists of the even and of the odd rounds
    uint32_t* counts = naive ? nullptr : (uint32_t*)ss.get((size_t)rounds * 4);  // counts[r]: seeds open after round r
    if (!tab || (!naive && (!lists || !counts))) return PLK_ERR_OOM;
    if (d_status) PLK_HIP_TRY(hipMemsetAsync(d_status, 0, count, stream));
    if (counts) PLK_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)rounds * 4, stream));
    k_h2c_root_table<P><<<1, 1, 0, stream>>>(tab);
    const uint32_t* list = nullptr;
    const uint32_t* open = nullptr;
    for (int r = 0; r < rounds; ++r) {
        uint32_t* next = lists + (size_t)(r & 1) * n;
        k_rescue_h2c_tries<P><<<blocks, RESCUE_H2C_LANES, 0, stream>>>((const uint4*)d_seeds, seed_start, n, b, tab, list, open, r, r, next, counts + r,
                                                                       (uint4*)d_out_xy, (uint8_t*)d_status, t);
        list = next;
        open = counts + r;
    }
    if (rounds < H2C_TRIES)
        k_rescue_h2c_tries<P><<<blocks, RESCUE_H2C_LANES, 0, stream>>>((const uint4*)d_seeds, seed_start, n, b, tab, list, open, rounds, H2C_TRIES - 1, nullptr,
                                                                       nullptr, (uint4*)d_out_xy, (uint8_t*)d_status, t);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

// the refusals every entry shares: nothing is launched or copied before they pass
int rescue_h2c_check(size_t count, const plk_rescue_ctx* ctx, int curve) {
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    int base_field = -1;
    PLK_TRY(or_bad_curve(with_curve(curve, [&](auto t) {
        base_field = tag_t<decltype(t)>::FP::FIELD_ID;
        return (int)PLK_OK;
    }), curve));
    if (ctx->field != base_field)
        return set_error(PLK_ERR_INVALID_ARG, "the context's field is %d, the base field of curve %d is %d", ctx->field, curve, base_field);
    PLK_TRY(rescue_on_ctx_device(ctx));
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call hashes at most 2^32 - 1 seeds", count);
    return PLK_OK;
}

// d_seeds == nullptr with field_seeds == 0: the integers seed_start + k.  d_status (nullable): one byte per seed, 0 ok, 2 i ran out;
// such a seed's coordinates are zero.
int rescue_h2c_dev_impl(size_t count, const plk_rescue_ctx* ctx, int curve, int field_seeds, const void* d_seeds, uint64_t seed_start, void* d_out_xy,
                        void* d_status, hipStream_t stream) {
    PLK_TRY(rescue_h2c_check(count, ctx, curve));
    if (count == 0) return PLK_OK;
    if (!d_out_xy || (field_seeds && !d_seeds)) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    return or_bad_curve(with_curve(curve, [&](auto t) {
        return rescue_h2c_t<tag_t<decltype(t)>>(curve, ctx, field_seeds ? d_seeds : nullptr, seed_start, count, d_out_xy, d_status, stream);
    }), curve);
}

}  // namespace plk
