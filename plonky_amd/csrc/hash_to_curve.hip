// hash_to_curve.hip -- the reference's BLAKE3 hash to the curve on the device: the Pedersen generators of a circuit.
//
// Reference path                                                            here
//   blake_field(iter, seed)                 hash_to_curve.rs:13-51      ->  h2c_step.cuh (h2c_blake_field), k_blake_field
//   blake_hash_base_field_to_curve(seed)    hash_to_curve.rs:57-76      ->  k_h2c_tries
//   blake_hash_usize_to_curve(seed)         hash_to_curve.rs:53-55      ->  the same with seed = seed_start + k (its canonical words
//                                                                           ARE the integer: no field arithmetic on the seed)
//   Field::square_root                      field.rs:440-472            ->  fe_sqrt.cuh, with the table of ROOT_2ADIC^(2^m)
//
// A curve try (one blake_field, one square root) succeeds with probability ~1/2, so a seed needs 2 tries on average with a geometric
// tail.  One lane per seed looping until it succeeds makes a wave wait for its unluckiest lane.  Instead the tries run in ROUNDS over
// a compacted work list: round r takes the seeds still open, runs try i = r, writes the point on success and appends the seed to the
// next round's list otherwise (one atomic per wave; every count stays on the device, the host reads nothing back).  The list halves
// every round.  After bit_length(count) + 2 rounds the expected number of open seeds is below one; a last launch loops whatever is
// left through the tries up to H2C_TRIES - 1, one lane per seed.  Every loop is bounded: a seed that runs out of i or of j gets a
// status byte and zero coordinates, never a spin.  PLK_H2C_NAIVE=1 runs the loop form alone from try 0 (the A/B of DESIGN.md).
// The order of a list depends on the order the waves arrive in; a point is written at its seed's index, so the output does not.
#include "common.h"
#include "ec.cuh"
#include "fe_sqrt.cuh"
#include "h2c_step.cuh"

namespace plk {

constexpr int H2C_LANES = 64;  // one wave per workgroup: the compaction is wave-wide, and short lists spread over the CUs

template <class P> PLK_DI Fe<P> h2c_words_to_fe(const uint32_t (&w)[P::NL]) {
    Fe<P> r;
#pragma unroll
    for (int k = 0; k < P::NL; ++k) r.v[k] = w[k];
    return r;
}

// Tries i_first ..= i_last of the seeds of a list (list == nullptr: the seeds 0 .. count-1 themselves).  open_count (nullable) holds
// the length of the list.  A seed none of the tries settles goes to next[] when there is one and gets status 2 otherwise.
// seeds == nullptr: seed k is the integer seed_start + k; else L limbs in Montgomery form.
template <class P>
__global__ void __launch_bounds__(H2C_LANES) k_h2c_tries(const uint4* __restrict__ seeds, uint64_t seed_start, uint32_t count, uint32_t b_coeff,
                                                         const uint4* __restrict__ root_tab, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ open_count, int i_first, int i_last, uint32_t* __restrict__ next,
                                                         uint32_t* __restrict__ next_count, uint4* __restrict__ out_xy, uint8_t* __restrict__ status) {
    constexpr int W = P::NL / 4;
    const uint32_t g = blockIdx.x * H2C_LANES + threadIdx.x;
    uint32_t open = count;
    if (open_count) open = min(*open_count, count);
    const bool active = g < open;
    uint32_t k = 0;
    bool settled = true;
    if (active) {
        k = list ? list[g] : g;
        settled = k >= count;  // never with a sound list: such an entry is dropped, not followed
    }
    if (!settled) {
        uint32_t seed[P::NL];
        if (seeds) {
            const Fe<P> c = fe_to_canonical<P>(fe_load<P>(seeds + (size_t)k * W));
#pragma unroll
            for (int q = 0; q < P::NL; ++q) seed[q] = c.v[q];
        } else {
            const uint64_t s = seed_start + k;
#pragma unroll
            for (int q = 0; q < P::NL; ++q) seed[q] = q == 0 ? (uint32_t)s : q == 1 ? (uint32_t)(s >> 32) : 0u;
        }
        Fe<P> bc = fe_zero<P>();
        bc.v[0] = b_coeff;
        const Fe<P> b_mont = fe_from_canonical<P>(bc);
        uint8_t st = 0;
        Fe<P> x = fe_zero<P>(), y = fe_zero<P>();
        for (int i = i_first; i <= i_last; ++i) {
            uint32_t xc[P::NL], y_neg = 0, j = 0;
            if (!h2c_blake_field<P>(seed, (uint32_t)i, xc, y_neg, j)) {
                st = 1;  // j ran out
                break;
            }
            x = fe_from_canonical<P>(h2c_words_to_fe<P>(xc));
            const Fe<P> rhs = fe_add<P>(fe_mul<P>(fe_sqr<P>(x), x), b_mont);  // x^3 + A x + B, A = 0 on every in-scope curve
            Fe<P> r;
            if (fe_sqrt_tabled<P>(rhs, r, root_tab)) {
                y = y_neg ? fe_neg<P>(r) : r;
                settled = true;
                break;
            }
        }
        if (!settled && !next) st = st ? st : 2;  // i ran out
        if (st) {
            settled = true;
            x = fe_zero<P>();
            y = fe_zero<P>();
            if (status) status[k] = st;
        }
        if (settled) {
            fe_store<P>(out_xy + (size_t)k * 2 * W, x);
            fe_store<P>(out_xy + (size_t)k * 2 * W + W, y);
        }
    }
    if (!next) return;
    // the seeds of this wave that stay open take consecutive places of the next list: one atomic per wave
    const unsigned long long m = __ballot(!settled);
    if (m == 0) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(next_count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (!settled) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (at < count) next[at] = k;  // at most `open` <= count seeds stay open
    }
}

template <class C>
static int hash_to_curve_t(int curve, const void* d_seeds, uint64_t seed_start, size_t count, void* d_out_xy, void* d_status, hipStream_t stream) {
    using P = typename C::FP;
    static const bool naive = getenv("PLK_H2C_NAIVE") != nullptr;
    const uint32_t n = (uint32_t)count, blocks = (n + H2C_LANES - 1) / H2C_LANES, b = curve_b(curve);
    const int rounds = naive ? 0 : h2c_rounds(count);
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
        k_h2c_tries<P><<<blocks, H2C_LANES, 0, stream>>>((const uint4*)d_seeds, seed_start, n, b, tab, list, open, r, r, next, counts + r, (uint4*)d_out_xy,
                                                         (uint8_t*)d_status);
        list = next;
        open = counts + r;
    }
    if (rounds < H2C_TRIES)
        k_h2c_tries<P><<<blocks, H2C_LANES, 0, stream>>>((const uint4*)d_seeds, seed_start, n, b, tab, list, open, rounds, H2C_TRIES - 1, nullptr, nullptr,
                                                         (uint4*)d_out_xy, (uint8_t*)d_status);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

// the refusals every entry shares: nothing is launched or copied before they pass
int hash_to_curve_check(int curve, size_t count) {
    PLK_TRY(or_bad_curve(with_curve(curve, [](auto) { return (int)PLK_OK; }), curve));
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call hashes at most 2^32 - 1 seeds", count);
    return PLK_OK;
}

// d_seeds == nullptr with field_seeds == 0: the integers seed_start + k.  d_status (nullable): one byte per seed, 0 ok, 1 j ran out,
// 2 i ran out; such a seed's coordinates are zero.
int hash_to_curve_dev_impl(int curve, int field_seeds, const void* d_seeds, uint64_t seed_start, size_t count, void* d_out_xy, void* d_status,
                           hipStream_t stream) {
    PLK_TRY(hash_to_curve_check(curve, count));
    if (count == 0) return PLK_OK;
    if (!d_out_xy || (field_seeds && !d_seeds)) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    return or_bad_curve(with_curve(curve, [&](auto t) {
        return hash_to_curve_t<tag_t<decltype(t)>>(curve, field_seeds ? d_seeds : nullptr, seed_start, count, d_out_xy, d_status, stream);
    }), curve);
}

// blake_field(iters[k], seeds[k]): seeds and x in Montgomery form; status[k] = 1 when j ran out (x = 0 then)
template <class P>
__global__ void __launch_bounds__(H2C_LANES) k_blake_field(const uint8_t* __restrict__ iters, const uint4* __restrict__ seeds, uint32_t count, uint4* __restrict__ out_x,
                                                           uint8_t* __restrict__ out_y_neg, uint8_t* __restrict__ status) {
    constexpr int W = P::NL / 4;
    const uint32_t k = blockIdx.x * H2C_LANES + threadIdx.x;
    if (k >= count) return;
    const Fe<P> c = fe_to_canonical<P>(fe_load<P>(seeds + (size_t)k * W));
    uint32_t seed[P::NL], xc[P::NL], y_neg = 0, j = 0;
#pragma unroll
    for (int q = 0; q < P::NL; ++q) seed[q] = c.v[q];
    const bool ok = h2c_blake_field<P>(seed, iters[k], xc, y_neg, j);
    fe_store<P>(out_x + (size_t)k * W, ok ? fe_from_canonical<P>(h2c_words_to_fe<P>(xc)) : fe_zero<P>());
    out_y_neg[k] = ok ? (uint8_t)y_neg : 0;
    status[k] = ok ? 0 : 1;
}

int blake_field_check(int field, size_t count) {
    PLK_TRY(or_bad_field(with_field(field, [](auto) { return (int)PLK_OK; }), field));
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call hashes at most 2^32 - 1 seeds", count);
    return PLK_OK;
}

int blake_field_dev_impl(int field, const void* d_iters, const void* d_seeds, size_t count, void* d_out_x, void* d_out_y_neg, void* d_status, hipStream_t stream) {
    PLK_TRY(blake_field_check(field, count));
    if (count == 0) return PLK_OK;
    if (!d_iters || !d_seeds || !d_out_x || !d_out_y_neg || !d_status) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    PLK_TRY(or_bad_field(with_field(field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        k_blake_field<P><<<(unsigned)((count + H2C_LANES - 1) / H2C_LANES), H2C_LANES, 0, stream>>>((const uint8_t*)d_iters, (const uint4*)d_seeds, (uint32_t)count,
                                                                                                 (uint4*)d_out_x, (uint8_t*)d_out_y_neg, (uint8_t*)d_status);
        return (int)PLK_OK;
    }), field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
