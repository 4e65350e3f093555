// rescue.hip -- the proof system's own hash on the device: batches of Rescue permutations, sponges and k-th roots.
//
// Reference path                                                            here
//   rescue_permutation(state, security_bits)   rescue.rs:70-88          ->  k_rescue_permute (rescue_step.cuh: the round)
//   apply_mds                                  mds.rs:43-77             ->  rescue_mds_row, the entries built by k_rescue_setup
//   rescue_sponge(inputs, num_outputs, ..)     rescue.rs:40-68          ->  k_rescue_sponge
//   Field::kth_root / kth_root_u32             field.rs:340-375         ->  k_field_kth_root (rescue_kth_root_exponent: the exponent)
//   generate_rescue_constants                  rescue.rs:97-121         ->  NOT here: the caller hands the constants over
//
// One state ELEMENT per lane, one state per quad of adjacent lanes.  A round is two long product chains per element (x^(1/alpha):
// ~320 products on a 255-bit field; x^alpha: 3 or 5) and two rows of the MDS matrix.  The four chains of a state are independent and
// equally long, so the four lanes run them side by side without divergence - the exponent is the same for every lane and its digits
// steer scalar branches.  For its row a lane fetches the three other elements from its neighbours with DPP quad broadcasts
// (ecz_coop.cuh) and forms the four products under one reduction.  A state stays in the registers of its four lanes from the load to
// the store; the sponge's absorb and squeeze loops run inside the kernel, so a call is one launch however many permutations it holds.
#include "rescue_lane.cuh"

namespace plk {

constexpr int RESCUE_LANES = 256;                          // 64 states per workgroup
constexpr int RESCUE_STATES = RESCUE_LANES / RESCUE_WIDTH;

struct RescueExponent {  // the exponent of a k-th root as a kernel argument
    uint32_t w[12];
    int windows;
};

// R-form constants -> table form; the Cauchy matrix in table form (mds_tab) and / or in R-form (mds_r)
template <class P>
__global__ void __launch_bounds__(64) k_rescue_setup(const uint4* __restrict__ consts_in, uint32_t n_consts, uint32_t* __restrict__ consts_tab,
                                                     uint32_t* __restrict__ mds_tab, uint4* __restrict__ mds_r) {
    constexpr int NZ = FzCfg<P>::NZ, W4 = P::NL / 4;
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n_consts) {
        const Fz<P> v = rescue_table_form<P>(fe_load<P>(consts_in + (size_t)i * W4));
        for (int l = 0; l < NZ; ++l) consts_tab[(size_t)i * NZ + l] = v.l[l];
    } else if (i < n_consts + RESCUE_WIDTH * RESCUE_WIDTH) {
        const uint32_t e = i - n_consts;
        const Fe<P> m = rescue_mds_entry<P>(RESCUE_WIDTH, (int)(e / RESCUE_WIDTH), (int)(e % RESCUE_WIDTH));
        if (mds_r) fe_store<P>(mds_r + (size_t)e * W4, m);
        if (mds_tab) {
            const Fz<P> v = rescue_table_form<P>(m);
            for (int l = 0; l < NZ; ++l) mds_tab[(size_t)e * NZ + l] = v.l[l];
        }
    }
}

template <class P>
__global__ void __launch_bounds__(RESCUE_LANES) k_rescue_permute(const uint4* states, uint4* out,  /* may be the same buffer */ uint32_t count, RescueTables t) {
    constexpr int W4 = P::NL / 4;
    const uint32_t s = blockIdx.x * RESCUE_STATES + threadIdx.x / RESCUE_WIDTH;
    const int e = threadIdx.x % RESCUE_WIDTH;
    if (s >= count) return;  // a whole quad leaves together
    const size_t at = ((size_t)s * RESCUE_WIDTH + e) * W4;
    const Fz<P> x = rescue_lane_permute<P>(rescue_enter<P>(fe_load<P>(states + at)), t, e);
    fe_store<P>(out + at, rescue_leave<P>(x));
}

// rescue_sponge per state: lane e < 3 of a quad absorbs input 3 chunk + e and squeezes output 3 block + e.  The loop is written so
// that the permutation has one call site: step `chunks + b` emits block b, and the last block ends the loop.
template <class P>
__global__ void __launch_bounds__(RESCUE_LANES) k_rescue_sponge(const uint4* __restrict__ inputs, uint32_t n_inputs, uint4* __restrict__ out, uint32_t n_outputs,
                                                                uint32_t count, RescueTables t) {
    constexpr int W4 = P::NL / 4;
    const uint32_t s = blockIdx.x * RESCUE_STATES + threadIdx.x / RESCUE_WIDTH;
    const uint32_t e = threadIdx.x % RESCUE_WIDTH;
    if (s >= count) return;
    const uint32_t chunks = (n_inputs + RESCUE_RATE - 1) / RESCUE_RATE, blocks = (n_outputs + RESCUE_RATE - 1) / RESCUE_RATE;
    Fz<P> x = fz_zero<P>();
#pragma unroll 1
    for (uint32_t step = 0;; ++step) {
        if (step < chunks) {
            const uint32_t i = RESCUE_RATE * step + e;
            if (e < RESCUE_RATE && i < n_inputs) x = fz_add<P>(x, rescue_enter<P>(fe_load<P>(inputs + ((size_t)s * n_inputs + i) * W4)));
        } else {
            const uint32_t b = step - chunks, o = RESCUE_RATE * b + e;
            if (e < RESCUE_RATE && o < n_outputs) fe_store<P>(out + ((size_t)s * n_outputs + o) * W4, rescue_leave<P>(x));
            if (b + 1 == blocks) break;
        }
        x = rescue_lane_permute<P>(x, t, (int)e);
    }
}

// Field::kth_root: one element per lane
template <class P>
__global__ void __launch_bounds__(RESCUE_LANES) k_field_kth_root(const uint4* in, uint4* out, uint32_t count, RescueExponent d) {
    constexpr int W4 = P::NL / 4;
    const uint32_t i = blockIdx.x * RESCUE_LANES + threadIdx.x;
    if (i >= count) return;
    fe_store<P>(out + (size_t)i * W4, rescue_leave<P>(rescue_pow<P>(rescue_enter<P>(fe_load<P>(in + (size_t)i * W4)), d.w, d.windows)));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int rescue_width_check(size_t width) {
    if (width != RESCUE_WIDTH) return set_error(PLK_ERR_INVALID_ARG, "width %zu: the Rescue kernels are built for width %d (RESCUE_SPONGE_WIDTH)", width, RESCUE_WIDTH);
    return PLK_OK;
}

int rescue_rounds_impl(size_t width, size_t security_bits, size_t* rounds) {
    if (!rounds) return set_error(PLK_ERR_INVALID_ARG, "null rounds");
    if (width == 0) return set_error(PLK_ERR_INVALID_ARG, "width 0");
    *rounds = rescue_rounds(width, security_bits);
    return PLK_OK;
}

// the matrix in R-form, W x W elements, device memory
int rescue_mds_dev_impl(int field, size_t width, void* d_out, hipStream_t stream) {
    PLK_TRY(or_bad_field(with_field(field, [](auto) { return (int)PLK_OK; }), field));
    PLK_TRY(rescue_width_check(width));
    if (!d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    PLK_TRY(ensure_device());
    PLK_TRY(or_bad_field(with_field(field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        k_rescue_setup<P><<<1, 64, 0, stream>>>(nullptr, 0, nullptr, nullptr, (uint4*)d_out);
        return (int)PLK_OK;
    }), field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

int rescue_create_impl(int field, size_t width, size_t rounds, const uint64_t* constants, plk_rescue_ctx** out) {
    if (!out) return set_error(PLK_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    PLK_TRY(or_bad_field(with_field(field, [](auto) { return (int)PLK_OK; }), field));
    PLK_TRY(rescue_width_check(width));
    if (rounds == 0 || rounds > 4096) return set_error(PLK_ERR_INVALID_ARG, "rounds %zu: a context takes 1 .. 4096 rounds", rounds);
    if (!constants) return set_error(PLK_ERR_INVALID_ARG, "null constants");
    PLK_TRY(ensure_device());
    return or_bad_field(with_field(field, [&](auto tag) {
        using P = tag_t<decltype(tag)>;
        constexpr int NZ = FzCfg<P>::NZ;
        uint32_t d[P::NL];
        if (rescue_alpha<P>() == 0u || !rescue_kth_root_exponent<P>(rescue_alpha<P>(), d))
            return set_error(PLK_ERR_INVALID_ARG, "field %d has no permuting alpha", field);
        std::unique_ptr<plk_rescue_ctx> c(new plk_rescue_ctx());
        c->field = field;
        c->width = width;
        c->rounds = rounds;
        c->windows = rescue_windows(rescue_exponent_bits(d));
        PLK_HIP_TRY(hipGetDevice(&c->device));
        const size_t n_consts = rounds * 2 * RESCUE_WIDTH;
        const size_t mds_bytes = (size_t)RESCUE_WIDTH * RESCUE_WIDTH * NZ * 4, consts_bytes = n_consts * NZ * 4, exp_bytes = 16 * 4;
        const size_t in_off = (mds_bytes + consts_bytes + exp_bytes + 15) / 16 * 16, in_bytes = n_consts * P::NL * 4;
        PLK_HIP_TRY(hipMalloc(&c->d_buf, in_off + in_bytes));
        struct Free {  // until the context is handed over
            std::unique_ptr<plk_rescue_ctx>& c;
            ~Free() {
                if (c && c->d_buf) (void)hipFree(c->d_buf);
            }
        } guard{c};
        uint8_t* base = (uint8_t*)c->d_buf;
        c->d_mds = (const uint32_t*)base;
        c->d_consts = (const uint32_t*)(base + mds_bytes);
        c->d_exp = (const uint32_t*)(base + mds_bytes + consts_bytes);
        c->d_consts_r = base + in_off;
        hipStream_t stream = stream_pool_acquire();
        if (!stream) return (int)PLK_ERR_HIP;
        hipError_t e = hipMemcpyAsync(base + in_off, constants, in_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)c->d_exp, d, sizeof(d), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) {
            k_rescue_setup<P><<<(unsigned)((n_consts + RESCUE_WIDTH * RESCUE_WIDTH + 63) / 64), 64, 0, stream>>>(
                (const uint4*)(base + in_off), (uint32_t)n_consts, (uint32_t*)c->d_consts, (uint32_t*)c->d_mds, nullptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);  // `constants` and d are the caller's / this frame's
        stream_pool_release(stream);
        if (e != hipSuccess) return set_error(PLK_ERR_HIP, "rescue context: %s", hipGetErrorString(e));
        *out = c.release();
        return (int)PLK_OK;
    }), field);
}

int rescue_free_impl(plk_rescue_ctx* ctx) {
    if (!ctx) return PLK_OK;
    if (ctx->d_buf) (void)hipFree(ctx->d_buf);
    delete ctx;
    return PLK_OK;
}

int rescue_ctx_field(const plk_rescue_ctx* ctx) { return ctx ? ctx->field : -1; }

// the refusals the host and device entries share: nothing is launched or copied before they pass
int rescue_check(size_t count, const plk_rescue_ctx* ctx) {
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call takes at most 2^32 - 1 states", count);
    return PLK_OK;
}
int rescue_sponge_check(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, size_t n_outputs) {
    PLK_TRY(rescue_check(count, ctx));
    if (n_outputs == 0) return set_error(PLK_ERR_INVALID_ARG, "n_outputs 0: a sponge squeezes at least one element");
    if (n_inputs > 0xFFFFFFFFu || n_outputs > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "%zu inputs, %zu outputs: below 2^32 of either", n_inputs, n_outputs);
    return PLK_OK;
}

static unsigned rescue_blocks(size_t count) { return (unsigned)((count + RESCUE_STATES - 1) / RESCUE_STATES); }

int rescue_permutation_dev_impl(size_t count, const plk_rescue_ctx* ctx, const void* d_states, void* d_out, hipStream_t stream) {
    PLK_TRY(rescue_check(count, ctx));
    if (count == 0) return PLK_OK;
    if (!d_states || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(rescue_on_ctx_device(ctx));
    PLK_TRY(or_bad_field(with_field(ctx->field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        k_rescue_permute<P><<<rescue_blocks(count), RESCUE_LANES, 0, stream>>>((const uint4*)d_states, (uint4*)d_out, (uint32_t)count, rescue_tables(ctx));
        return (int)PLK_OK;
    }), ctx->field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

int rescue_sponge_dev_impl(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, const void* d_inputs, size_t n_outputs, void* d_out, hipStream_t stream) {
    PLK_TRY(rescue_sponge_check(count, ctx, n_inputs, n_outputs));
    if (count == 0) return PLK_OK;
    if ((n_inputs && !d_inputs) || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(rescue_on_ctx_device(ctx));
    PLK_TRY(or_bad_field(with_field(ctx->field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        k_rescue_sponge<P><<<rescue_blocks(count), RESCUE_LANES, 0, stream>>>((const uint4*)d_inputs, (uint32_t)n_inputs, (uint4*)d_out, (uint32_t)n_outputs,
                                                                              (uint32_t)count, rescue_tables(ctx));
        return (int)PLK_OK;
    }), ctx->field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

// the exponent of x^(1/k) on `field`; the refusals of both k-th root entries
static int field_kth_root_exponent(int field, uint32_t k, RescueExponent& d) {
    return or_bad_field(with_field(field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        static_assert(P::NL <= 12, "RescueExponent holds 12 words");
        if (k == 0) return set_error(PLK_ERR_INVALID_ARG, "k = 0 has no root");
        uint32_t w[P::NL];
        if (!rescue_kth_root_exponent<P>(k, w)) return set_error(PLK_ERR_INVALID_ARG, "x^%u does not permute field %d: gcd(k, p - 1) != 1", k, field);
        for (int i = 0; i < 12; ++i) d.w[i] = i < P::NL ? w[i] : 0u;
        d.windows = rescue_windows(rescue_exponent_bits(w));
        return (int)PLK_OK;
    }), field);
}
int field_kth_root_check(size_t count, int field, uint32_t k) {
    RescueExponent d;
    PLK_TRY(field_kth_root_exponent(field, k, d));
    if (count > 0xFFFFFFFFu) return set_error(PLK_ERR_INVALID_ARG, "count %zu: a call takes at most 2^32 - 1 elements", count);
    return PLK_OK;
}

int field_kth_root_dev_impl(size_t count, int field, uint32_t k, const void* d_in, void* d_out, hipStream_t stream) {
    PLK_TRY(field_kth_root_check(count, field, k));
    if (count == 0) return PLK_OK;
    if (!d_in || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    RescueExponent d;
    PLK_TRY(field_kth_root_exponent(field, k, d));
    PLK_TRY(or_bad_field(with_field(field, [&](auto t) {
        using P = tag_t<decltype(t)>;
        k_field_kth_root<P><<<(unsigned)((count + RESCUE_LANES - 1) / RESCUE_LANES), RESCUE_LANES, 0, stream>>>((const uint4*)d_in, (uint4*)d_out, (uint32_t)count, d);
        return (int)PLK_OK;
    }), field));
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
