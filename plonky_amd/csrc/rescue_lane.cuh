// rescue_lane.cuh -- the Rescue context and the permutation as a quad of lanes walks it: what the kernels of rescue.hip and of
// rescue_h2c.hip share.  Device code (the round itself is rescue_step.cuh, which the host replays).
#pragma once
#include "common.h"
#include "ecz_coop.cuh"
#include "rescue_step.cuh"

struct plk_rescue_ctx {
    int field = -1;
    int device = -1;         // the physical device the tables live on
    size_t width = 0, rounds = 0;
    int windows = 0;         // 4-bit digits of the exponent of 1 / alpha
    void* d_buf = nullptr;   // mds | constants | exponent | (the constants as they came: read by the setup kernel only)
    const uint32_t* d_mds = nullptr;
    const uint32_t* d_consts = nullptr;
    const uint32_t* d_exp = nullptr;
    const void* d_consts_r = nullptr;  // the constants as they came (R-form): the gates' constant columns (gate_trace.hip)
};

namespace plk {

struct RescueTables {
    const uint32_t* mds;     // W x W entries, row-major, table form (rescue_step.cuh)
    const uint32_t* consts;  // rounds x 2 x W constants, step A then step B per round, table form
    const uint32_t* exp;     // NL words: the exponent of 1 / alpha
    int windows;
    uint32_t rounds;
};

// row e of the matrix over the quad's four elements (y: this lane's), plus the constant
template <class P> PLK_DI Fz<P> rescue_lane_row(const Fz<P>& y, const uint32_t* __restrict__ mrow, const uint32_t* __restrict__ k) {
    const Fz<P> x[RESCUE_WIDTH] = {quad_bcast<P, 0>(y), quad_bcast<P, 1>(y), quad_bcast<P, 2>(y), quad_bcast<P, 3>(y)};
    return rescue_mds_row<P>(x, mrow, k);
}

// the permutation of the quad's state; x: element e of it, lazy R'-form
template <class P> PLK_DI Fz<P> rescue_lane_permute(Fz<P> x, const RescueTables& t, int e) {
    constexpr int NZ = FzCfg<P>::NZ;
    const uint32_t* mrow = t.mds + e * RESCUE_WIDTH * NZ;
#pragma unroll 1
    for (uint32_t r = 0; r < t.rounds; ++r) {
        const uint32_t* k = t.consts + ((size_t)r * 2 * RESCUE_WIDTH + e) * NZ;
        x = rescue_lane_row<P>(rescue_pow<P>(x, t.exp, t.windows), mrow, k);
        x = rescue_lane_row<P>(rescue_pow_alpha<P>(x), mrow, k + RESCUE_WIDTH * NZ);
    }
    return x;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline int rescue_on_ctx_device(const plk_rescue_ctx* ctx) {
    PLK_TRY(ensure_device());
    int dev = -1;
    PLK_HIP_TRY(hipGetDevice(&dev));
    if (dev != ctx->device) return set_error(PLK_ERR_INVALID_ARG, "the context lives on device %d, the calling thread works on device %d", ctx->device, dev);
    return PLK_OK;
}
inline RescueTables rescue_tables(const plk_rescue_ctx* ctx) { return RescueTables{ctx->d_mds, ctx->d_consts, ctx->d_exp, ctx->windows, (uint32_t)ctx->rounds}; }

}  // namespace plk
