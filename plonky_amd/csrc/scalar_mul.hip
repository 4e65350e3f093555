// scalar_mul.hip -- n points times n scalars, one product per element, and the Halo endomorphism:
//   CurveScalar * ProjectivePoint   curve_multiplication.rs:5-85   ->  k_scalar_mul     out_i = [s_i] P_i
//   halo_n                          plonk_util.rs:50-75            ->  k_halo_n         n(s_i) = a ZETA_SCALAR + b
//   halo_n_mul                      plonk_util.rs:79-110           ->  k_halo_n_mul     out_i = [n(s_i)] P_i by Algorithm 1
// (the fold kernels share their scalars over all outputs and the MSM sums its products: neither returns n points for n scalars).
//
// One lane per element, lazy 29-bit-limb arithmetic and the complete group law of ecz.cuh; the steps are in scalar_mul_step.cuh.
// Every lane of a wave carries its own scalar, so every chain has a FIXED number of steps and a lane picks its addend by value
// (selects on the limbs); the only per-lane predicate is "this column adds nothing", which masks the one addition of the step.
//   * k_halo_n_mul: security_bits / 2 steps Acc = 2 Acc + S, S = (x or ZETA x, y or -y): no table, no scalar arithmetic.
//   * k_scalar_mul on the four curves with the endomorphism: the scalar is split (glv.cuh) into two halves below 2^GLV_BITS and the
//     halves are walked jointly, GLV_BITS steps of one doubling and at most one mixed addition of P, phi P or P +- phi P.
//     P + phi P = (beta^2 x, -y) is free; P - phi P is a real addition, made affine with the element's share of ONE batched
//     inversion (k_scalar_mul_prep writes the denominators (beta - 1) x, field_batch_inverse_dev_impl inverts them).
//   * k_scalar_mul on BLS12-377 (no endomorphism, even cofactor: no s -> r - s): carry-based signed base-4 digits of the 253-bit
//     integer over the table {P, 2P}: 128 steps of two doublings and one addition per non-zero digit; 2P is affine through the same batched
//     inversion (denominators 2y).  The table is two affine points per lane, in registers and picked by selects;
//     the one run-time index of these kernels is the word of the scalar (halves, digits) a step reads its bits from.
// The chains end in (X ZZZ : Y ZZ : ZZ ZZZ) and k_batch_to_affine (fieldops.hip) normalises them with its shared inversions: the
// result is the unique affine point, (0, 0) and the flag for the identity.
#include "common.h"
#include "ec.cuh"
#include "ecz.cuh"
#include "scalar_mul_step.cuh"

namespace plk {

constexpr int SM_LANES = 64;  // workgroups of one wave (fold.hip: waves of larger groups were seen to share SIMDs while others idle)

// den_i = (beta - 1) x_i (endomorphism curves) or 2 y_i (BLS12-377), R-form; a zero is taken care of by the batched inversion
template <class C> __global__ void __launch_bounds__(SM_LANES) k_scalar_mul_prep(const uint4* __restrict__ p_xy, uint32_t n_points, uint4* __restrict__ den) {
    using FP = typename C::FP;
    constexpr int W = FP::NL / 4;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_points) return;
    fe_store<FP>(den + (size_t)i * W, sm_table_den<C>(fe_load<FP>(p_xy + (size_t)i * 2 * W), fe_load<FP>(p_xy + (size_t)i * 2 * W + W)));
}

template <class C>
__global__ void __launch_bounds__(SM_LANES) k_scalar_mul(uint32_t count, const uint4* __restrict__ scalars, uint32_t n_scalars, const uint4* p_xy,
                                                         const uint8_t* p_zero, uint32_t n_points, const uint4* __restrict__ inv,
                                                         uint4* __restrict__ out_xyz, uint8_t* __restrict__ out_zero) {
    using FP = typename C::FP;
    using SP = typename C::SP;
    constexpr int W = FP::NL / 4, WS = SP::NL / 4;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t si = n_scalars == 1 ? 0 : i, pi = n_points == 1 ? 0 : i;
    const Fe<SP> s = fe_to_canonical<SP>(fe_load<SP>(scalars + (size_t)si * WS));
    const Fe<FP> px = fe_load<FP>(p_xy + (size_t)pi * 2 * W), py = fe_load<FP>(p_xy + (size_t)pi * 2 * W + W);
    const Fe<FP> iv = fe_load<FP>(inv + (size_t)pi * W);
    const bool ident = p_zero ? p_zero[pi] != 0 : false;
    XyzzZ<FP> acc = xyzzz_identity<FP>();
    if (!ident) acc = sm_scalar_mul_chain<C>(s.v, px, py, iv);
    emit_projective<FP>(acc, out_xyz + (size_t)i * 3 * W, out_zero + i);
}

template <class C>
__global__ void __launch_bounds__(SM_LANES) k_halo_n(uint32_t count, unsigned bits, const uint4* scalars, uint4* out) {
    using SP = typename C::SP;
    constexpr int WS = SP::NL / 4;
    if constexpr (C::Glv::ENABLED) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= count) return;
        const Fe<SP> s = fe_to_canonical<SP>(fe_load<SP>(scalars + (size_t)i * WS));
        fe_store<SP>(out + (size_t)i * WS, halo_n_value<C>(s.v, bits));
    }
}

template <class C>
__global__ void __launch_bounds__(SM_LANES) k_halo_n_mul(uint32_t count, unsigned bits, const uint4* __restrict__ scalars, uint32_t n_scalars, const uint4* p_xy,
                                                         const uint8_t* p_zero, uint32_t n_points, uint4* __restrict__ out_xyz, uint8_t* __restrict__ out_zero) {
    using FP = typename C::FP;
    using SP = typename C::SP;
    constexpr int W = FP::NL / 4, WS = SP::NL / 4;
    if constexpr (C::Glv::ENABLED) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= count) return;
        const uint32_t si = n_scalars == 1 ? 0 : i, pi = n_points == 1 ? 0 : i;
        const Fe<SP> s = fe_to_canonical<SP>(fe_load<SP>(scalars + (size_t)si * WS));
        const Fe<FP> px = fe_load<FP>(p_xy + (size_t)pi * 2 * W), py = fe_load<FP>(p_xy + (size_t)pi * 2 * W + W);
        const bool ident = p_zero ? p_zero[pi] != 0 : false;
        XyzzZ<FP> acc = xyzzz_identity<FP>();
        if (!ident) acc = halo_n_mul_chain<C>(s.v, bits, px, py);
        emit_projective<FP>(acc, out_xyz + (size_t)i * 3 * W, out_zero + i);
    }
}

// ---- host side ----
static unsigned sm_blocks(size_t n) { return (unsigned)((n + SM_LANES - 1) / SM_LANES); }

int curve_scalar_mul_check(size_t count, int curve, size_t n_scalars, size_t n_points) {
    if (curve_limbs(curve) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (count >> 32) return set_error(PLK_ERR_INVALID_ARG, "count %zu: below 2^32 elements per call", count);
    if (count == 0) return PLK_OK;
    if ((n_scalars != 1 && n_scalars != count) || (n_points != 1 && n_points != count))
        return set_error(PLK_ERR_INVALID_ARG, "n_scalars %zu / n_points %zu: each is count (%zu) or 1 (broadcast)", n_scalars, n_points, count);
    return PLK_OK;
}
int halo_n_check(size_t count, int curve, unsigned security_bits) {
    if (curve_limbs(curve) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    const int has_endo = with_curve(curve, [&](auto t) { return tag_t<decltype(t)>::Glv::ENABLED ? 1 : 0; });
    if (has_endo != 1) return set_error(PLK_ERR_INVALID_ARG, "curve %d has no endomorphism: n(s) is not defined on it", curve);
    const unsigned max_bits = (unsigned)curve_scalar_bits(curve) & ~1u;
    if (security_bits == 0 || (security_bits & 1u) || security_bits > max_bits)
        return set_error(PLK_ERR_INVALID_ARG, "security_bits %u: an even number in 2 .. %u", security_bits, max_bits);
    if (count >> 32) return set_error(PLK_ERR_INVALID_ARG, "count %zu: below 2^32 elements per call", count);
    return PLK_OK;
}
int halo_n_mul_check(size_t count, int curve, unsigned security_bits, size_t n_scalars, size_t n_points) {
    PLK_TRY(halo_n_check(count, curve, security_bits));
    return curve_scalar_mul_check(count, curve, n_scalars, n_points);
}

// (X : Y : Z) of `count` chains -> the caller's affine arrays
static int sm_normalise(int curve, size_t count, const void* xyz, const void* zero, void* d_out_xy, void* d_out_zero, hipStream_t stream) {
    PLK_HIP_TRY(hipGetLastError());
    return curve_batch_to_affine_dev_impl(curve, count, xyz, zero, d_out_xy, d_out_zero, stream);
}

int curve_scalar_mul_dev_impl(size_t count, int curve, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy, const void* d_p_zero,
                              void* d_out_xy, void* d_out_zero, hipStream_t stream) {
    PLK_TRY(curve_scalar_mul_check(count, curve, n_scalars, n_points));
    if (count == 0) return PLK_OK;
    if (!d_scalars || !d_p_xy || !d_out_xy || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    return with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        constexpr size_t FE = (size_t)C::FP::NL * 4;
        ScratchSet ss(stream);
        void *inv = ss.get(n_points * FE), *xyz = ss.get(count * 3 * FE), *zero = ss.get(count);
        if (!inv || !xyz || !zero) return (int)PLK_ERR_OOM;
        k_scalar_mul_prep<C><<<sm_blocks(n_points), SM_LANES, 0, stream>>>((const uint4*)d_p_xy, (uint32_t)n_points, (uint4*)inv);
        PLK_HIP_TRY(hipGetLastError());
        PLK_TRY(field_batch_inverse_dev_impl(C::FP::FIELD_ID, inv, inv, nullptr, nullptr, n_points, stream));
        k_scalar_mul<C><<<sm_blocks(count), SM_LANES, 0, stream>>>((uint32_t)count, (const uint4*)d_scalars, (uint32_t)n_scalars, (const uint4*)d_p_xy,
                                                                   (const uint8_t*)d_p_zero, (uint32_t)n_points, (const uint4*)inv, (uint4*)xyz, (uint8_t*)zero);
        return sm_normalise(curve, count, xyz, zero, d_out_xy, d_out_zero, stream);
    });
}

int halo_n_dev_impl(size_t count, int curve, unsigned security_bits, const void* d_scalars, void* d_out, hipStream_t stream) {
    PLK_TRY(halo_n_check(count, curve, security_bits));
    if (count == 0) return PLK_OK;
    if (!d_scalars || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    return with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        k_halo_n<C><<<sm_blocks(count), SM_LANES, 0, stream>>>((uint32_t)count, security_bits, (const uint4*)d_scalars, (uint4*)d_out);
        PLK_HIP_TRY(hipGetLastError());
        return (int)PLK_OK;
    });
}

int halo_n_mul_dev_impl(size_t count, int curve, unsigned security_bits, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy,
                        const void* d_p_zero, void* d_out_xy, void* d_out_zero, hipStream_t stream) {
    PLK_TRY(halo_n_mul_check(count, curve, security_bits, n_scalars, n_points));
    if (count == 0) return PLK_OK;
    if (!d_scalars || !d_p_xy || !d_out_xy || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    return with_curve(curve, [&](auto t) {
        using C = tag_t<decltype(t)>;
        constexpr size_t FE = (size_t)C::FP::NL * 4;
        ScratchSet ss(stream);
        void *xyz = ss.get(count * 3 * FE), *zero = ss.get(count);
        if (!xyz || !zero) return (int)PLK_ERR_OOM;
        k_halo_n_mul<C><<<sm_blocks(count), SM_LANES, 0, stream>>>((uint32_t)count, security_bits, (const uint4*)d_scalars, (uint32_t)n_scalars, (const uint4*)d_p_xy,
                                                                   (const uint8_t*)d_p_zero, (uint32_t)n_points, (uint4*)xyz, (uint8_t*)zero);
        return sm_normalise(curve, count, xyz, zero, d_out_xy, d_out_zero, stream);
    });
}

}  // namespace plk
