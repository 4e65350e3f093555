// sigma.hip -- the copy-constraint permutation on the device: WirePartitions::to_sigma (partition.rs:108-136) and sigma_polynomials
// (plonk_util.rs:264-280), the one step of CircuitBuilder::build (circuit_builder.rs:1107-1108, 1149) between the union-find and the
// transforms of S_sigma.
//
// The reference asks, wire by wire, for the wire's partition (a hash lookup), scans the partition for the wire and takes the next
// member; then maps every sigma entry x to k_(x / n) g^(x % n) with one exponentiation each.  Here the partitions arrive flattened
// (members / offsets, sigma_step.cuh) and the loop is turned inside out: a lane is a SLOT of members, so a wire's position in its
// partition is where the lane stands and no partition is ever scanned - a partition of 2^19 members is 2^19 lanes like any other
// 2^19 slots.  g^(x % n) is one product of two entries of the circuit-size tables the permutation argument already caches
// (plonk.hip: the powers of the 8n-th root at index 8 r), k_j one more.
//   k_sigma_slots  per slot: the partition (bisection over offsets, narrowed to the partitions the workgroup's slots touch and, when
//                  those fit, run on a copy of their offsets in LDS), the neighbour, sigma[id] and s_sigma[id]; counts the listings
//                  of routed wires, the non-routed wires in company and the ids out of range, one atomic per workgroup and word
//   k_sigma_unset  the sigma entries no slot wrote, twice (sigma_status0)
// The union-find that orders the members of a partition (partition.rs:38-52) stays on the host: c_s_sigmas depend on that order.
#include <algorithm>

#include "common.h"
#include "fp.cuh"
#include "tables.cuh"
#include "lz.cuh"
#include "sigma_step.cuh"

namespace plk {

struct SigmaShifts {
    uint32_t w[SIGMA_ROUTED][8];  // k_is[0..5], the reference's stored form (get_subgroup_shift, partition.rs:140-153: an input)
};

template <class F>
__global__ void __launch_bounds__(SIGMA_LANES) k_sigma_slots(const uint32_t* __restrict__ members, const uint32_t* __restrict__ offsets, uint32_t num_partitions,
                                                             uint32_t num_members, unsigned log_n, SigmaShifts shifts, const uint4* __restrict__ xs_lo,
                                                             const uint4* __restrict__ xs_hi, uint32_t* __restrict__ sigma, uint4* __restrict__ s_sigma,
                                                             uint32_t* __restrict__ status) {
    static_assert(F::NL == 8, "256-bit scalar fields");
    constexpr uint32_t STAGED = SIGMA_LANES + 2;  // offsets of up to SIGMA_LANES + 1 partitions and the end of the last
    __shared__ uint32_t s_off[STAGED];
    __shared__ uint32_t s_q[2];
    __shared__ uint32_t s_cnt[3];
    __shared__ uint32_t s_k[SIGMA_ROUTED][8];
    const uint32_t p0 = blockIdx.x * SIGMA_LANES, p = p0 + threadIdx.x;  // num_members <= 2^31: no wrap
    const uint32_t p_last = p0 + SIGMA_LANES - 1 < num_members ? p0 + SIGMA_LANES - 1 : num_members - 1;
    if (threadIdx.x < 2) s_q[threadIdx.x] = sigma_find([&](uint32_t q) { return offsets[q]; }, 0u, num_partitions - 1, threadIdx.x ? p_last : p0);
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < SIGMA_ROUTED * 8) s_k[threadIdx.x / 8][threadIdx.x % 8] = shifts.w[threadIdx.x / 8][threadIdx.x % 8];
    __syncthreads();
    const uint32_t q0 = s_q[0], q1 = s_q[1] > q0 ? s_q[1] : q0, span = q1 - q0 + 1;  // q1 >= q0 with non-decreasing offsets
    const bool staged = span + 1 <= STAGED;
    if (staged)
        for (uint32_t k = threadIdx.x; k <= span; k += SIGMA_LANES) s_off[k] = offsets[q0 + k];  // q0 + span = q1 + 1 <= num_partitions
    __syncthreads();
    bool listing = false, lonely = false, out_of_range = false;
    if (p < num_members) {
        uint32_t begin, end;
        if (staged) {
            const uint32_t k = sigma_find([&](uint32_t q) { return s_off[q]; }, 0u, span - 1, p);
            begin = s_off[k];
            end = s_off[k + 1];
        } else {
            const uint32_t q = sigma_find([&](uint32_t q_) { return offsets[q_]; }, q0, q1, p);
            begin = offsets[q];
            end = offsets[q + 1];
        }
        const uint32_t id = members[p], x = members[sigma_neighbour(p, begin, end, num_members)];
        const SigmaSlot s = sigma_classify(id, x, end - begin, log_n);
        listing = s.routed;
        lonely = s.lonely;
        out_of_range = s.out_of_range;
        if (s.routed && sigma) sigma[id] = s.sigma;
        if (s.value && s_sigma) {
            const Fe<F> g = plonk_x<F>(xs_lo, xs_hi, (size_t)sigma_gate(x, log_n) << 3);  // g_n^r = g_8n^(8 r)
            Fe<F> k;
            const uint32_t j = sigma_input(x, log_n);  // below 6
#pragma unroll
            for (int i = 0; i < 8; ++i) k.v[i] = s_k[j][i];
            fe_store<F>(s_sigma + (size_t)id * 2, fe_mul<F>(k, g));
        }
    }
    if (!status) return;  // uniform
    const unsigned long long m0 = __ballot(listing), m1 = __ballot(lonely), m2 = __ballot(out_of_range);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(&s_cnt[0], (uint32_t)__popcll(m0));
        if (m1) atomicAdd(&s_cnt[1], (uint32_t)__popcll(m1));
        if (m2) atomicAdd(&s_cnt[2], (uint32_t)__popcll(m2));
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(status + threadIdx.x, s_cnt[threadIdx.x]);
}

// status[0] += 2 * #{i < count : sigma[i] == SIGMA_UNSET}
__global__ void __launch_bounds__(SIGMA_LANES) k_sigma_unset(const uint32_t* __restrict__ sigma, uint32_t count, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t c = 0;
    for (size_t i = (size_t)blockIdx.x * SIGMA_LANES + threadIdx.x; i < count; i += (size_t)gridDim.x * SIGMA_LANES) c += sigma[i] == SIGMA_UNSET;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(status, 2u * s_cnt);
}

template <class F>
static int sigma_t(unsigned log_degree, const void* d_members, const void* d_offsets, uint32_t num_partitions, uint32_t num_members, const SigmaShifts& shifts,
                   void* d_sigma, void* d_s_sigma, void* d_status, hipStream_t stream) {
    const uint32_t n6 = SIGMA_ROUTED << log_degree;
    const void *xs_lo = nullptr, *xs_hi = nullptr;
    std::shared_ptr<const void> hold;  // the tables stay alive until the launch below is enqueued (a hipFree waits for the device)
    if (d_s_sigma) PLK_TRY(plonk_domain_powers(F::FIELD_ID, log_degree, stream, &xs_lo, &xs_hi, &hold));
    ScratchSet ss(stream);
    uint32_t* marks = (uint32_t*)d_sigma;  // the status needs every wire's "written" mark: sigma itself, or a stand-in
    if (d_status && !marks) {
        marks = (uint32_t*)ss.get((size_t)n6 * 4);
        if (!marks) return PLK_ERR_OOM;
    }
    hipError_t e = hipSuccess;
    if (d_status) {
        e = hipMemsetD32Async((hipDeviceptr_t)d_status, 0, 3, stream);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)d_status, (int)(0u - n6), 1, stream);  // sigma_status0
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)marks, (int)SIGMA_UNSET, n6, stream);
    }
    if (e == hipSuccess) {
        if (num_members)
            k_sigma_slots<F><<<(num_members + SIGMA_LANES - 1) / SIGMA_LANES, SIGMA_LANES, 0, stream>>>(
                (const uint32_t*)d_members, (const uint32_t*)d_offsets, num_partitions, num_members, log_degree, shifts, (const uint4*)xs_lo, (const uint4*)xs_hi, marks,
                (uint4*)d_s_sigma, (uint32_t*)d_status);
        if (d_status) k_sigma_unset<<<std::min((n6 + SIGMA_LANES - 1) / SIGMA_LANES, 4096u), SIGMA_LANES, 0, stream>>>(marks, n6, (uint32_t*)d_status);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "sigma launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

// the refusals both entries share: nothing is launched or copied before they pass
int plonk_sigma_check(unsigned log_degree, int field, size_t num_partitions, size_t num_members, const uint64_t* k_is) {
    PLK_TRY(or_invalid(with_field4(field, [](auto) { return (int)PLK_OK; }), "field %d is not a circuit scalar field", field));
    if (!k_is) return set_error(PLK_ERR_INVALID_ARG, "null k_is");
    if (log_degree > 27) return set_error(PLK_ERR_INVALID_ARG, "log_degree %u: sigma takes log_degree <= 27", log_degree);
    if (num_partitions > ((size_t)1 << 31) || num_members > ((size_t)1 << 31))
        return set_error(PLK_ERR_INVALID_ARG, "%zu partitions, %zu members: at most 2^31 of either", num_partitions, num_members);
    if (num_members && !num_partitions) return set_error(PLK_ERR_INVALID_ARG, "%zu members in no partition", num_members);
    return PLK_OK;
}

int plonk_sigma_dev_impl(unsigned log_degree, int field, const void* d_members, const void* d_offsets, size_t num_partitions, size_t num_members, const uint64_t* k_is,
                         void* d_sigma, void* d_s_sigma, void* d_status, hipStream_t stream) {
    PLK_TRY(plonk_sigma_check(log_degree, field, num_partitions, num_members, k_is));
    if (!d_offsets || (num_members && !d_members)) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    if (!d_sigma && !d_s_sigma) return set_error(PLK_ERR_INVALID_ARG, "neither d_sigma nor d_s_sigma is given");
    PLK_TRY(ensure_device());
    SigmaShifts shifts;
    for (uint32_t j = 0; j < SIGMA_ROUTED; ++j) limbs_to_words(shifts.w[j], k_is + 4 * j);
    return or_invalid(with_field4(field,
                                  [&](auto t) {
                                      return sigma_t<tag_t<decltype(t)>>(log_degree, d_members, d_offsets, (uint32_t)num_partitions, (uint32_t)num_members, shifts, d_sigma,
                                                                         d_s_sigma, d_status, stream);
                                  }),
                      "field %d is not a circuit scalar field", field);
}

}  // namespace plk
