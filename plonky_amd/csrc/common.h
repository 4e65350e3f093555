// common.h -- host-side plumbing shared by the translation units of libplonky_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/plonky_hip.h"
#include "../../include/plonky_hip_trace.h"
#include "../../include/plonky_hip_witness.h"
#include "dispatch.cuh"
#include "host_only.h"
#include "table_cache.h"

struct plk_msm_ctx;
struct plk_halo_ctx;

namespace plk {

// Every function one translation unit defines and another calls is declared ONCE, here or in a header this one includes, and the
// defining unit sees that declaration too: a return type or a default argument that diverges does not compile
// (tests/test_capi_symbols.py keeps prototypes out of the .hip / .cpp files).

// thread-local error text behind plk_last_error() (host_runtime.hip)
std::string& last_error_ref();
int set_error(int code, const char* fmt, ...);

#define PLK_HIP_TRY(expr)                                                                              \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return ::plk::set_error(_e == hipErrorOutOfMemory ? PLK_ERR_OOM : PLK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                                    hipGetErrorString(_e), __FILE__, __LINE__);                        \
    } while (0)

#define PLK_TRY(expr)              \
    do {                           \
        int _rc = (expr);          \
        if (_rc != PLK_OK) return _rc; \
    } while (0)

// what with_field / with_curve (dispatch.cuh, ec.cuh) return for an id outside their list, as the call site's PLK_ERR_INVALID_ARG text
// (fmt takes the id); any other rc passes
inline int or_invalid(int rc, const char* fmt, int id) { return rc == PLK_NO_MATCH ? set_error(PLK_ERR_INVALID_ARG, fmt, id) : rc; }
inline int or_bad_field(int rc, int field) { return or_invalid(rc, "bad field id %d", field); }
inline int or_bad_curve(int rc, int curve) { return or_invalid(rc, "bad curve id %d", curve); }

// n 64-bit limbs (the C ABI's form of a field element) as 2n 32-bit words (the kernels' form), little-endian
inline void limbs_to_words(uint32_t* words, const uint64_t* limbs, int n = 4) {
    for (int k = 0; k < n; ++k) {
        words[2 * k] = (uint32_t)limbs[k];
        words[2 * k + 1] = (uint32_t)(limbs[k] >> 32);
    }
}

// Makes sure the calling thread's device is selected (plk_init may have been called on another thread: hipSetDevice is per
// thread): the physical device of the thread's logical device in the group (multi.hip).
int ensure_device();

// ---- the device group (multi.hip): logical device d of the process -> physical HIP device ----
constexpr int PLK_MAX_DEVICES = 16;
int group_size();                            // logical devices in use (1 unless plk_init_devices made it more)
int group_phys(int logical);                 // physical HIP device of a logical device
int thread_logical_device();                 // the logical device the calling thread's calls run on
void set_thread_logical_device(int logical);
int next_round_robin_device();               // single-unit calls from many host threads take the devices in turn
unsigned multi_min_log_n();                  // size gate of the fan-out (PLK_MULTI_MIN_LOG_N)
struct DeviceScope {                         // the calling thread works on logical device `logical` for the scope; on exit the
    int prev;                                // thread's logical device AND its current HIP device are what they were
    int prev_hip;
    explicit DeviceScope(int logical);
    ~DeviceScope();
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
// Every public entry point (capi.hip: PLK_API) leaves the calling thread's current HIP device as it found it: the library selects
// devices freely inside a call (the thread's logical device, a context's device, the devices of a group taken in turn), and a host
// shim or torch that allocates on "the current device" afterwards must not land on another GPU.  Nested calls
// (plk_ntt -> plk_ntt_batch) restore once, at the outermost level.
struct ApiGuard {
    int dev = -1;
    bool outer;
    ApiGuard();
    ~ApiGuard();
    ApiGuard(const ApiGuard&) = delete;
    ApiGuard& operator=(const ApiGuard&) = delete;
};
#define PLK_API plk::ApiGuard plk_api_guard_
int group_init_single(int device);           // plk_init
int group_init(int n_devices);               // plk_init_devices
void group_shutdown();
// fn(d) on the worker thread of every logical device d < count, side by side; returns when all have; the first failure wins
int run_on_devices(int count, const std::function<int(int)>& fn);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// RAII device buffer: the host-pointer entry points' copies and every buffer of a cached table struct (table_cache.h).  Movable, not
// copyable: a copy would free the buffer twice.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        if (p) (void)hipFree(p);
        p = nullptr;
        if (bytes == 0) bytes = 16;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return set_error(e == hipErrorOutOfMemory ? PLK_ERR_OOM : PLK_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
        return PLK_OK;
    }
};

// Stream-aware scratch buffers owned by the library (no hipMallocAsync: the stream-ordered pool
// of the runtime is left to the host framework).  A buffer is handed out again only to work that
// is ordered after its previous use: same stream, or its last-use event has completed.
void* scratch_acquire(size_t bytes, hipStream_t stream);  // nullptr on allocation failure (error text set)
void scratch_release(void* p, hipStream_t stream);       // call after the last kernel using p is enqueued
void scratch_clear();

struct ScratchSet {  // scratch buffers of one call (opening.hip, polydiv.hip), released in stream order on every exit path
    hipStream_t stream;
    std::vector<void*> bufs;
    explicit ScratchSet(hipStream_t s) : stream(s) {}
    ScratchSet(const ScratchSet&) = delete;
    ScratchSet& operator=(const ScratchSet&) = delete;
    void* get(size_t bytes) {
        void* p = scratch_acquire(bytes ? bytes : 16, stream);
        if (p) bufs.push_back(p);
        return p;
    }
    ~ScratchSet() {
        for (void* p : bufs) scratch_release(p, stream);
    }
};

// Streams of the library's own (side streams of a context, the lanes of the host-pointer entry points) come from a process-wide
// pool and go back to it instead of being destroyed: events of the scratch pool (and of other contexts) may have been recorded on
// them last, and HIP keeps a pointer to the recording stream in an event - querying or waiting on such an event after
// hipStreamDestroy was seen to fail with "operation not permitted when stream is capturing" (tools/fuzz_gpu.py, round 3).
hipStream_t stream_pool_acquire();         // a non-blocking stream of the current device; nullptr on failure (error text set)
void stream_pool_release(hipStream_t s);   // work still in flight on it simply precedes the next user's

// Optional element-wise work fused into the first pass's loads and the last pass's stores of a transform
// (poly.hip: coset scaling, zero padding, division by the vanishing polynomial).  Tables hold canonical
// R'-form words (the form of the twiddle tables, see ntt.hip).  Geometric tables: b^i = hi[i >> 10] * lo[i & 1023].
constexpr int NTT_POW_LO_LOG = 10;
struct NttHooks {
    size_t in_len = 0;            // input elements per transform actually stored; the rest reads as zero
    size_t in_stride = 0;         // distance between the inputs of a batch, in elements
    const void* in_lo = nullptr;  // x_i *= b^i on load
    const void* in_hi = nullptr;
    const void* out_tab = nullptr;  // y_i *= out_tab[i & out_mask] on store
    size_t out_mask = 0;
    const void* out_lo = nullptr;  // y_i *= b^i on store
    const void* out_hi = nullptr;
};

// ---- entry points implemented in ntt.hip / msm.hip / fieldops.hip, wrapped by capi.hip ----
int ntt_precompute_impl(int field, unsigned log_n);
int ntt_dev_impl(int field, unsigned log_n, int inverse, unsigned batch, const void* d_in, void* d_out, hipStream_t stream);
int ntt_dev_hooked_impl(int field, unsigned log_n, int inverse, unsigned batch, const void* d_in, void* d_out, const NttHooks& hooks,
                        hipStream_t stream);
// device pointer to the power table of the (cached) plan: pw[b] = w^(2^b), b < log_t, w the primitive 2^log_t-th root
// (log_t = max(log_n, 10)), R-form
// *hold (when given) shares ownership of the plan: keep it until the kernels reading pw have been enqueued AND the stream has
// been synchronised or the hold is released after them (a concurrent plk_ntt_clear_cache frees the table otherwise)
int ntt_plan_pow_table(int field, unsigned log_n, const void** pw, int* log_t, std::shared_ptr<const void>* hold = nullptr);
int ntt_reference_table_dev_impl(int field, unsigned log_n, void* d_out, hipStream_t stream);
int field_inner_product_dev_impl(int field, const void* d_a, const void* d_b, size_t count, void* d_out, hipStream_t stream);
int field_fold_slices_dev_impl(int field, const void* d_lo, const void* d_hi, const uint64_t* s_lo, const uint64_t* s_hi, size_t count, void* d_out,
                               hipStream_t stream);
int field_bytes_impl(int field, int from_bytes, const void* d_in, size_t count, void* d_out, unsigned* d_bad, hipStream_t stream);
int point_bytes_impl(int curve, int from_bytes, const void* d_in, const void* d_zero, size_t count, void* d_out, void* d_out_zero, void* d_status,
                     hipStream_t stream);
uint32_t curve_b(int curve);  // the curve constant B (A = 0 on every in-scope curve); serial.hip
// the BLAKE3 hash to the curve (hash_to_curve.hip); the checks hold the refusals the host entries share
int hash_to_curve_check(int curve, size_t count);
int hash_to_curve_dev_impl(int curve, int field_seeds, const void* d_seeds, uint64_t seed_start, size_t count, void* d_out_xy, void* d_status,
                           hipStream_t stream);
int blake_field_check(int field, size_t count);
int blake_field_dev_impl(int field, const void* d_iters, const void* d_seeds, size_t count, void* d_out_x, void* d_out_y_neg, void* d_status, hipStream_t stream);
// Rescue (rescue.hip): count first, then the context or the field id; the checks hold the refusals the host entries share
int rescue_rounds_impl(size_t width, size_t security_bits, size_t* rounds);
int rescue_mds_dev_impl(int field, size_t width, void* d_out, hipStream_t stream);
int rescue_create_impl(int field, size_t width, size_t rounds, const uint64_t* constants, plk_rescue_ctx** out);
int rescue_free_impl(plk_rescue_ctx* ctx);
int rescue_ctx_field(const plk_rescue_ctx* ctx);
int rescue_check(size_t count, const plk_rescue_ctx* ctx);
int rescue_sponge_check(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, size_t n_outputs);
int rescue_permutation_dev_impl(size_t count, const plk_rescue_ctx* ctx, const void* d_states, void* d_out, hipStream_t stream);
int rescue_sponge_dev_impl(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, const void* d_inputs, size_t n_outputs, void* d_out, hipStream_t stream);
// the Rescue hash to the curve (rescue_h2c.hip): count first, context second; the check holds the refusals the host entries share
int rescue_h2c_check(size_t count, const plk_rescue_ctx* ctx, int curve);
int rescue_h2c_dev_impl(size_t count, const plk_rescue_ctx* ctx, int curve, int field_seeds, const void* d_seeds, uint64_t seed_start, void* d_out_xy,
                        void* d_status, hipStream_t stream);
int field_kth_root_check(size_t count, int field, uint32_t k);
int field_kth_root_dev_impl(size_t count, int field, uint32_t k, const void* d_in, void* d_out, hipStream_t stream);
// a point times a scalar of its own and the Halo endomorphism (scalar_mul.hip): count first, then the curve id; the checks hold the
// refusals the host entries share
int curve_scalar_mul_check(size_t count, int curve, size_t n_scalars, size_t n_points);
int curve_scalar_mul_dev_impl(size_t count, int curve, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy, const void* d_p_zero,
                              void* d_out_xy, void* d_out_zero, hipStream_t stream);
int halo_n_check(size_t count, int curve, unsigned security_bits);
int halo_n_dev_impl(size_t count, int curve, unsigned security_bits, const void* d_scalars, void* d_out, hipStream_t stream);
int halo_n_mul_check(size_t count, int curve, unsigned security_bits, size_t n_scalars, size_t n_points);
int halo_n_mul_dev_impl(size_t count, int curve, unsigned security_bits, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy,
                        const void* d_p_zero, void* d_out_xy, void* d_out_zero, hipStream_t stream);
int field_batch_inverse_dev_impl(int field, const void* d_x, void* d_out, void* d_is_zero, unsigned* d_zero_count, size_t count, hipStream_t stream);
int curve_batch_to_affine_dev_impl(int curve, size_t count, const void* d_xyz, const void* d_zero, void* d_out_xy, void* d_out_zero, hipStream_t stream);
int plonk_vanishing_points_dev_impl(int field, unsigned log_degree, const void* d_constants, const void* d_wires, const void* d_s_sigma, const void* d_z,
                                    const uint64_t* k_is, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* inner_zeta,
                                    const uint64_t* inner_a, void* d_out, hipStream_t stream);
int plonk_permutation_z_dev_impl(int field, unsigned log_degree, const void* d_wires, const void* d_s_sigma, unsigned sigma_stride, const uint64_t* k_is,
                                 const uint64_t* beta, const uint64_t* gamma, void* d_out, void* d_status, hipStream_t stream);
// the copy-constraint permutation (sigma.hip): size first, then the field id; the check holds the refusals the host entry shares
int plonk_sigma_check(unsigned log_degree, int field, size_t num_partitions, size_t num_members, const uint64_t* k_is);
int plonk_sigma_dev_impl(unsigned log_degree, int field, const void* d_members, const void* d_offsets, size_t num_partitions, size_t num_members, const uint64_t* k_is,
                         void* d_sigma, void* d_s_sigma, void* d_status, hipStream_t stream);
// the cached R-form powers of the 8n-th root (plonk.hip: PlonkTables::xs_lo / xs_hi); PLK_NO_MATCH for a field outside the 4-limb ones
int plonk_domain_powers(int field, unsigned log_degree, hipStream_t stream, const void** xs_lo, const void** xs_hi, std::shared_ptr<const void>* hold);
// the Plookup prover's two loops (plookup.hip): size first, then the field id (include/plonky_hip.h says why)
int plookup_grand_product_dev_impl(unsigned log_size, int field, const void* d_f, const void* d_t, const void* d_s, const uint64_t* beta, const uint64_t* gamma,
                                   void* d_out, void* d_status, hipStream_t stream);
int plookup_vanishing_points_dev_impl(unsigned log_size, int field, const void* d_values_4n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                      void* d_out, hipStream_t stream);
// the Plookup sorted multiset (plookup_sort.hip); the check holds the refusals the host entry shares
int plookup_sorted_multiset_check(unsigned log_size, int field);
int plookup_sorted_multiset_dev_impl(unsigned log_size, int field, const void* d_f, const void* d_t, void* d_s, void* d_status, hipStream_t stream);
// the opening step (opening.hip): d_polys / lens are HOST arrays of n_polys device pointers / lengths, the scalars host limbs
int plonk_eval_polys_dev_impl(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, unsigned n_points, const uint64_t* points, void* d_out,
                              hipStream_t stream);
int poly_reduce_dev_impl(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* scalars, size_t degree, void* d_out,
                         hipStream_t stream);
int halo_build_b_dev_impl(int field, unsigned n_points, const uint64_t* points, const uint64_t* v, size_t degree, void* d_out, hipStream_t stream);
int halo_s_dev_impl(int field, unsigned k, const uint64_t* us, void* d_out, hipStream_t stream);
// low-degree polynomial division (polydiv.hip): b is a HOST array of lb coefficients
int poly_division_check(int field, size_t la, const uint64_t* b, size_t lb, size_t q_len);
int poly_division_dev_impl(int field, const void* d_a, size_t la, const uint64_t* b, size_t lb, void* d_q, size_t q_len, void* d_rem, hipStream_t stream);
int poly_from_roots_impl(int field, unsigned k, const uint64_t* roots, uint64_t* out);
// the power-series inverse and the division by a divisor of any degree (polydiv_newton.hip): size first, then the field id; b is a
// DEVICE array; the checks hold the refusals the host entries share
int poly_inv_mod_xn_check(size_t n, int field, size_t lh);
int poly_inv_mod_xn_dev_impl(size_t n, int field, const void* d_h, size_t lh, void* d_out, uint32_t* d_status, hipStream_t stream);
int poly_div_rem_check(size_t la, int field, size_t lb, size_t q_len, bool want_rem);
int poly_div_rem_dev_impl(size_t la, int field, const void* d_a, const void* d_b, size_t lb, void* d_q, size_t q_len, void* d_rem, uint32_t* d_status,
                          hipStream_t stream);
int plonk_all_constraints_dev_impl(int field, size_t count, const void* d_constants, const void* d_local, const void* d_right, const void* d_below,
                                   const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_out, hipStream_t stream);
// the witness check (plonk.hip): size first, then the field id; the check holds the refusals the host entry shares
int plonk_check_witness_check(unsigned log_degree, int field, const void* constants, unsigned constants_stride, const void* wires, const uint64_t* inner_zeta,
                              const uint64_t* inner_a, const void* report);
int plonk_check_witness_dev_impl(unsigned log_degree, int field, const void* d_constants, unsigned constants_stride, const void* d_wires, const void* d_sigma,
                                 const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_report, void* d_row_masks, void* d_first_terms, hipStream_t stream);
// gate witness rows (gate_trace.hip): count first, then the context or the shape and the curve id; the checks hold the refusals the
// host entries share
int trace_rescue_check(size_t count, const plk_rescue_ctx* ctx, size_t n_rows);
int trace_rescue_dev_impl(size_t count, const plk_rescue_ctx* ctx, const void* d_inputs, size_t n_rows, void* d_wires, const void* d_first_rows,
                          void* d_constants, void* d_status, hipStream_t stream);
int trace_msm_check(size_t count, unsigned parts, unsigned n_bits, int curve, const uint64_t* start_xy, size_t n_rows);
int trace_msm_dev_impl(size_t count, unsigned parts, unsigned n_bits, int curve, const void* d_points, const void* d_scalars, const uint64_t* start_xy, size_t n_rows,
                       void* d_wires, const void* d_first_rows, void* d_constants, void* d_status, hipStream_t stream);

// per-vector generator ranges (and, optionally, bucket ranges) of a batched MSM execution (msm.hip: msm_execute_dev_impl; host arrays of
// `batch` entries; scalars[b]: a device pointer)
struct MsmParts {
    const uint64_t* first;
    const uint64_t* count;
    const void* const* scalars;
    const uint32_t* bucket_part = nullptr;   // optional: vector b keeps the bucket_part[b]-th of bucket_parts[b] ranges of the coarse bins
    const uint32_t* bucket_parts = nullptr;  // (absent, 0 or 1: every bucket)
};

// ---- msm.hip: contexts ----
int msm_precompute_dev_impl(int curve, size_t n, const void* d_bases, const void* d_zero, unsigned window_bits, unsigned flags, hipStream_t stream,
                            plk_msm_ctx** out_ctx, const void* d_extra = nullptr, size_t n_extra = 0, const size_t* also_n = nullptr,
                            int also_count = 0);
int msm_rebind_dev_impl(plk_msm_ctx* ctx, size_t n, const void* d_bases, const void* d_zero, const void* d_extra, size_t n_extra, hipStream_t stream);
int msm_execute_dev_impl(plk_msm_ctx* ctx, unsigned batch, const void* d_scalars, size_t n_scalars, void* d_out_xy, void* d_out_zero, hipStream_t stream,
                         hipEvent_t* ready = nullptr, const MsmParts* parts = nullptr, unsigned out_flags = 0);
int msm_reserve_workspaces_impl(plk_msm_ctx* ctx, unsigned count, hipStream_t stream);
size_t msm_ctx_len(const plk_msm_ctx* ctx);
unsigned msm_ctx_window(const plk_msm_ctx* ctx);
int msm_ctx_curve(const plk_msm_ctx* ctx);
int msm_ctx_is_comb(const plk_msm_ctx* ctx);
int msm_ctx_table_free(const plk_msm_ctx* ctx);
int msm_ctx_device(const plk_msm_ctx* ctx);
std::vector<plk_msm_ctx*>& msm_ctx_peers(plk_msm_ctx* ctx);
std::vector<plk_msm_ctx*>& msm_ctx_shards(plk_msm_ctx* ctx);
void msm_ctx_delete(plk_msm_ctx* ctx);
int msm_set_profiling_impl(plk_msm_ctx* ctx, int enable);
int msm_get_timings_impl(plk_msm_ctx* ctx, double* sum_ms, unsigned* calls);
int msm_table_digits(int curve, unsigned w);
int msm_reference_table_dev_impl(int curve, size_t n, const void* d_bases, const void* d_zero, unsigned w, void* d_out_xy, void* d_out_zero,
                                 hipStream_t stream);
int msm_debug_digits_impl(int curve, unsigned window_bits, size_t n, const void* d_scalars, void* d_digits, hipStream_t stream);
int msm_debug_digit_count(int curve, unsigned window_bits);
// comb.hip: small fixed-base MSMs without buckets (a table of every multiple a signed 4-bit digit can ask for)
struct CombPlan;
int comb_build(int curve, size_t n, const void* d_base0, const void* d_chain, hipStream_t stream, CombPlan** out);
void comb_free(CombPlan* p);
int comb_execute(const CombPlan* p, unsigned batch, const void* const* d_scalars, const uint64_t* first, const uint64_t* count, void* d_out_xy, void* d_out_zero,
                 hipStream_t stream);
// msm_acc.hip, msm_order.hip, plookup_sort.hip: the checked build's guard counters
int checked_build_impl();
int checked_failures_impl(unsigned* counts);
int msm_order_checked_failures(unsigned* counts);
int plookup_sort_checked_failures(unsigned* counts);
// multi.hip: a context over every device of the group
void multi_plan_slot(int world, unsigned batch, size_t n, int d, unsigned slot, unsigned* vec, size_t* first, size_t* count);
bool msm_ctx_is_multi(plk_msm_ctx* ctx);
void group_copy_stats(unsigned long long* peer, unsigned long long* staged);
int msm_precompute_multi(int curve, size_t n, const void* bases, const void* zero, bool host_src, unsigned window_bits, hipStream_t caller_stream,
                         plk_msm_ctx** out_ctx);
int msm_execute_multi(plk_msm_ctx* ctx, unsigned batch, const void* const* vecs, bool host_src, size_t n, void* d_out_xy, void* d_out_zero,
                      hipStream_t caller_stream);
// curve_ops.hip
int msm_affine_to_projective_impl(int curve, unsigned batch, const void* d_xy, const void* d_zero, void* d_xyz, hipStream_t stream);
int curve_sum_affine_dev_impl(int curve, size_t k, const void* d_pts, const void* d_zero, void* d_out_xy, void* d_out_zero, hipStream_t stream);
size_t msm_partials_bytes(int curve, unsigned slots);
int msm_combine_partials_dev_impl(int curve, unsigned world, unsigned batch, unsigned whole_per_rank, const void* d_gathered, void* d_out_xy, void* d_out_zero,
                                  hipStream_t stream);
int selftest_quad_dev_impl(int curve, const void* d_pts, uint32_t n, uint32_t quads, uint32_t* counts);
int curve_op_dev_impl(int curve, int op, unsigned param, uint32_t count, const void* d_a_xy, const void* d_a_zero, const void* d_a_lambda, const void* d_b_xy,
                      const void* d_b_zero, const void* d_b_lambda, const void* d_flags, void* d_out_xy, void* d_out_zero, void* d_mismatch);
int curve_gen_bases_dev_impl(int curve, size_t n, uint64_t first, const void* d_g0d, void* d_out, hipStream_t stream);
// fold.hip
int curve_fold_pairs_dev_impl(int curve, size_t m, const void* d_lo, const void* d_lo_zero, const void* d_hi, const void* d_hi_zero,
                              const uint64_t* a_mont, const uint64_t* b_mont, void* d_out_xy, void* d_out_zero, hipStream_t stream,
                              const void* d_scalars = nullptr, int plus_lo = 0);
int curve_fold_multi_dev_impl(int curve, size_t n_out, int r_bits, const void* d_g, const void* d_gz, const void* d_ratios, void* d_out_xy,
                              void* d_out_zero, hipStream_t stream);
// halo.hip: one inner-product argument
int halo_begin_dev_impl(int curve, size_t n, const void* d_a, const void* d_b, const void* d_g, const void* d_gz, const uint64_t* h_xy,
                        const uint64_t* u_xy, unsigned freeze_log, hipStream_t stream, plk_halo_ctx** out, plk_msm_ctx* tables = nullptr,
                        unsigned lead_rounds = 0, size_t h_index = (size_t)-1, size_t u_index = (size_t)-1, const uint64_t* u_prime_scalar = nullptr);
int halo_round_lr_impl(plk_halo_ctx* c, const uint64_t* l_blind, const uint64_t* r_blind, uint64_t* lr_xy, uint8_t* lr_zero);
int halo_round_fold_impl(plk_halo_ctx* c, const uint64_t* u_j, const uint64_t* u_j_inv);
size_t halo_len_impl(const plk_halo_ctx* c);
int halo_frozen_impl(const plk_halo_ctx* c);
int halo_read_impl(plk_halo_ctx* c, uint64_t* a, uint64_t* b, uint64_t* g_xy, uint8_t* g_zero);
void halo_delete(plk_halo_ctx* c);
// fieldops.hip, ceilings.hip, ntt.hip, poly.hip
int field_op_impl(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
int bench_ceilings_impl(double* out, unsigned n_out);
int ntt_set_profiling_impl(int enable);
int ntt_get_timings_impl(double* sum_ms, unsigned* launches);
int poly_divide_by_z_h_dev_impl(int field, const void* d_coeffs, size_t len, size_t n, void* d_out, size_t out_cap, size_t* out_len,
                                hipStream_t stream);
int poly_mul_dev_impl(int field, const void* d_a, size_t la, const void* d_b, size_t lb, void* d_out, size_t out_cap, size_t* out_len,
                      hipStream_t stream);
int ntt_padded_dev_impl(int field, unsigned log_n, unsigned batch, const void* d_in, size_t in_len, size_t in_stride, void* d_out,
                        hipStream_t stream);

// properties of an id, read from the parameter structs through the dispatchers (host_runtime.hip); PLK_ERR_INVALID_ARG for an unknown id
int field_limbs(int field);         // 64-bit limbs of an element
int curve_limbs(int curve);         // ... of a coordinate
int curve_scalar_field(int curve);  // PLK_FIELD_* of the scalars
int curve_scalar_bits(int curve);   // bits of the scalar field's modulus

}  // namespace plk
