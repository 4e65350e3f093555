// capi.hip -- the extern "C" surface declared in include/plonky_hip.h.
// Thin: argument validation, host<->device staging for the host-pointer variants (LaneCall, host_lane.h), dispatch.  Only the
// entry points and their file-local helpers live here: the state they lean on is host_runtime.hip's.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "host_lane.h"

using namespace plk;

extern "C" {

int plk_init(int device) { return group_init_single(device); }
int plk_init_devices(int n_devices) { return group_init(n_devices); }
int plk_device_count(void) { return group_size(); }
int plk_set_thread_device(int logical_device) {
    if (logical_device < 0 || logical_device >= group_size())
        return set_error(PLK_ERR_INVALID_ARG, "logical device %d out of range (%d in use)", logical_device, group_size());
    set_thread_logical_device(logical_device);
    return ensure_device();
}

int plk_thread_hip_device(int set_to) {
    if (set_to >= 0) PLK_HIP_TRY(hipSetDevice(set_to));
    int cur = -1;
    PLK_HIP_TRY(hipGetDevice(&cur));
    return cur;
}
int plk_group_copy_stats(unsigned long long* peer_copies, unsigned long long* staged_copies) {
    group_copy_stats(peer_copies, staged_copies);
    return PLK_OK;
}

int plk_multi_plan(unsigned world, unsigned batch, size_t n, unsigned device, unsigned* slots, unsigned* vec, uint64_t* first, uint64_t* count) {
    if (world == 0 || device >= world || !slots) return set_error(PLK_ERR_INVALID_ARG, "bad world / device");
    const unsigned whole = batch / world, total = whole + (batch - whole * world);
    *slots = total;
    for (unsigned s = 0; s < total && vec && first && count; ++s) {
        size_t f = 0, c = 0;
        multi_plan_slot((int)world, batch, n, (int)device, s, &vec[s], &f, &c);
        first[s] = f;
        count[s] = c;
    }
    return PLK_OK;
}

void plk_shutdown(void) {
    table_caches_clear();
    scratch_clear();
    group_shutdown();
}

// Not part of the ABI (include/plonky_hip.h does not declare it): the suite reads which route the host-pointer plumbing took.
// out[0 .. PIN_BRANCHES): calls per branch of the caller-buffer registry (pin_registry.h: PinBranch), then its waits and rechecks,
// then the copies per LaneRoute (host_lane.h).  Returns the number of values there are; writes at most n of them.
int plk_internal_host_stats(unsigned long long* out, unsigned n) { return host_stats(out, n); }

const char* plk_last_error(void) { return last_error_ref().c_str(); }
unsigned plk_min_gpu_log_n(void) {
    const char* e = getenv("PLK_MIN_GPU_LOG_N");
    // Default 12 - PROVISIONAL.  The crossover that is measured (profiles/r05_crossover_host_pointer_vs_cpu.txt: through the
    // HOST-pointer entry points, PCIe inside, a 2^10 transform takes 59 us against 148 us, a 2^8 one 34 against 37) is against the C++
    // RESTATEMENT of the reference's algorithm on this host, not against the reference's Rust on Rayon, which cannot be built here and is
    // faster by an unknown small factor; and the gate also covers MSM pairs, where a first call pays the precomputation.  Until the Rust
    // path itself has been timed beside it the gate stays at round 4's conservative 2^12; PLK_MIN_GPU_LOG_N=10 is the measured tie + 2.
    const int v = e ? atoi(e) : 12;
    return v < 0 ? 0u : (unsigned)v;
}
int plk_field_limbs(int field) { return field_limbs(field); }
int plk_curve_limbs(int curve) { return curve_limbs(curve); }
int plk_curve_scalar_field(int curve) { return curve_scalar_field(curve); }

// ---- NTT ----
int plk_ntt_precompute(int field, unsigned log_n) { PLK_API; return ntt_precompute_impl(field, log_n); }
int plk_ntt_clear_cache(void) {
    PLK_API;
    table_caches_clear();
    scratch_clear();  // "memory pressure": the idle scratch buffers go as well
    return PLK_OK;
}

int plk_ntt_precompute_table_dev(int field, unsigned log_n, void* d_out, void* stream) {
    PLK_API;
    return ntt_reference_table_dev_impl(field, log_n, d_out, as_stream(stream));
}
int plk_ntt_precompute_table(int field, unsigned log_n, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (log_n > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_n %u too large (max 30)", log_n);
    if (!out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t bytes = (((size_t)2 << log_n) - 1) * (size_t)field_limbs(field) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void* buf = nullptr;
    PLK_TRY(c.tmp(buf, bytes));
    PLK_TRY(ntt_reference_table_dev_impl(field, log_n, buf, c.stream()));
    PLK_TRY(c.out(out, buf, bytes));
    return c.finish();
}

int plk_ntt_dev(int field, unsigned log_n, int inverse, unsigned batch, const void* d_in, void* d_out, void* stream) {
    PLK_API;
    return ntt_dev_impl(field, log_n, inverse, batch, d_in, d_out, as_stream(stream));
}

// `batch` transforms from / to host memory on the calling thread's current device.  Over a device group (deal_units) the thread's
// share of a batch of `total` is every step-th transform from `first` on: transform b of the share is slot b * step from there.
static int ntt_batch_local(int field, unsigned log_n, int inverse, unsigned total, const uint64_t* const* in, uint64_t* const* out, unsigned first,
                           unsigned step) {
    if (first >= total) return PLK_OK;
    const unsigned batch = (total - first + step - 1) / step;
    in += first, out += first;
    const size_t bytes = ((size_t)1 << log_n) * (size_t)field_limbs(field) * 8;  // 32 per element, 48 for Bls12377Base
    LaneCall c;
    PLK_TRY(c.begin());
    HostLane* l = c.l;
    void* buf = nullptr;
    PLK_TRY(c.tmp(buf, bytes * batch));
    if (batch == 1 || bytes < ((size_t)1 << 20)) {
        // one transform, or small ones: upload, one batched launch, download
        for (unsigned b = 0; b < batch; ++b) PLK_TRY(lane_h2d(*l, (uint8_t*)buf + b * bytes, in[b * step], bytes));
        PLK_TRY(ntt_dev_impl(field, log_n, inverse, batch, buf, buf, l->stream));
        for (unsigned b = 0; b < batch; ++b) PLK_TRY(c.out(out[b * step], (uint8_t*)buf + b * bytes, bytes));
        return c.finish();
    }
    // several large transforms (the nine wire polynomials, plonk_util.rs:169-190): PCIe is the long pole (2 x 32 MiB per 2^20
    // transform against 0.12 ms of kernels).  Round 5: ONE stream per direction - the uploads follow each other at the full rate of
    // the link on aux[0], the kernels of transform b start on the main stream when its upload has landed (one event), its download
    // goes on aux[1] when they are done (one event): from the second transform on both directions of the link are busy all the time.
    // (Until round 4 transform b ran upload -> kernels -> download on stream b mod 3: three uploads shared the link, nothing ran
    // before all three had landed 1.8 ms in, and the last three downloads had the link to themselves; PLK_NTT_HOST_PIPE=0 is that form.)
    for (unsigned b = 0; b < batch; ++b) {
        c.pin(in[b * step], bytes);
        if ((const void*)out[b * step] != (const void*)in[b * step]) c.pin(out[b * step], bytes);
    }
    PLK_TRY(lane_fork(*l));
    const char* pe = getenv("PLK_NTT_HOST_PIPE");
    if (pe && atoi(pe) == 0) {
        for (unsigned b = 0; b < batch; ++b) {
            hipStream_t st = b % 3 == 0 ? l->stream : l->aux[b % 3 - 1];
            uint8_t* d = (uint8_t*)buf + b * bytes;
            PLK_TRY(lane_h2d(*l, d, in[b * step], bytes, st));
            PLK_TRY(ntt_dev_impl(field, log_n, inverse, 1, d, d, st));
            PLK_TRY(lane_d2h(*l, c.outs, out[b * step], d, bytes, st));
        }
    } else {
        while (l->ev_ready.size() < 2 * (size_t)batch) {
            hipEvent_t e = nullptr;
            PLK_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            l->ev_ready.push_back(e);
        }
        hipStream_t up = l->aux[0], down = l->aux[1];
        for (unsigned b = 0; b < batch; ++b) {
            uint8_t* d = (uint8_t*)buf + b * bytes;
            PLK_TRY(lane_h2d(*l, d, in[b * step], bytes, up));  // >= 1 MiB: direct, or in chunks where the runtime rejects that (host_lane.h)
            PLK_HIP_TRY(hipEventRecord(l->ev_ready[2 * b], up));
            PLK_HIP_TRY(hipStreamWaitEvent(l->stream, l->ev_ready[2 * b], 0));
            PLK_TRY(ntt_dev_impl(field, log_n, inverse, 1, d, d, l->stream));
            PLK_HIP_TRY(hipEventRecord(l->ev_ready[2 * b + 1], l->stream));
            PLK_HIP_TRY(hipStreamWaitEvent(down, l->ev_ready[2 * b + 1], 0));
            PLK_TRY(lane_d2h(*l, c.outs, out[b * step], d, bytes, down));
        }
    }
    PLK_TRY(lane_join(*l));  // before the registrations and the device buffer go
    return c.finish();
}

// Units that need no exchange (transforms) over the devices of the group: unit b runs on device b mod N, every device's share in
// one call of `local` on its worker thread.  A single unit - the reference's callers are nine Rayon threads with one transform
// each (plonk_util.rs:173-189) - runs on the calling thread, the calls taking the devices in turn.
static int deal_units(unsigned log_n, unsigned batch, const std::function<int(unsigned, unsigned)>& local) {
    const int world = group_size();
    if (world == 1 || log_n < multi_min_log_n()) return local(0, 1);
    if (batch == 1) {
        DeviceScope on(next_round_robin_device());
        return local(0, 1);
    }
    return run_on_devices(world, [&](int d) -> int { return local((unsigned)d, (unsigned)world); });
}

int plk_ntt_batch(int field, unsigned log_n, int inverse, unsigned batch, const uint64_t* const* in, uint64_t* const* out) {
    PLK_API;
    if (field_limbs(field) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (log_n > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_n %u too large (max 30)", log_n);
    if (batch == 0) return PLK_OK;
    if (!in || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned b = 0; b < batch; ++b)
        if (!in[b] || !out[b]) return set_error(PLK_ERR_INVALID_ARG, "null pointer in batch slot %u", b);
    return deal_units(log_n, batch,
                      [&](unsigned first, unsigned step) -> int { return ntt_batch_local(field, log_n, inverse, batch, in, out, first, step); });
}

int plk_ntt(int field, unsigned log_n, int inverse, const uint64_t* in, uint64_t* out) {
    PLK_API;
    return plk_ntt_batch(field, log_n, inverse, 1, &in, &out);
}

int plk_ntt_padded_dev(int field, unsigned log_n, unsigned batch, const void* d_in, size_t in_len, size_t in_stride, void* d_out,
                       void* stream) {
    PLK_API;
    if (batch == 0) return PLK_OK;
    return ntt_padded_dev_impl(field, log_n, batch, d_in, in_len, in_stride, d_out, as_stream(stream));
}

static int ntt_padded_batch_local(int field, unsigned log_n, unsigned total, const uint64_t* const* in, const size_t* n_in, uint64_t* const* out,
                                  unsigned first, unsigned step) {  // the share of a device: as in ntt_batch_local
    if (first >= total) return PLK_OK;
    const unsigned batch = (total - first + step - 1) / step;
    in += first, n_in += first, out += first;
    const size_t n = (size_t)1 << log_n;
    size_t max_in = 0;
    for (unsigned b = 0; b < batch; ++b)
        if (n_in[b * step] > max_in) max_in = n_in[b * step];
    LaneCall c;
    PLK_TRY(c.begin());
    void *din = nullptr, *dout = nullptr;
    const size_t EB = (size_t)field_limbs(field) * 8;  // bytes per element
    PLK_TRY(c.tmp(din, max_in * EB * batch));
    PLK_TRY(c.tmp(dout, n * EB * batch));
    for (unsigned b = 0; b < batch; ++b) {
        uint8_t* slot = (uint8_t*)din + (size_t)b * max_in * EB;
        const uint64_t* src = in[b * step];
        const size_t len = n_in[b * step];
        // in place (out == in): ONE registration of the larger range, made here
        c.pin(src, (const void*)out[b * step] == (const void*)src && n > len ? n * EB : len * EB);
        PLK_TRY(lane_h2d(*c.l, slot, src, len * EB));
        // shorter polynomials of the batch: F::ZERO is all-zero limbs in Montgomery form too
        if (len < max_in) PLK_HIP_TRY(hipMemsetAsync(slot + len * EB, 0, (max_in - len) * EB, c.stream()));
    }
    PLK_TRY(ntt_padded_dev_impl(field, log_n, batch, din, max_in, max_in, dout, c.stream()));
    for (unsigned b = 0; b < batch; ++b) {
        c.pin(out[b * step], n * EB);  // in place: inside the registration made above
        PLK_TRY(c.out(out[b * step], (uint8_t*)dout + (size_t)b * n * EB, n * EB));
    }
    return c.finish();
}

int plk_ntt_padded_batch(int field, unsigned log_n, unsigned batch, const uint64_t* const* in, const size_t* n_in, uint64_t* const* out) {
    PLK_API;
    if (field_limbs(field) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (log_n > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_n %u too large (max 30)", log_n);
    if (batch == 0) return PLK_OK;
    if (!in || !n_in || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t n = (size_t)1 << log_n;
    for (unsigned b = 0; b < batch; ++b) {
        if (n_in[b] > n) return set_error(PLK_ERR_INVALID_ARG, "n_in[%u] = %zu exceeds 2^%u", b, n_in[b], log_n);
        if ((n_in[b] && !in[b]) || !out[b]) return set_error(PLK_ERR_INVALID_ARG, "null pointer in batch slot %u", b);
    }
    return deal_units(log_n, batch,
                      [&](unsigned first, unsigned step) -> int { return ntt_padded_batch_local(field, log_n, batch, in, n_in, out, first, step); });
}

int plk_ntt_padded(int field, unsigned log_n, const uint64_t* in, size_t n_in, uint64_t* out) {
    PLK_API;
    return plk_ntt_padded_batch(field, log_n, 1, &in, &n_in, &out);
}

// ---- polynomial callers ----
static size_t pow2_ceil_sz(size_t v) {
    size_t s = 1;
    while (s < v) s <<= 1;
    return s;
}

int plk_poly_divide_by_z_h_dev(int field, const void* d_coeffs, size_t len, size_t n, void* d_out, size_t out_cap, size_t* out_len,
                               void* stream) {
    PLK_API;
    return poly_divide_by_z_h_dev_impl(field, d_coeffs, len, n, d_out, out_cap, out_len, as_stream(stream));
}

int plk_poly_divide_by_z_h(int field, const uint64_t* coeffs, size_t len, size_t n, uint64_t* out, size_t out_cap, size_t* out_len) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d has no NTT entry point", field);
    if (!out_len || (len && !coeffs)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t cap = len > pow2_ceil_sz(len) ? len : pow2_ceil_sz(len);
    LaneCall c;
    PLK_TRY(c.begin());
    void *din = nullptr, *dout = nullptr;
    PLK_TRY(c.in(din, coeffs, len * 32));
    PLK_TRY(c.tmp(dout, cap * 32));
    size_t got = 0;
    PLK_TRY(poly_divide_by_z_h_dev_impl(field, din, len, n, dout, cap, &got, c.stream()));  // synchronises the stream once (the degree)
    if (got > out_cap) return set_error(PLK_ERR_INVALID_ARG, "output capacity %zu < result length %zu", out_cap, got);
    if (got && !out) return set_error(PLK_ERR_INVALID_ARG, "null output");
    PLK_TRY(c.out(out, dout, got * 32));
    *out_len = got;
    return c.finish();
}

int plk_poly_mul_dev(int field, const void* d_a, size_t la, const void* d_b, size_t lb, void* d_out, size_t out_cap, size_t* out_len,
                     void* stream) {
    PLK_API;
    return poly_mul_dev_impl(field, d_a, la, d_b, lb, d_out, out_cap, out_len, as_stream(stream));
}

int plk_poly_mul(int field, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, uint64_t* out, size_t out_cap, size_t* out_len) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d has no NTT entry point", field);
    if (!out_len || (la && !a) || (lb && !b)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t cap = pow2_ceil_sz(la + lb);
    LaneCall c;
    PLK_TRY(c.begin());
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    PLK_TRY(c.in(da, a, la * 32));
    PLK_TRY(c.in(db, b, lb * 32));
    PLK_TRY(c.tmp(dout, cap * 32));
    size_t got = 0;
    PLK_TRY(poly_mul_dev_impl(field, da, la, db, lb, dout, cap, &got, c.stream()));
    if (got > out_cap) return set_error(PLK_ERR_INVALID_ARG, "output capacity %zu < result length %zu", out_cap, got);
    if (got && !out) return set_error(PLK_ERR_INVALID_ARG, "null output");
    PLK_TRY(c.out(out, dout, got * 32));
    *out_len = got;
    return c.finish();
}

// ---- low-degree polynomial division: the public-input quotient (polydiv.hip) ----
int plk_poly_division_dev(int field, const void* d_a, size_t la, const uint64_t* b, size_t lb, void* d_q, size_t q_len, void* d_rem, void* stream) {
    PLK_API;
    return poly_division_dev_impl(field, d_a, la, b, lb, d_q, q_len, d_rem, as_stream(stream));
}
int plk_poly_division(int field, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, uint64_t* q, size_t q_len, uint64_t* rem) {
    PLK_API;
    PLK_TRY(poly_division_check(field, la, b, lb, q_len));
    if (!a || !q) return set_error(PLK_ERR_INVALID_ARG, "null pointer: a / q");
    const size_t k = lb - 1;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(a, la * 32);
    c.pin(q, q_len * 32);
    void *da = nullptr, *dq = nullptr, *drem = nullptr;
    PLK_TRY(c.in(da, a, la * 32));
    PLK_TRY(c.tmp(dq, q_len * 32));
    PLK_TRY(c.tmp(drem, k * 32));
    PLK_TRY(poly_division_dev_impl(field, da, la, b, lb, dq, q_len, drem, c.stream()));
    PLK_TRY(c.out(q, dq, q_len * 32));
    if (rem) PLK_TRY(c.out(rem, drem, k * 32));
    return c.finish();
}
int plk_poly_from_roots(int field, unsigned k, const uint64_t* roots, uint64_t* out) {
    PLK_API;
    return poly_from_roots_impl(field, k, roots, out);
}

// ---- the power-series inverse and the division by a divisor of any degree (polydiv_newton.hip) ----
int plk_poly_inv_mod_xn_dev(size_t n, int field, const void* d_h, size_t lh, void* d_out, uint32_t* d_status, void* stream) {
    PLK_API;
    return poly_inv_mod_xn_dev_impl(n, field, d_h, lh, d_out, d_status, as_stream(stream));
}
static bool limbs4_zero(const uint64_t* x) { return !(x[0] | x[1] | x[2] | x[3]); }
int plk_poly_inv_mod_xn(size_t n, int field, const uint64_t* h, size_t lh, uint64_t* out) {
    PLK_API;
    PLK_TRY(poly_inv_mod_xn_check(n, field, lh));
    if (!h || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer: h / out");
    if (limbs4_zero(h)) return set_error(PLK_ERR_INVALID_ARG, "Inverse doesn't exist: h[0] is zero");
    if (lh > n) lh = n;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(h, lh * 32);
    c.pin(out, n * 32);
    void *dh = nullptr, *dout = nullptr;
    PLK_TRY(c.in(dh, h, lh * 32));
    PLK_TRY(c.tmp(dout, n * 32));
    PLK_TRY(poly_inv_mod_xn_dev_impl(n, field, dh, lh, dout, nullptr, c.stream()));
    PLK_TRY(c.out(out, dout, n * 32));
    return c.finish();
}
int plk_poly_div_rem_dev(size_t la, int field, const void* d_a, const void* d_b, size_t lb, void* d_q, size_t q_len, void* d_rem, uint32_t* d_status,
                         void* stream) {
    PLK_API;
    return poly_div_rem_dev_impl(la, field, d_a, d_b, lb, d_q, q_len, d_rem, d_status, as_stream(stream));
}
int plk_poly_div_rem(size_t la, int field, const uint64_t* a, const uint64_t* b, size_t lb, uint64_t* q, size_t q_len, uint64_t* rem) {
    PLK_API;
    PLK_TRY(poly_div_rem_check(la, field, lb, q_len, rem != nullptr));
    if (!a || !b || !q) return set_error(PLK_ERR_INVALID_ARG, "null pointer: a / b / q");
    const size_t k = lb - 1;
    if (limbs4_zero(b + 4 * k)) return set_error(PLK_ERR_INVALID_ARG, "the leading coefficient b[%zu] is zero", k);
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(a, la * 32);
    c.pin(b, lb * 32);
    c.pin(q, q_len * 32);
    void *da = nullptr, *db = nullptr, *dq = nullptr, *drem = nullptr;
    PLK_TRY(c.in(da, a, la * 32));
    PLK_TRY(c.tmp(dq, q_len * 32));
    PLK_TRY(c.tmp(drem, k * 32));
    if (k <= PLK_POLY_DIV_MAX_DEGREE) {  // b is on the host: the recurrence route (polydiv.hip) gives the same words
        PLK_TRY(poly_division_dev_impl(field, da, la, b, lb, dq, q_len, drem, c.stream()));
    } else {
        PLK_TRY(c.in(db, b, lb * 32));
        PLK_TRY(poly_div_rem_dev_impl(la, field, da, db, lb, dq, q_len, rem ? drem : nullptr, nullptr, c.stream()));
    }
    PLK_TRY(c.out(q, dq, q_len * 32));
    if (rem) PLK_TRY(c.out(rem, drem, k * 32));
    return c.finish();
}

// ---- the Plonk quotient numerator ----
int plk_plonk_vanishing_points_dev(int field, unsigned log_degree, const void* d_constants_8n, const void* d_wires_8n, const void* d_s_sigma_8n,
                                   const void* d_plonk_z_8n, const uint64_t* k_is, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                   const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_out, void* stream) {
    PLK_API;
    return plonk_vanishing_points_dev_impl(field, log_degree, d_constants_8n, d_wires_8n, d_s_sigma_8n, d_plonk_z_8n, k_is, alpha, beta, gamma, inner_zeta,
                                           inner_a, d_out, as_stream(stream));
}
int plk_plonk_vanishing_points(int field, unsigned log_degree, const uint64_t* constants_8n, const uint64_t* wires_8n, const uint64_t* s_sigma_8n,
                               const uint64_t* plonk_z_8n, const uint64_t* k_is, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                               const uint64_t* inner_zeta, const uint64_t* inner_a, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (log_degree + 3 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_degree %u too large", log_degree);
    if (!constants_8n || !wires_8n || !s_sigma_8n || !plonk_z_8n || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t row = ((size_t)8 << log_degree) * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(constants_8n, 6 * row);
    c.pin(wires_8n, 9 * row);
    c.pin(s_sigma_8n, 6 * row);
    c.pin(plonk_z_8n, row);
    c.pin(out, row);
    void *dc = nullptr, *dw = nullptr, *ds = nullptr, *dz = nullptr, *dout = nullptr;
    PLK_TRY(c.in(dc, constants_8n, 6 * row));
    PLK_TRY(c.in(dw, wires_8n, 9 * row));
    PLK_TRY(c.in(ds, s_sigma_8n, 6 * row));
    PLK_TRY(c.in(dz, plonk_z_8n, row));
    PLK_TRY(c.tmp(dout, row));
    PLK_TRY(plonk_vanishing_points_dev_impl(field, log_degree, dc, dw, ds, dz, k_is, alpha, beta, gamma, inner_zeta, inner_a, dout, c.stream()));
    PLK_TRY(c.out(out, dout, row));
    return c.finish();
}
int plk_plonk_permutation_z_dev(int field, unsigned log_degree, const void* d_wires, const void* d_s_sigma, unsigned sigma_stride, const uint64_t* k_is,
                                const uint64_t* beta, const uint64_t* gamma, void* d_out, void* d_status, void* stream) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    return plonk_permutation_z_dev_impl(field, log_degree, d_wires, d_s_sigma, sigma_stride, k_is, beta, gamma, d_out, d_status, as_stream(stream));
}
int plk_plonk_permutation_z(int field, unsigned log_degree, const uint64_t* wires, const uint64_t* s_sigma, unsigned sigma_stride, const uint64_t* k_is,
                            const uint64_t* beta, const uint64_t* gamma, uint64_t* out, int* wraps_to_one) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (sigma_stride != 1 && sigma_stride != 8) return set_error(PLK_ERR_INVALID_ARG, "sigma_stride %u is neither 1 nor 8", sigma_stride);
    if (log_degree + 3 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_degree %u too large", log_degree);
    if (!wires || !s_sigma || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t n = (size_t)1 << log_degree, row = n * 32;
    // the kernel reads one sigma element in eight of an 8n table: gather those on the host, so that 6 n elements cross PCIe, not 6 * 8n
    std::unique_ptr<uint64_t[]> gathered;
    if (sigma_stride == 8) {
        gathered.reset(new (std::nothrow) uint64_t[6 * n * 4]);
        if (!gathered) return set_error(PLK_ERR_OOM, "host buffer of %zu bytes for the sigma rows", 6 * row);
        for (size_t e = 0; e < 6 * n; ++e) memcpy(&gathered[e * 4], s_sigma + e * 8 * 4, 32);  // row j starts at j 8n = (j n) 8
        s_sigma = gathered.get();
    }
    LaneCall c;  // after `gathered`: its destructor waits for the copies out of that buffer
    PLK_TRY(c.begin());
    c.pin(wires, 6 * row);  // rows 0..5 of wire_values_by_wire_index: the routed wires
    c.pin(s_sigma, 6 * row);
    c.pin(out, row);
    void *dw = nullptr, *ds = nullptr, *dout = nullptr, *dst = nullptr;
    PLK_TRY(c.in(dw, wires, 6 * row));
    PLK_TRY(c.in(ds, s_sigma, 6 * row));
    PLK_TRY(c.tmp(dout, row));
    PLK_TRY(c.tmp(dst, 2 * sizeof(uint32_t)));
    PLK_TRY(plonk_permutation_z_dev_impl(field, log_degree, dw, ds, 1, k_is, beta, gamma, dout, dst, c.stream()));
    uint32_t st[2] = {0, 0};
    PLK_TRY(c.read(st, dst, sizeof(st)));
    if (st[0]) return c.refuse(PLK_ERR_INVALID_ARG, "No inverse: %u of the denominators of rows 0..n-2 are zero (plonk_util.rs:259)", st[0]);
    PLK_TRY(c.out(out, dout, row));
    if (wraps_to_one) *wraps_to_one = (int)st[1];
    return c.finish();
}
// ---- the Plookup prover's two loops (plookup.hip): the size comes first, the field id second ----
int plk_plookup_grand_product_dev(unsigned log_size, int field, const void* d_f, const void* d_t, const void* d_s, const uint64_t* beta,
                                  const uint64_t* gamma, void* d_out, void* d_status, void* stream) {
    PLK_API;
    return plookup_grand_product_dev_impl(log_size, field, d_f, d_t, d_s, beta, gamma, d_out, d_status, as_stream(stream));
}
int plk_plookup_grand_product(unsigned log_size, int field, const uint64_t* f, const uint64_t* t, const uint64_t* s, const uint64_t* beta,
                              const uint64_t* gamma, uint64_t* out, int* closes) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (log_size == 0) return set_error(PLK_ERR_INVALID_ARG, "log_size 0: the grand product reads f[0] (plookup.rs:187)");
    if (log_size > 28) return set_error(PLK_ERR_TWO_ADICITY, "log_size %u too large", log_size);
    if (!f || !t || !s || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t N = (size_t)1 << log_size, row = N * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(f, row);
    c.pin(t, row);
    c.pin(s, 2 * row - 32);
    c.pin(out, row);
    void *df = nullptr, *dt = nullptr, *ds = nullptr, *dout = nullptr, *dst = nullptr;
    PLK_TRY(c.in(df, f, row));
    PLK_TRY(c.in(dt, t, row));
    PLK_TRY(c.in(ds, s, 2 * row - 32));
    PLK_TRY(c.tmp(dout, row));
    PLK_TRY(c.tmp(dst, 2 * sizeof(uint32_t)));
    PLK_TRY(plookup_grand_product_dev_impl(log_size, field, df, dt, ds, beta, gamma, dout, dst, c.stream()));
    uint32_t st[2] = {0, 0};
    PLK_TRY(c.read(st, dst, sizeof(st)));
    if (st[0]) return c.refuse(PLK_ERR_INVALID_ARG, "No inverse: %u of the denominators of rows 0..n-2 are zero (plookup.rs:191)", st[0]);
    PLK_TRY(c.out(out, dout, row));
    if (closes) *closes = (int)st[1];
    return c.finish();
}
int plk_plookup_vanishing_points_dev(unsigned log_size, int field, const void* d_values_4n, const uint64_t* alpha, const uint64_t* beta,
                                     const uint64_t* gamma, void* d_out, void* stream) {
    PLK_API;
    return plookup_vanishing_points_dev_impl(log_size, field, d_values_4n, alpha, beta, gamma, d_out, as_stream(stream));
}
int plk_plookup_vanishing_points(unsigned log_size, int field, const uint64_t* values_4n, const uint64_t* alpha, const uint64_t* beta,
                                 const uint64_t* gamma, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (log_size == 0) return set_error(PLK_ERR_INVALID_ARG, "log_size 0: the prover pads to n + 1 >= 2 rows");
    if (log_size + 2 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_size %u too large", log_size);
    if (!values_4n || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t row = ((size_t)4 << log_size) * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(values_4n, 5 * row);
    c.pin(out, row);
    void *dv = nullptr, *dout = nullptr;
    PLK_TRY(c.in(dv, values_4n, 5 * row));
    PLK_TRY(c.tmp(dout, row));
    PLK_TRY(plookup_vanishing_points_dev_impl(log_size, field, dv, alpha, beta, gamma, dout, c.stream()));
    PLK_TRY(c.out(out, dout, row));
    return c.finish();
}
// ---- the Plookup sorted multiset (plookup_sort.hip) ----
int plk_plookup_sorted_multiset_dev(unsigned log_size, int field, const void* d_f, const void* d_t, void* d_s, void* d_status, void* stream) {
    PLK_API;
    return plookup_sorted_multiset_dev_impl(log_size, field, d_f, d_t, d_s, d_status, as_stream(stream));
}
int plk_plookup_sorted_multiset(unsigned log_size, int field, const uint64_t* f, const uint64_t* t, uint64_t* s, unsigned* missing) {
    PLK_API;
    PLK_TRY(plookup_sorted_multiset_check(log_size, field));
    if (!f || !t || !s) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t N = (size_t)1 << log_size, row = N * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(f, row);
    c.pin(t, row);
    c.pin(s, 2 * row - 32);
    void *df = nullptr, *dt = nullptr, *ds = nullptr, *dst = nullptr;
    PLK_TRY(c.in(df, f, row));
    PLK_TRY(c.in(dt, t, row));
    PLK_TRY(c.tmp(ds, 2 * row - 32));
    PLK_TRY(c.tmp(dst, 2 * sizeof(uint32_t)));
    PLK_TRY(plookup_sorted_multiset_dev_impl(log_size, field, df, dt, ds, dst, c.stream()));
    uint32_t st[2] = {0, 0};
    PLK_TRY(c.read(st, dst, sizeof(st)));
    if (missing) *missing = st[0];
    if (st[0]) return c.refuse(PLK_ERR_INVALID_ARG, "called `Option::unwrap()` on a `None` value: %u rows of f are not in t (plookup.rs:173)", st[0]);
    PLK_TRY(c.out(s, ds, 2 * row - 32));
    return c.finish();
}
// ---- the copy-constraint permutation (sigma.hip): the size comes first, the field id second ----
int plk_plonk_sigma_dev(unsigned log_degree, int field, const void* d_members, const void* d_offsets, size_t num_partitions, size_t num_members, const uint64_t* k_is,
                        void* d_sigma, void* d_s_sigma, void* d_status, void* stream) {
    PLK_API;
    return plonk_sigma_dev_impl(log_degree, field, d_members, d_offsets, num_partitions, num_members, k_is, d_sigma, d_s_sigma, d_status, as_stream(stream));
}
int plk_plonk_sigma(unsigned log_degree, int field, const uint32_t* members, const uint32_t* offsets, size_t num_partitions, const uint64_t* k_is, uint32_t* sigma,
                    uint64_t* s_sigma) {
    PLK_API;
    PLK_TRY(plonk_sigma_check(log_degree, field, num_partitions, 0, k_is));
    if (!offsets) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    if (!sigma && !s_sigma) return set_error(PLK_ERR_INVALID_ARG, "neither sigma nor s_sigma is given");
    // what the device form cannot see in time: the lanes' bisection needs offsets to start at 0 and never to decrease
    if (offsets[0] != 0) return set_error(PLK_ERR_INVALID_ARG, "offsets[0] is %u, not 0", offsets[0]);
    for (size_t q = 0; q < num_partitions; ++q)
        if (offsets[q + 1] < offsets[q]) return set_error(PLK_ERR_INVALID_ARG, "offsets decrease at partition %zu (%u after %u)", q, offsets[q + 1], offsets[q]);
    const size_t num_members = offsets[num_partitions];
    PLK_TRY(plonk_sigma_check(log_degree, field, num_partitions, num_members, k_is));
    if (num_members && !members) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t n6 = (size_t)6 << log_degree;
    LaneCall c;
    PLK_TRY(c.begin());
    void *dm = nullptr, *dof = nullptr, *dsig = nullptr, *dval = nullptr, *dst = nullptr;
    PLK_TRY(c.in(dm, members, num_members * 4));
    PLK_TRY(c.in(dof, offsets, (num_partitions + 1) * 4));
    PLK_TRY(c.tmp(dsig, n6 * 4));
    if (s_sigma) PLK_TRY(c.tmp(dval, n6 * 32));
    PLK_TRY(c.tmp(dst, 3 * sizeof(uint32_t)));
    PLK_TRY(plonk_sigma_dev_impl(log_degree, field, dm, dof, num_partitions, num_members, k_is, dsig, dval, dst, c.stream()));
    uint32_t st[3] = {0, 0, 0};
    PLK_TRY(c.read(st, dst, sizeof(st)));
    if (st[2]) return c.refuse(PLK_ERR_INVALID_ARG, "wire id out of range: %u members are not below 9 n", st[2]);
    if (st[1])
        return c.refuse(PLK_ERR_INVALID_ARG, "Non-routed wires should not be in a partition containing other wires: %u of them are (partition.rs:94-98)", st[1]);
    if (st[0]) return c.refuse(PLK_ERR_INVALID_ARG, "no entry found for key: %u routed wires are not listed exactly once (partition.rs:109)", st[0]);
    if (sigma) PLK_TRY(c.out(sigma, dsig, n6 * 4));
    if (s_sigma) PLK_TRY(c.out(s_sigma, dval, n6 * 32));
    return c.finish();
}
int plk_plonk_evaluate_all_constraints(int field, size_t count, const uint64_t* constants, const uint64_t* local_wires, const uint64_t* right_wires,
                                       const uint64_t* below_wires, const uint64_t* inner_zeta, const uint64_t* inner_a, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (count == 0) return PLK_OK;
    if (!constants || !local_wires || !right_wires || !below_wires || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dc = nullptr, *dl = nullptr, *dr = nullptr, *db = nullptr, *dout = nullptr;
    PLK_TRY(c.in(dc, constants, count * 6 * 32));
    PLK_TRY(c.in(dl, local_wires, count * 9 * 32));
    PLK_TRY(c.in(dr, right_wires, count * 9 * 32));
    PLK_TRY(c.in(db, below_wires, count * 9 * 32));
    PLK_TRY(c.tmp(dout, count * 8 * 32));
    PLK_TRY(plonk_all_constraints_dev_impl(field, count, dc, dl, dr, db, inner_zeta, inner_a, dout, c.stream()));
    PLK_TRY(c.out(out, dout, count * 8 * 32));
    return c.finish();
}
// ---- the witness check (plonk.hip; include/plonky_hip_witness.h): the size comes first, the field id second ----
int plk_plonk_check_witness_dev(unsigned log_degree, int field, const void* d_constants, unsigned constants_stride, const void* d_wires, const void* d_sigma,
                                const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_report, void* d_row_masks, void* d_first_terms, void* stream) {
    PLK_API;
    return plonk_check_witness_dev_impl(log_degree, field, d_constants, constants_stride, d_wires, d_sigma, inner_zeta, inner_a, d_report, d_row_masks,
                                        d_first_terms, as_stream(stream));
}
int plk_plonk_check_witness(unsigned log_degree, int field, const uint64_t* constants, unsigned constants_stride, const uint64_t* wires, const uint32_t* sigma,
                            const uint64_t* inner_zeta, const uint64_t* inner_a, uint32_t* report, uint8_t* row_masks, uint64_t* first_terms) {
    PLK_API;
    PLK_TRY(plonk_check_witness_check(log_degree, field, constants, constants_stride, wires, inner_zeta, inner_a, report));
    const size_t n = (size_t)1 << log_degree, row = n * 32;
    // the kernel reads one constant in eight of an 8n table: gather those on the host, so that 6 n elements cross PCIe, not 6 * 8n
    std::unique_ptr<uint64_t[]> gathered;
    if (constants_stride == 8) {
        gathered.reset(new (std::nothrow) uint64_t[6 * n * 4]);
        if (!gathered) return set_error(PLK_ERR_OOM, "host buffer of %zu bytes for the constants rows", 6 * row);
        for (size_t e = 0; e < 6 * n; ++e) memcpy(&gathered[e * 4], constants + e * 8 * 4, 32);  // row j starts at j 8n = (j n) 8
        constants = gathered.get();
    }
    LaneCall c;  // after `gathered`: its destructor waits for the copies out of that buffer
    PLK_TRY(c.begin());
    c.pin(constants, 6 * row);
    c.pin(wires, 9 * row);
    c.pin(sigma, 6 * n * 4);
    void *dc = nullptr, *dw = nullptr, *ds = nullptr, *drep = nullptr, *dmask = nullptr, *dterms = nullptr;
    PLK_TRY(c.in(dc, constants, 6 * row));
    PLK_TRY(c.in(dw, wires, 9 * row));
    PLK_TRY(c.in_opt(ds, sigma, 6 * n * 4));
    PLK_TRY(c.tmp(drep, 8 * sizeof(uint32_t)));
    if (row_masks) PLK_TRY(c.tmp(dmask, n));
    if (first_terms) PLK_TRY(c.tmp(dterms, 8 * 32));
    PLK_TRY(plonk_check_witness_dev_impl(log_degree, field, dc, 1, dw, ds, inner_zeta, inner_a, drep, dmask, dterms, c.stream()));
    PLK_TRY(c.out(report, drep, 8 * sizeof(uint32_t)));
    if (row_masks) PLK_TRY(c.out(row_masks, dmask, n));
    if (first_terms) PLK_TRY(c.out(first_terms, dterms, 8 * 32));
    return c.finish();
}

// ---- the opening step: evaluations, the reduced polynomial, halo_b, halo_s, powers (opening.hip) ----
int plk_field_powers_dev(int field, const uint64_t* x, size_t count, void* d_out, void* stream) {
    PLK_API;
    if (!x) return set_error(PLK_ERR_INVALID_ARG, "null pointer: x");
    static const uint64_t unused_v[4] = {0, 0, 0, 0};  // v^0 = 1 is the only power of v one point takes
    return halo_build_b_dev_impl(field, 1, x, unused_v, count, d_out, as_stream(stream));
}
int plk_field_powers(int field, const uint64_t* x, size_t count, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (!x || (count && !out)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(out, count * 32);
    void* dout = nullptr;
    PLK_TRY(c.tmp(dout, count * 32));
    static const uint64_t unused_v[4] = {0, 0, 0, 0};
    PLK_TRY(halo_build_b_dev_impl(field, 1, x, unused_v, count, dout, c.stream()));
    PLK_TRY(c.out(out, dout, count * 32));
    return c.finish();
}
int plk_plonk_eval_polys_dev(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, unsigned n_points, const uint64_t* points, void* d_out,
                             void* stream) {
    PLK_API;
    return plonk_eval_polys_dev_impl(field, n_polys, d_polys, lens, n_points, points, d_out, as_stream(stream));
}
// the polynomials of a host-pointer call, uploaded one by one on the lane
static int lane_upload_polys(LaneCall& c, unsigned n_polys, const uint64_t* const* polys, const size_t* lens, std::vector<const void*>& dev) {
    dev.assign(n_polys, nullptr);
    for (unsigned i = 0; i < n_polys; ++i) {
        if (lens[i] && !polys[i]) return set_error(PLK_ERR_INVALID_ARG, "null pointer: polynomial %u", i);
        c.pin(polys[i], lens[i] * 32);
        void* d = nullptr;
        PLK_TRY(c.in(d, polys[i], lens[i] * 32));
        dev[i] = d;
    }
    return PLK_OK;
}
int plk_plonk_eval_polys(int field, unsigned n_polys, const uint64_t* const* polys, const size_t* lens, unsigned n_points, const uint64_t* points, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (n_points < 1 || n_points > 8) return set_error(PLK_ERR_INVALID_ARG, "n_points %u is not in 1..8", n_points);
    if (!points || (n_polys && (!polys || !lens || !out))) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    std::vector<const void*> dev;
    PLK_TRY(lane_upload_polys(c, n_polys, polys, lens, dev));
    void* dout = nullptr;
    const size_t bytes = (size_t)n_polys * n_points * 32;
    PLK_TRY(c.tmp(dout, bytes));
    PLK_TRY(plonk_eval_polys_dev_impl(field, n_polys, dev.data(), lens, n_points, points, dout, c.stream()));
    PLK_TRY(c.out(out, dout, bytes));
    return c.finish();
}
int plk_poly_reduce_dev(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* scalars, size_t degree, void* d_out,
                        void* stream) {
    PLK_API;
    return poly_reduce_dev_impl(field, n_polys, d_polys, lens, scalars, degree, d_out, as_stream(stream));
}
int plk_poly_reduce(int field, unsigned n_polys, const uint64_t* const* polys, const size_t* lens, const uint64_t* scalars, size_t degree, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if ((n_polys && (!polys || !lens || !scalars)) || (degree && !out)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned i = 0; i < n_polys; ++i)
        if (lens[i] > degree) return set_error(PLK_ERR_INVALID_ARG, "polynomial %u has %zu coefficients, more than the degree %zu (halo.rs:41)", i, lens[i], degree);
    LaneCall c;
    PLK_TRY(c.begin());
    std::vector<const void*> dev;
    PLK_TRY(lane_upload_polys(c, n_polys, polys, lens, dev));
    c.pin(out, degree * 32);
    void* dout = nullptr;
    PLK_TRY(c.tmp(dout, degree * 32));
    PLK_TRY(poly_reduce_dev_impl(field, n_polys, dev.data(), lens, scalars, degree, dout, c.stream()));
    PLK_TRY(c.out(out, dout, degree * 32));
    return c.finish();
}
int plk_halo_build_b_dev(int field, unsigned n_points, const uint64_t* points, const uint64_t* v, size_t degree, void* d_out, void* stream) {
    PLK_API;
    return halo_build_b_dev_impl(field, n_points, points, v, degree, d_out, as_stream(stream));
}
int plk_halo_build_b(int field, unsigned n_points, const uint64_t* points, const uint64_t* v, size_t degree, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (n_points < 1 || n_points > 8) return set_error(PLK_ERR_INVALID_ARG, "n_points %u is not in 1..8", n_points);
    if (!points || !v || (degree && !out)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(out, degree * 32);
    void* dout = nullptr;
    PLK_TRY(c.tmp(dout, degree * 32));
    PLK_TRY(halo_build_b_dev_impl(field, n_points, points, v, degree, dout, c.stream()));
    PLK_TRY(c.out(out, dout, degree * 32));
    return c.finish();
}
int plk_halo_s_dev(int field, unsigned k, const uint64_t* us, void* d_out, void* stream) {
    PLK_API;
    return halo_s_dev_impl(field, k, us, d_out, as_stream(stream));
}
int plk_halo_s(int field, unsigned k, const uint64_t* us, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    if (k > 30) return set_error(PLK_ERR_INVALID_ARG, "%u challenges: at most 30", k);
    if ((k && !us) || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned j = 0; j < k; ++j)
        if (!(us[4 * j] | us[4 * j + 1] | us[4 * j + 2] | us[4 * j + 3]))
            return set_error(PLK_ERR_INVALID_ARG, "No inverse: challenge %u is zero (field.rs:266, from plonk_util.rs:314)", j);
    const size_t bytes = ((size_t)1 << k) * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(out, bytes);
    void* dout = nullptr;
    PLK_TRY(c.tmp(dout, bytes));
    PLK_TRY(halo_s_dev_impl(field, k, us, dout, c.stream()));
    PLK_TRY(c.out(out, dout, bytes));
    return c.finish();
}

// ---- MSM ----
// Over a device group (plk_init_devices) a tabled precomputation of at least 2^PLK_MULTI_MIN_LOG_N generators is built on every
// device (multi.hip); smaller ones, and table-free contexts (one-shot MSMs: latency, not throughput), stay on the caller's device.
static bool fan_out_msm(size_t n, unsigned flags) {
    return group_size() > 1 && !(flags & PLK_MSM_TABLE_FREE) && n >= ((size_t)1 << multi_min_log_n()) && n >= (size_t)group_size();
}
int plk_msm_precompute_dev_ex(int curve, size_t n, const void* d_bases_xy, const void* d_base_zero, unsigned window_bits, unsigned flags, void* stream,
                              plk_msm_ctx** out_ctx) {
    PLK_API;
    if (fan_out_msm(n, flags) && d_bases_xy) return msm_precompute_multi(curve, n, d_bases_xy, d_base_zero, false, window_bits, as_stream(stream), out_ctx);
    return msm_precompute_dev_impl(curve, n, d_bases_xy, d_base_zero, window_bits, flags, as_stream(stream), out_ctx);
}
int plk_msm_precompute_dev(int curve, size_t n, const void* d_bases_xy, const void* d_base_zero, unsigned window_bits, void* stream,
                           plk_msm_ctx** out_ctx) {
    PLK_API;
    return plk_msm_precompute_dev_ex(curve, n, d_bases_xy, d_base_zero, window_bits, 0, stream, out_ctx);
}

int plk_msm_precompute_ex(int curve, size_t n, const uint64_t* bases_xy, const uint8_t* base_zero, unsigned window_bits, unsigned flags,
                          plk_msm_ctx** out_ctx) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (n && !bases_xy) return set_error(PLK_ERR_INVALID_ARG, "null bases");
    if (fan_out_msm(n, flags)) {
        DeviceScope primary(0);
        return msm_precompute_multi(curve, n, bases_xy, base_zero, true, window_bits, nullptr, out_ctx);
    }
    LaneCall c;  // registers nothing: the generators are uploaded once per context
    PLK_TRY(c.begin());
    void *db = nullptr, *dz = nullptr;
    PLK_TRY(c.in(db, bases_xy, n * 2 * L * 8));
    PLK_TRY(c.in_opt(dz, base_zero, n));
    PLK_TRY(msm_precompute_dev_impl(curve, n, db, dz, window_bits, flags, c.stream(), out_ctx));  // synchronises the stream on success
    return c.finish();  // one more synchronisation of the then idle stream: accepted in a precomputation
}
int plk_msm_precompute(int curve, size_t n, const uint64_t* bases_xy, const uint8_t* base_zero, unsigned window_bits, plk_msm_ctx** out_ctx) {
    PLK_API;
    return plk_msm_precompute_ex(curve, n, bases_xy, base_zero, window_bits, 0, out_ctx);
}

int plk_msm_free(plk_msm_ctx* ctx) {
    PLK_API;
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    msm_ctx_delete(ctx);
    return PLK_OK;
}
size_t plk_msm_ctx_len(const plk_msm_ctx* ctx) { return ctx ? msm_ctx_len(ctx) : 0; }
unsigned plk_msm_ctx_window(const plk_msm_ctx* ctx) { return ctx ? msm_ctx_window(ctx) : 0; }

int plk_msm_execute_dev(plk_msm_ctx* ctx, unsigned batch, const void* d_scalars, size_t n_scalars, void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    if (msm_ctx_is_multi(ctx) && batch && d_scalars && n_scalars == msm_ctx_len(ctx)) {
        // a context that lives on every device of the group: the vectors (memory of the caller's device) reach the other devices
        // peer to peer, the results come back to the caller's device; asynchronous on `stream` like the one-device form
        std::vector<const void*> vecs(batch);
        for (unsigned b = 0; b < batch; ++b) vecs[b] = (const uint8_t*)d_scalars + (size_t)b * n_scalars * 32;
        return msm_execute_multi(ctx, batch, vecs.data(), false, n_scalars, d_out_xy, d_out_zero, as_stream(stream));
    }
    return msm_execute_dev_impl(ctx, batch, d_scalars, n_scalars, d_out_xy, d_out_zero, as_stream(stream));
}

// msm_execute_parallel's own return type (curve_msm.rs:102-157: a ProjectivePoint, not normalised): x | y | z per vector.  One-device
// bucket contexts end their reduction with six products instead of an inversion; combs and device-group contexts, which normalise on the
// way anyway, return their affine points with z = 1.
int plk_msm_execute_projective_dev(plk_msm_ctx* ctx, unsigned batch, const void* d_scalars, size_t n_scalars, void* d_out_xyz, void* d_out_zero, void* stream) {
    PLK_API;
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    if (!msm_ctx_is_multi(ctx) && !msm_ctx_is_comb(ctx))
        return msm_execute_dev_impl(ctx, batch, d_scalars, n_scalars, d_out_xyz, d_out_zero, as_stream(stream), nullptr, nullptr, 1u);
    if (batch == 0) return PLK_OK;
    if (!d_out_xyz || !d_out_zero) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    const size_t L = (size_t)curve_limbs(msm_ctx_curve(ctx));
    hipStream_t st = as_stream(stream);
    void* tmp = scratch_acquire((size_t)batch * 2 * L * 8, st);
    if (!tmp) return PLK_ERR_OOM;
    int rc = plk_msm_execute_dev(ctx, batch, d_scalars, n_scalars, tmp, d_out_zero, stream);
    if (rc == PLK_OK) rc = msm_affine_to_projective_impl(msm_ctx_curve(ctx), batch, tmp, d_out_zero, d_out_xyz, st);
    scratch_release(tmp, st);
    return rc;
}
int plk_msm_execute_projective(plk_msm_ctx* ctx, const uint64_t* scalars, size_t n_scalars, uint64_t* out_xyz, uint8_t* out_zero) {
    PLK_API;
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    if (n_scalars != msm_ctx_len(ctx))
        return set_error(PLK_ERR_SIZE_MISMATCH, "scalars.len() = %zu but the precomputation holds %zu generators (curve_msm.rs:67)", n_scalars, msm_ctx_len(ctx));
    if ((n_scalars && !scalars) || !out_xyz || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t L = (size_t)curve_limbs(msm_ctx_curve(ctx));
    DeviceScope primary(msm_ctx_is_multi(ctx) ? 0 : thread_logical_device());
    LaneCall c;
    PLK_TRY(c.begin());
    void *ds = nullptr, *dxyz = nullptr, *dz = nullptr;
    c.pin(scalars, n_scalars * 32);
    PLK_TRY(c.in(ds, scalars, n_scalars * 32));
    PLK_TRY(c.tmp(dxyz, 3 * L * 8));
    PLK_TRY(c.tmp(dz, 1));
    PLK_TRY(plk_msm_execute_projective_dev(ctx, 1, ds, n_scalars, dxyz, dz, (void*)c.stream()));
    PLK_TRY(c.out(out_xyz, dxyz, 3 * L * 8));
    PLK_TRY(c.out(out_zero, dz, 1));
    return c.finish();
}

int plk_msm_execute_parts_dev(plk_msm_ctx* ctx, unsigned batch, const uint64_t* first, const uint64_t* count, const void* const* d_scalars, void* d_out_xy,
                              void* d_out_zero, void* stream) {
    PLK_API;
    MsmParts parts{first, count, d_scalars};
    return msm_execute_dev_impl(ctx, batch, nullptr, 0, d_out_xy, d_out_zero, as_stream(stream), nullptr, &parts);
}

int plk_msm_execute_parts_buckets_dev(plk_msm_ctx* ctx, unsigned batch, const uint64_t* first, const uint64_t* count, const void* const* d_scalars,
                                      const uint32_t* bucket_part, const uint32_t* bucket_parts, void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    if (!bucket_part || !bucket_parts) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    MsmParts parts{first, count, d_scalars, bucket_part, bucket_parts};
    return msm_execute_dev_impl(ctx, batch, nullptr, 0, d_out_xy, d_out_zero, as_stream(stream), nullptr, &parts);
}

int plk_msm_execute_batch(plk_msm_ctx* ctx, unsigned batch, const uint64_t* const* scalars, size_t n_scalars, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    if (n_scalars != msm_ctx_len(ctx))
        return set_error(PLK_ERR_SIZE_MISMATCH, "scalars.len() = %zu but the precomputation holds %zu generators (curve_msm.rs:67)", n_scalars,
                         msm_ctx_len(ctx));
    if (batch == 0) return PLK_OK;
    if (!scalars || !out_xy || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned b = 0; b < batch; ++b)
        if (n_scalars && !scalars[b]) return set_error(PLK_ERR_INVALID_ARG, "null scalars in batch slot %u", b);
    const bool multi = msm_ctx_is_multi(ctx);
    DeviceScope primary(multi ? 0 : thread_logical_device());  // a group context's results are combined on its first device
    const size_t L = (size_t)curve_limbs(msm_ctx_curve(ctx));
    const size_t sb = n_scalars * 32;
    LaneCall c;
    PLK_TRY(c.begin());
    HostLane* l = c.l;
    void *dxy = nullptr, *dz = nullptr;
    PLK_TRY(c.tmp(dxy, (size_t)batch * 2 * L * 8));
    PLK_TRY(c.tmp(dz, batch));
    if (multi) {
        // every device uploads its own share over its own PCIe link (multi.hip); the vectors stay registered until this call's
        // final synchronisation, which - through the events the caller's stream waits for - covers the workers' copies
        for (unsigned b = 0; b < batch; ++b) c.pin(scalars[b], sb);
        PLK_TRY(msm_execute_multi(ctx, batch, (const void* const*)scalars, true, n_scalars, dxy, dz, l->stream));
    } else if (batch == 1 || sb < ((size_t)1 << 20)) {
        void* ds = nullptr;
        PLK_TRY(c.tmp(ds, sb * batch));
        for (unsigned b = 0; b < batch; ++b) PLK_TRY(lane_h2d(*l, (uint8_t*)ds + b * sb, scalars[b], sb));
        PLK_TRY(msm_execute_dev_impl(ctx, batch, ds, n_scalars, dxy, dz, l->stream));
    } else {
        // the scalar vectors of a batch (commit_polynomials, plonk_util.rs:215-231: nine 32 MiB vectors at 2^20) cross PCIe on a
        // second stream, vector b + 1 while vector b is being ordered and accumulated: one event per vector
        void* ds = nullptr;
        PLK_TRY(c.tmp(ds, sb * batch));
        for (unsigned b = 0; b < batch; ++b) c.pin(scalars[b], sb);
        PLK_TRY(lane_fork(*l));
        while (l->ev_ready.size() < batch) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return set_error(PLK_ERR_HIP, "hipEventCreate failed");
            l->ev_ready.push_back(e);
        }
        for (unsigned b = 0; b < batch; ++b) {
            PLK_TRY(lane_h2d(*l, (uint8_t*)ds + b * sb, scalars[b], sb, l->aux[0]));
            if (hipEventRecord(l->ev_ready[b], l->aux[0]) != hipSuccess) return set_error(PLK_ERR_HIP, "upload of scalar vector %u failed", b);
        }
        PLK_TRY(msm_execute_dev_impl(ctx, batch, ds, n_scalars, dxy, dz, l->stream, l->ev_ready.data()));
    }
    PLK_TRY(c.out(out_xy, dxy, (size_t)batch * 2 * L * 8));
    PLK_TRY(c.out(out_zero, dz, batch));
    return c.finish();
}

int plk_msm_execute(plk_msm_ctx* ctx, const uint64_t* scalars, size_t n_scalars, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    return plk_msm_execute_batch(ctx, 1, &scalars, n_scalars, out_xy, out_zero);
}

int plk_msm(int curve, size_t n, const uint64_t* bases_xy, const uint8_t* base_zero, const uint64_t* scalars, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    plk_msm_ctx* ctx = nullptr;
    // generators used once: no window tables (their construction costs ~30 executions)
    PLK_TRY(plk_msm_precompute_ex(curve, n, bases_xy, base_zero, 0, PLK_MSM_TABLE_FREE, &ctx));
    int rc = plk_msm_execute(ctx, scalars, n, out_xy, out_zero);
    msm_ctx_delete(ctx);
    return rc;
}

int plk_curve_sum_affine(int curve, size_t k, const uint64_t* pts_xy, const uint8_t* pts_zero, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if ((k && !pts_xy) || !out_xy || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dp = nullptr, *dz = nullptr, *dxy = nullptr, *doz = nullptr;
    PLK_TRY(c.in(dp, pts_xy, k * 2 * L * 8));
    PLK_TRY(c.in_opt(dz, pts_zero, k));
    PLK_TRY(c.tmp(dxy, 2 * L * 8));
    PLK_TRY(c.tmp(doz, 1));
    PLK_TRY(curve_sum_affine_dev_impl(curve, k, dp, dz, dxy, doz, c.stream()));
    PLK_TRY(c.out(out_xy, dxy, 2 * L * 8));
    PLK_TRY(c.out(out_zero, doz, 1));
    return c.finish();
}

// ---- multi-GPU exchange ----
size_t plk_msm_partials_bytes(int curve, unsigned slots) { return msm_partials_bytes(curve, slots); }
int plk_msm_combine_partials_dev(int curve, unsigned world, unsigned batch, unsigned whole_per_rank, const void* d_gathered, void* d_out_xy,
                                 void* d_out_zero, void* stream) {
    PLK_API;
    return msm_combine_partials_dev_impl(curve, world, batch, whole_per_rank, d_gathered, d_out_xy, d_out_zero, as_stream(stream));
}

// ---- the reference's own MsmPrecomputation contents ----
int plk_msm_table_digits(int curve, unsigned w) {
    if (curve_limbs(curve) < 0 || w == 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d or window 0", curve);
    return msm_table_digits(curve, w);
}
int plk_msm_precompute_table_dev(int curve, size_t n, const void* d_bases_xy, const void* d_base_zero, unsigned w, void* d_out_xy, void* d_out_zero,
                                 void* stream) {
    PLK_API;
    return msm_reference_table_dev_impl(curve, n, d_bases_xy, d_base_zero, w, d_out_xy, d_out_zero, as_stream(stream));
}
int plk_msm_precompute_table(int curve, size_t n, const uint64_t* bases_xy, const uint8_t* base_zero, unsigned w, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (w < 1 || w > 64) return set_error(PLK_ERR_INVALID_ARG, "window size %u outside [1, 64]", w);
    if (n && (!bases_xy || !out_xy || !out_zero)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    if (n == 0) return PLK_OK;
    const size_t digits = (size_t)msm_table_digits(curve, w);
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(out_xy, n * digits * 2 * L * 8);
    void *db = nullptr, *dz = nullptr, *dout = nullptr, *doz = nullptr;
    PLK_TRY(c.in(db, bases_xy, n * 2 * L * 8));
    PLK_TRY(c.in_opt(dz, base_zero, n));
    PLK_TRY(c.tmp(dout, n * digits * 2 * L * 8));
    PLK_TRY(c.tmp(doz, n * digits));
    PLK_TRY(msm_reference_table_dev_impl(curve, n, db, dz, w, dout, doz, c.stream()));
    PLK_TRY(c.out(out_xy, dout, n * digits * 2 * L * 8));
    PLK_TRY(c.out(out_zero, doz, n * digits));
    return c.finish();
}

// ---- IPA generator fold ----
int plk_curve_fold_pairs_dev(int curve, size_t m, const void* d_lo_xy, const void* d_lo_zero, const void* d_hi_xy, const void* d_hi_zero,
                             const uint64_t* scalar_lo, const uint64_t* scalar_hi, void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    return curve_fold_pairs_dev_impl(curve, m, d_lo_xy, d_lo_zero, d_hi_xy, d_hi_zero, scalar_lo, scalar_hi, d_out_xy, d_out_zero, as_stream(stream));
}

int plk_curve_fold_pairs(int curve, size_t m, const uint64_t* lo_xy, const uint8_t* lo_zero, const uint64_t* hi_xy, const uint8_t* hi_zero,
                         const uint64_t* scalar_lo, const uint64_t* scalar_hi, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (m && (!lo_xy || !hi_xy || !out_xy || !out_zero)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    if (!scalar_lo || !scalar_hi) return set_error(PLK_ERR_INVALID_ARG, "null scalar");
    if (m == 0) return PLK_OK;
    const size_t pb = m * 2 * L * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *dlo = nullptr, *dhi = nullptr, *dlz = nullptr, *dhz = nullptr, *dout = nullptr, *doz = nullptr;
    PLK_TRY(c.in(dlo, lo_xy, pb));
    PLK_TRY(c.in(dhi, hi_xy, pb));
    PLK_TRY(c.in_opt(dlz, lo_zero, m));
    PLK_TRY(c.in_opt(dhz, hi_zero, m));
    PLK_TRY(c.tmp(dout, pb));
    PLK_TRY(c.tmp(doz, m));
    PLK_TRY(curve_fold_pairs_dev_impl(curve, m, dlo, dlz, dhi, dhz, scalar_lo, scalar_hi, dout, doz, c.stream()));
    PLK_TRY(c.out(out_xy, dout, pb));
    PLK_TRY(c.out(out_zero, doz, m));
    return c.finish();
}

// ---- batch inversion ----
int plk_field_batch_inverse_dev(int field, const void* d_x, void* d_out, void* d_is_none, size_t count, void* stream) {
    PLK_API;
    if (field_limbs(field) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    return field_batch_inverse_dev_impl(field, d_x, d_out, d_is_none, nullptr, count, as_stream(stream));
}
static int batch_inverse_host(int field, const uint64_t* x, uint64_t* out, uint8_t* is_none, size_t count, bool strict) {
    const int L = field_limbs(field);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (count == 0) return PLK_OK;
    if (!x || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dx = nullptr, *dz = nullptr, *dc = nullptr;
    PLK_TRY(c.in(dx, x, count * L * 8));
    PLK_TRY(c.tmp(dz, count));
    PLK_TRY(c.tmp(dc, 4));
    PLK_HIP_TRY(hipMemsetAsync(dc, 0, 4, c.stream()));
    PLK_TRY(field_batch_inverse_dev_impl(field, dx, dx, dz, (unsigned*)dc, count, c.stream()));
    unsigned zeros = 0;
    PLK_TRY(c.read(&zeros, dc, 4));
    if (strict && zeros) return c.refuse(PLK_ERR_INVALID_ARG, "No inverse: %u of the %zu elements are zero (field.rs:266)", zeros, count);
    PLK_TRY(c.out(out, dx, count * L * 8));
    if (is_none) PLK_TRY(c.out(is_none, dz, count));
    return c.finish();
}
int plk_field_batch_inverse(int field, const uint64_t* x, uint64_t* out, size_t count) { PLK_API; return batch_inverse_host(field, x, out, nullptr, count, true); }
int plk_field_batch_inverse_opt(int field, const uint64_t* x, uint64_t* out, uint8_t* is_none, size_t count) {
    PLK_API;
    if (count && !is_none) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    return batch_inverse_host(field, x, out, is_none, count, false);
}
int plk_curve_batch_to_affine_dev(int curve, size_t count, const void* d_proj_xyz, const void* d_proj_zero, void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    return curve_batch_to_affine_dev_impl(curve, count, d_proj_xyz, d_proj_zero, d_out_xy, d_out_zero, as_stream(stream));
}
int plk_curve_batch_to_affine(int curve, size_t count, const uint64_t* proj_xyz, const uint8_t* proj_zero, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (count == 0) return PLK_OK;
    if (!proj_xyz || !out_xy || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dp = nullptr, *dz = nullptr, *dxy = nullptr, *doz = nullptr;
    PLK_TRY(c.in(dp, proj_xyz, count * 3 * L * 8));
    PLK_TRY(c.in_opt(dz, proj_zero, count));
    PLK_TRY(c.tmp(dxy, count * 2 * L * 8));
    PLK_TRY(c.tmp(doz, count));
    PLK_TRY(curve_batch_to_affine_dev_impl(curve, count, dp, dz, dxy, doz, c.stream()));
    PLK_TRY(c.out(out_xy, dxy, count * 2 * L * 8));
    PLK_TRY(c.out(out_zero, doz, count));
    return c.finish();
}

// ---- canonical byte encodings ----
int plk_field_to_bytes(int field, const uint64_t* x, size_t count, uint8_t* out_bytes) {
    PLK_API;
    const int L = field_limbs(field);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (count == 0) return PLK_OK;
    if (!x || !out_bytes) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dx = nullptr, *db = nullptr;
    PLK_TRY(c.in(dx, x, count * L * 8));
    PLK_TRY(c.tmp(db, count * L * 8));
    PLK_TRY(field_bytes_impl(field, 0, dx, count, db, nullptr, c.stream()));
    PLK_TRY(c.out(out_bytes, db, count * L * 8));
    return c.finish();
}
int plk_field_from_bytes(int field, const uint8_t* bytes, size_t count, uint64_t* out) {
    PLK_API;
    const int L = field_limbs(field);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (count == 0) return PLK_OK;
    if (!bytes || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void *dx = nullptr, *db = nullptr, *dc = nullptr;
    PLK_TRY(c.in(db, bytes, count * L * 8));
    PLK_TRY(c.tmp(dx, count * L * 8));
    PLK_TRY(c.tmp(dc, 4));
    PLK_HIP_TRY(hipMemsetAsync(dc, 0, 4, c.stream()));
    PLK_TRY(field_bytes_impl(field, 1, db, count, dx, (unsigned*)dc, c.stream()));
    unsigned bad = 0;
    PLK_TRY(c.out(&bad, dc, 4));
    PLK_TRY(c.out(out, dx, count * L * 8));
    PLK_TRY(c.finish());
    if (bad) return set_error(PLK_ERR_INVALID_ARG, "Out of range: %u of the %zu records are not below the modulus (field.rs:100)", bad, count);
    return PLK_OK;
}
int plk_curve_point_to_bytes(int curve, const uint64_t* xy, const uint8_t* zero, size_t count, uint8_t* out_bytes) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (count == 0) return PLK_OK;
    if (!xy || !out_bytes) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t rec = 1 + (size_t)L * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *dp = nullptr, *dz = nullptr, *db = nullptr;
    PLK_TRY(c.in(dp, xy, count * 2 * L * 8));
    PLK_TRY(c.in_opt(dz, zero, count));
    PLK_TRY(c.tmp(db, count * rec));
    PLK_TRY(point_bytes_impl(curve, 0, dp, dz, count, db, nullptr, nullptr, c.stream()));
    PLK_TRY(c.out(out_bytes, db, count * rec));
    return c.finish();
}
int plk_curve_point_from_bytes(int curve, const uint8_t* bytes, size_t count, uint64_t* out_xy, uint8_t* out_zero, uint8_t* status) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (count == 0) return PLK_OK;
    if (!bytes || !out_xy || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t rec = 1 + (size_t)L * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *dp = nullptr, *dz = nullptr, *ds = nullptr, *db = nullptr;
    PLK_TRY(c.in(db, bytes, count * rec));
    PLK_TRY(c.tmp(dp, count * 2 * L * 8));
    PLK_TRY(c.tmp(dz, count));
    PLK_TRY(c.tmp(ds, count));
    PLK_TRY(point_bytes_impl(curve, 1, db, nullptr, count, dp, dz, ds, c.stream()));
    std::vector<uint8_t> st(count);
    PLK_TRY(c.out(st.data(), ds, count));
    PLK_TRY(c.out(out_xy, dp, count * 2 * L * 8));
    PLK_TRY(c.out(out_zero, dz, count));
    PLK_TRY(c.finish());
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < count; ++i) {
        if (status) status[i] = st[i];
        if (st[i] && !bad++) first = i;
    }
    if (bad)
        return set_error(PLK_ERR_INVALID_ARG, "%zu of the %zu points do not decode (first: record %zu, %s)", bad, count, first,
                         st[first] == 1 ? "Out of range" : "Invalid x coordinate");
    return PLK_OK;
}

// ---- the BLAKE3 hash to the curve (hash_to_curve.hip): count first, id second (include/plonky_hip.h says why) ----
int plk_hash_to_curve_dev(size_t count, int curve, uint64_t seed_start, void* d_out_xy, void* stream) {
    PLK_API;
    return hash_to_curve_dev_impl(curve, 0, nullptr, seed_start, count, d_out_xy, nullptr, as_stream(stream));
}
int plk_hash_field_to_curve_dev(size_t count, int curve, const void* d_seeds, void* d_out_xy, void* stream) {
    PLK_API;
    return hash_to_curve_dev_impl(curve, 1, d_seeds, 0, count, d_out_xy, nullptr, as_stream(stream));
}
// the host-pointer forms: seeds == nullptr is the integer form
static int hash_to_curve_host(int curve, const uint64_t* seeds, int field_seeds, uint64_t seed_start, size_t count, uint64_t* out_xy) {
    PLK_TRY(hash_to_curve_check(curve, count));
    if (count == 0) return PLK_OK;
    if (!out_xy || (field_seeds && !seeds)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t coord = (size_t)curve_limbs(curve) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(seeds, count * coord);
    c.pin(out_xy, count * 2 * coord);
    void *dseeds = nullptr, *dp = nullptr, *ds = nullptr;
    if (field_seeds) PLK_TRY(c.in(dseeds, seeds, count * coord));
    PLK_TRY(c.tmp(dp, count * 2 * coord));
    PLK_TRY(c.tmp(ds, count));
    PLK_TRY(hash_to_curve_dev_impl(curve, field_seeds, dseeds, seed_start, count, dp, ds, c.stream()));
    std::vector<uint8_t> st(count);
    PLK_TRY(c.out(st.data(), ds, count));
    PLK_TRY(c.out(out_xy, dp, count * 2 * coord));
    PLK_TRY(c.finish());
    for (size_t k = 0; k < count; ++k)
        if (st[k])
            return set_error(PLK_ERR_INVALID_ARG, "seed %zu has no point: %s passed 255 (hash_to_curve.rs:%s)", k, st[k] == 1 ? "j" : "i", st[k] == 1 ? "48" : "74");
    return PLK_OK;
}
int plk_hash_to_curve(size_t count, int curve, uint64_t seed_start, uint64_t* out_xy) {
    PLK_API;
    return hash_to_curve_host(curve, nullptr, 0, seed_start, count, out_xy);
}
int plk_hash_field_to_curve(size_t count, int curve, const uint64_t* seeds, uint64_t* out_xy) {
    PLK_API;
    return hash_to_curve_host(curve, seeds, 1, 0, count, out_xy);
}
int plk_blake_field(size_t count, int field, const uint8_t* iters, const uint64_t* seeds, uint64_t* out_x, uint8_t* out_y_neg) {
    PLK_API;
    PLK_TRY(blake_field_check(field, count));
    if (count == 0) return PLK_OK;
    if (!iters || !seeds || !out_x || !out_y_neg) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t elem = (size_t)field_limbs(field) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *di = nullptr, *dseeds = nullptr, *dx = nullptr, *dy = nullptr, *ds = nullptr;
    PLK_TRY(c.in(di, iters, count));
    PLK_TRY(c.in(dseeds, seeds, count * elem));
    PLK_TRY(c.tmp(dx, count * elem));
    PLK_TRY(c.tmp(dy, count));
    PLK_TRY(c.tmp(ds, count));
    PLK_TRY(blake_field_dev_impl(field, di, dseeds, count, dx, dy, ds, c.stream()));
    std::vector<uint8_t> st(count);
    PLK_TRY(c.out(st.data(), ds, count));
    PLK_TRY(c.out(out_x, dx, count * elem));
    PLK_TRY(c.out(out_y_neg, dy, count));
    PLK_TRY(c.finish());
    for (size_t k = 0; k < count; ++k)
        if (st[k]) return set_error(PLK_ERR_INVALID_ARG, "seed %zu has no x: j passed 255 (hash_to_curve.rs:48)", k);
    return PLK_OK;
}

// ---- Rescue (rescue.hip): count or width first, context / field id second ----
int plk_rescue_create(size_t width, int field, size_t rounds, const uint64_t* constants, plk_rescue_ctx** out) {
    PLK_API;
    return rescue_create_impl(field, width, rounds, constants, out);
}
int plk_rescue_free(plk_rescue_ctx* ctx) {
    PLK_API;
    return rescue_free_impl(ctx);
}
int plk_rescue_rounds(size_t width, size_t security_bits, size_t* rounds) { return rescue_rounds_impl(width, security_bits, rounds); }
int plk_rescue_mds(size_t width, int field, uint64_t* out) {
    PLK_API;
    if (field_limbs(field) < 0) return set_error(PLK_ERR_INVALID_ARG, "bad field id %d", field);
    if (width != 4) return set_error(PLK_ERR_INVALID_ARG, "width %zu: the Rescue kernels are built for width 4 (RESCUE_SPONGE_WIDTH)", width);
    if (!out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t bytes = width * width * (size_t)field_limbs(field) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void* dm = nullptr;
    PLK_TRY(c.tmp(dm, bytes));
    PLK_TRY(rescue_mds_dev_impl(field, width, dm, c.stream()));
    PLK_TRY(c.out(out, dm, bytes));
    return c.finish();
}
int plk_rescue_permutation_dev(size_t count, const plk_rescue_ctx* ctx, const void* d_states, void* d_out, void* stream) {
    PLK_API;
    return rescue_permutation_dev_impl(count, ctx, d_states, d_out, as_stream(stream));
}
int plk_rescue_permutation(size_t count, const plk_rescue_ctx* ctx, const uint64_t* states, uint64_t* out) {
    PLK_API;
    PLK_TRY(rescue_check(count, ctx));
    if (count == 0) return PLK_OK;
    if (!states || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t bytes = count * 4 * (size_t)field_limbs(rescue_ctx_field(ctx)) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void* ds = nullptr;
    PLK_TRY(c.in(ds, states, bytes));
    PLK_TRY(rescue_permutation_dev_impl(count, ctx, ds, ds, c.stream()));
    PLK_TRY(c.out(out, ds, bytes));
    return c.finish();
}
int plk_rescue_sponge_dev(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, const void* d_inputs, size_t n_outputs, void* d_out, void* stream) {
    PLK_API;
    return rescue_sponge_dev_impl(count, ctx, n_inputs, d_inputs, n_outputs, d_out, as_stream(stream));
}
int plk_rescue_sponge(size_t count, const plk_rescue_ctx* ctx, size_t n_inputs, const uint64_t* inputs, size_t n_outputs, uint64_t* out) {
    PLK_API;
    PLK_TRY(rescue_sponge_check(count, ctx, n_inputs, n_outputs));
    if (count == 0) return PLK_OK;
    if ((n_inputs && !inputs) || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t elem = (size_t)field_limbs(rescue_ctx_field(ctx)) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *di = nullptr, *dout = nullptr;
    if (n_inputs) PLK_TRY(c.in(di, inputs, count * n_inputs * elem));
    PLK_TRY(c.tmp(dout, count * n_outputs * elem));
    PLK_TRY(rescue_sponge_dev_impl(count, ctx, n_inputs, di, n_outputs, dout, c.stream()));
    PLK_TRY(c.out(out, dout, count * n_outputs * elem));
    return c.finish();
}
int plk_field_kth_root_dev(size_t count, int field, uint32_t k, const void* d_in, void* d_out, void* stream) {
    PLK_API;
    return field_kth_root_dev_impl(count, field, k, d_in, d_out, as_stream(stream));
}
int plk_field_kth_root(size_t count, int field, uint32_t k, const uint64_t* in, uint64_t* out) {
    PLK_API;
    PLK_TRY(field_kth_root_check(count, field, k));
    if (count == 0) return PLK_OK;
    if (!in || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t bytes = count * (size_t)field_limbs(field) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void* dx = nullptr;
    PLK_TRY(c.in(dx, in, bytes));
    PLK_TRY(field_kth_root_dev_impl(count, field, k, dx, dx, c.stream()));
    PLK_TRY(c.out(out, dx, bytes));
    return c.finish();
}

// ---- the Rescue hash to the curve (rescue_h2c.hip): count first, context second ----
int plk_rescue_hash_to_curve_dev(size_t count, const plk_rescue_ctx* ctx, int curve, uint64_t seed_start, void* d_out_xy, void* stream) {
    PLK_API;
    return rescue_h2c_dev_impl(count, ctx, curve, 0, nullptr, seed_start, d_out_xy, nullptr, as_stream(stream));
}
int plk_rescue_hash_field_to_curve_dev(size_t count, const plk_rescue_ctx* ctx, int curve, const void* d_seeds, void* d_out_xy, void* stream) {
    PLK_API;
    return rescue_h2c_dev_impl(count, ctx, curve, 1, d_seeds, 0, d_out_xy, nullptr, as_stream(stream));
}
// the host-pointer forms: seeds == nullptr is the integer form
static int rescue_h2c_host(size_t count, const plk_rescue_ctx* ctx, int curve, const uint64_t* seeds, int field_seeds, uint64_t seed_start, uint64_t* out_xy) {
    PLK_TRY(rescue_h2c_check(count, ctx, curve));
    if (count == 0) return PLK_OK;
    if (!out_xy || (field_seeds && !seeds)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t coord = (size_t)curve_limbs(curve) * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    c.pin(seeds, count * coord);
    c.pin(out_xy, count * 2 * coord);
    void *dseeds = nullptr, *dp = nullptr, *ds = nullptr;
    if (field_seeds) PLK_TRY(c.in(dseeds, seeds, count * coord));
    PLK_TRY(c.tmp(dp, count * 2 * coord));
    PLK_TRY(c.tmp(ds, count));
    PLK_TRY(rescue_h2c_dev_impl(count, ctx, curve, field_seeds, dseeds, seed_start, dp, ds, c.stream()));
    std::vector<uint8_t> st(count);
    PLK_TRY(c.out(st.data(), ds, count));
    PLK_TRY(c.out(out_xy, dp, count * 2 * coord));
    PLK_TRY(c.finish());
    for (size_t k = 0; k < count; ++k)
        if (st[k]) return set_error(PLK_ERR_INVALID_ARG, "seed %zu has no point: i passed 255 (hash_to_curve.rs:84)", k);
    return PLK_OK;
}
int plk_rescue_hash_to_curve(size_t count, const plk_rescue_ctx* ctx, int curve, uint64_t seed_start, uint64_t* out_xy) {
    PLK_API;
    return rescue_h2c_host(count, ctx, curve, nullptr, 0, seed_start, out_xy);
}
int plk_rescue_hash_field_to_curve(size_t count, const plk_rescue_ctx* ctx, int curve, const uint64_t* seeds, uint64_t* out_xy) {
    PLK_API;
    return rescue_h2c_host(count, ctx, curve, seeds, 1, 0, out_xy);
}

// ---- gate witness rows (gate_trace.hip; include/plonky_hip_trace.h): count first, then the context or the shape and the curve id ----
int plk_trace_rescue_permutation_dev(size_t count, const plk_rescue_ctx* ctx, const void* d_inputs, size_t n_rows, void* d_wires, const void* d_first_rows,
                                     void* d_constants, void* d_status, void* stream) {
    PLK_API;
    return trace_rescue_dev_impl(count, ctx, d_inputs, n_rows, d_wires, d_first_rows, d_constants, d_status, as_stream(stream));
}
// the tables of a host-pointer trace call: up whole, written in place, down whole
struct TraceHostTables {
    void *dw = nullptr, *dk = nullptr, *df = nullptr, *dst = nullptr;
    size_t row = 0;
    int up(LaneCall& c, size_t count, size_t n_rows, uint64_t* wires, const uint32_t* first_rows, uint64_t* constants) {
        row = n_rows * 32;
        c.pin(wires, 9 * row);
        c.pin(constants, 6 * row);
        PLK_TRY(c.in(dw, wires, 9 * row));
        PLK_TRY(c.in_opt(dk, constants, 6 * row));
        PLK_TRY(c.in(df, first_rows, count * sizeof(uint32_t)));
        return c.tmp(dst, 4 * sizeof(uint32_t));
    }
    // the status words are on the host when this returns (st: 4 words of the caller's or of this frame)
    int down(LaneCall& c, uint64_t* wires, uint64_t* constants, uint32_t* st) {
        PLK_TRY(c.out(wires, dw, 9 * row));
        if (constants) PLK_TRY(c.out(constants, dk, 6 * row));
        return c.read(st, dst, 4 * sizeof(uint32_t));
    }
};
int plk_trace_rescue_permutation(size_t count, const plk_rescue_ctx* ctx, const uint64_t* inputs, size_t n_rows, uint64_t* wires, const uint32_t* first_rows,
                                 uint64_t* constants, uint32_t* status) {
    PLK_API;
    PLK_TRY(trace_rescue_check(count, ctx, n_rows));
    if (count == 0) return PLK_OK;
    if (!inputs) return set_error(PLK_ERR_INVALID_ARG, "null pointer: inputs");
    if (!wires) return set_error(PLK_ERR_INVALID_ARG, "null pointer: wires");
    if (!first_rows) return set_error(PLK_ERR_INVALID_ARG, "null pointer: first_rows");
    LaneCall c;
    PLK_TRY(c.begin());
    TraceHostTables t;
    void* di = nullptr;
    PLK_TRY(c.in(di, inputs, count * 4 * 32));
    PLK_TRY(t.up(c, count, n_rows, wires, first_rows, constants));
    PLK_TRY(trace_rescue_dev_impl(count, ctx, di, n_rows, t.dw, t.df, t.dk, t.dst, c.stream()));
    uint32_t st[4];
    PLK_TRY(t.down(c, wires, constants, st));
    if (status) memcpy(status, st, sizeof(st));
    return c.finish();
}
int plk_trace_curve_msm_dev(size_t count, unsigned parts, unsigned n_bits, int curve, const void* d_points, const void* d_scalars, const uint64_t* start_xy,
                            size_t n_rows, void* d_wires, const void* d_first_rows, void* d_constants, void* d_status, void* stream) {
    PLK_API;
    return trace_msm_dev_impl(count, parts, n_bits, curve, d_points, d_scalars, start_xy, n_rows, d_wires, d_first_rows, d_constants, d_status, as_stream(stream));
}
int plk_trace_curve_msm(size_t count, unsigned parts, unsigned n_bits, int curve, const uint64_t* points, const uint64_t* scalars, const uint64_t* start_xy,
                        size_t n_rows, uint64_t* wires, const uint32_t* first_rows, uint64_t* constants, uint32_t* status) {
    PLK_API;
    PLK_TRY(trace_msm_check(count, parts, n_bits, curve, start_xy, n_rows));
    if (count == 0) return PLK_OK;
    if (!points) return set_error(PLK_ERR_INVALID_ARG, "null pointer: points");
    if (!scalars) return set_error(PLK_ERR_INVALID_ARG, "null pointer: scalars");
    if (!wires) return set_error(PLK_ERR_INVALID_ARG, "null pointer: wires");
    if (!first_rows) return set_error(PLK_ERR_INVALID_ARG, "null pointer: first_rows");
    LaneCall c;
    PLK_TRY(c.begin());
    TraceHostTables t;
    void *dp = nullptr, *ds = nullptr;
    PLK_TRY(c.in(dp, points, count * parts * 2 * 32));
    PLK_TRY(c.in(ds, scalars, count * parts * 32));
    PLK_TRY(t.up(c, count, n_rows, wires, first_rows, constants));
    PLK_TRY(trace_msm_dev_impl(count, parts, n_bits, curve, dp, ds, start_xy, n_rows, t.dw, t.df, t.dk, t.dst, c.stream()));
    uint32_t st[4];
    PLK_TRY(t.down(c, wires, constants, st));
    if (status) memcpy(status, st, sizeof(st));
    if (st[1] == 0) return c.finish();
    // which case the first such instance met, off the rows it got back: no point of these curves has x = y = 0, so its first row
    // with wires 0 and 1 zero is where it stopped - an add row or a doubling row.  Row 0 is also where a scalar too long stops the
    // instance: that is the case when the first addend's x is not the starting point's (equal values are equal limbs).
    const uint32_t who = st[2], group = parts + 1;
    const uint64_t zero[4] = {0, 0, 0, 0};
    const uint64_t* block = wires + (size_t)first_rows[who] * 4;
    uint32_t k = 0;
    while (k + 1 < n_bits * group && (memcmp(block + (size_t)k * 4, zero, 32) || memcmp(block + (n_rows + k) * 4, zero, 32))) ++k;
    if (k == 0 && memcmp(points + (size_t)who * parts * 8, start_xy, 32))
        return c.refuse(PLK_ERR_INVALID_ARG, "scalar bit at or above n_bits %u: instance %u (%u instances met an exceptional case)", n_bits, who, st[1]);
    if (k % group == parts) return c.refuse(PLK_ERR_INVALID_ARG, "y = 0: instance %u, block row %u (curve_dbl.rs:157; %u instances met an exceptional case)", who, k, st[1]);
    return c.refuse(PLK_ERR_INVALID_ARG, "x_1 = x_2: instance %u, block row %u (curve_add.rs:244; %u instances met an exceptional case)", who, k, st[1]);
}

// ---- a point times a scalar of its own, the Halo endomorphism (scalar_mul.hip): count first, curve id second ----
int plk_curve_scalar_mul_dev(size_t count, int curve, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy, const void* d_p_zero,
                             void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    return curve_scalar_mul_dev_impl(count, curve, n_scalars, d_scalars, n_points, d_p_xy, d_p_zero, d_out_xy, d_out_zero, as_stream(stream));
}
int plk_halo_n_dev(size_t count, int curve, unsigned security_bits, const void* d_scalars, void* d_out, void* stream) {
    PLK_API;
    return halo_n_dev_impl(count, curve, security_bits, d_scalars, d_out, as_stream(stream));
}
int plk_halo_n_mul_dev(size_t count, int curve, unsigned security_bits, size_t n_scalars, const void* d_scalars, size_t n_points, const void* d_p_xy,
                       const void* d_p_zero, void* d_out_xy, void* d_out_zero, void* stream) {
    PLK_API;
    return halo_n_mul_dev_impl(count, curve, security_bits, n_scalars, d_scalars, n_points, d_p_xy, d_p_zero, d_out_xy, d_out_zero, as_stream(stream));
}
// the host-pointer form of the two point entries: security_bits == 0 selects plk_curve_scalar_mul
static int scalar_mul_host(size_t count, int curve, unsigned security_bits, size_t n_scalars, const uint64_t* scalars, size_t n_points, const uint64_t* p_xy,
                           const uint8_t* p_zero, uint64_t* out_xy, uint8_t* out_zero) {
    if (count == 0) return PLK_OK;
    if (!scalars || !p_xy || !out_xy || !out_zero) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    const size_t pt = (size_t)curve_limbs(curve) * 2 * 8;
    LaneCall c;
    PLK_TRY(c.begin());
    void *ds = nullptr, *dp = nullptr, *dz = nullptr, *dout = nullptr, *doz = nullptr;
    PLK_TRY(c.in(ds, scalars, n_scalars * 32));
    PLK_TRY(c.in(dp, p_xy, n_points * pt));
    PLK_TRY(c.in_opt(dz, p_zero, n_points));
    PLK_TRY(c.tmp(dout, count * pt));
    PLK_TRY(c.tmp(doz, count));
    if (security_bits) PLK_TRY(halo_n_mul_dev_impl(count, curve, security_bits, n_scalars, ds, n_points, dp, dz, dout, doz, c.stream()));
    else PLK_TRY(curve_scalar_mul_dev_impl(count, curve, n_scalars, ds, n_points, dp, dz, dout, doz, c.stream()));
    PLK_TRY(c.out(out_xy, dout, count * pt));
    PLK_TRY(c.out(out_zero, doz, count));
    return c.finish();
}
int plk_curve_scalar_mul(size_t count, int curve, size_t n_scalars, const uint64_t* scalars, size_t n_points, const uint64_t* p_xy, const uint8_t* p_zero,
                         uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    PLK_TRY(curve_scalar_mul_check(count, curve, n_scalars, n_points));
    return scalar_mul_host(count, curve, 0, n_scalars, scalars, n_points, p_xy, p_zero, out_xy, out_zero);
}
int plk_halo_n_mul(size_t count, int curve, unsigned security_bits, size_t n_scalars, const uint64_t* scalars, size_t n_points, const uint64_t* p_xy,
                   const uint8_t* p_zero, uint64_t* out_xy, uint8_t* out_zero) {
    PLK_API;
    PLK_TRY(halo_n_mul_check(count, curve, security_bits, n_scalars, n_points));
    return scalar_mul_host(count, curve, security_bits, n_scalars, scalars, n_points, p_xy, p_zero, out_xy, out_zero);
}
int plk_halo_n(size_t count, int curve, unsigned security_bits, const uint64_t* scalars, uint64_t* out) {
    PLK_API;
    PLK_TRY(halo_n_check(count, curve, security_bits));
    if (count == 0) return PLK_OK;
    if (!scalars || !out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;
    PLK_TRY(c.begin());
    void* ds = nullptr;
    PLK_TRY(c.in(ds, scalars, count * 32));
    PLK_TRY(halo_n_dev_impl(count, curve, security_bits, ds, ds, c.stream()));
    PLK_TRY(c.out(out, ds, count * 32));
    return c.finish();
}

// ---- scalar side of an IPA round ----
int plk_field_inner_product_dev(int field, const void* d_a, const void* d_b, size_t count, void* d_out, void* stream) {
    PLK_API;
    return field_inner_product_dev_impl(field, d_a, d_b, count, d_out, as_stream(stream));
}
int plk_field_fold_slices_dev(int field, const void* d_lo, const void* d_hi, const uint64_t* scalar_lo, const uint64_t* scalar_hi, size_t count,
                              void* d_out, void* stream) {
    PLK_API;
    return field_fold_slices_dev_impl(field, d_lo, d_hi, scalar_lo, scalar_hi, count, d_out, as_stream(stream));
}

// ---- one inner-product argument ----
int plk_halo_begin_dev(int curve, size_t n, const void* d_halo_a, const void* d_halo_b, const void* d_halo_g_xy, const void* d_halo_g_zero,
                       const uint64_t* pedersen_h_xy, const uint64_t* u_prime_xy, unsigned freeze_log, void* stream, plk_halo_ctx** out_ctx) {
    PLK_API;
    return halo_begin_dev_impl(curve, n, d_halo_a, d_halo_b, d_halo_g_xy, d_halo_g_zero, pedersen_h_xy, u_prime_xy, freeze_log, as_stream(stream), out_ctx);
}
int plk_halo_begin_tabled_dev(int curve, size_t n, const void* d_halo_a, const void* d_halo_b, const void* d_halo_g_xy, const void* d_halo_g_zero,
                              plk_msm_ctx* pedersen_g_tables, const uint64_t* pedersen_h_xy, const uint64_t* u_prime_xy, size_t h_index, size_t u_index,
                              const uint64_t* u_prime_scalar, unsigned freeze_log, unsigned lead_rounds, void* stream, plk_halo_ctx** out_ctx) {
    PLK_API;
    if (!pedersen_g_tables) return set_error(PLK_ERR_INVALID_ARG, "null tables");
    // the argument runs on the calling thread's device, on `stream`; the tables must live there too.  A device-group context
    // (plk_init_devices) is kept on logical device 0 whatever thread built it: open over it from a thread on that device
    PLK_TRY(ensure_device());
    int cur = -1;
    PLK_HIP_TRY(hipGetDevice(&cur));
    if (cur != msm_ctx_device(pedersen_g_tables))
        return set_error(PLK_ERR_INVALID_ARG, "the commitment tables live on HIP device %d but the calling thread works on device %d%s", msm_ctx_device(pedersen_g_tables),
                         cur, msm_ctx_is_multi(pedersen_g_tables) ? " (a device-group context is kept on logical device 0: plk_set_thread_device(0))" : "");
    return halo_begin_dev_impl(curve, n, d_halo_a, d_halo_b, d_halo_g_xy, d_halo_g_zero, pedersen_h_xy, u_prime_xy, freeze_log, as_stream(stream), out_ctx,
                               pedersen_g_tables, lead_rounds, h_index, u_index, u_prime_scalar);
}
int plk_curve_fold_multi_dev(int curve, size_t n_out, unsigned log_inputs, const void* d_g_xy, const void* d_g_zero, const void* d_scalars, void* d_out_xy,
                             void* d_out_zero, void* stream) {
    PLK_API;
    return curve_fold_multi_dev_impl(curve, n_out, (int)log_inputs, d_g_xy, d_g_zero, d_scalars, d_out_xy, d_out_zero, as_stream(stream));
}
int plk_halo_begin(int curve, size_t n, const uint64_t* halo_a, const uint64_t* halo_b, const uint64_t* halo_g_xy, const uint8_t* halo_g_zero,
                   const uint64_t* pedersen_h_xy, const uint64_t* u_prime_xy, unsigned freeze_log, plk_halo_ctx** out_ctx) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (!halo_a || !halo_b || !halo_g_xy) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    LaneCall c;  // registers nothing
    PLK_TRY(c.begin());
    void *da = nullptr, *db = nullptr, *dg = nullptr, *dz = nullptr;
    PLK_TRY(c.in(da, halo_a, n * 32));
    PLK_TRY(c.in(db, halo_b, n * 32));
    PLK_TRY(c.in(dg, halo_g_xy, n * 2 * L * 8));
    PLK_TRY(c.in_opt(dz, halo_g_zero, n));
    // the context works on the lane's stream from here on (one host thread per context)
    PLK_TRY(halo_begin_dev_impl(curve, n, da, db, dg, dz, pedersen_h_xy, u_prime_xy, freeze_log, c.stream(), out_ctx));
    return c.finish();
}
int plk_halo_round_lr(plk_halo_ctx* ctx, const uint64_t* l_blinding, const uint64_t* r_blinding, uint64_t* lr_xy, uint8_t* lr_zero) {
    PLK_API;
    return halo_round_lr_impl(ctx, l_blinding, r_blinding, lr_xy, lr_zero);
}
int plk_halo_round_fold(plk_halo_ctx* ctx, const uint64_t* u_j, const uint64_t* u_j_inv) { PLK_API; return halo_round_fold_impl(ctx, u_j, u_j_inv); }
size_t plk_halo_len(const plk_halo_ctx* ctx) { return halo_len_impl(ctx); }
int plk_halo_frozen(const plk_halo_ctx* ctx) { return halo_frozen_impl(ctx); }
int plk_halo_read(plk_halo_ctx* ctx, uint64_t* halo_a, uint64_t* halo_b, uint64_t* halo_g_xy, uint8_t* halo_g_zero) {
    PLK_API;
    return halo_read_impl(ctx, halo_a, halo_b, halo_g_xy, halo_g_zero);
}
int plk_halo_free(plk_halo_ctx* ctx) {
    PLK_API;
    if (!ctx) return set_error(PLK_ERR_INVALID_ARG, "null context");
    halo_delete(ctx);
    return PLK_OK;
}

// ---- self-test ----
// (this entry, plk_curve_op, plk_msm_debug_digits and plk_curve_gen_bases_dev keep DevBuf and blocking copies: their impls take no stream)
int plk_selftest_quad(int curve, const uint64_t* pts_xy, size_t n, unsigned quads, unsigned* mismatches) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (!pts_xy || !mismatches || n == 0 || n > 0xffffffffu) return set_error(PLK_ERR_INVALID_ARG, "bad argument");
    PLK_TRY(ensure_device());
    DevBuf dp;
    PLK_TRY(dp.alloc(n * 2 * L * 8));
    PLK_HIP_TRY(hipMemcpy(dp.p, pts_xy, n * 2 * L * 8, hipMemcpyHostToDevice));
    return selftest_quad_dev_impl(curve, dp.p, (uint32_t)n, quads, mismatches);
}

// ---- checked build ----
int plk_checked_build(void) { return checked_build_impl(); }
int plk_checked_failures(unsigned* counts) { PLK_API; return checked_failures_impl(counts); }

// ---- measurement hooks ----
int plk_ntt_set_profiling(int enable) { return ntt_set_profiling_impl(enable); }
int plk_ntt_get_timings(double* sum_ms, unsigned* launches) { PLK_API; return ntt_get_timings_impl(sum_ms, launches); }
// A device-group context runs its executions on its per-device parts (full tables on every device, a share context per device):
// the handle's own stage events would stay empty - refused instead of returning stale or empty numbers.
static int refuse_group_profiling(plk_msm_ctx* ctx) {
    if (msm_ctx_is_multi(ctx))
        return set_error(PLK_ERR_INVALID_ARG, "per-stage timings are collected on one-device contexts only: a device-group context executes on its per-device parts");
    return PLK_OK;
}
int plk_msm_set_profiling(plk_msm_ctx* ctx, int enable) {
    if (enable) PLK_TRY(refuse_group_profiling(ctx));
    return msm_set_profiling_impl(ctx, enable);
}
int plk_msm_get_timings(plk_msm_ctx* ctx, double* sum_ms, unsigned* calls) {
    PLK_API;
    PLK_TRY(refuse_group_profiling(ctx));
    return msm_get_timings_impl(ctx, sum_ms, calls);
}

// ---- utilities ----
int plk_msm_debug_digits(int curve, unsigned window_bits, size_t n, const uint64_t* scalars, int32_t* digits, unsigned* n_digits) {
    PLK_API;
    const int nd = msm_debug_digit_count(curve, window_bits);
    if (nd < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d or window of %u bits", curve, window_bits);
    if (n_digits) *n_digits = (unsigned)nd;
    if (!digits || !n) return PLK_OK;
    if (!scalars) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    PLK_TRY(ensure_device());
    DevBuf ds, dd;
    PLK_TRY(ds.alloc(n * 32));
    PLK_TRY(dd.alloc(n * (size_t)nd * 4));
    PLK_HIP_TRY(hipMemcpy(ds.p, scalars, n * 32, hipMemcpyHostToDevice));
    PLK_TRY(msm_debug_digits_impl(curve, window_bits, n, ds.p, dd.p, nullptr));
    PLK_HIP_TRY(hipDeviceSynchronize());
    PLK_HIP_TRY(hipMemcpy(digits, dd.p, n * (size_t)nd * 4, hipMemcpyDeviceToHost));
    return PLK_OK;
}

int plk_bench_ceilings(double* out, unsigned n_out) { PLK_API; return bench_ceilings_impl(out, n_out); }

int plk_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
    PLK_API;
    return field_op_impl(field, op, a, b, out, count);
}

int plk_curve_op(int curve, int op, unsigned param, size_t count, const uint64_t* a_xy, const uint8_t* a_zero, const uint64_t* a_lambda, const uint64_t* b_xy,
                 const uint8_t* b_zero, const uint64_t* b_lambda, const uint8_t* flags, uint64_t* out_xy, uint8_t* out_zero, unsigned* mismatch) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (op < 0 || op > 8) return set_error(PLK_ERR_INVALID_ARG, "bad curve op %d", op);
    if (count > 2048) return set_error(PLK_ERR_INVALID_ARG, "%zu elements (at most 2048 per call)", count);
    if (op == 6 && (param < 1 || param > 24)) return set_error(PLK_ERR_INVALID_ARG, "%u doublings (1..24)", param);
    if (op == 7 && !(param == 1 || param == 2 || param == 4 || param == 8 || param == 16)) return set_error(PLK_ERR_INVALID_ARG, "groups of %u quads (1, 2, 4, 8, 16)", param);
    if (!mismatch) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    *mismatch = 0;
    if (count == 0) return PLK_OK;
    const bool has_b = op == 0 || op == 2 || op == 4 || op == 5 || op == 8, b_affine = op == 4 || op == 5;
    if (!a_xy || !a_lambda || !flags || !out_xy || !out_zero || (has_b && (!b_xy || (!b_affine && !b_lambda)))) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    PLK_TRY(ensure_device());
    const size_t results = op == 7 ? (count + param - 1) / param : count, pt = (size_t)2 * L * 8;
    DevBuf da, daz, dal, db, dbz, dbl, df, dout, doz, dm;
    auto up = [&](DevBuf& d, const void* src, size_t bytes) -> int {
        PLK_TRY(d.alloc(bytes));
        PLK_HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return PLK_OK;
    };
    PLK_TRY(up(da, a_xy, count * pt));
    PLK_TRY(up(dal, a_lambda, count * pt / 2));
    PLK_TRY(up(df, flags, count));
    if (a_zero) PLK_TRY(up(daz, a_zero, count));
    if (has_b) PLK_TRY(up(db, b_xy, count * pt));
    if (has_b && !b_affine) PLK_TRY(up(dbl, b_lambda, count * pt / 2));
    if (has_b && b_zero) PLK_TRY(up(dbz, b_zero, count));
    PLK_TRY(dout.alloc(results * pt));
    PLK_TRY(doz.alloc(results));
    PLK_TRY(dm.alloc(4));
    PLK_HIP_TRY(hipMemset(dm.p, 0, 4));
    PLK_TRY(curve_op_dev_impl(curve, op, param, (uint32_t)count, da.p, daz.p, dal.p, db.p, dbz.p, dbl.p, df.p, dout.p, doz.p, dm.p));
    PLK_HIP_TRY(hipMemcpy(out_xy, dout.p, results * pt, hipMemcpyDeviceToHost));
    PLK_HIP_TRY(hipMemcpy(out_zero, doz.p, results, hipMemcpyDeviceToHost));
    PLK_HIP_TRY(hipMemcpy(mismatch, dm.p, 4, hipMemcpyDeviceToHost));
    return PLK_OK;
}

int plk_curve_gen_bases_dev(int curve, size_t n, uint64_t first, const uint64_t* g0_xy, const uint64_t* d_xy, void* d_out_xy, void* stream) {
    PLK_API;
    const int L = curve_limbs(curve);
    if (L < 0) return set_error(PLK_ERR_INVALID_ARG, "bad curve id %d", curve);
    if (!g0_xy || !d_xy || (n && !d_out_xy)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    PLK_TRY(ensure_device());
    DevBuf dg;
    PLK_TRY(dg.alloc(4 * L * 8));
    PLK_HIP_TRY(hipMemcpy(dg.p, g0_xy, 2 * L * 8, hipMemcpyHostToDevice));
    PLK_HIP_TRY(hipMemcpy((uint8_t*)dg.p + 2 * L * 8, d_xy, 2 * L * 8, hipMemcpyHostToDevice));
    PLK_TRY(curve_gen_bases_dev_impl(curve, n, first, dg.p, d_out_xy, as_stream(stream)));
    PLK_HIP_TRY(hipStreamSynchronize(as_stream(stream)));  // dg is freed on return
    return PLK_OK;
}

}  // extern "C"
