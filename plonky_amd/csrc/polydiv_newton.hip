// polydiv_newton.hip -- Polynomial::inv_mod_xn (polynomial.rs:261-294) and Polynomial::polynomial_division (polynomial.rs:299-327) for
// a divisor of ANY degree, on device-resident coefficients, asynchronous: every size follows from la, lb, n alone and nothing is read
// back.  polydiv.hip keeps the recurrence route for divisors of degree 1..32 held on the host.  The inverse, the quotient and the
// remainder are unique and every stored word is fully reduced: the words are the reference's.
//
// With m = la - k and h = rev(b) mod X^m (h_0 = b_k):  g = 1 / h mod X^m,  rev(q) = g rev(a) mod X^m,  rem = a - q b mod X^k.
//
//   seed     g mod X^64 by the triangular recurrence, 1 / h_0 by fp.cuh's inversion: one wave (k_pinv_seed).
//   level    l -> t = min(2 l, n):  g (2 - h g) = 2 g - g^2 h, which below X^l is g again, so g_t = -(g^2 h)_t for l <= t < 2 l.
//            Two zero-padded forward transforms of N = 4 l points (g: l coefficients; h mod X^t), the pointwise G^2 H
//            (k_pinv_pointwise), one inverse transform, and k_pinv_update on [l, t).  deg g^2 h <= 4 l - 3 < N: nothing wraps.
//            Three transforms per level; the reference runs nine (three Polynomial::mul) and builds three tables.
//   reversal no reversed array is made.  The chunk B = b[k + 1 - t' .. k], t' = min(t, k + 1), IS h mod X^t backwards:
//            h(X) = X^(t' - 1) B(1 / X), and B(1 / w^i) = FFT(B)[-i mod N].  So the level multiplies by FFT(B) read at the negated
//            index and gets g^2 h rotated down by t' - 1, which k_pinv_update undoes on its loads (pinv_shift_index).
//   quotient q_s = sum_i g_i A_(i + s) with A = a[k .. la) (the top m coefficients): a correlation, FFT(g)[-i] FFT(A)[i], on
//            N >= 2 m - 1 points; for s < m no index pair wraps.  k_pinv_quotient copies q and fills the zeros up to q_len.
//   rem      (q mod X^k) (b mod X^k) on N >= min(m, k) + k - 1 points, then k_pinv_rem: a_i - (q b)_i, i < k.
// The evaluations of g (of q for the remainder) leave their transform in R'-form through its store hook, as in Polynomial::mul
// (poly.hip), so a pointwise product is two (one) 29-bit-limb products and ends in the reference's form (polyinv_step.cuh).
// Products run on at least 2^8 points: the smallest size the Newton levels use.
#include "common.h"
#include "fp.cuh"
#include "fz.cuh"
#include "polyinv_step.cuh"
#include "tables.cuh"

namespace plk {

constexpr int PINV_LANES = 256;
constexpr int PINV_MIN_LOG = PINV_SEED_LOG + 2;  // the first Newton level's transform
constexpr int PINV_MAX_LOG = 30;                 // ntt_dev_impl's largest transform

// g[0 .. cnt) of the series whose coefficient j is src[pinv_series_index(j)]; cst[0] = R' / R in R'-form (the store hook's factor);
// a zero h_0 ORs `bit` into *status (g is then all zero: nothing downstream depends on its value for addresses).  One wave.
template <class P>
__global__ void __launch_bounds__(PINV_SEED) k_pinv_seed(const uint4* __restrict__ src, size_t len, int reversed, int cnt, uint4* __restrict__ g,
                                                         uint4* __restrict__ cst, uint32_t* __restrict__ status, uint32_t bit) {
    constexpr int W = P::NL / 4;
    __shared__ uint4 s_h[PINV_SEED * W], s_g[PINV_SEED * W];
    const int t = threadIdx.x;
    size_t idx = 0;
    const Fe<P> h_t = t < cnt && pinv_series_index(reversed != 0, len, (size_t)t, idx) ? fe_load<P>(src + idx * W) : fe_zero<P>();
    fe_store<P>(s_h + t * W, h_t);
    __syncthreads();
    const Fe<P> h0 = fe_load<P>(s_h);
    const Fe<P> inv = fe_inv_safegcd<P>(h0), neg_inv = fe_neg<P>(inv);
    if (t == 0) {
        fe_store<P>(cst, to_rprime<P>(fz_to_fe_canonical<P>(fz_one_rprime<P>())));
        if (status && fe_is_zero<P>(h0)) status[0] |= bit;
    }
    Fe<P> acc = fe_zero<P>();
    for (int i = 0; i < cnt; ++i) {
        if (t == i) {
            const Fe<P> gi = pinv_seed_coeff<P>((size_t)i, acc, inv, neg_inv);
            fe_store<P>(s_g + i * W, gi);
            fe_store<P>(g + (size_t)i * W, gi);
        }
        __syncthreads();
        if (t > i && t < cnt) acc = pinv_seed_accumulate<P>(acc, fe_load<P>(s_h + (t - i) * W), fe_load<P>(s_g + i * W));
    }
}

// out[i] = X[i]^2 Y[+-i] (SQUARE: a Newton level) or X[+-i] Y[i] (a product); X in R'-form.  out may be X (SQUARE) or Y (product):
// a lane reads the aliased array at its own index only.
template <class P, bool SQUARE>
__global__ void __launch_bounds__(PINV_LANES) k_pinv_pointwise(const uint4* x, const uint4* y, uint4* out, size_t n, int negate) {
    constexpr int W = P::NL / 4;
    const size_t i = (size_t)blockIdx.x * PINV_LANES + threadIdx.x;
    if (i >= n) return;
    const size_t o = negate ? pinv_neg_index(i, n) : i;
    if constexpr (SQUARE) fe_store<P>(out + i * W, pinv_newton_point<P>(fe_load<P>(x + i * W), fe_load<P>(y + o * W)));
    else fe_store<P>(out + i * W, pinv_product_point<P>(fe_load<P>(x + o * W), fe_load<P>(y + i * W)));
}

// g[t] = -(g^2 h)[t] for from <= t < to; the product's coefficients are rotated down by `shift`
template <class P>
__global__ void __launch_bounds__(PINV_LANES) k_pinv_update(const uint4* __restrict__ prod, size_t n, size_t shift, uint4* __restrict__ g, size_t from, size_t to) {
    constexpr int W = P::NL / 4;
    const size_t t = from + (size_t)blockIdx.x * PINV_LANES + threadIdx.x;
    if (t >= to) return;
    fe_store<P>(g + t * W, pinv_update_coeff<P>(fe_load<P>(prod + pinv_shift_index(t, shift, n) * W)));
}

template <class P>
__global__ void __launch_bounds__(PINV_LANES) k_pinv_quotient(const uint4* __restrict__ prod, size_t m, uint4* __restrict__ q, size_t q_len) {
    constexpr int W = P::NL / 4;
    const size_t s = (size_t)blockIdx.x * PINV_LANES + threadIdx.x;
    if (s >= q_len) return;
    size_t src = 0;
    fe_store<P>(q + s * W, pinv_quotient_index(s, m, src) ? fe_load<P>(prod + src * W) : fe_zero<P>());
}

template <class P>
__global__ void __launch_bounds__(PINV_LANES) k_pinv_rem(const uint4* __restrict__ a, const uint4* __restrict__ prod, size_t k, uint4* __restrict__ rem) {
    constexpr int W = P::NL / 4;
    const size_t i = (size_t)blockIdx.x * PINV_LANES + threadIdx.x;
    if (i >= k) return;
    fe_store<P>(rem + i * W, pinv_rem_coeff<P>(fe_load<P>(a + i * W), fe_load<P>(prod + i * W)));
}

// ---- host side ----
static unsigned pinv_grid(size_t count) { return (unsigned)((count + PINV_LANES - 1) / PINV_LANES); }

static int pinv_log2_ceil(size_t v) {
    int l = 0;
    while (l < 63 && ((size_t)1 << l) < v) ++l;
    return l;
}
// log2 of the largest Newton transform of an inverse mod X^n (0: the seed is all of it)
static int pinv_newton_log(size_t n) {
    if (n <= (size_t)PINV_SEED) return 0;
    int lg = PINV_SEED_LOG;
    while (((size_t)2 << lg) < n) ++lg;  // the last level starts from l = 2^lg, the largest SEED 2^j below n
    return lg + 2;
}
static int pinv_product_log(size_t len) {
    const int l = pinv_log2_ceil(len);
    return l < PINV_MIN_LOG ? PINV_MIN_LOG : l;
}
static int pinv_transform_check(int field, int log_size, const char* what) {
    const int adicity = with_field4(field, [](auto t) { return (int)tag_t<decltype(t)>::TWO_ADICITY; });
    if (log_size > adicity || log_size > PINV_MAX_LOG)
        return set_error(PLK_ERR_INVALID_ARG, "%s needs a transform of 2^%d points: beyond the field's 2-adicity %d or the largest transform 2^%d", what, log_size,
                         adicity, PINV_MAX_LOG);
    return PLK_OK;
}
static bool ranges_overlap(const void* x, size_t xb, const void* y, size_t yb) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + yb && b < a + xb;
}

struct PinvSeries {  // the series to invert: coefficient j is p[pinv_series_index(reversed, len, j)]
    const uint4* p;
    size_t len;
    bool reversed;
};

// a forward transform of 2^log_size points of in[0 .. in_len), zero-padded; rprime: the evaluations leave in R'-form
static int pinv_forward(int field, int log_size, const uint4* in, size_t in_len, uint4* out, const uint4* cst, bool rprime, hipStream_t stream) {
    NttHooks h;
    h.in_len = in_len;
    h.in_stride = in_len;
    if (rprime) {
        h.out_tab = cst;
        h.out_mask = 0;
    }
    return ntt_dev_hooked_impl(field, (unsigned)log_size, 0, 1, in, out, h, stream);
}

// g = 1 / series mod X^n into g[0 .. n); ev_x, ev_y: 2^pinv_newton_log(n) elements each
template <class P>
static int pinv_inverse_t(const PinvSeries& s, size_t n, uint4* g, uint4* ev_x, uint4* ev_y, uint4* cst, uint32_t* status, uint32_t bit, hipStream_t stream) {
    const int cnt = n < (size_t)PINV_SEED ? (int)n : PINV_SEED;
    k_pinv_seed<P><<<1, PINV_SEED, 0, stream>>>(s.p, s.len, s.reversed ? 1 : 0, cnt, g, cst, status, bit);
    int log_l = PINV_SEED_LOG;
    for (size_t l = PINV_SEED; l < n; l *= 2, ++log_l) {
        const size_t t = n - l < l ? n : 2 * l, tp = t < s.len ? t : s.len, size = 4 * l;
        const uint4* chunk = s.reversed ? s.p + (s.len - tp) * 2 : s.p;
        PLK_TRY(pinv_forward(P::FIELD_ID, log_l + 2, g, l, ev_x, cst, true, stream));
        PLK_TRY(pinv_forward(P::FIELD_ID, log_l + 2, chunk, tp, ev_y, cst, false, stream));
        k_pinv_pointwise<P, true><<<pinv_grid(size), PINV_LANES, 0, stream>>>(ev_x, ev_y, ev_x, size, s.reversed ? 1 : 0);
        PLK_TRY(ntt_dev_impl(P::FIELD_ID, (unsigned)(log_l + 2), 1, 1, ev_x, ev_x, stream));
        k_pinv_update<P><<<pinv_grid(t - l), PINV_LANES, 0, stream>>>(ev_x, size, s.reversed ? tp - 1 : 0, g, l, t);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "series inverse launch (seed, pointwise or update) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

static int pinv_field_check(int field) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    return PLK_OK;
}

int poly_inv_mod_xn_check(size_t n, int field, size_t lh) {
    PLK_TRY(pinv_field_check(field));
    if (n < 1 || lh < 1) return set_error(PLK_ERR_INVALID_ARG, "inverse mod X^%zu of %zu coefficients: n >= 1 and lh >= 1 are required", n, lh);
    if (n > ((size_t)1 << PINV_MAX_LOG)) return pinv_transform_check(field, pinv_log2_ceil(n) + 1, "the inverse");
    return pinv_transform_check(field, pinv_newton_log(n), "the inverse");
}

int poly_inv_mod_xn_dev_impl(size_t n, int field, const void* d_h, size_t lh, void* d_out, uint32_t* d_status, hipStream_t stream) {
    PLK_TRY(poly_inv_mod_xn_check(n, field, lh));
    if (!d_h || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer: h / out");
    if (lh > n) lh = n;  // the surplus is never read
    if (ranges_overlap(d_out, n * 32, d_h, lh * 32)) return set_error(PLK_ERR_INVALID_ARG, "out must not overlap h (h is read at every level)");
    PLK_TRY(ensure_device());
    return with_field4(field, [&](auto tag) {
        using P = tag_t<decltype(tag)>;
        const size_t ev = (size_t)1 << pinv_newton_log(n);
        ScratchSet ss(stream);
        uint4 *ev_x = (uint4*)ss.get(ev * 32), *ev_y = (uint4*)ss.get(ev * 32), *cst = (uint4*)ss.get(32);
        if (!ev_x || !ev_y || !cst) return (int)PLK_ERR_OOM;  // scratch_acquire has set the error text
        return pinv_inverse_t<P>({(const uint4*)d_h, lh, false}, n, (uint4*)d_out, ev_x, ev_y, cst, d_status, PINV_STATUS_NO_INVERSE, stream);
    });
}

int poly_div_rem_check(size_t la, int field, size_t lb, size_t q_len, bool want_rem) {
    PLK_TRY(pinv_field_check(field));
    if (lb < 2) return set_error(PLK_ERR_INVALID_ARG, "divisor of %zu coefficients: a degree of at least 1 is required", lb);
    const size_t k = lb - 1;
    if (la <= k) return set_error(PLK_ERR_INVALID_ARG, "a has %zu coefficients: more than the divisor's degree %zu are required", la, k);
    const size_t m = la - k;
    if (q_len < m) return set_error(PLK_ERR_INVALID_ARG, "q_len %zu is below la - k = %zu", q_len, m);
    if (la > ((size_t)1 << PINV_MAX_LOG)) return pinv_transform_check(field, pinv_log2_ceil(la), "the division");
    PLK_TRY(pinv_transform_check(field, pinv_newton_log(m), "the inverse of the reversed divisor"));
    PLK_TRY(pinv_transform_check(field, pinv_product_log(2 * m - 1), "the quotient"));
    if (want_rem) PLK_TRY(pinv_transform_check(field, pinv_product_log((m < k ? m : k) + k - 1), "the remainder"));
    return PLK_OK;
}

template <class P>
static int pdiv_newton_t(const uint4* a, size_t la, const uint4* b, size_t lb, uint4* q, size_t q_len, uint4* rem, uint32_t* status, hipStream_t stream) {
    const size_t k = lb - 1, m = la - k, lq = m < k ? m : k;
    const int log_q = pinv_product_log(2 * m - 1), log_r = rem ? pinv_product_log(lq + k - 1) : 0, log_g = pinv_newton_log(m);
    const int log_ev = log_q > log_r ? (log_q > log_g ? log_q : log_g) : (log_r > log_g ? log_r : log_g);
    ScratchSet ss(stream);
    uint4 *g = (uint4*)ss.get(m * 32), *ev_x = (uint4*)ss.get(((size_t)32) << log_ev), *ev_y = (uint4*)ss.get(((size_t)32) << log_ev), *cst = (uint4*)ss.get(32);
    if (!g || !ev_x || !ev_y || !cst) return PLK_ERR_OOM;  // scratch_acquire has set the error text
    PLK_TRY(pinv_inverse_t<P>({b, lb, true}, m, g, ev_x, ev_y, cst, status, PINV_STATUS_ZERO_LEAD, stream));
    // q_s = sum_i g_i a_(k + i + s)
    PLK_TRY(pinv_forward(P::FIELD_ID, log_q, g, m, ev_x, cst, true, stream));
    PLK_TRY(pinv_forward(P::FIELD_ID, log_q, a + k * 2, m, ev_y, cst, false, stream));
    k_pinv_pointwise<P, false><<<pinv_grid((size_t)1 << log_q), PINV_LANES, 0, stream>>>(ev_x, ev_y, ev_y, (size_t)1 << log_q, 1);
    PLK_TRY(ntt_dev_impl(P::FIELD_ID, (unsigned)log_q, 1, 1, ev_y, ev_y, stream));
    k_pinv_quotient<P><<<pinv_grid(q_len), PINV_LANES, 0, stream>>>(ev_y, m, q, q_len);
    if (rem) {
        PLK_TRY(pinv_forward(P::FIELD_ID, log_r, q, lq, ev_x, cst, true, stream));
        PLK_TRY(pinv_forward(P::FIELD_ID, log_r, b, k, ev_y, cst, false, stream));
        k_pinv_pointwise<P, false><<<pinv_grid((size_t)1 << log_r), PINV_LANES, 0, stream>>>(ev_x, ev_y, ev_y, (size_t)1 << log_r, 0);
        PLK_TRY(ntt_dev_impl(P::FIELD_ID, (unsigned)log_r, 1, 1, ev_y, ev_y, stream));
        k_pinv_rem<P><<<pinv_grid(k), PINV_LANES, 0, stream>>>(a, ev_y, k, rem);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "polynomial division launch (pointwise, quotient or remainder) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

int poly_div_rem_dev_impl(size_t la, int field, const void* d_a, const void* d_b, size_t lb, void* d_q, size_t q_len, void* d_rem, uint32_t* d_status,
                          hipStream_t stream) {
    PLK_TRY(poly_div_rem_check(la, field, lb, q_len, d_rem != nullptr));
    if (!d_a || !d_b || !d_q) return set_error(PLK_ERR_INVALID_ARG, "null pointer: a / b / q");
    const size_t k = lb - 1;
    if (ranges_overlap(d_q, q_len * 32, d_a, la * 32) || ranges_overlap(d_q, q_len * 32, d_b, lb * 32))
        return set_error(PLK_ERR_INVALID_ARG, "q must not overlap a or b (both are read after q is written)");
    if (d_rem && (ranges_overlap(d_rem, k * 32, d_a, la * 32) || ranges_overlap(d_rem, k * 32, d_b, lb * 32) || ranges_overlap(d_rem, k * 32, d_q, q_len * 32)))
        return set_error(PLK_ERR_INVALID_ARG, "the remainder must not overlap a, b or q");
    PLK_TRY(ensure_device());
    return with_field4(field, [&](auto tag) {
        return pdiv_newton_t<tag_t<decltype(tag)>>((const uint4*)d_a, la, (const uint4*)d_b, lb, (uint4*)d_q, q_len, (uint4*)d_rem, d_status, stream);
    });
}

}  // namespace plk
