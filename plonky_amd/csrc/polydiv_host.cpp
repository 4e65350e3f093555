// polydiv_host.cpp -- the host-only field work of the low-degree polynomial division (polydiv.hip), plain C++ over fp.cuh like
// hostnorm.cpp: the divisor made monic (one inversion, skipped when it is monic already) and the product of the linear factors
// prod (X - s_i) of the public-input denominator (plonk.rs:207-215), at most k^2 / 2 products for k <= 32 roots.
#include <cstring>

#include "dispatch.cuh"
#include "fp.cuh"
#include "host_only.h"

namespace plk {

// b: lb coefficients, b[lb - 1] != 0, lb - 1 <= 32.  negb[i] = -b[i] / lead, i < lb - 1; factor = 1 / lead (1 for a monic b): what
// the quotient of the division by b / lead is multiplied by.  R-form words in and out.
template <class P> static void prepare_t(const uint64_t* b, size_t lb, uint64_t* negb, uint64_t* factor) {
    constexpr size_t B = (size_t)P::NL * 4;
    const size_t k = lb - 1;
    Fe<P> lead;
    memcpy(lead.v, b + 4 * k, B);
    const bool monic = fe_eq<P>(lead, fe_one<P>());
    const Fe<P> inv = monic ? fe_one<P>() : fe_inv_safegcd_var<P>(lead);
    for (size_t i = 0; i < k; ++i) {
        Fe<P> c;
        memcpy(c.v, b + 4 * i, B);
        const Fe<P> n = fe_neg<P>(monic ? c : fe_mul<P>(c, inv));
        memcpy(negb + 4 * i, n.v, B);
    }
    memcpy(factor, inv.v, B);
}

// out[0..k] = coefficients of prod_{i < k} (X - roots[i]): monic, [1] for k = 0
template <class P> static void from_roots_t(unsigned k, const uint64_t* roots, uint64_t* out) {
    constexpr size_t B = (size_t)P::NL * 4;
    Fe<P> c[33];
    c[0] = fe_one<P>();
    for (unsigned n = 0; n < k; ++n) {  // c has n + 1 coefficients; times (X - r)
        Fe<P> r;
        memcpy(r.v, roots + 4 * n, B);
        c[n + 1] = c[n];
        for (unsigned j = n; j >= 1; --j) c[j] = fe_sub<P>(c[j - 1], fe_mul<P>(r, c[j]));
        c[0] = fe_neg<P>(fe_mul<P>(r, c[0]));
    }
    for (unsigned j = 0; j <= k; ++j) memcpy(out + 4 * j, c[j].v, B);
}

// field: PLK_FIELD_* (include/plonky_hip.h), the five 4-limb fields.  Return 0, or -1 for another field.
int host_pdiv_prepare(int field, const uint64_t* b, size_t lb, uint64_t* negb, uint64_t* factor) {
    const int rc = with_field4(field, [&](auto t) {
        prepare_t<tag_t<decltype(t)>>(b, lb, negb, factor);
        return 0;
    });
    return rc == PLK_NO_MATCH ? -1 : rc;
}
int host_poly_from_roots(int field, unsigned k, const uint64_t* roots, uint64_t* out) {
    const int rc = with_field4(field, [&](auto t) {
        from_roots_t<tag_t<decltype(t)>>(k, roots, out);
        return 0;
    });
    return rc == PLK_NO_MATCH ? -1 : rc;
}

}  // namespace plk
