// dispatch.cuh -- from a run-time PLK_FIELD_* id to code instantiated on the field's parameter struct (field_params.cuh).
// The one place that lists the fields; the curves' twin, with_curve, sits with the curve structs in ec.cuh.  Plain C++17: hipcc and
// g++ (hostnorm.cpp, polydiv_host.cpp) both include it.
//
//   return with_field(field, [&](auto t) { using P = tag_t<decltype(t)>; return field_op_t<P>(op, a, b, out, count); });
//
// f is a generic lambda that returns int and is instantiated once per listed type.  An id outside the list never reaches f:
// the dispatcher returns PLK_NO_MATCH, and the call site turns that into its own error text (common.h: or_bad_field, or_bad_curve).
#pragma once
#include <climits>

#include "field_params.cuh"

namespace plk {

constexpr int PLK_NO_MATCH = INT_MIN;  // no PLK_ERR_* code (include/plonky_hip.h: -1 .. -7), no count a visitor returns

template <class T> struct TypeTag { using type = T; };
template <class Tag> using tag_t = typename Tag::type;

// the six fields, in the order of their ids (P::FIELD_ID is the PLK_FIELD_* value)
#define PLK_FOR_EACH_FIELD(X) \
    X(TweedledeeBaseParams) X(TweedledumBaseParams) X(Bls12377ScalarParams) X(Bls12377BaseParams) X(PallasBaseParams) X(VestaBaseParams)

template <class F> int with_field(int field, F&& f) {
#define PLK_FIELD_CASE(P) \
    if (field == P::FIELD_ID) return f(TypeTag<P>{});
    PLK_FOR_EACH_FIELD(PLK_FIELD_CASE)
#undef PLK_FIELD_CASE
    return PLK_NO_MATCH;
}

// the 4-limb fields only (the circuit scalar fields: what the NTT, polynomial and Plonk kernels are instantiated on); f is not
// instantiated on the 6-limb base field of BLS12-377
template <class F> int with_field4(int field, F&& f) {
    return with_field(field, [&](auto t) {
        if constexpr (tag_t<decltype(t)>::NL == 8) return f(t);
        else return PLK_NO_MATCH;
    });
}

}  // namespace plk
