// host_only.h -- entry points of the two translation units built by the host compiler without HIP (hostnorm.cpp,
// polydiv_host.cpp).  No HIP type appears here: the .cpp files and their callers (through common.h) include the same lines.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace plk {

// hostnorm.cpp: ProjectivePoint::to_affine on the host for `count` points (x | y | z -> x | y).  curve: PLK_CURVE_*; -1 for an unknown one
int host_projective_to_affine(int curve, unsigned count, const uint8_t* xyz, const uint8_t* zero, uint8_t* xy);
// polydiv_host.cpp: host-only field work of a low-degree division (polydiv.hip).  field: a 4-limb PLK_FIELD_*; -1 for another one
int host_pdiv_prepare(int field, const uint64_t* b, size_t lb, uint64_t* negb, uint64_t* factor);
int host_poly_from_roots(int field, unsigned k, const uint64_t* roots, uint64_t* out);

}  // namespace plk
