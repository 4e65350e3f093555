/* plonky_hip_witness.h -- C ABI of the witness check: which gate a witness does not satisfy, which routed wire differs from its copy.
 *
 * A header of its own next to plonky_hip.h: the entries of plonky_hip.h form a pinned set, and these two were added after it.  The
 * conventions, the PLK_* status codes and the field ids are those of plonky_hip.h, which this header includes; the two entries live in
 * the same library (libplonky_hip.so and its checked twin).
 */
#ifndef PLONKY_HIP_WITNESS_H
#define PLONKY_HIP_WITNESS_H

#include "plonky_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the witness check  (src/plonk.rs:158-167, debug builds of the reference only) ------------------------------------------------ */
/* The reference evaluates the degree-8n vanishing polynomial at each of the n subgroup points (O(n^2)) and panics with
 * "{}-th gate constraints are not satisfied".  Here the unified constraint set (evaluate_all_constraints, gates/mod.rs:46-125) is
 * evaluated at the n rows themselves, straight off the tables the prover holds, and the copy constraints are checked wire by wire;
 * the L_1 and Z terms of the vanishing polynomial are not part of it (Z is the prover's own output: status word [1] of
 * plk_plonk_permutation_z_dev is its wrap check).  n = 2^log_degree; like the sigma and Plookup entries these two take the SIZE first
 * and the field id second.  Fields: the 4-limb circuit scalar fields.  Elements are canonical Montgomery form, 4 x u64.
 *
 * Arguments
 *   log_degree        n = 2^log_degree gate rows, log_degree <= 27.
 *   field             PLK_FIELD_*, a 4-limb circuit scalar field.
 *   d_constants       [6][n * constants_stride] elements; constant j of row i is element (j n + i) constants_stride.
 *   constants_stride  8 takes constants_8n (the values over the 8n domain) as it is, one point in eight; 1 the n-point columns.
 *   d_wires           wire_values_by_wire_index, [9][n] elements.  Row i reads its own 9 wires, wires 0..3 of row (i + 1) mod n (right)
 *                     and wires 2, 3 of row (i + 65) mod n (below; plonk.rs:408-409 on the subgroup).
 *   d_sigma           nullable; uint32[6n], the return value of to_sigma (plk_plonk_sigma_dev): sigma[w] for wire id
 *                     w = input * n + gate, the flat index into d_wires.  Null: the copy check is skipped, words [3]..[5] are zero.
 *   inner_zeta        host scalar, InnerC::ZETA of CurveEndoGate, as for plk_plonk_vanishing_points_dev.
 *   inner_a           host scalar, InnerC::A of CurveDblGate.
 *   d_report          device, 8 x uint32, initialised and written in stream order (see below).
 *   d_row_masks       nullable; device, uint8[n]: bit t of mask i is set iff term t of the unified constraint set of row i - the SUM of
 *                     the ten gates' filtered constraints t, reduced to the unique representative - is nonzero.
 *   d_first_terms     nullable; device, 8 elements, canonical Montgomery form: the eight terms of the first failing row, what
 *                     plk_plonk_evaluate_all_constraints returns for that row; zeros when no row fails.
 *   stream            hipStream_t as void*; everything is asynchronous on it, on the calling thread's device.
 *
 * The report
 *   [0] rows whose mask is nonzero                  [1] the smallest such row, 0xFFFFFFFF when there is none
 *   [2] the mask of that row (0 when there is none)
 *   [3] routed wires w < 6n with sigma[w] < 6n whose 32 bytes differ from the 32 bytes at sigma[w] (elements are canonical by
 *       contract: equal values are equal words)     [4] the smallest such w, 0xFFFFFFFF when there is none
 *   [5] entries sigma[w] >= 6n: compared with 6n before they index anything, counted, not followed
 *   [6], [7] zero
 * The counts and minima are integer atomics over waves: the report is the same whatever the order of execution.
 *
 * A witness that fails is a RESULT, not an error: the return value is PLK_OK and the report says what failed.
 *
 * Refusals, PLK_ERR_INVALID_ARG before anything is launched or copied, in this order (plk_last_error() starts with the quoted text):
 *   "bad field id"                      an unknown field id
 *   "field F has 6 limbs"               a six-limb field (PLK_FIELD_BLS12_377_BASE)
 *   "log_degree L"                      log_degree > 27
 *   "constants_stride S"                a stride other than 1 or 8
 *   "null pointer: constants"           (d_)constants is null
 *   "null pointer: wires"               (d_)wires is null
 *   "null pointer: report"              (d_)report is null
 *   "null pointer: inner_zeta"          inner_zeta is null
 *   "null pointer: inner_a"             inner_a is null
 * then PLK_ERR_NO_DEVICE without a device, PLK_ERR_OOM / PLK_ERR_HIP from the runtime.  The first call for a field builds a small cached
 * table (the inverses 1/1 .. 1/7 of the MDS matrix and the table of the input conversion). */
int plk_plonk_check_witness_dev(unsigned log_degree, int field, const void* d_constants, unsigned constants_stride, const void* d_wires, const void* d_sigma,
                                const uint64_t* inner_zeta, const uint64_t* inner_a, void* d_report, void* d_row_masks, void* d_first_terms, void* stream);
/* Same with host pointers, through the calling thread's lane: report 8 words, row_masks (nullable) n bytes, first_terms (nullable)
 * 8 elements, sigma (nullable) 6n words.  With constants_stride 8 the n elements of each constants row are gathered on the host first,
 * so 6 n elements cross PCIe in either form.  Same refusals, same PLK_OK for a witness that fails. */
int plk_plonk_check_witness(unsigned log_degree, int field, const uint64_t* constants, unsigned constants_stride, const uint64_t* wires, const uint32_t* sigma,
                            const uint64_t* inner_zeta, const uint64_t* inner_a, uint32_t* report, uint8_t* row_masks, uint64_t* first_terms);

#ifdef __cplusplus
}
#endif

#endif /* PLONKY_HIP_WITNESS_H */
