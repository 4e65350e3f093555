/* plonky_hip_trace.h -- C ABI of the gate witness rows: the blocks of rows that the in-circuit Rescue permutation and the in-circuit
 * MSM (curve_msm) lay down, written into the prover's wire table on the device.
 *
 * A header of its own next to plonky_hip.h and plonky_hip_witness.h, for the reason the witness header gives: the entries of
 * plonky_hip.h form a pinned set.  The conventions, the PLK_* status codes and the field / curve ids are those of plonky_hip.h, which
 * this header includes; the four entries live in the same library (libplonky_hip.so and its checked twin).
 *
 * The reference generates these rows one generator at a time inside generate_partial_witness (witness.rs), which runs to a fixed point
 * over the copy constraints; that iteration stays on the host.  The two gadgets here are fixed chains of rows per instance,
 * independent across instances: a caller hands over each instance's inputs and the row its block starts at.
 */
#ifndef PLONKY_HIP_TRACE_H
#define PLONKY_HIP_TRACE_H

#include "plonky_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- common to both entries ----------------------------------------------------------------------------------------------------------
 * The count comes first, then the context or the shape and the curve id.  Elements are canonical Montgomery form, 4 x u64.
 *
 *   n_rows        gate rows of the table, 1 .. 2^27 (a power of two where plk_plonk_check_witness_dev is to read it; not needed here).
 *   d_wires       wire_values_by_wire_index, [9][n_rows] elements: wire j of row i is element j n_rows + i.  The layout
 *                 plk_plonk_check_witness_dev and the NTT batch read.  Written IN PLACE: rows outside the blocks, and wires of a
 *                 block row that its gate does not define, are not touched.
 *   d_first_rows  uint32[count]: the first row of each instance's block.  Overlapping blocks are the caller's error and undefined.
 *   d_constants   nullable; [6][n_rows] elements at stride 1 (the n-point columns of the witness check).  When given, the entry also
 *                 writes the gate constants of its block rows: the gate's prefix (as the code has it: the PREFIX of each gate file) in the first
 *                 columns and, for the Rescue gates, the round constants in columns 2..5.  Columns past a gate's prefix that the gate
 *                 does not read are not touched.
 *   d_status      nullable; device, 4 x uint32, initialised and written in stream order:
 *                   [0] instances refused because first_row + block_rows > n_rows (compared in 64 bits): nothing of them is written
 *                   [1] instances that met an exceptional case (curve_msm only; see there)
 *                   [2] the smallest such instance index, 0xFFFFFFFF when there is none        [3] zero
 *                 Integer atomics: the words are the same whatever the order of execution.
 *   stream        hipStream_t as void*; the _dev forms are asynchronous on it and do not synchronise.
 *
 * The host-pointer forms go through the calling thread's lane: the tables travel to the device, are written there in place and
 * travel back whole; status (nullable) is 4 words of host memory.
 */

/* ---- the in-circuit Rescue permutation  (circuit_builder.rs:931-970; rescue_a.rs:116-155, rescue_b.rs generate) ---------------------
 * ctx: a plk_rescue_ctx; its rounds and constants are the gadget's.  d_inputs: count x 4 elements.  A block is 2 rounds + 1 rows.
 * For instance c with first row r and round k < rounds:
 *   row r + 2k      RescueStepAGate: wires 0..3 the state entering the round, wires 4..7 its four fifth roots (kth_root_u32(5))
 *   row r + 2k + 1  RescueStepBGate: wires 0..3 MDS roots + the step-A constants
 *   the next A row, or the receiving row r + 2 rounds (a BufferGate): wires 0..3 MDS (state^5) + the step-B constants
 * so wires 0..3 of row r + 2 rounds are plk_rescue_permutation of the input.  Wire 8 of an A row and wires 4..8 of the other rows
 * are not touched.  Constants: A rows prefix 00 and the four step-A constants in columns 2..5, B rows prefix 01 and the step-B
 * constants, the receiving row the BufferGate prefix 101000.  There is no exceptional case: status [1] = 0, [2] = 0xFFFFFFFF.
 *
 * Refusals, PLK_ERR_INVALID_ARG before anything is launched or copied, in this order (plk_last_error() starts with the quoted text):
 *   "null context"                      ctx is null
 *   "count C"                           count > 2^32 - 1
 *   "field F has 6 limbs"               a context over PLK_FIELD_BLS12_377_BASE
 *   "field F: Rescue exponent 11"       a context over PLK_FIELD_BLS12_377_SCALAR: the gates hard-code exp_usize(5)
 *   "n_rows R"                          n_rows = 0 or n_rows > 2^27
 * then count == 0 is PLK_OK and launches nothing; then
 *   "null pointer: inputs"   "null pointer: wires"   "null pointer: first_rows"
 * then PLK_ERR_NO_DEVICE without a device, a context of another device (as plk_rescue_permutation_dev), PLK_ERR_HIP from the runtime. */
int plk_trace_rescue_permutation_dev(size_t count, const plk_rescue_ctx* ctx, const void* d_inputs, size_t n_rows, void* d_wires, const void* d_first_rows,
                                     void* d_constants, void* d_status, void* stream);
int plk_trace_rescue_permutation(size_t count, const plk_rescue_ctx* ctx, const uint64_t* inputs, size_t n_rows, uint64_t* wires, const uint32_t* first_rows,
                                 uint64_t* constants, uint32_t* status);

/* ---- the in-circuit MSM  (circuit_curve.rs:287-410 curve_msm; curve_add.rs:173-262, curve_dbl.rs generate) ---------------------------
 * curve: the INNER curve; the wires live in its base field, so the curves are those whose base field has 4 limbs (Tweedledee,
 * Tweedledum, Pallas, Vesta).  d_points: count x parts affine points (x || y); d_scalars: count x parts elements of that same base
 * field, read through their canonical form (part.scalar.convert() as the builder splits it).  1 <= parts <= 8;
 * 1 <= n_bits <= BITS - 1 (the builder's f_bits is BITS - 1; a shorter chain is the same gadget for a bounded scalar).  start_xy: the
 * host affine starting accumulator (the builder's `filler`), 8 x u64.  A block is n_bits (parts + 1) rows.  For bit i from
 * n_bits - 1 down to 0:
 *   `parts` CurveAddGate rows: wires 0/1 the accumulator, 2 scalar_acc_old, 3 scalar_acc_new, 4/5 the addend, 6 the bit, 7 the inverse
 *   of x1 - x2, 8 lambda; inverse and lambda are computed whether or not the bit is set, as the generator does
 *   one CurveDblGate row: wires 0/1 the accumulator after the last add, 2/3 its double, 4 the inverse of 2 y, 5 lambda (InnerC::A = 0
 *   on these curves); wires 6..8 are not touched
 * The next group's first add row takes the doubled point.  The doubled point of the last group is still written (the gate is there);
 * the result, sum s_j P_j + 2^(n_bits - 1) start, is that row's wires 0/1.  Constants: prefix 10101 on the add rows, 10111 on the
 * doubling rows, columns 0..4; column 5 is not touched.
 *
 * Exceptional cases: a scalar with a bit set at or above n_bits (found before the first row); x1 = x2 in an add row (the reference
 * panics "x_1 = x_2"); y = 0 in a doubling ("y = 0").  The instance is counted in status [1]; its rows from that one on are written
 * as zero (every wire its gate defines); its constants are written as for any other instance.  For the _dev form that is a RESULT:
 * PLK_OK.  The host-pointer form returns PLK_ERR_INVALID_ARG for the first such instance, the text starting with the reference's
 * panic text ("x_1 = x_2" / "y = 0") or with "scalar bit"; the tables and the status are written all the same.
 *
 * Refusals, PLK_ERR_INVALID_ARG before anything is launched or copied, in this order:
 *   "bad curve id"                      an unknown curve id
 *   "curve C has a 6-limb base field"   PLK_CURVE_BLS12_377
 *   "count C"                           count > 2^32 - 1
 *   "parts P"                           parts outside 1 .. 8
 *   "n_bits B"                          n_bits outside 1 .. BITS - 1
 *   "n_rows R"                          n_rows = 0 or n_rows > 2^27
 *   "null pointer: start_xy"
 * then count == 0 is PLK_OK and launches nothing; then
 *   "null pointer: points"   "null pointer: scalars"   "null pointer: wires"   "null pointer: first_rows"
 * then PLK_ERR_NO_DEVICE without a device, PLK_ERR_HIP from the runtime. */
int plk_trace_curve_msm_dev(size_t count, unsigned parts, unsigned n_bits, int curve, const void* d_points, const void* d_scalars, const uint64_t* start_xy,
                            size_t n_rows, void* d_wires, const void* d_first_rows, void* d_constants, void* d_status, void* stream);
int plk_trace_curve_msm(size_t count, unsigned parts, unsigned n_bits, int curve, const uint64_t* points, const uint64_t* scalars, const uint64_t* start_xy,
                        size_t n_rows, uint64_t* wires, const uint32_t* first_rows, uint64_t* constants, uint32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* PLONKY_HIP_TRACE_H */
