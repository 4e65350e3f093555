// witness_step.cuh -- the lane-level steps of the witness check (plonk.hip: k_check_rows, k_check_first, k_check_copies) that hold no
// field arithmetic: the neighbour rows of a gate, what a routed wire's sigma entry makes its lane do, and the rule by which a wave
// merges its lanes' findings into the report.  Kept apart from the kernels so that tests/check_witness_host_replay.cpp walks the
// same code on the host.  Plain C++17.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WITNESS_HD __host__ __device__ __forceinline__
#else
#define WITNESS_HD inline
#endif

namespace plk {

constexpr uint32_t WITNESS_GRID_WIDTH = 65;      // GRID_WIDTH (plonk.rs:25)
constexpr uint32_t WITNESS_ROUTED = 6;           // NUM_ROUTED_WIRES (plonk.rs:22)
constexpr uint32_t WITNESS_NONE = 0xFFFFFFFFu;   // report words [1] and [4] when nothing failed (no row or wire id reaches it: n <= 2^27)
constexpr int WITNESS_REPORT_WORDS = 8;
// the report: [0] failing rows, [1] first failing row, [2] its mask, [3] mismatching wires, [4] first mismatching wire, [5] sigma
// entries >= 6n, [6], [7] zero
enum WitnessWord : int { WITNESS_BAD_ROWS = 0, WITNESS_FIRST_ROW, WITNESS_FIRST_MASK, WITNESS_BAD_COPIES, WITNESS_FIRST_COPY, WITNESS_SIGMA_RANGE };

// the report before any launch
WITNESS_HD uint32_t witness_report_init(int word) { return word == WITNESS_FIRST_ROW || word == WITNESS_FIRST_COPY ? WITNESS_NONE : 0u; }

// The rows a gate reads besides its own, on the subgroup of n = 2^log_n rows (plonk.rs:408-409 there): right is row i + 1, below is row
// i + GRID_WIDTH, both mod n.  n is a power of two, so the remainder is a mask - for n <= 64 the below index wraps more than once, which
// one conditional subtraction would miss.
WITNESS_HD uint32_t witness_right(uint32_t i, unsigned log_n) { return (i + 1u) & ((1u << log_n) - 1u); }
WITNESS_HD uint32_t witness_below(uint32_t i, unsigned log_n) { return (i + WITNESS_GRID_WIDTH) & ((1u << log_n) - 1u); }

// what the lane of routed wire w does with s = sigma[w]: s is compared with 6n before it indexes anything
enum WitnessCopy : int { WITNESS_COPY_SELF = 0, WITNESS_COPY_COMPARE, WITNESS_COPY_OUT_OF_RANGE };
WITNESS_HD WitnessCopy witness_copy_class(uint32_t w, uint32_t s, unsigned log_n) {
    if (s >= (WITNESS_ROUTED << log_n)) return WITNESS_COPY_OUT_OF_RANGE;  // counted in word [5], not followed
    return s == w ? WITNESS_COPY_SELF : WITNESS_COPY_COMPARE;              // a wire equals itself: no load
}

// A wave's share of (count, first): `flagged` has bit k set iff lane k found something, and the lanes hold consecutive ids starting at
// `base`, so the smallest flagged id is base + the lowest set bit.  The wave then adds `count` to one report word and takes the minimum
// of `first` into the next - integer operations whose result does not depend on the order the waves arrive in.
struct WitnessWave {
    uint32_t count, first;
};
WITNESS_HD WitnessWave witness_wave_merge(uint64_t flagged, uint32_t base) {
    if (!flagged) return {0u, WITNESS_NONE};
    return {(uint32_t)__builtin_popcountll(flagged), base + (uint32_t)__builtin_ctzll(flagged)};
}
// the same merge applied to a report word pair (what atomicAdd / atomicMin do, replayed on the host)
WITNESS_HD void witness_report_merge(uint32_t& count_word, uint32_t& first_word, const WitnessWave& w) {
    count_word += w.count;
    if (w.first < first_word) first_word = w.first;
}

}  // namespace plk
