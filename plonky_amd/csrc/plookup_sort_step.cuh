// plookup_sort_step.cuh -- the lane-level steps of the Plookup sorted multiset (plookup_sort.hip), kept apart from the kernels so that
// tests/plookup_sort_host_replay.cpp walks the same code on the host.  Plain C++17, no field arithmetic: a row is the 8 words of an
// element in the reference's stored form, and equality of rows is equality of the words (what the reference's == compares).
//
// The table over t: open addressing, 2N slots of 32 bits for N rows (load at most 1/2), a slot holds an index into t or PSORT_EMPTY.
// All rows of one value meet in ONE slot: a row claims the first empty slot of its probe sequence or stops at the first slot whose
// row equals its own, slots never change hands, and a slot that was passed was held by another value.  The slot ends at the smallest
// index among its rows - position() of plookup.rs:173 - whatever the order the rows arrive in; WHICH slot a value takes depends on
// that order, the index in it does not.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PSORT_HD __host__ __device__ __forceinline__
#else
#define PSORT_HD inline
#endif

namespace plk {

constexpr uint32_t PSORT_EMPTY = 0xFFFFFFFFu;
constexpr int PSORT_LANES = 256;                             // lanes of a workgroup of the insert, scan and expansion kernels
constexpr int PSORT_ROWS = 4;                                // counts a lane of the scan owns (one 16-byte access)
constexpr int PSORT_TILE = PSORT_LANES * PSORT_ROWS;         // counts a workgroup of the scan owns
constexpr int PSORT_CHUNK = PSORT_LANES;                     // tile totals the single workgroup of the tile scan takes per step
constexpr int PSORT_COUNT_LANES = 1024;                      // lanes of a workgroup of the count kernel
constexpr int PSORT_COUNT_SLOTS = 2 * PSORT_COUNT_LANES;     // slots of its table in LDS (load at most 1/2)

struct SortRow {
    uint32_t w[8];
};

PSORT_HD bool psort_row_eq(const SortRow& a, const SortRow& b) {
    uint32_t d = 0;
    for (int k = 0; k < 8; ++k) d |= a.w[k] ^ b.w[k];
    return d == 0;
}

PSORT_HD uint32_t psort_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// MurmurHash3 (x86, 32 bit; public domain) over the 32 bytes of a row: every word goes through two multiplications and the final
// avalanche, so rows that differ in one word only ([i,0,..,0], [0,..,0,i], counters in Montgomery form) spread over the slots
PSORT_HD uint32_t psort_hash(const SortRow& r) {
    uint32_t h = 0x9747B28Cu;
    for (int k = 0; k < 8; ++k) {
        uint32_t x = r.w[k] * 0xCC9E2D51u;
        x = psort_rotl(x, 15) * 0x1B873593u;
        h = psort_rotl(h ^ x, 13) * 5u + 0xE6546B64u;
    }
    h ^= 32u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// the count kernel's table in LDS is keyed by an index into t (Fibonacci hashing: consecutive indices land apart)
PSORT_HD uint32_t psort_hash_index(uint32_t i) { return (i * 0x9E3779B1u) >> 16; }

PSORT_HD uint32_t psort_next(uint32_t h, uint32_t mask) { return (h + 1) & mask; }

// Row i of t enters the table.  ops: load(h) (a read that sees other lanes' atomics), cas(h, expected, value) -> the old value,
// lower(h, value) (atomic minimum); row_at(s): row s of t.  The slot is READ first and the atomic issued only when i is smaller.
// Returns the number of slots visited (at most mask + 1: the table is never full).
template <class Ops, class RowAt> PSORT_HD uint32_t psort_insert(Ops& ops, RowAt row_at, uint32_t i, const SortRow& row, uint32_t mask) {
    uint32_t h = psort_hash(row) & mask;
    for (uint32_t probes = 1; probes <= mask; ++probes, h = psort_next(h, mask)) {
        uint32_t s = ops.load(h);
        if (s == PSORT_EMPTY) {
            s = ops.cas(h, PSORT_EMPTY, i);
            if (s == PSORT_EMPTY) return probes;
        }
        if (s == i) return probes;
        if (psort_row_eq(row_at(s), row)) {
            if (i < s) ops.lower(h, i);
            return probes;
        }
    }
    return mask + 1;
}

// the representative (first occurrence in t) of a row, PSORT_EMPTY when t does not hold it; load(h): a plain read of slot h
template <class Load, class RowAt> PSORT_HD uint32_t psort_lookup(Load load, RowAt row_at, const SortRow& row, uint32_t mask, uint32_t* probes = nullptr) {
    uint32_t h = psort_hash(row) & mask, rep = PSORT_EMPTY, k = 1;
    for (; k <= mask; ++k, h = psort_next(h, mask)) {
        const uint32_t s = load(h);
        if (s == PSORT_EMPTY) break;
        if (psort_row_eq(row_at(s), row)) {
            rep = s;
            break;
        }
    }
    if (probes) *probes = k;
    return rep;
}

// the row of t that output row j repeats: the LAST i < rows with off(i) <= j (off: the exclusive scan of the counts, off(0) = 0;
// rows with a count of zero share their successor's offset and are stepped over).  The caller compares j with the total.
template <class Off> PSORT_HD uint32_t psort_find(Off off, uint32_t rows, uint32_t j) {
    uint32_t lo = 0, hi = rows - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off(mid) <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace plk
