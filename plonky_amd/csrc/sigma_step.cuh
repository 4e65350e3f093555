// sigma_step.cuh -- the lane-level steps of the copy-constraint permutation (sigma.hip), kept apart from the kernels so that
// tests/sigma_host_replay.cpp walks the same code on the host.  Plain C++17, no field arithmetic.
//
// The wire partitions (partition.rs:84-87, the live ones) arrive in CSR form: members[M] holds wire ids input * n + gate (the
// reference's own sigma indexing, partition.rs:132, extended to all NUM_WIRES inputs), offsets[P + 1] the start of every partition.
// A slot p of members is one lane: its partition by bisection, its neighbour slot by get_neighbor's (i + 1) % len
// (partition.rs:108-118), and the class of the pair (id, neighbour id) that decides what the lane stores and counts.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SIGMA_HD __host__ __device__ __forceinline__
#else
#define SIGMA_HD inline
#endif

namespace plk {

constexpr int SIGMA_LANES = 256;              // lanes (member slots) of a workgroup
constexpr uint32_t SIGMA_ROUTED = 6;          // NUM_ROUTED_WIRES (plonk.rs:22)
constexpr uint32_t SIGMA_WIRES = 9;           // NUM_WIRES (plonk.rs:21)
constexpr uint32_t SIGMA_UNSET = 0xFFFFFFFFu;  // a sigma entry no slot has written (no id reaches it: ids are below 9 * 2^27)
constexpr uint32_t SIGMA_BAD = 0xFFFFFFFEu;    // written for a routed wire whose neighbour's id is out of range

// the partition of slot p: the LAST q in [lo, hi] with off(q) <= p (off(lo) <= p is the caller's; empty partitions share their
// successor's offset and are stepped over, so the q found is never an empty one when p < off(hi + 1))
template <class Off> SIGMA_HD uint32_t sigma_find(Off off, uint32_t lo, uint32_t hi, uint32_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off(mid) <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// get_neighbor (partition.rs:113): the slot after p inside [begin, end), wrapping to begin.  With a sound offsets array the result is
// below num_members; with any other it is forced there (p itself), so that no input makes a lane read outside members.
SIGMA_HD uint32_t sigma_neighbour(uint32_t p, uint32_t begin, uint32_t end, uint32_t num_members) {
    const uint32_t nb = (p + 1 < end) ? p + 1 : begin;
    return nb < num_members ? nb : p;
}

// id = input * n + gate, n = 2^log_n
SIGMA_HD uint32_t sigma_input(uint32_t id, unsigned log_n) { return id >> log_n; }
SIGMA_HD uint32_t sigma_gate(uint32_t id, unsigned log_n) { return id & ((1u << log_n) - 1u); }

// what a slot does, from its id, its neighbour's id x and the length of its partition; every id is compared with its bound here,
// before anything is indexed by it
struct SigmaSlot {
    bool out_of_range;  // id >= 9n: status word [2]; nothing else happens
    bool lonely;        // a non-routed wire in a partition of more than one member: status word [1] (assert_valid, partition.rs:90-102)
    bool routed;        // id < 6n: one listing of a routed wire, sigma[id] is written
    bool value;         // ... and x < 6n too: s_sigma[id] = k_is[x / n] g^(x % n) is written
    uint32_t sigma;     // what sigma[id] receives: x, or SIGMA_BAD when x >= 9n
};
SIGMA_HD SigmaSlot sigma_classify(uint32_t id, uint32_t x, uint32_t len, unsigned log_n) {
    const uint32_t n = 1u << log_n;
    SigmaSlot s{false, false, false, false, SIGMA_BAD};
    if (id >= SIGMA_WIRES * n) {
        s.out_of_range = true;
        return s;
    }
    if (id >= SIGMA_ROUTED * n) {
        s.lonely = len > 1;
        return s;
    }
    s.routed = true;
    if (x < SIGMA_WIRES * n) s.sigma = x;
    s.value = x < SIGMA_ROUTED * n;
    return s;
}

// status word [0]: routed wires not listed exactly once = missing ones + surplus listings, from the number of routed listings
// and the number of sigma entries left unwritten: the distinct wires listed are 6n - unset, the surplus listings - (6n - unset).
// Unsigned arithmetic modulo 2^32, the way the kernels' atomic additions meet it: word[0] starts at -6n.
SIGMA_HD uint32_t sigma_status0(uint32_t listings, uint32_t unset, unsigned log_n) {
    return 0u - SIGMA_ROUTED * (1u << log_n) + listings + 2u * unset;
}

}  // namespace plk
