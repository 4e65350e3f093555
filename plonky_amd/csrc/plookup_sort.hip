// plookup_sort.hip -- the sorted multiset of the Plookup prover on the device: s = f ++ t ordered by the position of each value's first
// occurrence in t (plookup/src/plookup.rs:20-22 and sort_by, 171-177).
//
// Rows with the same key hold the same value, so s is fixed by counts alone: for each row i of t that is the first occurrence of its
// value, c_i = #{j < n : f_j = t_i} + #{k < N : t_k = t_i}, and s is t_i repeated c_i times in order of i.  No field arithmetic, no
// comparison sort:
//   k_sort_insert   a table over t (plookup_sort_step.cuh): every value's slot ends at its first row
//   k_sort_count    every row of f[0..n) and of t finds its representative and adds 1 to cnt[rep]; rows of f outside t are counted
//   k_sort_tiles    sums of the counts per tile of PSORT_TILE rows               \  the exclusive scan of the N counts
//   k_sort_scan     the exclusive scan of the tile sums, the status words         >  (an integer scan: the scans of lz.cuh are
//   k_sort_offsets  off[i] = tile prefix + prefix inside the tile                /   product scans)
//   k_sort_expand   one lane per row j of s: the i with off[i] <= j < off[i+1] by bisection, then t_i as two 16-byte accesses
// pad_inputs (plookup.rs:155-167) pads f and t with ZERO, so one value fills a large share of f and a long run of t.  No lane's work
// grows with a value's multiplicity: the insert drops a row that repeats its predecessor and lets the lanes of a wave that hold equal
// rows elect the first; the count gathers a workgroup's additions in LDS and sends ONE atomic per (workgroup, representative); the
// expansion is per output row.  The counts are integers and a slot's final index is a minimum, so s is bit-identical from run to run.
#include "common.h"
#include "plookup_sort_step.cuh"

namespace plk {

// -DPLK_CHECKED (libplonky_hip_checked.so): every index read from the table or found by the bisection is compared with its bound; a
// violation is counted (site 7 of plk_checked_failures) and the access skipped
#ifdef PLK_CHECKED
static __device__ unsigned g_sort_chk[8];
#define PSORT_CHK(cond) (!(cond) ? (atomicAdd(&g_sort_chk[7], 1u), false) : true)
int plookup_sort_checked_failures(unsigned* counts) {
    PLK_HIP_TRY(hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_sort_chk), 8 * sizeof(unsigned)));
    return PLK_OK;
}
#else
#define PSORT_CHK(cond) (true)
int plookup_sort_checked_failures(unsigned* counts) {
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    return PLK_OK;
}
#endif

#define PSORT_DI __device__ __forceinline__

PSORT_DI SortRow sort_row_load(const uint4* __restrict__ p, size_t i) {
    const uint4 a = p[2 * i], b = p[2 * i + 1];
    return SortRow{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
PSORT_DI void sort_row_store(uint4* __restrict__ p, size_t i, const SortRow& r) {
    p[2 * i] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    p[2 * i + 1] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
}
// row s of t for the probe loops; an index outside t (never with a sound table) reads as row 0 in the checked build
struct SortRowAt {
    const uint4* t;
    uint32_t rows;
    PSORT_DI SortRow operator()(uint32_t s) const { return sort_row_load(t, PSORT_CHK(s < rows) ? s : 0); }
};
// slots as other lanes' atomics leave them: the read goes to L2 (a CU's vector L1 is not refreshed by another CU's atomics)
struct SortSlotOps {
    uint32_t* slots;
    PSORT_DI uint32_t load(uint32_t h) { return __hip_atomic_load(slots + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    PSORT_DI uint32_t cas(uint32_t h, uint32_t expected, uint32_t value) { return atomicCAS(slots + h, expected, value); }
    PSORT_DI void lower(uint32_t h, uint32_t value) { atomicMin(slots + h, value); }
};

// Of the lanes of a wave with `todo` set, the lowest lane of every group of EQUAL rows keeps it.  Groups are found by the hash; the
// rows are compared only when more than one lane shares it.  One round per distinct hash in the wave; every lane of the wave calls this.
PSORT_DI bool sort_wave_first_of_equal(bool todo, uint32_t key, const SortRow& row) {
    const int lane = threadIdx.x & 63;
    unsigned long long pend = __ballot(todo);
    bool keep = false;
    while (pend) {
        const int leader = __ffsll((long long)pend) - 1;
        const bool same_key = todo && key == (uint32_t)__shfl((int)key, leader);
        unsigned long long m = __ballot(same_key) & pend;
        if (m != (1ull << leader)) {
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) d |= row.w[k] ^ (uint32_t)__shfl((int)row.w[k], leader);
            m = __ballot(same_key && d == 0) & pend;
        }
        if (lane == leader) keep = true;
        pend &= ~m;  // the leader is always in m
    }
    return keep;
}

__global__ void __launch_bounds__(PSORT_LANES) k_sort_insert(const uint4* __restrict__ t, uint32_t rows, uint32_t* __restrict__ slots, uint32_t mask) {
    const uint32_t i = blockIdx.x * PSORT_LANES + threadIdx.x;
    bool todo = i < rows;
    SortRow row{};
    if (todo) {
        row = sort_row_load(t, i);
        if (i > 0 && psort_row_eq(sort_row_load(t, i - 1), row)) todo = false;  // a run: its first row enters, with the smaller index
    }
    todo = sort_wave_first_of_equal(todo, psort_hash(row), row);
    if (!todo) return;
    SortSlotOps ops{slots};
    (void)psort_insert(ops, SortRowAt{t, rows}, i, row, mask);
}

// lanes 0..n-1 take the rows of f, lanes n..n+rows-1 the rows of t.  Additions meet in a table in LDS keyed by the representative: a
// wave whose lanes all found the same one sends their number through one lane, the others go lane by lane; after the barrier every
// occupied slot is ONE atomic on cnt.  misses[0] += rows of f outside t, once per workgroup.
__global__ void __launch_bounds__(PSORT_COUNT_LANES) k_sort_count(const uint4* __restrict__ f, const uint4* __restrict__ t, uint32_t n, uint32_t rows,
                                                                  const uint32_t* __restrict__ slots, uint32_t mask, uint32_t* __restrict__ cnt,
                                                                  uint32_t* __restrict__ misses) {
    __shared__ uint32_t s_key[PSORT_COUNT_SLOTS], s_cnt[PSORT_COUNT_SLOTS];
    __shared__ uint32_t s_miss;
    for (int k = threadIdx.x; k < PSORT_COUNT_SLOTS; k += PSORT_COUNT_LANES) {
        s_key[k] = PSORT_EMPTY;
        s_cnt[k] = 0;
    }
    if (threadIdx.x == 0) s_miss = 0;
    __syncthreads();
    const uint32_t g = blockIdx.x * PSORT_COUNT_LANES + threadIdx.x;  // n + rows = 2 rows - 1 <= 2^29 - 1
    const bool valid = g < n + rows;
    uint32_t rep = PSORT_EMPTY;
    if (valid) {
        const SortRow row = g < n ? sort_row_load(f, g) : sort_row_load(t, g - n);
        rep = psort_lookup([&](uint32_t h) { return slots[h]; }, SortRowAt{t, rows}, row, mask);
        if (!PSORT_CHK(rep == PSORT_EMPTY || rep < rows)) rep = PSORT_EMPTY;
    }
    const bool found = rep != PSORT_EMPTY;
    const int lane = threadIdx.x & 63;
    const unsigned long long found_m = __ballot(found), miss_m = __ballot(valid && !found);
    if (miss_m && lane == 0) atomicAdd(&s_miss, (uint32_t)__popcll(miss_m));
    if (found_m) {
        const int leader = __ffsll((long long)found_m) - 1;
        const uint32_t lead_rep = (uint32_t)__shfl((int)rep, leader);
        const bool uniform = __ballot(found && rep == lead_rep) == found_m;
        const uint32_t add = uniform ? (uint32_t)__popcll(found_m) : 1u;
        if (found && (!uniform || lane == leader)) {
            uint32_t h = psort_hash_index(rep) & (PSORT_COUNT_SLOTS - 1);
            for (int k = 0; k < PSORT_COUNT_SLOTS; ++k, h = psort_next(h, PSORT_COUNT_SLOTS - 1)) {  // at most PSORT_COUNT_LANES keys: ends
                const uint32_t prev = atomicCAS(&s_key[h], PSORT_EMPTY, rep);
                if (prev == PSORT_EMPTY || prev == rep) {
                    atomicAdd(&s_cnt[h], add);
                    break;
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PSORT_COUNT_SLOTS; k += PSORT_COUNT_LANES)
        if (s_key[k] != PSORT_EMPTY) atomicAdd(cnt + s_key[k], s_cnt[k]);
    if (threadIdx.x == 0 && s_miss) atomicAdd(misses, s_miss);
}

// ---- the exclusive scan of the counts -----------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's PSORT_LANES lanes and the workgroup's total; ends with a barrier-free read of s_wave
// that the NEXT call's first barrier protects
PSORT_DI uint32_t sort_wg_exclusive(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    constexpr int WAVES = PSORT_LANES / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += up;
    }
    __syncthreads();  // the previous call's readers are done with s_wave
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    return before + inc - v;
}

// cnt is padded with zeros to whole tiles: a lane reads its PSORT_ROWS counts as one 16-byte access
__global__ void __launch_bounds__(PSORT_LANES) k_sort_tiles(const uint4* __restrict__ cnt4, uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_reps) {
    __shared__ uint32_t s_wave[PSORT_LANES / 64];
    const uint4 c = cnt4[(size_t)blockIdx.x * PSORT_LANES + threadIdx.x];
    uint32_t total = 0, reps = 0;
    (void)sort_wg_exclusive(c.x + c.y + c.z + c.w, s_wave, total);
    (void)sort_wg_exclusive((c.x != 0) + (c.y != 0) + (c.z != 0) + (c.w != 0), s_wave, reps);
    if (threadIdx.x == 0) {
        tile_sum[blockIdx.x] = total;
        tile_reps[blockIdx.x] = reps;
    }
}
// one workgroup, PSORT_CHUNK tile sums per step with a running carry: tile_sum becomes its exclusive scan, tile_sum[tiles] the total.
// status (nullable): [0] rows of f outside t, [1] distinct values of t (a row of t is a representative iff its count is not zero).
__global__ void __launch_bounds__(PSORT_LANES) k_sort_scan(uint32_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_reps, uint32_t tiles,
                                                           const uint32_t* __restrict__ misses, uint32_t* __restrict__ status) {
    static_assert(PSORT_CHUNK == PSORT_LANES, "one tile sum per lane and step");
    __shared__ uint32_t s_wave[PSORT_LANES / 64];
    uint32_t carry = 0, reps = 0;
    for (uint32_t base = 0; base < tiles; base += PSORT_CHUNK) {
        const uint32_t k = base + threadIdx.x;
        uint32_t total = 0, r = 0;
        const uint32_t ex = sort_wg_exclusive(k < tiles ? tile_sum[k] : 0, s_wave, total);
        (void)sort_wg_exclusive(k < tiles ? tile_reps[k] : 0, s_wave, r);
        if (k < tiles) tile_sum[k] = carry + ex;
        carry += total;
        reps += r;
    }
    if (threadIdx.x == 0) {
        tile_sum[tiles] = carry;
        if (status) {
            status[0] = misses[0];
            status[1] = reps;
        }
    }
}
__global__ void __launch_bounds__(PSORT_LANES) k_sort_offsets(const uint4* __restrict__ cnt4, const uint32_t* __restrict__ tile_pre, uint4* __restrict__ off4) {
    __shared__ uint32_t s_wave[PSORT_LANES / 64];
    const size_t q = (size_t)blockIdx.x * PSORT_LANES + threadIdx.x;
    const uint4 c = cnt4[q];
    uint32_t total = 0;
    const uint32_t o = tile_pre[blockIdx.x] + sort_wg_exclusive(c.x + c.y + c.z + c.w, s_wave, total);
    off4[q] = make_uint4(o, o + c.x, o + c.x + c.y, o + c.x + c.y + c.z);
}

// rows of s beyond the total (rows of f were outside t) are written as zero
__global__ void __launch_bounds__(PSORT_LANES) k_sort_expand(const uint4* __restrict__ t, const uint32_t* __restrict__ off, const uint32_t* __restrict__ total_at,
                                                             uint32_t rows, uint4* __restrict__ s) {
    const uint32_t j = blockIdx.x * PSORT_LANES + threadIdx.x;
    if (j >= 2 * rows - 1) return;
    SortRow r{};
    if (j < *total_at) {
        const uint32_t i = psort_find([&](uint32_t k) { return off[k]; }, rows, j);
        if (PSORT_CHK(i < rows)) r = sort_row_load(t, i);
    }
    sort_row_store(s, j, r);
}

// P only names the field the dispatcher matched: the 4-limb fields share the 32-byte row, and nothing here does arithmetic in it
template <class P>
static int sorted_multiset_t(unsigned log_size, const void* d_f, const void* d_t, void* d_s, void* d_status, hipStream_t stream) {
    static_assert(P::NL == 8, "256-bit scalar fields: a row is 8 words");
    const uint32_t rows = 1u << log_size, n = rows - 1, mask = 2 * rows - 1;
    const uint32_t tiles = (rows + PSORT_TILE - 1) / PSORT_TILE;
    const size_t padded = (size_t)tiles * PSORT_TILE;
    ScratchSet ss(stream);
    uint32_t* slots = (uint32_t*)ss.get((size_t)2 * rows * 4);
    uint32_t* cnt = (uint32_t*)ss.get((padded + 4) * 4);  // the counts, then the count of rows of f outside t (16-byte aligned)
    uint32_t* off = (uint32_t*)ss.get(padded * 4);
    uint32_t* tile_sum = (uint32_t*)ss.get(((size_t)tiles + 1) * 4);
    uint32_t* tile_reps = (uint32_t*)ss.get((size_t)tiles * 4);
    if (!slots || !cnt || !off || !tile_sum || !tile_reps) return PLK_ERR_OOM;
    uint32_t* misses = cnt + padded;
    hipError_t e = hipMemsetAsync(slots, 0xFF, (size_t)2 * rows * 4, stream);  // PSORT_EMPTY
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (padded + 4) * 4, stream);
    if (e == hipSuccess) {
        k_sort_insert<<<(rows + PSORT_LANES - 1) / PSORT_LANES, PSORT_LANES, 0, stream>>>((const uint4*)d_t, rows, slots, mask);
        k_sort_count<<<(n + rows + PSORT_COUNT_LANES - 1) / PSORT_COUNT_LANES, PSORT_COUNT_LANES, 0, stream>>>((const uint4*)d_f, (const uint4*)d_t, n, rows, slots,
                                                                                                             mask, cnt, misses);
        k_sort_tiles<<<tiles, PSORT_LANES, 0, stream>>>((const uint4*)cnt, tile_sum, tile_reps);
        k_sort_scan<<<1, PSORT_LANES, 0, stream>>>(tile_sum, tile_reps, tiles, misses, (uint32_t*)d_status);
        k_sort_offsets<<<tiles, PSORT_LANES, 0, stream>>>((const uint4*)cnt, tile_sum, (uint4*)off);
        k_sort_expand<<<(2 * rows - 1 + PSORT_LANES - 1) / PSORT_LANES, PSORT_LANES, 0, stream>>>((const uint4*)d_t, off, tile_sum + tiles, rows, (uint4*)d_s);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "plookup sorted multiset launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

// the refusals both entries share: nothing is launched or copied before they pass
int plookup_sorted_multiset_check(unsigned log_size, int field) {
    if (log_size == 0 || log_size > 28) return set_error(PLK_ERR_INVALID_ARG, "log_size %u: the sorted multiset takes 1 <= log_size <= 28", log_size);
    return or_bad_field(with_field4(field, [](auto) { return (int)PLK_OK; }), field);
}

int plookup_sorted_multiset_dev_impl(unsigned log_size, int field, const void* d_f, const void* d_t, void* d_s, void* d_status, hipStream_t stream) {
    PLK_TRY(plookup_sorted_multiset_check(log_size, field));
    if (!d_f || !d_t || !d_s) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    PLK_TRY(ensure_device());
    return or_bad_field(with_field4(field, [&](auto t) { return sorted_multiset_t<tag_t<decltype(t)>>(log_size, d_f, d_t, d_s, d_status, stream); }), field);
}

}  // namespace plk
