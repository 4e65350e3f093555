// plookup_sort_host_replay.cpp -- the steps of the Plookup sorted multiset (plonky_amd/csrc/plookup_sort_step.cuh: hash, row comparison,
// probe step, insert, lookup, bisection) walked on the host, lane by lane, in the shape of the kernels of plookup_sort.hip: insert,
// lookup and count, the tiled scan with its chunked tile scan, expansion.  Every case runs with the lanes of the insert in ascending
// and in descending order (the second makes every duplicate lower its slot), with and without the kernel's skip of a row that repeats
// its predecessor, and is compared with a direct restatement (first-occurrence map, stable order).
//
//   plookup_sort_host_replay <cases.bin> <out.bin>
// cases.bin: uint32 count, then per case uint32 log_size, f (N rows of 8 words; row N - 1 is not read), t (N rows).
// out.bin:   per case uint32 missing, distinct, longest probe sequence, then s (2 N - 1 rows).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../plonky_amd/csrc/plookup_sort_step.cuh"

using namespace plk;

struct HostSlots {
    std::vector<uint32_t>& slots;
    uint32_t load(uint32_t h) { return slots[h]; }
    uint32_t cas(uint32_t h, uint32_t expected, uint32_t value) {
        const uint32_t old = slots[h];
        if (old == expected) slots[h] = value;
        return old;
    }
    void lower(uint32_t h, uint32_t value) { slots[h] = std::min(slots[h], value); }
};

struct Result {
    uint32_t missing = 0, distinct = 0, longest = 0;
    std::vector<SortRow> s;
};

static Result replay(const std::vector<SortRow>& f, const std::vector<SortRow>& t, bool descending, bool skip_runs) {
    const uint32_t rows = (uint32_t)t.size(), n = rows - 1, mask = 2 * rows - 1;
    Result r;
    auto row_at = [&](uint32_t s) { return t.at(s); };
    // k_sort_insert
    std::vector<uint32_t> slots(2 * (size_t)rows, PSORT_EMPTY);
    HostSlots ops{slots};
    for (uint32_t k = 0; k < rows; ++k) {
        const uint32_t i = descending ? rows - 1 - k : k;
        if (skip_runs && i > 0 && psort_row_eq(t[i - 1], t[i])) continue;
        r.longest = std::max(r.longest, psort_insert(ops, row_at, i, t[i], mask));
    }
    // k_sort_count
    const uint32_t tiles = (rows + PSORT_TILE - 1) / PSORT_TILE;
    std::vector<uint32_t> cnt((size_t)tiles * PSORT_TILE, 0);
    for (uint32_t g = 0; g < n + rows; ++g) {
        uint32_t probes = 0;
        const uint32_t rep = psort_lookup([&](uint32_t h) { return slots.at(h); }, row_at, g < n ? f[g] : t[g - n], mask, &probes);
        r.longest = std::max(r.longest, probes);
        if (rep == PSORT_EMPTY) ++r.missing;
        else ++cnt.at(rep);
    }
    // k_sort_tiles, k_sort_scan (PSORT_CHUNK tile sums per step, a running carry), k_sort_offsets
    std::vector<uint32_t> tile_sum(tiles + 1, 0), off(cnt.size());
    for (uint32_t b = 0; b < tiles; ++b)
        for (int k = 0; k < PSORT_TILE; ++k) {
            tile_sum[b] += cnt[(size_t)b * PSORT_TILE + k];
            r.distinct += cnt[(size_t)b * PSORT_TILE + k] != 0;
        }
    uint32_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += PSORT_CHUNK) {
        uint32_t run = 0;
        for (uint32_t k = base; k < std::min(tiles, base + PSORT_CHUNK); ++k) {
            const uint32_t v = tile_sum[k];
            tile_sum[k] = carry + run;
            run += v;
        }
        carry += run;
    }
    tile_sum[tiles] = carry;
    for (uint32_t b = 0; b < tiles; ++b) {
        uint32_t o = tile_sum[b];
        for (int k = 0; k < PSORT_TILE; ++k) {
            off[(size_t)b * PSORT_TILE + k] = o;
            o += cnt[(size_t)b * PSORT_TILE + k];
        }
    }
    // k_sort_expand
    r.s.assign(2 * (size_t)rows - 1, SortRow{});
    for (uint32_t j = 0; j < 2 * rows - 1; ++j)
        if (j < tile_sum[tiles]) r.s[j] = t.at(psort_find([&](uint32_t k) { return off.at(k); }, rows, j));
    return r;
}

// f ++ t in the order of each value's first occurrence in t, rows outside t dropped and the tail left zero
static Result restatement(const std::vector<SortRow>& f, const std::vector<SortRow>& t) {
    auto less = [](const SortRow& a, const SortRow& b) { return std::lexicographical_compare(a.w, a.w + 8, b.w, b.w + 8); };
    std::map<SortRow, uint32_t, decltype(less)> first(less);
    for (uint32_t i = 0; i < t.size(); ++i) first.emplace(t[i], i);
    Result r;
    r.distinct = (uint32_t)first.size();
    std::vector<std::pair<uint32_t, SortRow>> keyed;
    for (size_t j = 0; j + 1 < t.size(); ++j) {
        auto it = first.find(f[j]);
        if (it == first.end()) ++r.missing;
        else keyed.emplace_back(it->second, f[j]);
    }
    for (const SortRow& row : t) keyed.emplace_back(first.find(row)->second, row);
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    r.s.assign(2 * t.size() - 1, SortRow{});
    for (size_t j = 0; j < keyed.size(); ++j) r.s[j] = keyed[j].second;
    return r;
}

static bool same(const Result& a, const Result& b) {
    if (a.missing != b.missing || a.distinct != b.distinct || a.s.size() != b.s.size()) return false;
    for (size_t j = 0; j < a.s.size(); ++j)
        if (!psort_row_eq(a.s[j], b.s[j])) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t cases = 0;
    if (fread(&cases, 4, 1, in) != 1) return 2;
    int mismatches = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t log_size = 0;
        if (fread(&log_size, 4, 1, in) != 1 || log_size == 0 || log_size > 20) return 2;
        const size_t rows = (size_t)1 << log_size;
        std::vector<SortRow> f(rows), t(rows);
        if (fread(f.data(), sizeof(SortRow), rows, in) != rows || fread(t.data(), sizeof(SortRow), rows, in) != rows) return 2;
        const Result want = restatement(f, t);
        Result first;
        uint32_t longest = 0;
        for (int variant = 0; variant < 4; ++variant) {
            const Result got = replay(f, t, (variant & 1) != 0, (variant & 2) != 0);
            if (!same(got, want)) {
                ++mismatches;
                printf("case %u variant %d differs from the restatement\n", c, variant);
            }
            longest = std::max(longest, got.longest);
            if (variant == 0) first = got;
        }
        printf("case %u rows %zu missing %u distinct %u longest probe sequence %u\n", c, rows, first.missing, first.distinct, longest);
        const uint32_t head[3] = {first.missing, first.distinct, longest};
        fwrite(head, 4, 3, out);
        fwrite(first.s.data(), sizeof(SortRow), first.s.size(), out);
    }
    fclose(in);
    fclose(out);
    printf("cases: %u mismatches: %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
