// check_witness_host_replay.cpp -- the lane-level steps of the witness check (plonky_amd/csrc/witness_step.cuh) walked on the host in the
// shape of the kernels: waves of 64 lanes over consecutive ids, a ballot per wave, one merge per wave into the report - with the waves
// taken in ascending and in descending order, which must give the same report.  No field arithmetic: a row's mask is an input.
//   in : u32 cases; per case u32 log_n, u32 has_sigma, u8 masks[n], u32 wires[6n][8] (the routed rows only: nothing else may be read),
//        u32 sigma[6n] when has_sigma
//   out: per case u32 report[8], u32 right[n], u32 below[n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "witness_step.cuh"

using namespace plk;

static bool differs(const uint32_t* a, const uint32_t* b) { return memcmp(a, b, 32) != 0; }

// one pass over `lanes` ids in waves of 64, the waves in the given order; flag(id) is what the lane found
template <class F> static void waves(uint32_t lanes, bool descending, uint32_t& count_word, uint32_t* first_word, F flag) {
    const uint32_t n_waves = (lanes + 63) / 64;
    for (uint32_t k = 0; k < n_waves; ++k) {
        const uint32_t base = (descending ? n_waves - 1 - k : k) * 64;
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (base + lane < lanes && flag(base + lane)) ballot |= (uint64_t)1 << lane;
        const WitnessWave w = witness_wave_merge(ballot, base);
        uint32_t unused = WITNESS_NONE;
        witness_report_merge(count_word, first_word ? *first_word : unused, w);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t cases = 0;
    if (fread(&cases, 4, 1, in) != 1) return 2;
    unsigned mismatches = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t head[2];
        if (fread(head, 4, 2, in) != 2) return 2;
        const unsigned log_n = head[0];
        const uint32_t n = 1u << log_n, n6 = WITNESS_ROUTED << log_n;
        std::vector<uint8_t> masks(n);
        std::vector<uint32_t> wires((size_t)n6 * 8), sigma(head[1] ? n6 : 0);
        if (fread(masks.data(), 1, n, in) != n || fread(wires.data(), 4, wires.size(), in) != wires.size()) return 2;
        if (head[1] && fread(sigma.data(), 4, n6, in) != n6) return 2;
        uint32_t report[2][WITNESS_REPORT_WORDS];
        for (int order = 0; order < 2; ++order) {
            uint32_t* r = report[order];
            for (int w = 0; w < WITNESS_REPORT_WORDS; ++w) r[w] = witness_report_init(w);
            waves(n, order == 1, r[WITNESS_BAD_ROWS], &r[WITNESS_FIRST_ROW], [&](uint32_t i) { return masks[i] != 0; });
            r[WITNESS_FIRST_MASK] = r[WITNESS_FIRST_ROW] < n ? masks[r[WITNESS_FIRST_ROW]] : 0u;  // k_check_first
            if (head[1]) {
                waves(n6, order == 1, r[WITNESS_BAD_COPIES], &r[WITNESS_FIRST_COPY], [&](uint32_t w) {
                    return witness_copy_class(w, sigma[w], log_n) == WITNESS_COPY_COMPARE && differs(&wires[(size_t)w * 8], &wires[(size_t)sigma[w] * 8]);
                });
                waves(n6, order == 1, r[WITNESS_SIGMA_RANGE], nullptr, [&](uint32_t w) { return witness_copy_class(w, sigma[w], log_n) == WITNESS_COPY_OUT_OF_RANGE; });
            }
        }
        if (memcmp(report[0], report[1], sizeof(report[0])) != 0) ++mismatches;
        fwrite(report[0], 4, WITNESS_REPORT_WORDS, out);
        std::vector<uint32_t> right(n), below(n);
        for (uint32_t i = 0; i < n; ++i) {
            right[i] = witness_right(i, log_n);
            below[i] = witness_below(i, log_n);
            if (right[i] >= n || below[i] >= n) ++mismatches;
        }
        fwrite(right.data(), 4, n, out);
        fwrite(below.data(), 4, n, out);
    }
    fclose(in);
    fclose(out);
    printf("cases: %u, order mismatches: %u\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
