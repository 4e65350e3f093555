// sigma_host_replay.cpp -- the lane-level steps of the copy-constraint permutation (plonky_amd/csrc/sigma_step.cuh) walked on the
// host in the shape of k_sigma_slots (sigma.hip): workgroups of SIGMA_LANES slots, the workgroup's range of partitions from its
// first and last slot, the bisection on a staged copy of the offsets when the range fits and on the whole array when it does not,
// the neighbour, the class of the slot, the stores and the three counters; then the unset entries (k_sigma_unset) and
// sigma_status0.  Every case is replayed with the slots in ascending and in descending order; the two must agree.
//
//   sigma_host_replay cases.bin out.bin
// cases.bin: uint32 count, then per case uint32 log_n, P, M, offsets[P + 1], members[M].
// out.bin:   per case uint32 status[3], sigma[6n], input[6n], gate[6n] (the split of sigma[w] where a value is stored, else 0xFFFFFFFF).
// A stand-alone program: built plain and under AddressSanitizer + UBSan by tests/test_sigma_host_replay.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../plonky_amd/csrc/sigma_step.cuh"

using namespace plk;

struct Result {
    uint32_t status[3];
    std::vector<uint32_t> sigma, input, gate;
    bool operator==(const Result& o) const {
        return status[0] == o.status[0] && status[1] == o.status[1] && status[2] == o.status[2] && sigma == o.sigma && input == o.input && gate == o.gate;
    }
};

static Result replay(unsigned log_n, const std::vector<uint32_t>& offsets, const std::vector<uint32_t>& members, bool descending) {
    const uint32_t n6 = SIGMA_ROUTED << log_n, M = (uint32_t)members.size(), P = (uint32_t)offsets.size() - 1;
    Result r;
    r.sigma.assign(n6, SIGMA_UNSET);
    r.input.assign(n6, 0xFFFFFFFFu);
    r.gate.assign(n6, 0xFFFFFFFFu);
    uint32_t listings = 0, lonely = 0, out_of_range = 0;
    const uint32_t groups = (M + SIGMA_LANES - 1) / SIGMA_LANES;
    std::vector<uint32_t> staged_off(SIGMA_LANES + 2);
    for (uint32_t gi = 0; gi < groups; ++gi) {
        const uint32_t g = descending ? groups - 1 - gi : gi;
        const uint32_t p0 = g * SIGMA_LANES, p_last = p0 + SIGMA_LANES - 1 < M ? p0 + SIGMA_LANES - 1 : M - 1;
        auto global_off = [&](uint32_t q) { return offsets.at(q); };
        const uint32_t q0 = sigma_find(global_off, 0u, P - 1, p0);
        uint32_t q1 = sigma_find(global_off, 0u, P - 1, p_last);
        if (q1 < q0) q1 = q0;
        const uint32_t span = q1 - q0 + 1;
        const bool staged = span + 1 <= (uint32_t)staged_off.size();
        if (staged)
            for (uint32_t k = 0; k <= span; ++k) staged_off.at(k) = offsets.at(q0 + k);
        for (uint32_t li = 0; li < (uint32_t)SIGMA_LANES; ++li) {
            const uint32_t p = p0 + (descending ? SIGMA_LANES - 1 - li : li);
            if (p >= M) continue;
            uint32_t begin, end;
            if (staged) {
                const uint32_t k = sigma_find([&](uint32_t q) { return staged_off.at(q); }, 0u, span - 1, p);
                begin = staged_off.at(k);
                end = staged_off.at(k + 1);
            } else {
                const uint32_t q = sigma_find(global_off, q0, q1, p);
                begin = offsets.at(q);
                end = offsets.at(q + 1);
            }
            const uint32_t id = members.at(p), x = members.at(sigma_neighbour(p, begin, end, M));
            const SigmaSlot s = sigma_classify(id, x, end - begin, log_n);
            listings += s.routed;
            lonely += s.lonely;
            out_of_range += s.out_of_range;
            if (s.routed) r.sigma.at(id) = s.sigma;
            if (s.value) {
                r.input.at(id) = sigma_input(x, log_n);
                r.gate.at(id) = sigma_gate(x, log_n);
            }
        }
    }
    uint32_t unset = 0;
    for (uint32_t w = 0; w < n6; ++w) unset += r.sigma[w] == SIGMA_UNSET;
    r.status[0] = sigma_status0(listings, unset, log_n);
    r.status[1] = lonely;
    r.status[2] = out_of_range;
    return r;
}

static bool read_words(FILE* f, std::vector<uint32_t>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), 4, count, f) == count;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    unsigned mismatches = 0;
    for (uint32_t c = 0; c < count; ++c) {
        uint32_t head[3];
        if (fread(head, 4, 3, in) != 3) return 2;
        std::vector<uint32_t> offsets, members;
        if (!read_words(in, offsets, (size_t)head[1] + 1) || !read_words(in, members, head[2])) return 2;
        const Result up = replay(head[0], offsets, members, false), down = replay(head[0], offsets, members, true);
        // the one store that depends on the order is sigma[id] of a wire listed twice: such a case may differ there and nowhere else
        if (!(up == down) && !(up.status[0] != 0 && up.status[0] == down.status[0] && up.status[1] == down.status[1] && up.status[2] == down.status[2])) {
            ++mismatches;
            printf("case %u: ascending and descending order disagree\n", c);
        }
        fwrite(up.status, 4, 3, out);
        fwrite(up.sigma.data(), 4, up.sigma.size(), out);
        fwrite(up.input.data(), 4, up.input.size(), out);
        fwrite(up.gate.data(), 4, up.gate.size(), out);
    }
    fclose(in);
    fclose(out);
    printf("cases: %u, mismatches: %u\n", count, mismatches);
    return mismatches ? 1 : 0;
}
