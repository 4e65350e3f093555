// gate_trace_host_replay.cpp -- plonky_amd/csrc/gate_trace_step.cuh (the table addressing, the block bounds, the gate prefixes, the
// Rescue round emitting its two rows, the add / double rows and the chain of a curve_msm instance: the code the kernels of
// gate_trace.hip run) compiled for the host and run as a program of its own: tests/test_gate_trace_host_replay.py builds it plain and
// under AddressSanitizer + UBSan and compares what it prints with tests/gate_trace_ref.py.  The tables are exactly [9][n_rows] and
// [6][n_rows] elements, so the sanitized build also shows that a block that would pass n_rows writes nothing.
//
//   gate_trace_host_replay CASES [time]
// CASES is a stream of tokens; values are Montgomery words, 64 hex digits, most significant first; `field` is a 4-limb field id:
//   R field rounds c[rounds * 8] n_rows count { first s0 s1 s2 s3 } * count
//   M field parts n_bits n_rows count start_x start_y { first (x y) * parts (s) * parts } * count
// Per case: "W j row v" for every wire written, "K j row v" for every constant, in table order, then "S s0 s1 s2 s3", the status.
// With `time` the writes are not printed: one line "T kind count ms" per case, the block generation alone on this one core.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../plonky_amd/csrc/dispatch.cuh"
#include "../plonky_amd/csrc/gate_trace_step.cuh"
#include "replay_io.h"

using namespace plk;

template <class P> struct Tables {
    uint32_t n_rows;
    std::vector<Fe<P>> wires, constants;
    std::vector<uint8_t> wrote_w, wrote_k;
    explicit Tables(uint32_t n) : n_rows(n), wires((size_t)TRACE_WIRES * n), constants((size_t)TRACE_CONSTANTS * n), wrote_w(wires.size()), wrote_k(constants.size()) {}
    void wire(uint32_t j, uint32_t row, const Fe<P>& v) {
        wires.at(trace_at(j, row, n_rows)) = v;
        wrote_w[trace_at(j, row, n_rows)] = 1;
    }
    void constant(uint32_t j, uint32_t row, const Fe<P>& v) {
        constants.at(trace_at(j, row, n_rows)) = v;
        wrote_k[trace_at(j, row, n_rows)] = 1;
    }
    void print(const uint32_t (&status)[TRACE_STATUS_WORDS]) const {
        for (uint32_t j = 0; j < TRACE_WIRES; ++j)
            for (uint32_t i = 0; i < n_rows; ++i)
                if (wrote_w[trace_at(j, i, n_rows)]) printf("W %u %u %s\n", j, i, hex_words(wires[trace_at(j, i, n_rows)].v).c_str());
        for (uint32_t j = 0; j < TRACE_CONSTANTS; ++j)
            for (uint32_t i = 0; i < n_rows; ++i)
                if (wrote_k[trace_at(j, i, n_rows)]) printf("K %u %u %s\n", j, i, hex_words(constants[trace_at(j, i, n_rows)].v).c_str());
        printf("S %u %u %u %u\n", status[0], status[1], status[2], status[3]);
    }
};

static bool number(FILE* fh, uint32_t& v) {
    std::string s;
    if (!token(fh, s)) return false;
    v = (uint32_t)strtoul(s.c_str(), nullptr, 10);
    return true;
}
static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

template <class P> static int rescue(FILE* fh, bool timing) {
    constexpr int NZ = FzCfg<P>::NZ;
    if constexpr (P::NL != 8 || rescue_alpha<P>() != 5u) {
        return 1;
    } else {
        uint32_t rounds, n_rows, count;
        if (!number(fh, rounds) || rounds < 1 || rounds > 64) return 1;
        std::vector<Fe<P>> consts_r((size_t)rounds * 2 * RESCUE_WIDTH);
        std::vector<uint32_t> consts(consts_r.size() * NZ), mds((size_t)RESCUE_WIDTH * RESCUE_WIDTH * NZ);
        for (size_t i = 0; i < consts_r.size(); ++i) {
            if (!read_fe<P>(fh, consts_r[i])) return 1;
            const Fz<P> v = rescue_table_form<P>(consts_r[i]);
            for (int l = 0; l < NZ; ++l) consts[i * NZ + l] = v.l[l];
        }
        for (int e = 0; e < RESCUE_WIDTH * RESCUE_WIDTH; ++e) {
            const Fz<P> v = rescue_table_form<P>(rescue_mds_entry<P>(RESCUE_WIDTH, e / RESCUE_WIDTH, e % RESCUE_WIDTH));
            for (int l = 0; l < NZ; ++l) mds[(size_t)e * NZ + l] = v.l[l];
        }
        uint32_t d[P::NL];
        if (!rescue_kth_root_exponent<P>(5u, d)) return 1;
        const int windows = rescue_windows(rescue_exponent_bits(d));
        if (!number(fh, n_rows) || !number(fh, count) || n_rows < 1 || n_rows > (1u << 20)) return 1;
        std::vector<uint32_t> first(count);
        std::vector<Fe<P>> inputs((size_t)count * RESCUE_WIDTH);
        for (uint32_t c = 0; c < count; ++c) {
            if (!number(fh, first[c])) return 1;
            for (int e = 0; e < RESCUE_WIDTH; ++e)
                if (!read_fe<P>(fh, inputs[(size_t)c * RESCUE_WIDTH + e])) return 1;
        }
        Tables<P> t(n_rows);
        uint32_t status[TRACE_STATUS_WORDS];
        for (int w = 0; w < TRACE_STATUS_WORDS; ++w) status[w] = trace_status_init(w);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t c = 0; c < count; ++c) {
            if (!trace_block_fits(first[c], trace_rescue_block_rows(rounds), n_rows)) {
                ++status[TRACE_OVERRUN];
                continue;
            }
            Fz<P> state[RESCUE_WIDTH];
            for (int e = 0; e < RESCUE_WIDTH; ++e) state[e] = rescue_enter<P>(inputs[(size_t)c * RESCUE_WIDTH + e]);
            for (uint32_t r = 0; r < rounds; ++r) {
                const size_t at = (size_t)r * 2 * RESCUE_WIDTH;
                trace_rescue_round<P>(state, first[c] + 2 * r, d, windows, mds.data(), consts.data() + at * NZ, consts.data() + (at + RESCUE_WIDTH) * NZ,
                                      consts_r.data() + at, consts_r.data() + at + RESCUE_WIDTH, t);
            }
            trace_rescue_receive<P>(state, first[c] + 2 * rounds, t);
        }
        if (timing) printf("T R %u %.3f\n", count, ms_since(t0));
        else t.print(status);
        return 0;
    }
}

template <class P> struct Parts {
    const Fe<P>* pts;
    const Fe<P>* scs;
    void point(uint32_t j, Fe<P>& x, Fe<P>& y) const {
        x = pts[2 * j];
        y = pts[2 * j + 1];
    }
    Fe<P> scalar(uint32_t j) const { return scs[j]; }
};

template <class P> static int msm(FILE* fh, bool timing) {
    if constexpr (P::NL != 8) {
        return 1;
    } else {
        uint32_t parts, n_bits, n_rows, count;
        if (!number(fh, parts) || !number(fh, n_bits) || !number(fh, n_rows) || !number(fh, count)) return 1;
        if (parts < 1 || parts > TRACE_MSM_MAX_PARTS || n_bits < 1 || n_bits > (uint32_t)P::BITS - 1 || n_rows < 1 || n_rows > (1u << 22)) return 1;
        Fe<P> sx, sy;
        if (!read_fe<P>(fh, sx) || !read_fe<P>(fh, sy)) return 1;
        std::vector<uint32_t> first(count);
        std::vector<Fe<P>> pts((size_t)count * parts * 2), scs((size_t)count * parts);
        for (uint32_t c = 0; c < count; ++c) {
            if (!number(fh, first[c])) return 1;
            for (uint32_t k = 0; k < 2 * parts; ++k)
                if (!read_fe<P>(fh, pts[(size_t)c * parts * 2 + k])) return 1;
            for (uint32_t k = 0; k < parts; ++k)
                if (!read_fe<P>(fh, scs[(size_t)c * parts + k])) return 1;
        }
        Tables<P> t(n_rows);
        uint32_t status[TRACE_STATUS_WORDS];
        for (int w = 0; w < TRACE_STATUS_WORDS; ++w) status[w] = trace_status_init(w);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t c = 0; c < count; ++c) {
            if (!trace_block_fits(first[c], trace_msm_block_rows(parts, n_bits), n_rows)) {
                ++status[TRACE_OVERRUN];
                continue;
            }
            Parts<P> in{pts.data() + (size_t)c * parts * 2, scs.data() + (size_t)c * parts};
            if (trace_msm_instance<P>(parts, n_bits, first[c], sx, sy, in, t)) {
                ++status[TRACE_EXCEPTIONAL];
                if (c < status[TRACE_FIRST_EXCEPTIONAL]) status[TRACE_FIRST_EXCEPTIONAL] = c;
            }
        }
        if (timing) printf("T M %u %.3f\n", count, ms_since(t0));
        else t.print(status);
        return 0;
    }
}

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) {
        fprintf(stderr, "usage: %s CASES [time]\n", argv[0]);
        return 2;
    }
    FILE* fh = fopen(argv[1], "r");
    if (!fh) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const bool timing = argc == 3;
    std::string kind, fs;
    int rc = 0;
    while (rc == 0 && token(fh, kind) && token(fh, fs)) {
        const int field = atoi(fs.c_str());
        const int m = with_field(field, [&](auto t) {
            using P = tag_t<decltype(t)>;
            if (kind == "R") return rescue<P>(fh, timing);
            if (kind == "M") return msm<P>(fh, timing);
            return 1;
        });
        if (m != 0) {
            fprintf(stderr, "bad case: %s %s\n", kind.c_str(), fs.c_str());
            rc = 1;
        }
    }
    fclose(fh);
    return rc;
}
