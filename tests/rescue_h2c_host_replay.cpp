// rescue_h2c_host_replay.cpp -- plonky_amd/csrc/rescue_h2c_step.cuh (the seed formation, the y_neg bit, the curve half of a try and the
// bounded loop over the tries: the code k_rescue_h2c_tries runs) compiled for the host and run as a program of its own:
// tests/test_rescue_h2c_host_replay.py builds it plain and under AddressSanitizer + UBSan and compares what it prints with
// tests/rescue_h2c_ref.py.  The sponge is rescue_h2c_sponge_state (a whole state through rescue_permutation_step), the root fe_sqrt.
//
//   rescue_h2c_host_replay CASES
// CASES is a stream of tokens; values are Montgomery words, 8 NL hex digits, most significant first:
//   S field n                                              ->  "S field v"             v = from_canonical_u64(n), n decimal
//   Y field v                                              ->  "Y field bit"           bit 0 of the canonical form of v
//   T field b rounds i_first i_last c[rounds * 8] seed     ->  "T field status x y"    tries i_first ..= i_last; status 2 and zeros when
//                                                                                      none of them gives a point (b: the curve's B)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../plonky_amd/csrc/dispatch.cuh"
#include "../plonky_amd/csrc/rescue_h2c_step.cuh"
#include "replay_io.h"

using namespace plk;

template <class P> static int seed_case(FILE* fh, int field) {
    std::string ns;
    if (!token(fh, ns)) return 1;
    printf("S %d %s\n", field, hex_words(rescue_h2c_from_u64<P>(strtoull(ns.c_str(), nullptr, 10)).v).c_str());
    return 0;
}

template <class P> static int y_neg_case(FILE* fh, int field) {
    Fe<P> v;
    if (!read_fe<P>(fh, v)) return 1;
    printf("Y %d %u\n", field, rescue_h2c_y_neg<P>(v));
    return 0;
}

template <class P> static int tries_case(FILE* fh, int field) {
    constexpr int NZ = FzCfg<P>::NZ;
    std::string bs, rs, fs, ls;
    if (!token(fh, bs) || !token(fh, rs) || !token(fh, fs) || !token(fh, ls)) return 1;
    const int rounds = atoi(rs.c_str()), i_first = atoi(fs.c_str()), i_last = atoi(ls.c_str());
    if (rounds < 1 || rounds > 64 || i_first < 0 || i_last >= H2C_TRIES) return 1;
    std::vector<uint32_t> consts((size_t)rounds * 2 * RESCUE_WIDTH * NZ), mds((size_t)RESCUE_WIDTH * RESCUE_WIDTH * NZ);
    for (size_t i = 0; i < (size_t)rounds * 2 * RESCUE_WIDTH; ++i) {
        Fe<P> c;
        if (!read_fe<P>(fh, c)) return 1;
        const Fz<P> v = rescue_table_form<P>(c);
        for (int l = 0; l < NZ; ++l) consts[i * NZ + l] = v.l[l];
    }
    for (int e = 0; e < RESCUE_WIDTH * RESCUE_WIDTH; ++e) {
        const Fz<P> v = rescue_table_form<P>(rescue_mds_entry<P>(RESCUE_WIDTH, e / RESCUE_WIDTH, e % RESCUE_WIDTH));
        for (int l = 0; l < NZ; ++l) mds[(size_t)e * NZ + l] = v.l[l];
    }
    uint32_t d[P::NL];
    if (!rescue_kth_root_exponent<P>(rescue_alpha<P>(), d)) return 1;
    const int windows = rescue_windows(rescue_exponent_bits(d));
    Fe<P> seed;
    if (!read_fe<P>(fh, seed)) return 1;
    const Fe<P> b_mont = rescue_h2c_from_u64<P>(strtoull(bs.c_str(), nullptr, 10));
    const auto sponge = [&](const Fe<P>& s, uint32_t i, Fe<P>& o0, Fe<P>& o1) {
        rescue_h2c_sponge_state<P>(s, i, (uint32_t)rounds, d, windows, mds.data(), consts.data(), o0, o1);
    };
    const auto square_root = [](const Fe<P>& a, Fe<P>& r) { return fe_sqrt<P>(a, r); };
    Fe<P> x = fe_zero<P>(), y = fe_zero<P>();
    int status = 0;
    if (!rescue_h2c_tries<P>(seed, i_first, i_last, b_mont, sponge, square_root, x, y)) {  // i ran out: what the kernel's last launch writes
        status = 2;
        x = fe_zero<P>();
        y = fe_zero<P>();
    }
    printf("T %d %d %s %s\n", field, status, hex_words(x.v).c_str(), hex_words(y.v).c_str());
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE* fh = fopen(argv[1], "r");
    if (!fh) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string kind, fs;
    int rc = 0;
    while (rc == 0 && token(fh, kind) && token(fh, fs)) {
        const int field = atoi(fs.c_str());
        const int m = with_field(field, [&](auto t) {
            using P = tag_t<decltype(t)>;
            if (kind == "S") return seed_case<P>(fh, field);
            if (kind == "Y") return y_neg_case<P>(fh, field);
            if (kind == "T") return tries_case<P>(fh, field);
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
