// rescue_host_replay.cpp -- plonky_amd/csrc/rescue_step.cuh (the exponent of a k-th root, the Cauchy matrix, the windowed power chain,
// the row sum and the round: the code the kernels of rescue.hip run) compiled for the host and run as a program of its own:
// tests/test_rescue_host_replay.py builds it plain and under AddressSanitizer + UBSan and compares what it prints with
// tests/rescue_ref.py.
//
//   rescue_host_replay CASES
// CASES is a stream of tokens; values are Montgomery words, 8 NL hex digits, most significant first:
//   M field                                       ->  "M field alpha m00 m01 .. m33"       the matrix, row-major
//   K field k x                                   ->  "K field k ok d y"                   d: the exponent (hex), y = x^d (zeros if !ok)
//   P field rounds c[rounds * 8] s0 s1 s2 s3      ->  "P field rounds o0 o1 o2 o3"         one permutation
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../plonky_amd/csrc/dispatch.cuh"
#include "../plonky_amd/csrc/rescue_step.cuh"
#include "replay_io.h"

using namespace plk;

template <class P> static int matrix(int field) {
    printf("M %d %u", field, rescue_alpha<P>());
    for (int r = 0; r < RESCUE_WIDTH; ++r)
        for (int c = 0; c < RESCUE_WIDTH; ++c) printf(" %s", hex_words(rescue_mds_entry<P>(RESCUE_WIDTH, r, c).v).c_str());
    printf("\n");
    return 0;
}

template <class P> static int root(FILE* fh, int field) {
    std::string ks;
    Fe<P> x;
    if (!token(fh, ks) || !read_fe<P>(fh, x)) return 1;
    const uint32_t k = (uint32_t)strtoul(ks.c_str(), nullptr, 10);
    uint32_t d[P::NL];
    const bool ok = rescue_kth_root_exponent<P>(k, d);
    Fe<P> y = fe_zero<P>();
    if (ok) y = rescue_leave<P>(rescue_pow<P>(rescue_enter<P>(x), d, rescue_windows(rescue_exponent_bits(d))));
    printf("K %d %u %d %s %s\n", field, k, ok ? 1 : 0, hex_words(d).c_str(), hex_words(y.v).c_str());
    return 0;
}

template <class P> static int permutation(FILE* fh, int field) {
    constexpr int NZ = FzCfg<P>::NZ;
    std::string rs;
    if (!token(fh, rs)) return 1;
    const int rounds = atoi(rs.c_str());
    if (rounds < 1 || rounds > 64) return 1;
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
    Fz<P> state[RESCUE_WIDTH];
    for (int e = 0; e < RESCUE_WIDTH; ++e) {
        Fe<P> s;
        if (!read_fe<P>(fh, s)) return 1;
        state[e] = rescue_enter<P>(s);
    }
    for (int r = 0; r < rounds; ++r) {
        const uint32_t* ka = consts.data() + (size_t)r * 2 * RESCUE_WIDTH * NZ;
        rescue_permutation_step<P>(state, d, windows, mds.data(), ka, ka + RESCUE_WIDTH * NZ);
    }
    printf("P %d %d", field, rounds);
    for (int e = 0; e < RESCUE_WIDTH; ++e) printf(" %s", hex_words(rescue_leave<P>(state[e]).v).c_str());
    printf("\n");
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
            if (kind == "M") return matrix<P>(field);
            if (kind == "K") return root<P>(fh, field);
            if (kind == "P") return permutation<P>(fh, field);
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
