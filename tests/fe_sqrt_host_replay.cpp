// fe_sqrt_host_replay.cpp -- plonky_amd/csrc/fe_sqrt.cuh (fe_sqrt_with: the Tonelli-Shanks loop that the point decompression and the two
// hashes to the curve run) compiled for the host and run as a program of its own: tests/test_fe_sqrt_host_replay.py builds it plain and
// under AddressSanitizer + UBSan and compares what it prints with tests/sqrt_cases.py.  Every input goes through the loop twice: with
// SqrtRootBySquaring (fe_sqrt) and with a host table functor that indexes tab[m] = ROOT_2ADIC^(2^m) exactly as SqrtRootFromTable does
// (fe_sqrt_tabled); the table is built by the loop of k_h2c_root_table.
//
//   fe_sqrt_host_replay CASES
// CASES is a stream of tokens; values are Montgomery words, 8 NL hex digits, most significant first:
//   Q field a   ->  "Q field ok root ok_tabled root_tabled"    ok 0: a non-residue, the root printed as all words ffffffff
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../plonky_amd/csrc/dispatch.cuh"
#include "../plonky_amd/csrc/fe_sqrt.cuh"
#include "replay_io.h"

using namespace plk;

// SqrtRootFromTable on a host vector: the same index, checked against the table's length
template <class P> struct HostRootFromTable {
    const std::vector<Fe<P>>* tab;
    Fe<P> operator()(const Fe<P>& /*z*/, int /*j*/, int m) const { return tab->at((size_t)m); }
};

template <class P> static int sqrt_case(FILE* fh, int field) {
    Fe<P> a;
    if (!read_fe<P>(fh, a)) return 1;
    std::vector<Fe<P>> tab;
    Fe<P> w = fe_const<P>(P::ROOT_2ADIC);
    for (int m = 0; m < P::TWO_ADICITY; ++m) {  // k_h2c_root_table
        tab.push_back(w);
        w = fe_sqr<P>(w);
    }
    Fe<P> none;
    for (int k = 0; k < P::NL; ++k) none.v[k] = 0xFFFFFFFFu;
    Fe<P> r0 = none, r1 = none;
    const bool ok0 = fe_sqrt_with<P>(a, r0, SqrtRootBySquaring<P>{});
    const bool ok1 = fe_sqrt_with<P>(a, r1, HostRootFromTable<P>{&tab});
    printf("Q %d %d %s %d %s\n", field, ok0 ? 1 : 0, hex_words((ok0 ? r0 : none).v).c_str(), ok1 ? 1 : 0, hex_words((ok1 ? r1 : none).v).c_str());
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
            if (kind == "Q") return sqrt_case<P>(fh, field);
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
