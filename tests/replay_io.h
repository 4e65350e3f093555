// replay_io.h -- the text I/O and the seeded inputs the host replay programs (tests/*_host_replay.cpp) share.  Plain C++17 over
// fp.cuh / fz.cuh only.  Field elements travel as words, 8 NL hex digits, most significant first.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../plonky_amd/csrc/fp.cuh"
#include "../plonky_amd/csrc/fz.cuh"

inline bool token(FILE* fh, std::string& s) {
    char buf[256];
    if (fscanf(fh, "%255s", buf) != 1) return false;
    s = buf;
    return true;
}
template <int NL> bool read_words(FILE* fh, uint32_t (&v)[NL]) {
    std::string s;
    if (!token(fh, s) || s.size() != (size_t)NL * 8) return false;
    for (int k = 0; k < NL; ++k) v[k] = (uint32_t)strtoul(s.substr((size_t)(NL - 1 - k) * 8, 8).c_str(), nullptr, 16);
    return true;
}
template <class P> bool read_fe(FILE* fh, plk::Fe<P>& v) { return read_words(fh, v.v); }
template <int NL> std::string hex_words(const uint32_t (&w)[NL]) {
    std::string s;
    char buf[9];
    for (int k = NL - 1; k >= 0; --k) {
        snprintf(buf, sizeof(buf), "%08x", w[k]);
        s += buf;
    }
    return s;
}

// a Montgomery word (factor R = 2^(32 NL)) as the word of the same value in the working form's R'
template <class P> plk::Fe<P> to_rprime(const plk::Fe<P>& v) {
    using namespace plk;
    return fz_to_fe_canonical<P>(fz_mul<P>(fz_from_fe<P>(v), fz_const_r_to_rprime<P>()));
}
// the next element of the rand() sequence the program seeded; 2 NL draws whatever `edge` is, so a program's values keep their order
template <class P> plk::Fe<P> rnd(int edge) {
    using namespace plk;
    Fe<P> r;
    for (int i = 0; i < P::NL; ++i) r.v[i] = (uint32_t)rand() * 2654435761u ^ (uint32_t)rand();
    r.v[P::NL - 1] &= 0x0fffffffu;
    if (edge == 1) r = fe_zero<P>();                               // the stored word 0
    if (edge == 2) r = fe_neg<P>(fe_one<P>());                     // the value p - 1
    if (edge == 3) r = fe_to_canonical<P>(fe_neg<P>(fe_one<P>()));  // the stored word p - 1
    if (edge == 4) { r = fe_zero<P>(); r.v[0] = 1; }                 // the stored word 1
    return r;
}
