// opening_host_replay.cpp -- the arithmetic of opening.hip (forms, limb bounds, tiling, two-level tables, the running total of the
// reduction) restated lane by lane on the host over the same fp.cuh / fz.cuh, against plain Montgomery arithmetic (fe_mul / fe_add).
// Built and run by tests/test_opening_host_replay.py; exit status 0 = no mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../plonky_amd/csrc/fp.cuh"
#include "../plonky_amd/csrc/fz.cuh"
#include "replay_io.h"
using namespace plk;
template <class P> Fe<P> fe_pow_u64(Fe<P> x, uint64_t e) { Fe<P> r = fe_one<P>(); while (e) { if (e & 1) r = fe_mul<P>(r, x); x = fe_sqr<P>(x); e >>= 1; } return r; }
template <class P> int run() {
    const int LANES = 256, G = 6, ROWS = 4, T = 24; const size_t TILE = LANES * T;
    int bad = 0;
    for (int trial = 0; trial < 6; ++trial) {
        size_t len = trial == 0 ? 1 : trial == 1 ? 6144 : trial == 2 ? 6145 : trial == 3 ? 20000 : trial == 4 ? 1537 : 12288;
        std::vector<Fe<P>> c(len);
        for (size_t j = 0; j < len; ++j) c[j] = rnd<P>((trial == 5) ? 3 - (int)(j % 2) : (rand() % 16 < 3 ? rand() % 4 : 0));
        Fe<P> x = rnd<P>(trial == 3 ? 2 : 0);
        Fe<P> ref = fe_zero<P>();
        for (size_t j = len; j-- > 0;) ref = fe_add<P>(fe_mul<P>(ref, x), c[j]);
        std::vector<Fz<P>> ytab(T); std::vector<Fe<P>> ltab(LANES);
        for (int m = 0; m < T; ++m) ytab[m] = fz_from_fe<P>(to_rprime<P>(fe_pow_u64<P>(x, (uint64_t)LANES * m)));
        for (int l = 0; l < LANES; ++l) ltab[l] = to_rprime<P>(fe_pow_u64<P>(x, l));
        Fe<P> xt = fe_pow_u64<P>(x, TILE);
        size_t tiles = (len + TILE - 1) / TILE;
        Fe<P> total = fe_zero<P>();
        for (size_t tile = 0; tile < tiles; ++tile) {
            Fe<P> part = fe_zero<P>();
            for (int l = 0; l < LANES; ++l) {
                Fz<P> acc = fz_zero<P>();
                for (int r = 0; r < ROWS; ++r) {
                    size_t row = tile * TILE + (size_t)r * G * LANES;
                    if (row >= len) continue;
                    FzWide<P> w; fz_wide_clear<P>(w);
                    for (int t = 0; t < G; ++t) {
                        size_t j = row + (size_t)t * LANES + l;
                        Fz<P> cf = j < len ? fz_from_fe<P>(c[j]) : fz_zero<P>();
                        fz_wide_mac<P>(w, cf, ytab[r * G + t]);
                    }
                    acc = fz_add<P>(acc, fz_wide_reduce<P>(w));
                }
                part = fe_add<P>(part, fz_to_fe_canonical<P>(fz_mul<P>(acc, fz_from_fe<P>(ltab[l]))));
            }
            total = fe_add<P>(total, fe_mul<P>(part, fe_pow_u64<P>(xt, tile)));
        }
        if (!fe_eq<P>(total, ref)) { ++bad; printf("eval mismatch trial %d\n", trial); }
        // reduction: 13 polys at one index, 6 at a time, squash every 5 groups (emulated with 40 polys)
        const int NPOL = 40;
        std::vector<Fe<P>> s(NPOL), cc(NPOL);
        Fe<P> rr = fe_zero<P>();
        for (int i = 0; i < NPOL; ++i) { s[i] = rnd<P>(trial == 5 ? 2 : 0); cc[i] = rnd<P>(trial == 5 ? 3 : 0); rr = fe_add<P>(rr, fe_mul<P>(s[i], cc[i])); }
        Fz<P> tot = fz_zero<P>(); int groups = 0;
        for (int i0 = 0; i0 < NPOL; i0 += G) {
            FzWide<P> w; fz_wide_clear<P>(w);
            for (int t = 0; t < G && i0 + t < NPOL; ++t) fz_wide_mac<P>(w, fz_from_fe<P>(cc[i0 + t]), fz_from_fe<P>(to_rprime<P>(s[i0 + t])));
            tot = fz_add<P>(tot, fz_wide_reduce<P>(w));
            if (++groups == 5) { tot = fz_mul<P>(tot, fz_one_rprime<P>()); groups = 0; }
        }
        if (!fe_eq<P>(fz_to_fe_canonical<P>(fz_mul<P>(tot, fz_one_rprime<P>())), rr)) { ++bad; printf("reduce mismatch trial %d\n", trial); }
        // two-level: sum_k lo_k hi_k with 8 points
        Fe<P> v = rnd<P>(0); size_t j = 1024 * 37 + 1023;
        Fe<P> rb = fe_zero<P>(), res = fe_zero<P>();
        Fe<P> pts[8];
        for (int k = 0; k < 8; ++k) { pts[k] = rnd<P>(k == 3 ? 2 : k == 5 ? 1 : 0); rb = fe_add<P>(rb, fe_mul<P>(fe_pow_u64<P>(v, k), fe_pow_u64<P>(pts[k], j))); }
        for (int k0 = 0; k0 < 8; k0 += G) {
            FzWide<P> w; fz_wide_clear<P>(w);
            for (int k = k0; k < 8 && k < k0 + G; ++k) {
                Fe<P> y = pts[k]; for (int q = 0; q < 10; ++q) y = fe_sqr<P>(y);
                Fe<P> hi = to_rprime<P>(fe_mul<P>(fe_pow_u64<P>(v, k), fe_pow_u64<P>(y, j >> 10)));
                fz_wide_mac<P>(w, fz_from_fe<P>(fe_pow_u64<P>(pts[k], j & 1023)), fz_from_fe<P>(hi));
            }
            Fe<P> sres = fz_to_fe_canonical<P>(fz_wide_reduce<P>(w));
            res = k0 == 0 ? sres : fe_add<P>(res, sres);
        }
        if (!fe_eq<P>(res, rb)) { ++bad; printf("two-level mismatch trial %d\n", trial); }
    }
    return bad;
}
int main() {
    int bad = run<TweedledeeBaseParams>() + run<TweedledumBaseParams>() + run<Bls12377ScalarParams>() + run<PallasBaseParams>() + run<VestaBaseParams>();
    printf("mismatches: %d\n", bad);
    return bad != 0;
}
