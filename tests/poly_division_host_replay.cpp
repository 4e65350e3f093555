// poly_division_host_replay.cpp -- the arithmetic of polydiv.hip restated on the host over the same headers (fp.cuh / fz.cuh and the
// lane step, the row sum and the companion matrix of polydiv_step.cuh): the lazy and the reduced step over whole segments, the
// transition tables by repeated squaring, the two-level scan and the second pass from the scanned states, against plain fe_mul /
// fe_sub long division.  Built and run by tests/test_poly_division_host_replay.py; exit status 0 = no mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../plonky_amd/csrc/fp.cuh"
#include "../plonky_amd/csrc/fz.cuh"
#include "../plonky_amd/csrc/polydiv_step.cuh"
#include "replay_io.h"
using namespace plk;
template <class P> Fe<P> rnd_mixed() { return rnd<P>(rand() % 16 < 4 ? 1 + rand() % 4 : 0); }

// one pass over a segment, as pdiv_run_segment does it on the kp lanes of a group
template <class P, bool REDUCE, class EMIT>
void run_segment(const std::vector<Fe<P>>& a, size_t top, std::vector<Fz<P>>& R, const std::vector<Fz<P>>& negb, int k, int kp, EMIT emit) {
    for (int s = 0; s < PDIV_S; ++s) {
        const size_t j = top - s;
        const Fz<P> c = j < a.size() ? fz_from_fe<P>(a[j]) : fz_zero<P>();
        const Fz<P> t = R[k - 1];
        emit(j, t);
        std::vector<Fz<P>> n(kp);
        for (int i = 0; i < kp; ++i) n[i] = pdiv_lane_step<P, REDUCE>(i ? R[i - 1] : c, t, negb[i]);
        R = n;
    }
}
// items in blocks of bsize from the top item of a block down (k_pdiv_scan)
template <class P>
void scan(const std::vector<Fe<P>>& rho, size_t n, size_t bsize, const std::vector<Fe<P>>& tab, const std::vector<Fe<P>>* in, std::vector<Fe<P>>* out_states,
          std::vector<Fe<P>>* totals, int kp) {
    const size_t nblk = (n + bsize - 1) / bsize;
    for (size_t blk = 0; blk < nblk; ++blk) {
        const size_t first = blk * bsize, count = n - first < bsize ? n - first : bsize;
        std::vector<Fe<P>> cur(kp, fe_zero<P>());
        if (in) for (int i = 0; i < kp; ++i) cur[i] = (*in)[blk * kp + i];
        for (size_t it = 0; it < count; ++it) {
            const size_t g = first + count - 1 - it;
            if (out_states) for (int i = 0; i < kp; ++i) (*out_states)[g * kp + i] = cur[i];
            std::vector<Fe<P>> nw(kp);
            for (int i = 0; i < kp; ++i)
                nw[i] = pdiv_row<P>(rho[g * kp + i], kp, [&](int j) { return fz_from_fe<P>(cur[j]); }, [&](int j) { return fz_from_fe<P>(tab[(size_t)j * kp + i]); });
            cur = nw;
        }
        if (totals) for (int i = 0; i < kp; ++i) (*totals)[blk * kp + i] = cur[i];
    }
}
template <class P, bool REDUCE> int run_case(int k, size_t la, bool monic, int edge_mode) {
    int kp = 1; while (kp < k) kp <<= 1;
    int bad = 0;
    std::vector<Fe<P>> a(la), b(k + 1);
    for (auto& v : a) v = edge_mode == 2 ? rnd<P>(3) : edge_mode ? rnd_mixed<P>() : rnd<P>(0);
    for (auto& v : b) v = edge_mode == 2 ? rnd<P>(2 + rand() % 2) : edge_mode ? rnd_mixed<P>() : rnd<P>(0);
    b[k] = monic ? fe_one<P>() : edge_mode ? fe_neg<P>(fe_one<P>()) : rnd<P>(0);
    // reference: schoolbook long division (polynomial.rs:232-259) in plain Montgomery arithmetic
    const Fe<P> inv = fe_inv_safegcd_var<P>(b[k]);
    std::vector<Fe<P>> rem = a, q(la - k);
    for (size_t j = la - k; j-- > 0;) {
        const Fe<P> c = fe_mul<P>(rem[j + k], inv);
        q[j] = c;
        for (int i = 0; i <= k; ++i) rem[j + i] = fe_sub<P>(rem[j + i], fe_mul<P>(c, b[i]));
    }
    // the device's route
    std::vector<Fz<P>> negb(kp, fz_zero<P>());
    std::vector<Fe<P>> negb_rp(kp, fe_zero<P>());
    for (int i = 0; i < k; ++i) { negb_rp[i] = to_rprime<P>(fe_neg<P>(fe_mul<P>(b[i], inv))); negb[i] = fz_from_fe<P>(negb_rp[i]); }
    const Fz<P> factor = fz_from_fe<P>(to_rprime<P>(monic ? fe_one<P>() : inv));
    const size_t nseg = (la + PDIV_S - 1) / PDIV_S, nblk = (nseg + PDIV_B - 1) / PDIV_B;
    std::vector<Fe<P>> m((size_t)kp * kp), t_s, t_sb;
    for (int j = 0; j < kp; ++j) for (int i = 0; i < kp; ++i) m[(size_t)j * kp + i] = pdiv_companion_entry<P>(i, j, k, negb_rp[i]);
    for (int s = 0; s < PDIV_S_LOG + (nblk > 1 ? PDIV_B_LOG : 0); ++s) {
        std::vector<Fe<P>> n2(m.size());
        for (int j = 0; j < kp; ++j) for (int i = 0; i < kp; ++i)
            n2[(size_t)j * kp + i] = pdiv_row<P>(fe_zero<P>(), kp, [&](int l) { return fz_from_fe<P>(m[(size_t)j * kp + l]); }, [&](int l) { return fz_from_fe<P>(m[(size_t)l * kp + i]); });
        m = n2;
        if (s == PDIV_S_LOG - 1) t_s = m;
    }
    t_sb = m;
    std::vector<Fe<P>> rho(nseg * kp), states(nseg * kp), totals(nblk * kp), block_in(nblk * kp);
    for (size_t g = 0; g < nseg; ++g) {
        std::vector<Fz<P>> R(kp, fz_zero<P>());
        run_segment<P, REDUCE>(a, (g + 1) * PDIV_S - 1, R, negb, k, kp, [](size_t, const Fz<P>&) {});
        for (int i = 0; i < kp; ++i) rho[g * kp + i] = i < k ? pdiv_settle<P>(R[i], fz_one_rprime<P>()) : fe_zero<P>();
    }
    if (nblk > 1) {
        scan<P>(rho, nseg, PDIV_B, t_s, nullptr, nullptr, &totals, kp);
        scan<P>(totals, nblk, nblk, t_sb, nullptr, &block_in, nullptr, kp);
    }
    scan<P>(rho, nseg, PDIV_B, t_s, nblk > 1 ? &block_in : nullptr, &states, nullptr, kp);
    std::vector<Fe<P>> gq(nseg * PDIV_S), grem(k);
    for (size_t g = 0; g < nseg; ++g) {
        std::vector<Fz<P>> R(kp);
        for (int i = 0; i < kp; ++i) R[i] = fz_from_fe<P>(states[g * kp + i]);
        run_segment<P, REDUCE>(a, (g + 1) * PDIV_S - 1, R, negb, k, kp, [&](size_t j, const Fz<P>& t) { gq[j] = pdiv_settle<P>(t, factor); });
        if (g == 0) for (int i = 0; i < k; ++i) grem[i] = pdiv_settle<P>(R[i], fz_one_rprime<P>());
    }
    for (size_t j = 0; j < gq.size(); ++j) if (!fe_eq<P>(gq[j], j < la - k ? q[j] : fe_zero<P>())) { if (++bad < 4) printf("q mismatch k %d la %zu j %zu\n", k, la, j); }
    for (int i = 0; i < k; ++i) if (!fe_eq<P>(grem[i], rem[i])) { if (++bad < 4) printf("rem mismatch k %d la %zu i %d\n", k, la, i); }
    return bad;
}
template <class P> int run() {
    int bad = 0;
    const int ks[4] = {1, 3, 8, 32};
    for (int k : ks) {
        const size_t two_level = (size_t)PDIV_S * PDIV_B + 1 + k;  // the first lengths that need the second scan level
        const size_t las[4] = {(size_t)k + 1, (size_t)PDIV_S + k, 2 * (size_t)PDIV_S + 7, two_level + PDIV_S};
        for (int c = 0; c < 4; ++c)
            for (int mode = 0; mode < (c == 3 ? 1 : 3); ++mode) {
                const bool monic = (c + mode) % 2 == 0;
                bad += k > PDIV_LAZY_MAX_K ? run_case<P, true>(k, las[c], monic, mode) : run_case<P, false>(k, las[c], monic, mode);
                if (k <= PDIV_LAZY_MAX_K && c < 3) bad += run_case<P, true>(k, las[c], monic, mode);  // the reduced step is valid at any k
            }
    }
    return bad;
}
int main() {
    srand(20240917);
    int bad = 0;
    bad += run<TweedledeeBaseParams>();
    bad += run<TweedledumBaseParams>();
    bad += run<Bls12377ScalarParams>();
    bad += run<PallasBaseParams>();
    bad += run<VestaBaseParams>();
    printf("mismatches: %d\n", bad);
    return bad ? 1 : 0;
}
