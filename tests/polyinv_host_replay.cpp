// polyinv_host_replay.cpp -- the per-lane steps of polydiv_newton.hip (polyinv_step.cuh) walked on the host, lane by lane, in the order
// the kernels and their host side use them: the seed recurrence, Newton levels (the transforms are plain O(N^2) sums here), the
// quotient's correlation, the remainder, and the index maps.  Reads commands from the file named on the command line and prints stored
// words; tests/test_poly_div_rem_host_replay.py compares them with Python integers.
//   inv <field> <reversed> <n> <len> <len words>            -> g: n words (reversed: the series is rev of the words)
//   div <field> <la> <lb> <q_len> <la words> <lb words>     -> q: q_len words, rem: lb - 1 words
//   maps <m> <q_len>                                        -> the index maps, as integers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../plonky_amd/csrc/fp.cuh"
#include "../plonky_amd/csrc/fz.cuh"
#include "../plonky_amd/csrc/polyinv_step.cuh"
#include "replay_io.h"
using namespace plk;

template <class P> Fe<P> read_word(FILE* f) {  // big-endian hex of the 256-bit stored word
    Fe<P> r;
    if (!read_fe<P>(f, r)) exit(2);
    return r;
}
template <class P> void print_words(const char* tag, const std::vector<Fe<P>>& v) {
    printf("%s", tag);
    for (const auto& e : v) printf(" %s", hex_words(e.v).c_str());
    printf("\n");
}
template <class P> using Vec = std::vector<Fe<P>>;

// the transform the device runs, as a plain sum: out[k] = sum_i in[i] w^(i k), in zero-padded to n; inverse: w^-1 and 1 / n
template <class P> Vec<P> dft(const Fe<P>* in, size_t in_len, size_t n, bool inverse, bool rprime) {
    int log_n = 0;
    while (((size_t)1 << log_n) < n) ++log_n;
    Fe<P> w = fe_from_words<P>(P::ROOT_2ADIC);
    for (int i = 0; i < P::TWO_ADICITY - log_n; ++i) w = fe_sqr<P>(w);
    Vec<P> pw(n);
    pw[0] = fe_one<P>();
    for (size_t i = 1; i < n; ++i) pw[i] = fe_mul<P>(pw[i - 1], w);
    Fe<P> scale = fe_one<P>();
    if (inverse) {
        Fe<P> c = fe_zero<P>();
        c.v[0] = (uint32_t)n;
        scale = fe_inv_safegcd_var<P>(fe_from_canonical<P>(c));
    }
    Vec<P> out(n);
    for (size_t k = 0; k < n; ++k) {
        Fe<P> s = fe_zero<P>();
        for (size_t i = 0; i < in_len; ++i) s = fe_add<P>(s, fe_mul<P>(in[i], pw[((inverse ? n - k : k) * i) & (n - 1)]));
        s = fe_mul<P>(s, scale);
        out[k] = rprime ? to_rprime<P>(s) : s;
    }
    return out;
}

// pinv_inverse_t: g[0 .. n) of the series src (len words, reversed or not)
template <class P> Vec<P> inverse(const Vec<P>& src, bool reversed, size_t n) {
    Vec<P> g(n, fe_zero<P>());
    const size_t len = src.size(), cnt = n < (size_t)PINV_SEED ? n : (size_t)PINV_SEED;
    // k_pinv_seed, lane by lane
    Vec<P> h(cnt), acc(cnt, fe_zero<P>());
    for (size_t t = 0; t < cnt; ++t) {
        size_t idx = 0;
        h[t] = pinv_series_index(reversed, len, t, idx) ? src[idx] : fe_zero<P>();
    }
    const Fe<P> inv = fe_inv_safegcd<P>(h[0]), neg_inv = fe_neg<P>(inv);
    for (size_t i = 0; i < cnt; ++i) {
        g[i] = pinv_seed_coeff<P>(i, acc[i], inv, neg_inv);
        for (size_t t = i + 1; t < cnt; ++t) acc[t] = pinv_seed_accumulate<P>(acc[t], h[t - i], g[i]);
    }
    for (size_t l = PINV_SEED; l < n; l *= 2) {
        const size_t t = n - l < l ? n : 2 * l, tp = t < len ? t : len, size = 4 * l;
        const Fe<P>* chunk = reversed ? src.data() + (len - tp) : src.data();
        Vec<P> ex = dft<P>(g.data(), l, size, false, true), ey = dft<P>(chunk, tp, size, false, false);
        for (size_t i = 0; i < size; ++i) ex[i] = pinv_newton_point<P>(ex[i], ey[reversed ? pinv_neg_index(i, size) : i]);  // k_pinv_pointwise
        const Vec<P> prod = dft<P>(ex.data(), size, size, true, false);
        for (size_t u = l; u < t; ++u) g[u] = pinv_update_coeff<P>(prod[pinv_shift_index(u, reversed ? tp - 1 : 0, size)]);  // k_pinv_update
    }
    return g;
}

template <class P> int cmd_inv(FILE* f) {
    int reversed = 0;
    size_t n = 0, len = 0;
    if (fscanf(f, "%d %zu %zu", &reversed, &n, &len) != 3) return 2;
    Vec<P> src(len);
    for (auto& e : src) e = read_word<P>(f);
    print_words<P>("g", inverse<P>(src, reversed != 0, n));
    return 0;
}

static size_t product_size(size_t len) {
    size_t n = (size_t)4 * PINV_SEED;
    while (n < len) n *= 2;
    return n;
}

// pdiv_newton_t
template <class P> int cmd_div(FILE* f) {
    size_t la = 0, lb = 0, q_len = 0;
    if (fscanf(f, "%zu %zu %zu", &la, &lb, &q_len) != 3) return 2;
    Vec<P> a(la), b(lb);
    for (auto& e : a) e = read_word<P>(f);
    for (auto& e : b) e = read_word<P>(f);
    const size_t k = lb - 1, m = la - k, lq = m < k ? m : k;
    const Vec<P> g = inverse<P>(b, true, m);
    const size_t nq = product_size(2 * m - 1);
    Vec<P> ex = dft<P>(g.data(), m, nq, false, true), ey = dft<P>(a.data() + k, m, nq, false, false);
    for (size_t i = 0; i < nq; ++i) ey[i] = pinv_product_point<P>(ex[pinv_neg_index(i, nq)], ey[i]);
    Vec<P> prod = dft<P>(ey.data(), nq, nq, true, false), q(q_len);
    for (size_t s = 0; s < q_len; ++s) {  // k_pinv_quotient
        size_t src = 0;
        q[s] = pinv_quotient_index(s, m, src) ? prod[src] : fe_zero<P>();
    }
    const size_t nr = product_size(lq + k - 1);
    ex = dft<P>(q.data(), lq, nr, false, true);
    ey = dft<P>(b.data(), k, nr, false, false);
    for (size_t i = 0; i < nr; ++i) ey[i] = pinv_product_point<P>(ex[i], ey[i]);
    prod = dft<P>(ey.data(), nr, nr, true, false);
    Vec<P> rem(k);
    for (size_t i = 0; i < k; ++i) rem[i] = pinv_rem_coeff<P>(a[i], prod[i]);  // k_pinv_rem
    print_words<P>("q", q);
    print_words<P>("rem", rem);
    return 0;
}

static int cmd_maps(FILE* f) {
    size_t m = 0, q_len = 0;
    if (fscanf(f, "%zu %zu", &m, &q_len) != 2) return 2;
    printf("maps");
    for (size_t s = 0; s < q_len; ++s) {  // the quotient's sources, -1: zero
        size_t src = 0;
        printf(" %ld", pinv_quotient_index(s, m, src) ? (long)src : -1L);
    }
    printf(" |");
    for (int reversed = 0; reversed < 2; ++reversed)  // coefficient j of a series of m words, one past its end included
        for (size_t j = 0; j <= m; ++j) {
            size_t src = 0;
            printf(" %ld", pinv_series_index(reversed != 0, m, j, src) ? (long)src : -1L);
        }
    printf(" |");
    for (size_t i = 0; i < 8; ++i) printf(" %zu", pinv_neg_index(i, 8));
    printf(" |");
    for (size_t t = 0; t < 8; ++t) printf(" %zu", pinv_shift_index(t, m, 8));
    printf("\n");
    return 0;
}

template <class P> int run_field(const std::string& cmd, FILE* f) { return cmd == "inv" ? cmd_inv<P>(f) : cmd_div<P>(f); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        int rc = 2, field = -1;
        if (std::string(cmd) == "maps") rc = cmd_maps(f);
        else if (fscanf(f, "%d", &field) == 1) {
            if (field == 0) rc = run_field<TweedledeeBaseParams>(cmd, f);
            if (field == 1) rc = run_field<TweedledumBaseParams>(cmd, f);
            if (field == 2) rc = run_field<Bls12377ScalarParams>(cmd, f);
            if (field == 4) rc = run_field<PallasBaseParams>(cmd, f);
            if (field == 5) rc = run_field<VestaBaseParams>(cmd, f);
        }
        if (rc) return rc;
    }
    fclose(f);
    return 0;
}
