// scalar_mul_host_replay.cpp -- plonky_amd/csrc/scalar_mul_step.cuh (the chunk decoding and n(s), the signed-digit recoding, the
// split along the endomorphism and the addend selections: the code the kernels of scalar_mul.hip run) compiled for the host and run
// as a program of its own: tests/test_scalar_mul_host_replay.py builds it plain and under AddressSanitizer + UBSan and compares
// what it prints with tests/halo_endo_ref.py.
//
//   scalar_mul_host_replay CASES
// CASES is a stream of tokens; field elements are Montgomery words, 8 NL hex digits, most significant first:
//   N curve bits s          ->  "N curve bits c0c1..  n"        the chunks (one digit each, chunk 0 first) and n(s)
//   D curve k               ->  "D curve carry d0 d1 .. d127"   k: 64 hex digits, a plain 256-bit integer; signed base-4 digits
//   G curve s               ->  "G curve squared n1 k1 n2 k2"   the halves of glv_split: signs and magnitudes (64 hex digits)
//   A curve x y             ->  "A curve tx0 ty0 .. tx3 ty3"    the addend of halo_addend for chunks 0 .. 3
//   S curve n1 n2 x y       ->  "S curve tx1 ty1 tx2 ty2 tx3 ty3"   the addend of sm_glv_addend for column codes 1 .. 3
//   W curve x y             ->  "W curve x2 y2 tx ty (d = -1) tx ty (d = 1) tx ty (d = 2)"   sm_affine_double and sm_w2_addend over {P, 2P}
//   M curve s x y           ->  "M curve zero x y"              sm_scalar_mul_chain: every chain step of k_scalar_mul, then x = X / ZZ, y = Y / ZZZ
//   H curve bits s x y      ->  "H curve bits zero x y"         halo_n_mul_chain: every halo_chain_step of k_halo_n_mul
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../plonky_amd/csrc/ec.cuh"
#include "../plonky_amd/csrc/scalar_mul_step.cuh"
#include "replay_io.h"

using namespace plk;

template <class C> static int halo_n_case(FILE* fh, int curve) {
    using SP = typename C::SP;
    std::string bs;
    Fe<SP> s;
    if (!token(fh, bs) || !read_words(fh, s.v)) return 1;
    const unsigned bits = (unsigned)atoi(bs.c_str());
    if (bits == 0 || (bits & 1u) || bits > (unsigned)SP::BITS) return 1;
    const Fe<SP> k = fe_to_canonical<SP>(s);
    printf("N %d %u ", curve, bits);
    for (unsigned c = 0; c < bits / 2; ++c) printf("%u", halo_chunk(k.v, (int)c));
    printf(" %s\n", hex_words(halo_n_value<C>(k.v, bits).v).c_str());
    return 0;
}

static int digits_case(FILE* fh, int curve) {
    uint32_t k[8], e[8];
    if (!read_words(fh, k)) return 1;
    const uint32_t carry = sm_recode_w2(k, e);
    printf("D %d %u", curve, carry);
    for (int j = 0; j < SM_W2_DIGITS; ++j) printf(" %d", sm_digit_w2(e, j));
    printf("\n");
    return 0;
}

template <class C> static int glv_case(FILE* fh, int curve) {
    using SP = typename C::SP;
    Fe<SP> s;
    if (!read_words(fh, s.v)) return 1;
    const Fe<SP> k = fe_to_canonical<SP>(s);
    uint32_t k1[8], k2[8];
    glv_split<typename C::Glv>(k.v, k1, k2);
    const int n1 = (int)(k1[7] >> 31), n2 = (int)(k2[7] >> 31);
    k1[7] &= 0x7fffffffu;
    k2[7] &= 0x7fffffffu;
    printf("G %d %d %d %s %d %s\n", curve, HaloZeta<typename C::Glv>::SQUARED ? 1 : 0, n1, hex_words(k1).c_str(), n2, hex_words(k2).c_str());
    return 0;
}

template <class C> static int halo_addend_case(FILE* fh, int curve) {
    using FP = typename C::FP;
    Fe<FP> px, py;
    if (!read_words(fh, px.v) || !read_words(fh, py.v)) return 1;
    const Fz<FP> x = sm_enter<FP>(px), y = sm_enter<FP>(py), zx = sm_enter<FP>(fe_mul<FP>(halo_zeta<C>(), px)), ny = fz_neg_canonical<FP>(y);
    printf("A %d", curve);
    for (uint32_t ch = 0; ch < 4; ++ch) {
        Fz<FP> tx, ty;
        halo_addend<FP>(ch, x, zx, y, ny, tx, ty);
        printf(" %s %s", hex_words(sm_leave<FP>(tx).v).c_str(), hex_words(sm_leave<FP>(ty).v).c_str());
    }
    printf("\n");
    return 0;
}

template <class C> static int glv_addend_case(FILE* fh, int curve) {
    using FP = typename C::FP;
    std::string a, b;
    Fe<FP> px, py;
    if (!token(fh, a) || !token(fh, b) || !read_words(fh, px.v) || !read_words(fh, py.v)) return 1;
    const bool n1 = a == "1", n2 = b == "1";
    const Fe<FP> inv = fe_inv<FP>(sm_glv_den<C>(px));
    Fz<FP> x, y, bx, x3, y3;
    sm_glv_table<C>(px, py, inv, n1, n2, x, y, bx, x3, y3);
    printf("S %d", curve);
    for (uint32_t c = 1; c < 4; ++c) {
        Fz<FP> tx, ty;
        sm_glv_addend<FP>(c, n1, n2, x, bx, x3, y, y3, tx, ty);
        printf(" %s %s", hex_words(sm_leave<FP>(tx).v).c_str(), hex_words(sm_leave<FP>(ty).v).c_str());
    }
    printf("\n");
    return 0;
}

template <class C> static int w2_addend_case(FILE* fh, int curve) {
    using FP = typename C::FP;
    Fe<FP> px, py, x2_r, y2_r;
    if (!read_words(fh, px.v) || !read_words(fh, py.v)) return 1;
    sm_affine_double<FP>(px, py, fe_inv<FP>(fe_dbl<FP>(py)), x2_r, y2_r);
    const Fz<FP> x1 = sm_enter<FP>(px), y1 = sm_enter<FP>(py), x2 = sm_enter<FP>(x2_r), y2 = sm_enter<FP>(y2_r);
    printf("W %d %s %s", curve, hex_words(x2_r.v).c_str(), hex_words(y2_r.v).c_str());
    for (int d : {-1, 1, 2}) {
        Fz<FP> tx, ty;
        bool two;
        sm_w2_addend<FP>(d, x1, y1, x2, y2, tx, ty, two);
        if (two != (d == 2)) return 1;
        printf(" %s %s", hex_words(sm_leave<FP>(tx).v).c_str(), hex_words(sm_leave<FP>(ty).v).c_str());
    }
    printf("\n");
    return 0;
}

// the affine point of a chain's result: "zero x y"
template <class FP> static void print_affine(const XyzzZ<FP>& acc) {
    Fe<FP> x = fe_zero<FP>(), y = fe_zero<FP>();
    const Fe<FP> zz = acc.inf ? fe_zero<FP>() : sm_leave<FP>(acc.zz);
    const bool zero = acc.inf || fe_is_zero<FP>(zz);
    if (!zero) {
        x = fe_mul<FP>(sm_leave<FP>(acc.x), fe_inv<FP>(zz));
        y = fe_mul<FP>(sm_leave<FP>(acc.y), fe_inv<FP>(sm_leave<FP>(acc.zzz)));
    }
    printf(" %d %s %s\n", zero ? 1 : 0, hex_words(x.v).c_str(), hex_words(y.v).c_str());
}

template <class C> static int scalar_mul_case(FILE* fh, int curve) {
    using FP = typename C::FP;
    using SP = typename C::SP;
    Fe<SP> s;
    Fe<FP> px, py;
    if (!read_words(fh, s.v) || !read_words(fh, px.v) || !read_words(fh, py.v)) return 1;
    const Fe<SP> k = fe_to_canonical<SP>(s);
    printf("M %d", curve);
    print_affine<FP>(sm_scalar_mul_chain<C>(k.v, px, py, fe_inv<FP>(sm_table_den<C>(px, py))));
    return 0;
}

template <class C> static int halo_n_mul_case(FILE* fh, int curve) {
    using FP = typename C::FP;
    using SP = typename C::SP;
    std::string bs;
    Fe<SP> s;
    Fe<FP> px, py;
    if (!token(fh, bs) || !read_words(fh, s.v) || !read_words(fh, px.v) || !read_words(fh, py.v)) return 1;
    const unsigned bits = (unsigned)atoi(bs.c_str());
    if (bits == 0 || (bits & 1u) || bits > (unsigned)SP::BITS) return 1;
    const Fe<SP> k = fe_to_canonical<SP>(s);
    printf("H %d %u", curve, bits);
    print_affine<FP>(halo_n_mul_chain<C>(k.v, bits, px, py));
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
    std::string kind, cs;
    int rc = 0;
    while (rc == 0 && token(fh, kind) && token(fh, cs)) {
        const int curve = atoi(cs.c_str());
        int m = 1;
        if (kind == "D") {
            m = digits_case(fh, curve);
        } else {
            m = with_curve(curve, [&](auto t) {
                using C = tag_t<decltype(t)>;
                if (kind == "W") return w2_addend_case<C>(fh, curve);
                if (kind == "M") return scalar_mul_case<C>(fh, curve);
                if constexpr (C::Glv::ENABLED) {
                    if (kind == "H") return halo_n_mul_case<C>(fh, curve);
                    if (kind == "N") return halo_n_case<C>(fh, curve);
                    if (kind == "G") return glv_case<C>(fh, curve);
                    if (kind == "A") return halo_addend_case<C>(fh, curve);
                    if (kind == "S") return glv_addend_case<C>(fh, curve);
                }
                return 1;
            });
        }
        if (m != 0) {
            fprintf(stderr, "bad case: %s %s\n", kind.c_str(), cs.c_str());
            rc = 1;
        }
    }
    fclose(fh);
    return rc;
}
