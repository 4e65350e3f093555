// h2c_step.cuh -- blake_field (src/hash_to_curve.rs:13-51) for one (seed, iter), kept apart from the kernels (hash_to_curve.hip) so
// that tests/hash_to_curve_host_replay.cpp walks the same code on the host.  Plain C++17, no field arithmetic: the seed and x are the
// 32-bit little-endian words of CANONICAL values.
//
// The message is seed.to_canonical_u8_vec() || iter || j: 4 NL + 2 <= 50 bytes, and BYTES + 1 <= 49 bytes of extended output are read,
// so the whole hash is ONE call of the BLAKE3 compression function (BLAKE3 specification, section 2.2 - 2.6): chaining value = IV,
// counter 0, block_len = the message length, flags CHUNK_START | CHUNK_END | ROOT, and the 16 output words are the first 64 bytes
// of the extended output.  No tree, no chunk counter, no multi-block path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field_params.cuh"

#ifdef __HIPCC__
#define H2C_HD __host__ __device__ __forceinline__
#else
#define H2C_HD inline
#endif

namespace plk {

constexpr int H2C_TRIES = 256;  // the reference's counters i and j are u8: a 257th try is an overflow there, a status byte here
constexpr uint32_t H2C_B3_FLAGS = 1u | 2u | 8u;  // CHUNK_START | CHUNK_END | ROOT

H2C_HD uint32_t h2c_rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

H2C_HD void h2c_b3_g(uint32_t (&v)[16], int a, int b, int c, int d, uint32_t mx, uint32_t my) {
    v[a] = v[a] + v[b] + mx;
    v[d] = h2c_rotr(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];
    v[b] = h2c_rotr(v[b] ^ v[c], 12);
    v[a] = v[a] + v[b] + my;
    v[d] = h2c_rotr(v[d] ^ v[a], 8);
    v[c] = v[c] + v[d];
    v[b] = h2c_rotr(v[b] ^ v[c], 7);
}

// the root output block of a message of len <= 64 bytes, given as 16 little-endian words padded with zeros
H2C_HD void h2c_blake3_block(const uint32_t (&msg)[16], uint32_t len, uint32_t (&out)[16]) {
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    const int perm[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    uint32_t v[16], m[16];
    for (int k = 0; k < 8; ++k) v[k] = iv[k];
    for (int k = 0; k < 4; ++k) v[8 + k] = iv[k];
    v[12] = 0;  // counter, low and high
    v[13] = 0;
    v[14] = len;
    v[15] = H2C_B3_FLAGS;
    for (int k = 0; k < 16; ++k) m[k] = msg[k];
    for (int round = 0; round < 7; ++round) {
        h2c_b3_g(v, 0, 4, 8, 12, m[0], m[1]);
        h2c_b3_g(v, 1, 5, 9, 13, m[2], m[3]);
        h2c_b3_g(v, 2, 6, 10, 14, m[4], m[5]);
        h2c_b3_g(v, 3, 7, 11, 15, m[6], m[7]);
        h2c_b3_g(v, 0, 5, 10, 15, m[8], m[9]);
        h2c_b3_g(v, 1, 6, 11, 12, m[10], m[11]);
        h2c_b3_g(v, 2, 7, 8, 13, m[12], m[13]);
        h2c_b3_g(v, 3, 4, 9, 14, m[14], m[15]);
        uint32_t t[16];
        for (int k = 0; k < 16; ++k) t[k] = m[perm[k]];
        for (int k = 0; k < 16; ++k) m[k] = t[k];
    }
    for (int k = 0; k < 8; ++k) {
        out[k] = v[k] ^ v[k + 8];
        out[k + 8] = v[k + 8] ^ iv[k];
    }
}

// bit_length(count) + 2 rounds over the work list of either hash to the curve: the expected number of seeds open afterwards is below one
inline int h2c_rounds(size_t count) {
    int bits = 0;
    for (size_t c = count; c; c >>= 1) ++bits;
    return bits + 2 < H2C_TRIES ? bits + 2 : H2C_TRIES;
}

// is_valid_canonical: the value is below the modulus
template <class P> H2C_HD bool h2c_below_modulus(const uint32_t (&c)[P::NL]) {
    for (int k = P::NL - 1; k >= 0; --k)
        if (c[k] != P::MOD[k]) return c[k] < P::MOD[k];
    return false;
}

// blake_field(iter, seed): x (canonical words), y_neg (0/1) and the j at which the hash fell below the modulus.  false when no
// j < H2C_TRIES did (x and y_neg are then unset).
template <class P> H2C_HD bool h2c_blake_field(const uint32_t (&seed)[P::NL], uint32_t iter, uint32_t (&x)[P::NL], uint32_t& y_neg, uint32_t& j_used) {
    constexpr int NL = P::NL;
    constexpr int SHIFT = 32 * NL - P::BITS;  // hash_container[BYTES - 1] >>= 8 * BYTES - BITS: 1, 3 (Bls12377Scalar) or 7 (Bls12377Base)
    static_assert(NL < 16 && SHIFT >= 0 && SHIFT < 8, "one block holds the message, and the shift stays inside the top byte");
    uint32_t m[16], out[16];
    for (int k = 0; k < 16; ++k) m[k] = k < NL ? seed[k] : 0u;
    for (uint32_t j = 0; j < (uint32_t)H2C_TRIES; ++j) {
        m[NL] = (iter & 0xFFu) | (j << 8);  // bytes[BYTES] = iter, bytes[BYTES + 1] = j
        h2c_blake3_block(m, 4u * NL + 2u, out);
        for (int k = 0; k < NL; ++k) x[k] = out[k];
        x[NL - 1] = (out[NL - 1] & 0x00FFFFFFu) | (((out[NL - 1] >> 24) >> SHIFT) << 24);
        if (h2c_below_modulus<P>(x)) {
            y_neg = out[NL] & 1u;  // hash_container[BYTES] & 1
            j_used = j;
            return true;
        }
    }
    return false;
}

}  // namespace plk
