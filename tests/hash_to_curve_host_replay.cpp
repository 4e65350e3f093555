// hash_to_curve_host_replay.cpp -- plonky_amd/csrc/h2c_step.cuh (the BLAKE3 block and blake_field) compiled for the host and run as a
// program of its own: tests/test_hash_to_curve_host_replay.py builds it plain and under AddressSanitizer + UBSan and compares what
// it prints with tests/hash_to_curve_ref.py.
//
//   hash_to_curve_host_replay CASES
// prints three digest lines (BLAKE3(""), bytes 32..63 of its extended output, BLAKE3("abc")), then one line per case of CASES
// ("field seed_hex iter" per line, seed canonical): "field seed_hex iter ok x_hex y_neg j".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../plonky_amd/csrc/dispatch.cuh"
#include "../plonky_amd/csrc/h2c_step.cuh"
#include "replay_io.h"

using namespace plk;

static std::string hex_bytes(const uint32_t* w, int first_byte, int n_bytes) {  // bytes in order, as a digest is written
    std::string s;
    char buf[3];
    for (int b = first_byte; b < first_byte + n_bytes; ++b) {
        snprintf(buf, sizeof(buf), "%02x", (unsigned)((w[b / 4] >> (8 * (b % 4))) & 0xFF));
        s += buf;
    }
    return s;
}
static void digest(const char* text, int first_byte) {
    uint32_t m[16] = {0}, out[16];
    const size_t len = strlen(text);
    for (size_t k = 0; k < len; ++k) m[k / 4] |= (uint32_t)(unsigned char)text[k] << (8 * (k % 4));
    h2c_blake3_block(m, (uint32_t)len, out);
    printf("%s\n", hex_bytes(out, first_byte, 32).c_str());
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    digest("", 0);
    digest("", 32);
    digest("abc", 0);
    FILE* fh = fopen(argv[1], "r");
    if (!fh) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int field = 0;
    unsigned iter = 0;
    char seed_hex[128];
    int rc = 0;
    while (fscanf(fh, "%d %127s %u", &field, seed_hex, &iter) == 3) {
        const std::string sh(seed_hex);
        const int m = with_field(field, [&](auto t) {
            using P = tag_t<decltype(t)>;
            if (sh.size() != (size_t)P::NL * 8) return 1;
            uint32_t seed[P::NL], x[P::NL] = {0}, y_neg = 0, j = 0;
            for (int k = 0; k < P::NL; ++k) seed[k] = (uint32_t)strtoul(sh.substr((size_t)(P::NL - 1 - k) * 8, 8).c_str(), nullptr, 16);
            const bool ok = h2c_blake_field<P>(seed, iter, x, y_neg, j);
            printf("%d %s %u %d %s %u %u\n", field, sh.c_str(), iter, ok ? 1 : 0, hex_words(x).c_str(), y_neg, j);
            return 0;
        });
        if (m != 0) {
            fprintf(stderr, "bad case: field %d seed %s\n", field, seed_hex);
            rc = 1;
        }
    }
    fclose(fh);
    return rc;
}
