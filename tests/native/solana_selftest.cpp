// solana_selftest.cpp — a stand-alone program over the host build of the Solana format's code: field functions, multiplication, filter
// compile and host derivation on edge and random inputs, checked against identities that hold whatever the inputs (no reference
// needed).  Built with -fsanitize=address,undefined by tests/native/solana.mk and run as a subprocess by tests/test_solana.py: the
// sanitizers see every shift, index and overflow of the code the kernels share.  Exit status 0 and "ok" on success.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed25519.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/ed_host.h"
#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                       \
        }                                                     \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static bool same(fe25 a, fe25 b) {
    fe25_reduce(a);
    fe25_reduce(b);
    return memcmp(a.n, b.n, sizeof a.n) == 0;
}

static void field_cases(const u32 w[8]) {
    fe25 a, one, t, u, inv;
    fe25_from_words(a, w);
    fe25_set_one(one);
    fe25_mul(t, a, one);
    CHECK(same(t, a));
    fe25_sqr(t, a);
    fe25_mul(u, a, a);
    CHECK(same(t, u));
    fe25_add(t, a, a);          // magnitude 2: (2a)^2 = 4 a^2
    fe25_sqr(t, t);
    fe25_add(u, u, u);
    fe25_add(u, u, u);
    CHECK(same(t, u));
    fe25_sub<1>(t, a, a);
    fe25 zero;
    fe25_set_zero(zero);
    CHECK(same(t, zero));
    fe25_inv(inv, a);
    fe25_mul(t, inv, a);
    fe25 ar = a;
    fe25_reduce(ar);
    bool is_zero = true;
    for (int i = 0; i < 9; i++) is_zero = is_zero && ar.n[i] == 0;
    CHECK(same(t, is_zero ? zero : one));
    // canonical form: limbs strict, top limb below 2^23, and the words round-trip
    CHECK(ar.n[8] < (1u << 23));
    for (int i = 0; i < 9; i++) CHECK(ar.n[i] <= F25_M29);
    u32 back[8];
    fe25_to_words(back, ar);
    fe25 again;
    fe25_from_words(again, back);
    CHECK(memcmp(again.n, ar.n, sizeof ar.n) == 0);
}

int main() {
    // field: the edges of the byte input and random values
    const u32 P[8] = {0xffffffedu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};
    u32 w[8];
    for (int c = 0; c < 8; c++) {
        memset(w, 0, sizeof w);
        switch (c) {
        case 1: w[0] = 1; break;
        case 2: w[0] = 19; break;
        case 3: memcpy(w, P, sizeof w); w[0]--; break;
        case 4: memcpy(w, P, sizeof w); break;
        case 5: memcpy(w, P, sizeof w); w[0]++; break;
        case 6: memset(w, 0xff, sizeof w); w[7] = 0x7fffffffu; break;
        case 7: memset(w, 0xff, sizeof w); break;
        }
        field_cases(w);
    }
    for (int r = 0; r < 200; r++) {
        for (int i = 0; i < 8; i++) w[i] = rnd32();
        field_cases(w);
    }
    // limb patterns of all ones at the magnitudes the functions state: products at m_a * m_b = 6, the carry at 7
    {
        fe25 a, b, t, u, v;
        for (int i = 0; i < 9; i++) {
            a.n[i] = 2u * ((1u << 29) + (1u << 17));
            b.n[i] = 3u * ((1u << 29) + (1u << 17));
        }
        fe25_mul(t, a, b);
        u = a;
        v = b;
        fe25_carry(u);
        fe25_carry(v);
        fe25_mul(u, u, v);
        CHECK(same(t, u));
        for (int i = 0; i < 9; i++) a.n[i] = 7u * ((1u << 29) + (1u << 17));
        u = a;
        fe25_carry(u);
        CHECK(same(u, a));
    }
    // multiplication: (k + 1) B = k B + B through the group law is what the table encodes; here the order: L * B is the neutral element
    const u32 L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
    uint8_t out[32], neutral[32] = {1};
    ed_mul_base_encode(L, out);
    CHECK(memcmp(out, neutral, 32) == 0);
    memset(w, 0, sizeof w);
    ed_mul_base_encode(w, out);
    CHECK(memcmp(out, neutral, 32) == 0);
    {   // L + 1 and 1 give the base point; L - 1 its negative (same y, other sign)
        uint8_t b1[32], b2[32];
        memcpy(w, L, sizeof w);
        w[0]++;
        ed_mul_base_encode(w, b1);
        memset(w, 0, sizeof w);
        w[0] = 1;
        ed_mul_base_encode(w, b2);
        CHECK(memcmp(b1, b2, 32) == 0);
        memcpy(w, L, sizeof w);
        w[0]--;
        ed_mul_base_encode(w, b1);
        b1[31] ^= 0x80;
        CHECK(memcmp(b1, b2, 32) == 0);
        memset(w, 0xff, sizeof w);   // every window 255
        ed_mul_base_encode(w, b1);
        CHECK(b1[0] != 0 || b1[1] != 0);
    }
    // derivation, strings and the filter on random seeds
    for (int r = 0; r < 3; r++) {
        uint8_t seed[32], pub[32], dec[32];
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)rnd32();
        ed_public_key(seed, pub);
        const std::string addr = address_from_payload(VGF_SOLANA, pub);
        CHECK(addr.size() >= 32 && addr.size() <= 44);
        CHECK(solana_decode(addr, dec) && memcmp(dec, pub, 32) == 0);
        CHECK(solana_keypair_base58(seed).size() <= 88);
        for (int plen = 1; plen <= 2; plen++)
            for (int ci = 0; ci < 2; ci++) {
                vgen_filter f;
                std::string err;
                const std::string pats[3] = {"^" + addr.substr(0, plen), addr.substr(addr.size() - plen) + "$",
                                             "^" + addr.substr(0, 1) + ".*" + addr.substr(addr.size() - plen) + "$"};
                for (const std::string &pat : pats) {
                    CHECK(filter_compile(pat, ci != 0, VGF_SOLANA, f, err));
                    u32 pl[8];
                    memcpy(pl, pub, 32);
                    CHECK(f.dfa.is_match(addr));
                    CHECK(f.dev.kind == DEVF_HOST_ALL || filter_eval_sol(&f.dev, pl));   // superset: a match is never rejected
                }
            }
    }
    CHECK(!solana_decode("", out) && !solana_decode("0", out) && !solana_decode("1", out) && !solana_decode(std::string(45, 'z'), out));
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
