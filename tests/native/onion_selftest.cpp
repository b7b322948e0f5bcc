// onion_selftest.cpp — a stand-alone program over the host build of the onion format's code: the walk's pair formulas against the
// extended-coordinate addition of core/ed25519.h, strings, the expanded key, the scalar arithmetic at its edges, the filter compiler and
// filter_eval_onion on random and edge inputs, checked against identities that hold whatever the inputs (no reference needed).  Built
// with -fsanitize=address,undefined by tests/native/onion.mk and run as a subprocess by tests/test_onion_cli.py: the sanitizers see every
// shift, index and overflow of the code the kernels share.  Exit status 0 and "ok" on success.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed_walk.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/filter.h"
#include "../../vgen_amd/csrc/host/onion_host.h"

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

static void affine_of(const u32 k[8], fe25 &x, fe25 &y) {
    ed_pt e;
    ed_mul_base(e, ed_host_table(), k);
    fe25 zi;
    fe25_inv(zi, e.Z);
    fe25_mul(x, e.X, zi);
    fe25_mul(y, e.Y, zi);
}

// (a + b) B and (a - b) B by the pair formulas against the multiplication itself, a >= b
static void pair_case(const u32 a[8], uint64_t b) {
    const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u32 kb[8], ks[8], kd[8];
    (void)edw_add_u64(kb, zero, b);
    (void)edw_add_u64(ks, a, b);
    {   // kd = a - b
        uint64_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t sub = (uint64_t)kb[i] + borrow;
            borrow = a[i] < sub;
            kd[i] = (u32)(a[i] - sub);
        }
    }
    edw_pt p, q;
    affine_of(a, p.x, p.y);
    affine_of(kb, q.x, q.y);
    fe25 d;
    edw_d(d);
    fe25_mul(p.t, p.x, p.y);
    fe25_mul(p.t, p.t, d);
    fe25_mul(q.t, q.x, q.y);
    fe25 dm, dp, im, ip, xs, ys, xd, yd;
    edw_dens(dm, dp, p.t, q.t);
    fe25_carry(dm);
    fe25_carry(dp);
    fe25_inv(im, dm);
    fe25_inv(ip, dp);
    edw_pair_y(ys, yd, p, q, im, ip);
    edw_pair_x(xs, xd, p, q, im, ip);
    u32 got_s[8], got_d[8], want[8];
    ed_encode(got_s, xs, ys);
    ed_encode(got_d, xd, yd);
    uint8_t enc[32];
    ed_mul_base_encode(ks, enc);
    memcpy(want, enc, 32);
    CHECK(memcmp(got_s, want, 32) == 0);
    ed_mul_base_encode(kd, enc);
    memcpy(want, enc, 32);
    CHECK(memcmp(got_d, want, 32) == 0);
    u32 yo[8];
    edw_encode_y(yo, ys);
    CHECK((yo[7] >> 31) == 0 && (yo[7] | (edw_sign(xs) << 31)) == got_s[7]);
}

int main() {
    // pairs: random scalars with small and large partners, P = Q (b = a is covered by a small a), the neutral partner
    for (int it = 0; it < 24; it++) {
        u32 a[8];
        for (int i = 0; i < 8; i++) a[i] = rnd32();
        a[7] &= 0x7FFFFFFFu;
        a[0] &= ~7u;
        pair_case(a, 0);
        pair_case(a, 8);
        pair_case(a, 8ull * (rnd32() | 1u));
        pair_case(a, ((uint64_t)rnd32() << 32 | rnd32()) & ~7ull);
    }
    {
        const u32 small[8] = {4096, 0, 0, 0, 0, 0, 0, 0};
        pair_case(small, 4096);   // P = Q: the difference is the neutral element
        pair_case(small, 0);
    }
    // strings
    for (int it = 0; it < 64; it++) {
        uint8_t pub[32], back[32];
        for (int i = 0; i < 32; i++) pub[i] = (uint8_t)rnd32();
        if (it == 0) memset(pub, 0, 32);
        if (it == 1) memset(pub, 0xff, 32);
        const std::string s = onion_encode(pub);
        CHECK(s.size() == 56 && s[55] == 'd' && strchr("aiqy", s[54]) != nullptr);
        CHECK(onion_decode(s, back) && memcmp(pub, back, 32) == 0);
        CHECK(onion_decode(s + ".onion", back));
        std::string t = s;
        t[10] = t[10] == 'a' ? 'b' : 'a';
        CHECK(!onion_decode(t, back));                         // checksum
        t = s;
        t[3] = (char)(t[3] >= 'a' ? t[3] - 32 : '1');
        CHECK(!onion_decode(t, back));                         // upper case / outside the alphabet
        CHECK(!onion_decode(s.substr(1), back) && !onion_decode(s + "a", back) && !onion_decode("", back));
        CHECK(address_from_payload(VGF_ONION, pub) == (it == 0 ? std::string() : s));   // (all zero: the dump's "no key" mark has no address)
        uint8_t pl[32];
        CHECK(payload_from_address(VGF_ONION, s, pl) && memcmp(pl, pub, 32) == 0);
    }
    // the expanded key and the scalars
    {
        uint8_t a[32] = {0}, b[32], ea[64], eb[64];
        a[0] = 8;
        a[31] = 0x40;
        CHECK(onion_scalar_at(a, 1, b) && b[0] == 16);
        onion_expand(a, ea);
        onion_expand(b, eb);
        CHECK(memcmp(ea, a, 32) == 0 && memcmp(eb, b, 32) == 0 && memcmp(ea + 32, eb + 32, 32) != 0);
        uint8_t top[32];
        memset(top, 0xff, 32);
        top[0] = 0xf8;
        top[31] = 0x7f;                                        // 2^255 - 8: the last scalar
        CHECK(onion_scalar_at(top, 0, b) && !onion_scalar_at(top, 1, b) && !onion_scalar_at(top, UINT64_MAX, b));
        CHECK(!onion_scalar_at(a, UINT64_MAX, b) || b[31] < 0x80);
        uint8_t seed[24] = {1}, base[32];
        onion_base(rnd_seed_from_bytes(seed), 3, base);
        CHECK((base[0] & 7) == 0 && (base[31] & 0xC0) == 0x40);
        uint8_t pub[32], pl[32];
        onion_public_key(base, pub);
        CHECK(payload_from_key(VGF_ONION, base, pl) == 32 && memcmp(pl, pub, 32) == 0);
    }
    // the filter compiler and the device test: a prefix taken from an address accepts it, whatever bit 7 of byte 31 says
    const char *shapes[] = {"^%.1s", "^%.6s", "^%.7s", "^%.13s", "^%.49s", "^%.52s", "%.3s$", "%.2s", "^[a-d]%.0s", "^.*%.0s", "^%.3s.*d$"};
    for (const char *shape : shapes)
        for (int it = 0; it < 8; it++) {
            uint8_t pub[32];
            for (int i = 0; i < 32; i++) pub[i] = (uint8_t)rnd32();
            const std::string s = onion_encode(pub);
            char pat[96];
            if (strstr(shape, "$") && shape[0] == '%') snprintf(pat, sizeof pat, "%s$", s.substr(56 - 3).c_str());
            else snprintf(pat, sizeof pat, shape, s.c_str());
            vgen_filter f;
            std::string err;
            CHECK(filter_compile(pat, it & 1, VGF_ONION, f, err));
            CHECK(f.dev.kind == DEVF_MASKED || f.dev.kind == DEVF_ALL || f.dev.kind == DEVF_HOST_ALL);
            CHECK(f.dev.count <= DEVF_MAX_TESTS);
            u32 pl[8];
            memcpy(pl, pub, 32);
            const bool full = f.dfa.is_match(s);
            if (f.dev.kind != DEVF_HOST_ALL && full) CHECK(filter_eval_onion(&f.dev, pl));
            pl[7] ^= 0x80000000u;
            if (f.dev.kind != DEVF_HOST_ALL && full) CHECK(filter_eval_onion(&f.dev, pl));
            if (f.dev.kind == DEVF_MASKED)
                for (u32 t = 0; t < f.dev.count; t++) CHECK((f.dev.tests[t].a[7] & 0xFFu) == 0);   // nothing past character 48
        }
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
