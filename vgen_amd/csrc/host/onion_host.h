// onion_host.h — the host's side of the onion format (VGF_ONION): Tor v3 address strings, the expanded secret key Tor loads, and the
// scalars a scan walks.  Header-only, like ed_host.h, whose table and multiplication it uses.
//   sha3_256               FIPS 202 (Keccak-f of core/hash.h, padding byte 0x06)
//   onion_encode           56 lowercase Base32 characters of A[32] || checksum[2] || 0x03, checksum = SHA3-256(".onion checksum" || A || 0x03)[0..2]
//   onion_decode           strict: 56 characters of a-z2-7 (an optional trailing ".onion"), version 3, a matching checksum
//   onion_public_key       A = a B for a scalar given as 32 little-endian bytes (any 256-bit value)
//   onion_expand           the 64 bytes of hs_ed25519_secret_key's body: the scalar || a nonce key that is a hash of the scalar
//   onion_base             the base scalar of stream `stream` of a scan's seed: clamped, so in [2^254, 2^255) and a multiple of 8
//   onion_scalar_at        base + 8 index as little-endian bytes; false when that reaches 2^255
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../core/ed_walk.h"
#include "../core/hash.h"
#include "../core/rnd.h"
#include "../core/sha512.h"
#include "ed_host.h"
#include "scalar.h"

namespace vg {

inline void sha3_256(const uint8_t *msg, size_t len, uint8_t out[32]) {
    const size_t RATE = 136;
    u64 a[25];
    memset(a, 0, sizeof a);
    std::vector<uint8_t> buf(msg, msg + len);
    buf.push_back(0x06);
    while (buf.size() % RATE != 0) buf.push_back(0);
    buf.back() |= 0x80;
    for (size_t off = 0; off < buf.size(); off += RATE) {
        for (size_t i = 0; i < RATE / 8; i++) {
            u64 w = 0;
            for (int j = 7; j >= 0; j--) w = (w << 8) | buf[off + 8 * i + j];
            a[i] ^= w;
        }
        keccak_f1600(a);
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++) out[8 * i + j] = (uint8_t)(a[i] >> (8 * j));
}

inline const char *onion_alphabet() { return "abcdefghijklmnopqrstuvwxyz234567"; }

inline void onion_checksum(const uint8_t pub[32], uint8_t chk[2]) {
    uint8_t m[15 + 32 + 1], h[32];
    memcpy(m, ".onion checksum", 15);
    memcpy(m + 15, pub, 32);
    m[47] = 0x03;
    sha3_256(m, sizeof m, h);
    chk[0] = h[0];
    chk[1] = h[1];
}

inline std::string onion_encode(const uint8_t pub[32]) {
    uint8_t b[35];
    memcpy(b, pub, 32);
    onion_checksum(pub, b + 32);
    b[34] = 0x03;
    std::string s(56, 'a');
    for (int c = 0; c < 56; c++) {
        const int bit = 5 * c, by = bit >> 3, o = bit & 7;
        const unsigned v = ((unsigned)b[by] << 8 | (by + 1 < 35 ? b[by + 1] : 0u)) >> (11 - o);
        s[c] = onion_alphabet()[v & 31u];
    }
    return s;
}

inline bool onion_decode(const std::string &text, uint8_t pub[32]) {
    std::string s = text;
    if (s.size() == 62 && s.compare(56, 6, ".onion") == 0) s.resize(56);
    if (s.size() != 56) return false;
    uint8_t b[35];
    memset(b, 0, sizeof b);
    for (int c = 0; c < 56; c++) {
        const char *p = s[c] ? strchr(onion_alphabet(), s[c]) : nullptr;
        if (!p) return false;   // (upper case, 0 1 8 9 and everything else)
        const unsigned v = (unsigned)(p - onion_alphabet());
        for (int k = 0; k < 5; k++) {
            const int bit = 5 * c + k;
            if ((v >> (4 - k)) & 1u) b[bit >> 3] |= (uint8_t)(0x80u >> (bit & 7));
        }
    }
    uint8_t chk[2];
    onion_checksum(b, chk);
    if (b[34] != 0x03 || b[32] != chk[0] || b[33] != chk[1]) return false;
    memcpy(pub, b, 32);
    return true;
}

inline void onion_words_le(const uint8_t b[32], u32 w[8]) {
    for (int i = 0; i < 8; i++) w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
}
inline void onion_bytes_le(const u32 w[8], uint8_t b[32]) {
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) b[4 * i + k] = (uint8_t)(w[i] >> (8 * k));
}

inline void onion_public_key(const uint8_t scalar_le[32], uint8_t pub[32]) {
    u32 k[8];
    onion_words_le(scalar_le, k);
    ed_mul_base_encode(k, pub);
}

// SHA-512 of a message of at most 111 bytes (one block).
inline void sha512_short(const uint8_t *msg, size_t len, uint8_t out[64]) {
    uint8_t blk[128];
    memset(blk, 0, sizeof blk);
    memcpy(blk, msg, len);
    blk[len] = 0x80;
    blk[126] = (uint8_t)((len * 8) >> 8);
    blk[127] = (uint8_t)(len * 8);
    u64 w[16];
    for (int i = 0; i < 16; i++) {
        w[i] = 0;
        for (int j = 0; j < 8; j++) w[i] = w[i] << 8 | blk[8 * i + j];
    }
    u64 st[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    sha512_compress(st, w);
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) out[8 * i + j] = (uint8_t)(st[i] >> (56 - 8 * j));
}

// The nonce key is a function of the scalar alone and differs from key to key of a walk (a nonce key shared by a walk's keys would
// leak them once two of them sign the same message).
inline void onion_expand(const uint8_t scalar_le[32], uint8_t out[64]) {
    static const char TAG[] = "vgen-mi355x onion nonce key";
    uint8_t m[sizeof TAG - 1 + 32], h[64];
    memcpy(m, TAG, sizeof TAG - 1);
    memcpy(m + sizeof TAG - 1, scalar_le, 32);
    sha512_short(m, sizeof m, h);
    memcpy(out, scalar_le, 32);
    memcpy(out + 32, h + 32, 32);
}

inline void onion_base(const RndSeed &seed, uint32_t stream, uint8_t scalar_le[32]) {
    u32 d[8], s[8], k[8];
    rnd_scalar(seed, stream, 0, 0, d);
    for (int j = 0; j < 8; j++) s[j] = d[7 - j];   // candidate 0 of the stream as an Ed25519 seed (vgen_solana_seed), big-endian words
    ed_scalar_from_seed(s, k);
    onion_bytes_le(k, scalar_le);
}

inline bool onion_scalar_at(const uint8_t base_le[32], uint64_t index, uint8_t scalar_le[32]) {
    u32 b[8], r[8];
    onion_words_le(base_le, b);
    u32 carry = edw_add_u64(r, b, index << 3);
    u64 cy = (u64)r[2] + (u32)(index >> 61);
    r[2] = (u32)cy;
    for (int i = 3; i < 8; i++) {
        cy = (cy >> 32) + r[i];
        r[i] = (u32)cy;
    }
    carry |= (u32)(cy >> 32);
    onion_bytes_le(r, scalar_le);
    return !carry && !(r[7] >> 31) && !(b[7] >> 31);
}

}  // namespace vg
