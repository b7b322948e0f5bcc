// ed_host.h — the host's side of the Solana format (VGF_SOLANA): the Ed25519 table the device multiplies over, the public key of a
// seed, and the strings.  The arithmetic is the host build of core/ed25519.h, the code the kernels run.  Header-only (inline
// functions, one table per process): every program that links the host sources gets it without a source file of its own.
//   ed_host_table          the fixed-base table (core/ed25519.h: ED_TABLE_WORDS words), built at first use, once per process
//   ed_mul_base_encode     k * B for any 256-bit k (eight little-endian words), RFC 8032 encoding
//   ed_public_key          RFC 8032 5.1.5: the public key of a 32-byte seed
//   solana_keypair_base58  Base58 of seed || public key: the keypair string wallets import (87 or 88 characters, fewer with leading zero bytes)
//   solana_decode          strict: every character in the Base58 alphabet and a value of exactly 32 bytes (a leading '1' is a leading zero byte)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../core/ed25519.h"
#include "encode.h"

namespace vg {

namespace ed_host_detail {

// d = -121665 / 121666 and the base point B = (x, 4/5), x even (RFC 8032 5.1), as little-endian words.
inline constexpr u32 ED_D[8] = {0x135978a3u, 0x75eb4dcau, 0x4141d8abu, 0x00700a4du, 0x7779e898u, 0x8cc74079u, 0x2b6ffe73u, 0x52036ceeu};
inline constexpr u32 ED_BX[8] = {0x8f25d51au, 0xc9562d60u, 0x9525a7b2u, 0x692cc760u, 0xfdd6dc5cu, 0xc0a4e231u, 0xcd6e53feu, 0x216936d3u};
inline constexpr u32 ED_BY[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};

inline void entry_from_affine(u32 *e, const fe25 &x, const fe25 &y, const fe25 &d2) {
    fe25 yp, ym, t;
    fe25_add(yp, y, x);
    fe25_sub<1>(ym, y, x);
    fe25_mul(t, x, y);
    fe25_mul(t, t, d2);
    fe25_reduce(yp);
    fe25_reduce(ym);
    fe25_reduce(t);
    for (int i = 0; i < 9; i++) {
        e[i] = yp.n[i];
        e[9 + i] = ym.n[i];
        e[18 + i] = t.n[i];
    }
    e[27] = 0;
}

inline std::vector<u32> build_table() {
    std::vector<u32> tab(ED_TABLE_WORDS);
    fe25 d2, bx, by;
    fe25_from_words(d2, ED_D);
    fe25_add(d2, d2, d2);
    fe25_carry(d2);
    fe25_from_words(bx, ED_BX);
    fe25_from_words(by, ED_BY);
    std::vector<ed_pt> acc(257);
    std::vector<fe25> pre(257), inv(257);
    for (int w = 0; w < ED_WINDOWS; w++) {
        // acc[j] = j * base, the window's base 256^w * B as a precomputed entry; acc[256] is the next window's base
        u32 be[ED_ENTRY_WORDS];
        entry_from_affine(be, bx, by, d2);
        ed_pre q;
        ed_load_entry(q, be);
        ed_set_neutral(acc[0]);
        for (int j = 1; j <= 256; j++) {
            acc[j] = acc[j - 1];
            ed_madd(acc[j], q);
        }
        // one inversion for the 257 Z's (none is 0: the addition is complete)
        pre[0] = acc[0].Z;
        for (int j = 1; j <= 256; j++) fe25_mul(pre[j], pre[j - 1], acc[j].Z);
        fe25 run;
        fe25_inv(run, pre[256]);
        for (int j = 256; j >= 1; j--) {
            fe25_mul(inv[j], run, pre[j - 1]);
            fe25_mul(run, run, acc[j].Z);
        }
        inv[0] = run;
        for (int j = 0; j <= 256; j++) {
            fe25 x, y;
            fe25_mul(x, acc[j].X, inv[j]);
            fe25_mul(y, acc[j].Y, inv[j]);
            if (j < 256) entry_from_affine(&tab[((size_t)w * 256 + j) * ED_ENTRY_WORDS], x, y, d2);
            else {
                bx = x;
                by = y;
            }
        }
    }
    return tab;
}

}  // namespace ed_host_detail

inline const uint32_t *ed_host_table() {
    static std::vector<u32> tab;
    static std::once_flag once;
    std::call_once(once, [] { tab = ed_host_detail::build_table(); });
    return tab.data();
}

inline void ed_mul_base_encode(const uint32_t k[8], uint8_t out[32]) {
    ed_pt p;
    ed_mul_base(p, ed_host_table(), k);
    fe25 zi, x, y;
    fe25_inv(zi, p.Z);
    fe25_mul(x, p.X, zi);
    fe25_mul(y, p.Y, zi);
    u32 w[8];
    ed_encode(w, x, y);
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(w[i] >> (8 * b));
}

inline void ed_public_key(const uint8_t seed[32], uint8_t pub[32]) {
    u32 s[8], k[8];
    for (int i = 0; i < 8; i++) s[i] = (u32)seed[4 * i] << 24 | (u32)seed[4 * i + 1] << 16 | (u32)seed[4 * i + 2] << 8 | seed[4 * i + 3];
    ed_scalar_from_seed(s, k);
    ed_mul_base_encode(k, pub);
}

inline std::string solana_keypair_base58(const uint8_t seed[32]) {
    uint8_t kp[64];
    memcpy(kp, seed, 32);
    ed_public_key(seed, kp + 32);
    return base58_encode(kp, 64);
}

inline bool solana_decode(const std::string &s, uint8_t out[32]) {
    static const char *ALPHA = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
    if (s.empty() || s.size() > 44) return false;
    size_t zeros = 0;
    while (zeros < s.size() && s[zeros] == '1') zeros++;
    uint8_t num[40] = {0};   // big-endian, right-aligned: 44 digits stay below 2^258
    for (size_t i = zeros; i < s.size(); i++) {
        const char *p = s[i] ? strchr(ALPHA, s[i]) : nullptr;
        if (!p) return false;
        uint32_t carry = (uint32_t)(p - ALPHA);
        for (int b = 39; b >= 0; b--) {
            carry += 58u * num[b];
            num[b] = (uint8_t)carry;
            carry >>= 8;
        }
    }
    size_t lead = 0;
    while (lead < 40 && num[lead] == 0) lead++;
    if (zeros + (40 - lead) != 32) return false;
    memset(out, 0, 32);
    memcpy(out + zeros, num + lead, 40 - lead);
    return true;
}

}  // namespace vg
