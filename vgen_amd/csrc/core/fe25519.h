// fe25519.h — arithmetic in F_p, p = 2^255 - 19 (the Ed25519 base field), 9 limbs x 29 bits.
//
// Single source for the HIP kernels (hipcc, gfx950) and the host (table construction, match confirmation, CPU tests), as fe.h is
// for secp256k1, and for the same reason the same radix: 81 partial products accumulated in 64-bit column sums by v_mad_u64_u32
// with no carry flags, additions as nine independent 32-bit adds.  Nine limbs hold 261 bits and 2^261 = 2^6 * 2^255 = 64 * 19 =
// 1216 (mod p): the high columns fold into the low ones with one small multiplier and, unlike fe.h, every limb - the top one
// included - is a full 29-bit limb.
//
// Representation: value = sum n[i] * 2^(29 i).  "weak": every limb < 2^29 + 2^17 (what a product or a carry pass leaves: the top
// fold lands in limbs 0 and 1 and is not rippled further).  "magnitude m": every limb <= m * (2^29 + 2^17); m <= 7 keeps a limb in
// 32 bits.  Products take m_a * m_b <= 6: a column of nine products then stays below 54 * 2^58.0007 < 2^63.76 and the fold terms
// (< 2^46) leave room.  A value is only ever defined mod p: two weak representations of one residue may differ.
// Canonical = limbs < 2^29, top limb < 2^23, value < p (fe25_reduce).
#pragma once
#include "fe.h"   // VG_HD, u32, u64

namespace vg {

struct fe25 {
    u32 n[9];
};

constexpr u32 F25_M29 = 0x1FFFFFFFu;
constexpr u32 F25_FOLD = 1216u;   // 2^261 mod p

VG_HD void fe25_set_zero(fe25 &r) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.n[i] = 0;
}

VG_HD void fe25_set_one(fe25 &r) {
    fe25_set_zero(r);
    r.n[0] = 1;
}

// r = a + b.  magnitude m_a + m_b.
VG_HD void fe25_add(fe25 &r, const fe25 &a, const fe25 &b) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.n[i] = a.n[i] + b.n[i];
}

// r = a - b for b of magnitude <= MB.  Adds 2 MB (2^261 - 1216) = 128 MB p limb-wise (limbs 2 MB (2^29 - 1216) and 2 MB (2^29 - 1),
// each above MB (2^29 + 2^17)): no borrows.  Result magnitude m_a + 2 MB.
template <u32 MB>
VG_HD void fe25_sub(fe25 &r, const fe25 &a, const fe25 &b) {
    r.n[0] = a.n[0] + 2u * MB * (F25_M29 + 1u - F25_FOLD) - b.n[0];
#pragma unroll
    for (int i = 1; i < 9; i++) r.n[i] = a.n[i] + 2u * MB * F25_M29 - b.n[i];
}

// ---- multiplication: column form (fe.h explains the shape) ----------------------------------------------------
// Column sums S_k, k = 16 .. 0, each accumulated on its own in 64 bits.  A high column is folded at once as two 32-bit halves:
//     S_k 2^(29 k), k >= 9:  2^261 = 1216,  S_k = lo + 2^32 hi,  2^32 = 8 * 2^29   ->   D_{k-9} += 1216 lo;  D_{k-8} += 9728 hi
// then one carry pass; the carry out of limb 8 (< 2^36, weight 2^261) times 1216 goes into limb 0 and its overflow into limb 1.
template <bool SQR>
VG_HD void fe25_mul_columns_(fe25 &r, const fe25 &a, const fe25 &b) {
    u32 d[9];   // SQR: doubled limbs for the cross terms (a of magnitude <= 2)
#pragma unroll
    for (int i = 0; i < 9; i++) d[i] = SQR ? (a.n[i] << 1) : 0u;
    u64 D[9];
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = 0;
#pragma unroll
    for (int k = 16; k >= 0; k--) {
        u64 s = k < 9 ? D[k] : 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int j = k - i;
            if (j < 0 || j >= 9) continue;
            if (!SQR) s += (u64)a.n[i] * b.n[j];
            else if (i < j) s += (u64)d[i] * a.n[j];
            else if (i == j) s += (u64)a.n[i] * a.n[i];
        }
        if (k >= 9) {
            const u32 lo = (u32)s, hi = (u32)(s >> 32);
            D[k - 9] += (u64)lo * F25_FOLD;
            D[k - 8] += (u64)hi * (8u * F25_FOLD);
        } else {
            D[k] = s;
        }
    }
    u32 f[9];
    u64 c = D[0];
    f[0] = (u32)c & F25_M29; c >>= 29;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        c += D[k];
        f[k] = (u32)c & F25_M29; c >>= 29;
    }
    c = c * F25_FOLD + f[0];                     // < 2^36 * 1216 + 2^29 < 2^47
    r.n[0] = (u32)c & F25_M29;
    r.n[1] = f[1] + (u32)(c >> 29);              // < 2^29 + 2^18 / 2: weak
#pragma unroll
    for (int k = 2; k < 9; k++) r.n[k] = f[k];
}

// r = a * b.  Requires m_a * m_b <= 6.  Result weak.
VG_HD void fe25_mul(fe25 &r, const fe25 &a, const fe25 &b) { fe25_mul_columns_<false>(r, a, b); }
// r = a^2.  Requires m_a <= 2.  Result weak.
VG_HD void fe25_sqr(fe25 &r, const fe25 &a) { fe25_mul_columns_<true>(r, a, a); }

// One carry pass over a value of magnitude <= 7.  Result weak.
VG_HD void fe25_carry(fe25 &r) {
    u32 f[9];
    u32 c = r.n[0];
    f[0] = c & F25_M29; c >>= 29;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        c += r.n[k];                             // <= 7 (2^29 + 2^17) + 7 < 2^32
        f[k] = c & F25_M29; c >>= 29;
    }
    r.n[0] = f[0] + c * F25_FOLD;                // c <= 7
#pragma unroll
    for (int k = 1; k < 9; k++) r.n[k] = f[k];
}

// The canonical representative of a value of magnitude <= 7: strict limbs, value < p.
VG_HD void fe25_reduce(fe25 &r) {
    u32 v[9], u[9];
    u32 c = r.n[0];
    v[0] = c & F25_M29; c >>= 29;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        c += r.n[k];
        v[k] = c & F25_M29; c >>= 29;
    }
    // bits 255 and up (limb 8 holds bits 232 .. 260, c the bits from 261 on) have weight 19 each: q <= 63 + 7 * 64
    const u32 q = (v[8] >> 23) + (c << 6);
    v[8] &= 0x7FFFFFu;
    c = v[0] + 19u * q;
    v[0] = c & F25_M29; c >>= 29;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        c += v[k];
        v[k] = c & F25_M29; c >>= 29;            // (limb 8 < 2^23 + 1: nothing leaves it)
    }
    // v < 2^255 + 2^14.  u = v + 19 reaches 2^255 exactly when v >= p, and then u - 2^255 = v - p.
    c = v[0] + 19u;
    u[0] = c & F25_M29; c >>= 29;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        c += v[k];
        u[k] = c & F25_M29; c >>= 29;
    }
    const bool ge_p = (u[8] >> 23) != 0;
    u[8] &= 0x7FFFFFu;
#pragma unroll
    for (int k = 0; k < 9; k++) r.n[k] = ge_p ? u[k] : v[k];
}

// Any 256-bit value as eight little-endian words (w[0] least significant) -> weak limbs (value < 2^256: not reduced).
VG_HD void fe25_from_words(fe25 &r, const u32 w[8]) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        u32 x = w[j] >> sh;
        if (sh > 3 && j + 1 < 8) x |= w[j + 1] << (32 - sh);
        r.n[i] = x & F25_M29;
    }
}

// Canonical limbs -> eight little-endian words (bit 255 clear).
VG_HD void fe25_to_words(u32 w[8], const fe25 &a) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int bit = 32 * j, i = bit / 29, sh = bit % 29;
        u32 x = a.n[i] >> sh;
        if (i + 1 < 9) x |= a.n[i + 1] << (29 - sh);
        if (58 - sh < 32 && i + 2 < 9) x |= a.n[i + 2] << (58 - sh);
        w[j] = x;
    }
}

// r = a^(2^n), a weak.
VG_HD void fe25_sqr_n(fe25 &r, const fe25 &a, int n) {
    r = a;
#pragma unroll 1
    for (int i = 0; i < n; i++) fe25_sqr(r, r);
}

// r = a^(p - 2) = 1 / a (0 for a = 0), a weak: 254 squarings and 11 products, the chain of the reference implementations.
VG_HD void fe25_inv(fe25 &r, const fe25 &a) {
    fe25 z2, z9, z11, z5, z10, z20, z50, z100, t;
    fe25_sqr(z2, a);                  // 2
    fe25_sqr_n(t, z2, 2);             // 8
    fe25_mul(z9, t, a);               // 9
    fe25_mul(z11, z9, z2);            // 11
    fe25_sqr(t, z11);                 // 22
    fe25_mul(z5, t, z9);              // 2^5 - 1
    fe25_sqr_n(t, z5, 5);
    fe25_mul(z10, t, z5);             // 2^10 - 1
    fe25_sqr_n(t, z10, 10);
    fe25_mul(z20, t, z10);            // 2^20 - 1
    fe25_sqr_n(t, z20, 20);
    fe25_mul(t, t, z20);              // 2^40 - 1
    fe25_sqr_n(t, t, 10);
    fe25_mul(z50, t, z10);            // 2^50 - 1
    fe25_sqr_n(t, z50, 50);
    fe25_mul(z100, t, z50);           // 2^100 - 1
    fe25_sqr_n(t, z100, 100);
    fe25_mul(t, t, z100);             // 2^200 - 1
    fe25_sqr_n(t, t, 50);
    fe25_mul(t, t, z50);              // 2^250 - 1
    fe25_sqr_n(t, t, 5);              // 2^255 - 2^5
    fe25_mul(r, t, z11);              // 2^255 - 21
}

}  // namespace vg
