// ed25519.h — the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over 2^255 - 19 as far as a key search needs it: the
// fixed-base multiplication a*B over a table of precomputed multiples, and the RFC 8032 encoding of the result.  Single source for
// the HIP kernels and the host (table construction, match confirmation, CPU tests).
//
// Points are in extended coordinates (X : Y : Z : T), x = X/Z, y = Y/Z, T = XY/Z.  The only addition is the mixed one with a
// precomputed affine entry (y + x, y - x, 2 d x y) - Hisil, Wong, Carter, Dawson 2008, 7 products.  With a = -1 and d a non-square
// the formula is COMPLETE: no exceptional pairs, the neutral element (0, 1) -> (1, 1, 0) is added like any other entry, Z is never 0.
//
// Table: ED_WINDOWS x 256 entries, entry (w, j) = j * 256^w * B, ED_ENTRY_WORDS words each (yp[9], ym[9], t2d[9], one pad word: 112
// bytes, so an entry is seven aligned 16-byte loads): 917 504 bytes.  The scalar's 32 unsigned 8-bit windows select one entry each:
// 32 additions, no doubling, no branch.
#pragma once
#include "fe25519.h"
#include "sha512.h"

namespace vg {

constexpr int ED_WINDOWS = 32;
constexpr int ED_ENTRY_WORDS = 28;
constexpr size_t ED_TABLE_WORDS = (size_t)ED_WINDOWS * 256 * ED_ENTRY_WORDS;

struct ed_pt {
    fe25 X, Y, Z, T;
};
struct ed_pre {
    fe25 yp, ym, t2d;   // y + x, y - x, 2 d x y: canonical limbs
};

VG_HD void ed_set_neutral(ed_pt &p) {
    fe25_set_zero(p.X);
    fe25_set_one(p.Y);
    fe25_set_one(p.Z);
    fe25_set_zero(p.T);
}

// p += q.  p's coordinates weak in, weak out.  Magnitudes in brackets; every product stays within m_a * m_b <= 6.
VG_HD void ed_madd(ed_pt &p, const ed_pre &q) {
    fe25 a, b, c, d, e, f, g, h, t;
    fe25_sub<1>(t, p.Y, p.X);    // [3]
    fe25_mul(a, t, q.ym);
    fe25_add(t, p.Y, p.X);       // [2]
    fe25_mul(b, t, q.yp);
    fe25_mul(c, p.T, q.t2d);
    fe25_add(d, p.Z, p.Z);       // [2]
    fe25_sub<1>(e, b, a);        // [3]
    fe25_sub<1>(f, d, c);        // [4]
    fe25_carry(f);               // [1]
    fe25_add(g, d, c);           // [3]
    fe25_add(h, b, a);           // [2]
    fe25_mul(p.X, e, f);
    fe25_mul(p.Y, g, h);
    fe25_mul(p.T, e, h);
    fe25_mul(p.Z, f, g);
}

VG_HD void ed_load_entry(ed_pre &q, const u32 *e) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *v = reinterpret_cast<const uint4 *>(e);
    u32 w[ED_ENTRY_WORDS];
#pragma unroll
    for (int i = 0; i < ED_ENTRY_WORDS / 4; i++) {
        const uint4 x = v[i];
        w[4 * i] = x.x; w[4 * i + 1] = x.y; w[4 * i + 2] = x.z; w[4 * i + 3] = x.w;
    }
#else
    const u32 *w = e;
#endif
#pragma unroll
    for (int i = 0; i < 9; i++) {
        q.yp.n[i] = w[i];
        q.ym.n[i] = w[9 + i];
        q.t2d.n[i] = w[18 + i];
    }
}

// p = k * B for ANY 256-bit k given as eight little-endian words (the table covers all 32 windows: no reduction mod the group
// order is needed, a clamped scalar is just one case).  The loop consumes the scalar from its low byte and shifts it down, so no
// array is indexed by the loop counter; it is not unrolled (seven products per step: the code of one step is what fits a cache).
VG_HD void ed_mul_base(ed_pt &p, const u32 *table, const u32 k_in[8]) {
    u32 k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = k_in[i];
    ed_set_neutral(p);
#pragma unroll 1
    for (int w = 0; w < ED_WINDOWS; w++) {
        const u32 j = k[0] & 255u;
        ed_pre q;
        ed_load_entry(q, table + ((size_t)w * 256 + j) * ED_ENTRY_WORDS);
        ed_madd(p, q);
#pragma unroll
        for (int i = 0; i < 7; i++) k[i] = (k[i] >> 8) | (k[i + 1] << 24);
        k[7] >>= 8;
    }
}

// RFC 8032 5.1.5: the secret scalar of a seed.  seed_be: the 32 seed bytes as eight big-endian words; k: little-endian words.
VG_HD void ed_scalar_from_seed(const u32 seed_be[8], u32 k[8]) {
    sha512_seed32(seed_be, k);
    k[0] &= ~7u;
    k[7] = (k[7] & 0x7FFFFFFFu) | 0x40000000u;
}

// RFC 8032 5.1.2: the 32 bytes of a point, given its affine coordinates in any weak form: y little-endian, fully reduced, the low bit
// of the fully reduced x in bit 255.  out: eight words in memory order.
VG_HD void ed_encode(u32 out[8], fe25 x, fe25 y) {
    fe25_reduce(x);
    fe25_reduce(y);
    fe25_to_words(out, y);
    out[7] |= (x.n[0] & 1u) << 31;
}

}  // namespace vg
