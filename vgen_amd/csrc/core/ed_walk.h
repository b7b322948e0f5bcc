// ed_walk.h — the Ed25519 key walk of the onion format (VGF_ONION): keys a, a + 8, a + 16, ... are points A + i (8B), and every
// one of them is reached as P + Q or P - Q from a point P the dispatch shares and a point Q the lane owns, both AFFINE.  Single source
// for the HIP kernels (kernels.hip: onion_fwd_kernel / onion_bwd_kernel) and the host (CPU tests, the stand-in of the runtime).
//
// Twisted Edwards, a = -1:  with k = d x1 x2 y1 y2
//     y(P + Q) = (y1 y2 + x1 x2) / (1 - k)        y(P - Q) = (y1 y2 - x1 x2) / (1 + k)
//     x(P + Q) = (x1 y2 + y1 x2) / (1 + k)        x(P - Q) = (x1 y2 - y1 x2) / (1 - k)
// d is a non-square, so the addition is COMPLETE: 1 - k and 1 + k are never 0 for points of the curve - the neutral element, P = Q,
// P = -Q and the points of order 2, 4 and 8 go through the same formulas.  A point carries a third field beside x and y: the
// shared point holds e = d x y, the lane's point t = x y, so that k = e1 t2 is ONE product and the pair's two denominators depend on
// nothing else.  The denominators of a lane are inverted together (prefix products, one inversion a workgroup); per pair then
//     1 (k) + 2 (x1 x2, y1 y2) + 2 (the two y)   products, and 2 + 2 more where x is wanted (x1 y2, y1 x2, the two x).
#pragma once
#include "fe25519.h"

namespace vg {

// An affine point with its third field (e = d x y or t = x y, see above).  Weak limbs.
struct edw_pt {
    fe25 x, y, t;
};

// d = -121665 / 121666
VG_HD void edw_d(fe25 &r) {
    const u32 w[8] = {0x135978a3u, 0x75eb4dcau, 0x4141d8abu, 0x00700a4du, 0x7779e898u, 0x8cc74079u, 0x2b6ffe73u, 0x52036ceeu};
    fe25_from_words(r, w);
}

// The two denominators of the pair P +- Q:  dm = 1 - k [3],  dp = 1 + k [2],  k = e1 t2.
VG_HD void edw_dens(fe25 &dm, fe25 &dp, const fe25 &e1, const fe25 &t2) {
    fe25 k, one;
    fe25_mul(k, e1, t2);
    fe25_set_one(one);
    fe25_sub<1>(dm, one, k);
    fe25_add(dp, one, k);
}

// y of P + Q and of P - Q, given im = 1 / (1 - k) and ip = 1 / (1 + k) (weak).
VG_HD void edw_pair_y(fe25 &y_sum, fe25 &y_dif, const edw_pt &p, const edw_pt &q, const fe25 &im, const fe25 &ip) {
    fe25 a, b, n;
    fe25_mul(a, p.x, q.x);
    fe25_mul(b, p.y, q.y);
    fe25_add(n, b, a);           // [2]
    fe25_mul(y_sum, n, im);
    fe25_sub<1>(n, b, a);        // [3]
    fe25_mul(y_dif, n, ip);
}

// x of P + Q and of P - Q (the denominators change places).
VG_HD void edw_pair_x(fe25 &x_sum, fe25 &x_dif, const edw_pt &p, const edw_pt &q, const fe25 &im, const fe25 &ip) {
    fe25 c, d, n;
    fe25_mul(c, p.x, q.y);
    fe25_mul(d, p.y, q.x);
    fe25_add(n, c, d);
    fe25_mul(x_sum, n, ip);
    fe25_sub<1>(n, c, d);
    fe25_mul(x_dif, n, im);
}

// RFC 8032 bytes of y alone (bit 255 clear): what a prefix of the address up to its 49th character depends on.
VG_HD void edw_encode_y(u32 out[8], fe25 y) {
    fe25_reduce(y);
    fe25_to_words(out, y);
}

// ... and the sign of x to go into bit 255.
VG_HD u32 edw_sign(fe25 x) {
    fe25_reduce(x);
    return x.n[0] & 1u;
}

// 256-bit little-endian words: r = a + m (m < 2^64).  Returns the carry out of bit 255 (into bit 256).
VG_HD u32 edw_add_u64(u32 r[8], const u32 a[8], u64 m) {
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (u64)a[i] + (i == 0 ? (u32)m : i == 1 ? (u32)(m >> 32) : 0u);
        r[i] = (u32)c;
        c >>= 32;
    }
    return (u32)c;
}

}  // namespace vg
