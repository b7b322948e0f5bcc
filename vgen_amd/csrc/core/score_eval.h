// score_eval.h — evaluation of a score specification ("score:zero-bytes>=2&leading:0>=4", host/filter.cpp) on one 20-byte payload;
// single source for the two score kernels (kernels.hip: payload_score_kernel, create2_score_kernel) and for the host
// (vgen_filter_matches, vgen_score, the CPU tests).  Not part of filter_eval_n, which every matching kernel carries.
//
// The metrics are functions of the 40 hex digits of the address (EIP-55 casing plays no part), computed word-wise on the five
// BIG-endian payload words: an equality mask per word (one bit per byte / per hex digit that equals the wanted value), a
// popcount for the counting metrics, and for the leading runs a count-leading-zeros of the INVERTED mask — the first byte /
// digit that differs.  No loop over the 40 digits, no byte loads.
//
// The equality mask is the exact, carry-free form: with L = 0x7f.. (0x77.. for digits),  ~(((x & L) + L) | x | L)  has the top
// bit of a field set exactly when the field is zero — the sum cannot carry out of a field (0x7f + 0x7f < 0x100).  The shorter
// (x - 0x0101..) & ~x & 0x8080.. borrows across fields: it also flags a 0x01 byte that sits above a zero byte.
#pragma once
#include "../device/device_types.h"
#include "hash.h"

namespace vg {

// top bit of every BYTE of x that is 0x00
VG_HD u32 score_zero_bytes_mask(u32 x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
// top bit of every 4-bit DIGIT of x that is 0
VG_HD u32 score_zero_digits_mask(u32 x) { return ~(((x & 0x77777777u) + 0x77777777u) | x | 0x77777777u); }

VG_HD u32 score_popc(u32 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (u32)__popc(x);
#else
    return (u32)__builtin_popcount(x);
#endif
}

// leading zero bits, 32 for 0
VG_HD u32 score_clz(u32 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (u32)__clz((int)x);
#else
    return x ? (u32)__builtin_clz(x) : 32u;
#endif
}

// Value of one metric on the big-endian words H[0..4].  `digit`: the hex digit of the two per-digit metrics (0 .. 15).
VG_HD u32 score_metric(u32 metric, u32 digit, const u32 H[5]) {
    const bool bytes = metric == SCORE_ZERO_BYTES || metric == SCORE_LEADING_ZERO_BYTES;
    const bool leading = metric == SCORE_LEADING_ZERO_BYTES || metric == SCORE_LEADING_DIGIT;
    const u32 top = bytes ? 0x80808080u : 0x88888888u;   // the mask's bit of every field
    const u32 shift = bytes ? 3u : 2u;                   // bits per field, as a shift
    const u32 per_word = bytes ? 4u : 8u;
    const u32 want = digit * 0x11111111u;
    u32 count = 0, run = 0;
    bool open = true;   // every field before this word matched
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const u32 eq = bytes ? score_zero_bytes_mask(H[i]) : score_zero_digits_mask(H[i] ^ want);
        count += score_popc(eq);
        const u32 lead = score_clz(~eq & top) >> shift;   // fields before the first that differs: per_word when none does
        run += open ? lead : 0u;
        open = open && lead == per_word;
    }
    return leading ? run : count;
}

// payload: five words in memory order (little-endian words of the byte string), as the kernels hold them.
// -> every term holds; *score (optional): the value of the first term's metric.
VG_HD bool score_eval(const ScoreTerms &s, const u32 payload[5], u32 *score) {
    u32 H[5];
#pragma unroll
    for (int i = 0; i < 5; i++) H[i] = bswap32(payload[i]);
    bool ok = s.n != 0;
    u32 first = 0;
#pragma unroll
    for (u32 k = 0; k < SCORE_MAX_TERMS; k++) {
        if (k < s.n) {
            const u32 v = score_metric(s.t[k].metric, s.t[k].digit, H);
            if (k == 0) first = v;
            ok = ok && v >= s.t[k].min;
        }
    }
    if (score) *score = first;
    return ok;
}

}  // namespace vg
