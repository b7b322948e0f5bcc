// ptab_eval.h — the pattern-list lookup (DEVF_LIST) on one payload; single source for the list kernel (kernels.hip:
// ptab_lookup_kernel) and for the host, where vgen_filter_which and the scan loop use it to go from a candidate to the
// interval that names its patterns (host/filter.cpp).  The CPU tests compile this header on its own.
//
// A list of prefix patterns is a set of ranges of the big-endian payload; cut to its top 64 bits (lo rounded down, hi
// taken as the last 64-bit value it reaches: a superset the host confirms) and split into disjoint sorted intervals, it
// is searched in two steps: the bucket of the top `bits` bits (a bitmap rejects almost every key with one load), then a
// binary search over the few intervals that meet the bucket.
#pragma once
#include "../device/device_types.h"
#include "fe.h"

namespace vg {

// The top 64 bits of a payload given in memory order (little-endian words of the byte string).
VG_HD u64 ptab_top64(const u32 *payload) {
    const u32 a = payload[0], b = payload[1];
    const u32 ha = (a >> 24) | ((a >> 8) & 0xFF00u) | ((a << 8) & 0xFF0000u) | (a << 24);
    const u32 hb = (b >> 24) | ((b >> 8) & 0xFF00u) | ((b << 8) & 0xFF0000u) | (b << 24);
    return ((u64)ha << 32) | hb;
}

// Index of the interval that holds x, or -1.  `t` may hold device or host pointers.
VG_HD int ptab_find(const DevPtab &t, u64 x) {
    const u32 b = (u32)(x >> (64 - t.bits));
    if (((t.bitmap[b >> 5] >> (b & 31)) & 1u) == 0) return -1;
    // intervals that can hold x: from the first whose hi reaches the bucket up to the first of the next bucket (inclusive:
    // it may start inside this one)
    u32 lo = t.offsets[b], hi = t.offsets[b + 1] + 1;
    if (hi > t.n) hi = t.n;
    // the last interval in [lo, hi) with lo_j <= x
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (t.lo[mid] <= x) lo = mid;
        else hi = mid;
    }
    if (lo >= t.n || t.lo[lo] > x || x > t.hi[lo]) return -1;
    return (int)lo;
}

}  // namespace vg
