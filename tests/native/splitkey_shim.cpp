// splitkey_shim.cpp — host build (g++) of the per-dispatch uniform points of the sequential walk with a base point: vg::host_seq_points
// over a SeqBaseCache the test keeps across calls, so that consecutive dispatches go through the cache's stride point and its
// look-ahead exactly as rt_dispatch drives them.  (tests/test_splitkey.py)
#include <string.h>

#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/host_ec.h"

using namespace vg;

extern "C" {

void *seqpts_new() { return new SeqBaseCache(); }
void seqpts_free(void *c) { delete static_cast<SeqBaseCache *>(c); }

// out[j] = (kb + j)*G + base for j < S as 64 bytes each (x, y big-endian); base65: a SEC1 public key of 33 / 65 bytes, or NULL / 0
// for no base.  1 = points written, 0 = host_seq_points said "point at infinity", -1 = bad arguments.  *state (optional) receives the
// cache's look-ahead position and fill after the call: (ahead_pos << 8) | ahead_n.
int seqpts_get(void *cache, const unsigned char kb_be[32], unsigned S, const unsigned char *base, unsigned base_len, unsigned char *out, unsigned *state) {
    if (!cache || !kb_be || !out || S == 0 || S > 32) return -1;
    ge b;
    if (base && !point_from_sec1(base, base_len, b)) return -1;
    Scalar kb;
    scalar_from_be(kb, kb_be);
    ge pts[32];
    SeqBaseCache &c = *static_cast<SeqBaseCache *>(cache);
    const bool ok = host_seq_points(c, kb, S, pts, base ? &b : nullptr);
    if (state) *state = (c.ahead_pos << 8) | c.ahead_n;
    if (!ok) return 0;
    for (unsigned j = 0; j < S; j++) {
        unsigned char sec[65];
        point_to_sec1(pts[j], sec);
        memcpy(out + 64 * j, sec + 1, 64);
    }
    return 1;
}

}
