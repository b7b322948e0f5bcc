// onion_shim.cpp — host build (g++) of what the kernels evaluate for the onion format (VGF_ONION): the pair formulas of
// core/ed_walk.h on points the test chooses, the prefilter (core/filter_eval.h filter_eval_onion) on payloads the test chooses beside
// the exact automaton on the host-encoded string, and the host's SHA3-256.  (tests/test_onion.py)
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed_walk.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/filter.h"
#include "../../vgen_amd/csrc/host/onion_host.h"

using namespace vg;

namespace {
void fe_of(const unsigned char *b, fe25 &a) {
    u32 w[8];
    memcpy(w, b, 32);   // 32 little-endian bytes (little-endian host)
    fe25_from_words(a, w);
}
void out_bytes(fe25 a, unsigned char *out) {
    fe25_reduce(a);
    u32 w[8];
    fe25_to_words(w, a);
    memcpy(out, w, 32);
}
}  // namespace

extern "C" {

// P = (x1, y1), Q = (x2, y2) as 32 little-endian bytes each (canonical or not).  out: x(P+Q), y(P+Q), x(P-Q), y(P-Q), canonical.
// The third fields are made here as the kernels' point builder makes them (e1 = d x1 y1, t2 = x2 y2), the two denominators are
// inverted one by one.
void onion_pair(const unsigned char *p64, const unsigned char *q64, unsigned char *out128) {
    edw_pt p, q;
    fe_of(p64, p.x);
    fe_of(p64 + 32, p.y);
    fe_of(q64, q.x);
    fe_of(q64 + 32, q.y);
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
    out_bytes(xs, out128);
    out_bytes(ys, out128 + 32);
    out_bytes(xd, out128 + 64);
    out_bytes(yd, out128 + 96);
}

void onion_sha3_256(const unsigned char *msg, size_t len, unsigned char *out) { sha3_256(msg, len, out); }

// Compiles `pattern` for the format and judges n payloads of 32 bytes.  out_flags[i]: bit 0 = the device test (filter_eval_onion)
// accepts, bit 1 = the exact automaton accepts the address string.  info: kind, count.  tests_out (optional): count x 16 words, mask
// then value of every test.  -1 on a pattern error.
int onion_filter_check(const char *pattern, int ci, const unsigned char *payloads, int n, unsigned char *out_flags, unsigned *info, unsigned *tests_out) {
    vgen_filter f;
    std::string err;
    if (!filter_compile(pattern, ci != 0, VGF_ONION, f, err)) return -1;
    info[0] = f.dev.kind;
    info[1] = f.dev.count;
    if (tests_out && f.dev.kind == DEVF_MASKED)
        for (unsigned t = 0; t < f.dev.count; t++) {
            memcpy(tests_out + 16 * t, f.dev.tests[t].a, 32);
            memcpy(tests_out + 16 * t + 8, f.dev.tests[t].b, 32);
        }
    for (int i = 0; i < n; i++) {
        u32 pl[8];
        memcpy(pl, payloads + 32 * i, 32);
        const int dev = filter_eval_onion(&f.dev, pl) ? 1 : 0;
        const std::string addr = address_from_payload(VGF_ONION, payloads + 32 * i);
        out_flags[i] = (unsigned char)(dev | ((f.dfa.is_match(addr) ? 1 : 0) << 1));
    }
    return 0;
}

}
