// solana_shim.cpp — host build (g++) of what the kernels evaluate for the Solana format (VGF_SOLANA): the field functions of
// core/fe25519.h, the SHA-512 block of core/sha512.h, the fixed-base multiplication of core/ed25519.h on raw scalars, and the
// prefilter (core/filter_eval.h filter_eval_sol) on payloads the test chooses, beside the exact automaton on the host-encoded
// string.  (tests/test_solana.py)
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed25519.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/ed_host.h"
#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

namespace {
void words_of(const unsigned char *b, u32 w[8]) { memcpy(w, b, 32); }   // 32 little-endian bytes (little-endian host)
void limbs_of(const unsigned *l, fe25 &a) {
    for (int i = 0; i < 9; i++) a.n[i] = l[i];
}
void out_bytes(fe25 a, unsigned char *out) {
    fe25_reduce(a);
    u32 w[8];
    fe25_to_words(w, a);
    memcpy(out, w, 32);
}
}  // namespace

extern "C" {

// op on field elements given as 32 little-endian bytes (any 256-bit value): 0 = reduce(a), 1 = a * b, 2 = a^2, 3 = 1 / a, 4 = a + b,
// 5 = a - b.  out: the canonical result, 32 little-endian bytes.
void sol_fe_op(int op, const unsigned char *a32, const unsigned char *b32, unsigned char *out) {
    u32 aw[8], bw[8];
    words_of(a32, aw);
    words_of(b32, bw);
    fe25 a, b, r;
    fe25_from_words(a, aw);
    fe25_from_words(b, bw);
    switch (op) {
    case 1: fe25_mul(r, a, b); break;
    case 2: fe25_sqr(r, a); break;
    case 3: fe25_inv(r, a); break;
    case 4: fe25_add(r, a, b); break;
    case 5: fe25_sub<1>(r, a, b); break;
    default: r = a; break;
    }
    out_bytes(r, out);
}

// The same on raw limbs (nine words each, any pattern within the function's stated magnitude): 0 = reduce, 1 = mul, 2 = sqr, 6 = carry.
void sol_fe_op_limbs(int op, const unsigned *al, const unsigned *bl, unsigned char *out) {
    fe25 a, b, r;
    limbs_of(al, a);
    limbs_of(bl, b);
    switch (op) {
    case 1: fe25_mul(r, a, b); break;
    case 2: fe25_sqr(r, a); break;
    case 6: r = a; fe25_carry(r); break;
    default: r = a; break;
    }
    out_bytes(r, out);
}

// first 32 bytes of SHA-512(seed)
void sol_sha512_half(const unsigned char *seed, unsigned char *out) {
    u32 s[8], k[8];
    for (int i = 0; i < 8; i++) s[i] = (u32)seed[4 * i] << 24 | (u32)seed[4 * i + 1] << 16 | (u32)seed[4 * i + 2] << 8 | seed[4 * i + 3];
    sha512_seed32(s, k);
    memcpy(out, k, 32);
}

// k * B for a raw 256-bit scalar (32 little-endian bytes), encoded
void sol_mul_base(const unsigned char *k32, unsigned char *out) {
    u32 k[8];
    words_of(k32, k);
    ed_mul_base_encode(k, out);
}

// Compiles `pattern` for the format and judges n payloads of 32 bytes.  out_flags[i]: bit 0 = the device test (filter_eval_sol)
// accepts, bit 1 = the exact automaton accepts the address string.  info: kind, count, n_ranges, modulus.  tests_out (optional):
// count x 16 words, a then b of every test.  -1 on a pattern error.
int sol_filter_check(const char *pattern, int ci, const unsigned char *payloads, int n, unsigned char *out_flags, unsigned *info, unsigned *tests_out) {
    vgen_filter f;
    std::string err;
    if (!filter_compile(pattern, ci != 0, VGF_SOLANA, f, err)) return -1;
    info[0] = f.dev.kind;
    info[1] = f.dev.count;
    info[2] = f.dev.kind == DEVF_SOL_RESIDUE ? f.dev.chk_base : f.dev.kind == DEVF_RANGES ? f.dev.count : 0;
    info[3] = f.dev.kind == DEVF_SOL_RESIDUE ? f.dev.witver : 0;
    if (tests_out && (f.dev.kind == DEVF_RANGES || f.dev.kind == DEVF_SOL_RESIDUE))
        for (unsigned t = 0; t < f.dev.count; t++) {
            memcpy(tests_out + 16 * t, f.dev.tests[t].a, 32);
            memcpy(tests_out + 16 * t + 8, f.dev.tests[t].b, 32);
        }
    for (int i = 0; i < n; i++) {
        u32 pl[8];
        memcpy(pl, payloads + 32 * i, 32);
        const int dev = filter_eval_sol(&f.dev, pl) ? 1 : 0;
        const std::string addr = address_from_payload(VGF_SOLANA, payloads + 32 * i);
        out_flags[i] = (unsigned char)(dev | ((f.dfa.is_match(addr) ? 1 : 0) << 1));
    }
    return 0;
}

}
