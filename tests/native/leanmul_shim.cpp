// leanmul_shim.cpp — TEST-ONLY host build (g++) of the forms of core/fe.h that the sequential scan kernels' key loop takes:
// the LEAN products with an addend (the addend as the column accumulators' starting value).  tests/test_leanmul.py checks them
// against Python integers and against the plain forms.
#include <stdint.h>

#include "../../vgen_amd/csrc/core/fe.h"

using namespace vg;

static fe load(const u32 *p) {
    fe x;
    for (int i = 0; i < 9; i++) x.n[i] = p[i];
    return x;
}

extern "C" {

// r = a * b + c (square: a^2 + c), LEAN form; lean = 0: the plain form, for the bit-for-bit comparison
void leanmul_mul_add(const u32 *a, const u32 *b, const u32 *c, u32 *r, int square, int lean) {
    const fe x = load(a), y = load(b), z = load(c);
    fe w;
    if (lean) {
        if (square) fe_sqr_add<true>(w, x, z); else fe_mul_add<true>(w, x, y, z);
    } else {
        if (square) fe_sqr_add(w, x, z); else fe_mul_add(w, x, y, z);
    }
    for (int i = 0; i < 9; i++) r[i] = w.n[i];
}

}
