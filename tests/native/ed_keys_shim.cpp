// ed_keys_shim.cpp — host build (g++) of what one lane of ed_keys_kernel computes, on a table the CALLER supplies: the scalar of a
// seed, core/ed25519.h ed_mul_base over that table, one fe25_inv of Z, two fe25_mul, ed_encode.  The same single-source functions the
// kernel inlines, with an inversion per key in place of the workgroup's shared one.  It holds the Python vectors of the crafted
// tables (tests/ed_keys_vectors.py) against something other than themselves before a GPU is involved, and reports whether any Z
// was zero.  (tests/test_ed_keys_vectors.py)
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/ed25519.h"
#include "../../vgen_amd/csrc/host/ed_host.h"

using namespace vg;

extern "C" {

uint32_t edkshim_table_words() { return (uint32_t)ED_TABLE_WORDS; }

// the product's table, for a word-by-word comparison with the vectors' own
void edkshim_real_table(uint32_t *out) { memcpy(out, ed_host_table(), ED_TABLE_WORDS * sizeof(uint32_t)); }

// n seeds of 32 bytes over `table` (nullptr: the product's).  out: 32 bytes a key; z_nonzero: 1 a key where the fully reduced Z of
// the sum was not 0.
void edkshim_keys(const uint32_t *table, const uint8_t *seeds, int n, uint8_t *out, uint8_t *z_nonzero) {
    if (!table) table = ed_host_table();
    for (int i = 0; i < n; i++) {
        const uint8_t *seed = seeds + 32 * (size_t)i;
        u32 s[8], k[8];
        for (int q = 0; q < 8; q++) s[q] = (u32)seed[4 * q] << 24 | (u32)seed[4 * q + 1] << 16 | (u32)seed[4 * q + 2] << 8 | seed[4 * q + 3];
        ed_scalar_from_seed(s, k);
        ed_pt p;
        ed_mul_base(p, table, k);
        fe25 z = p.Z;
        fe25_reduce(z);
        u32 any = 0;
        for (int q = 0; q < 9; q++) any |= z.n[q];
        z_nonzero[i] = any ? 1 : 0;
        fe25 zi, x, y;
        fe25_inv(zi, p.Z);
        fe25_mul(x, p.X, zi);
        fe25_mul(y, p.Y, zi);
        u32 w[8];
        ed_encode(w, x, y);
        memcpy(out + 32 * (size_t)i, w, 32);   // (little-endian host)
    }
}

}
