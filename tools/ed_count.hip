// ed_count.hip — the pieces of ed_keys_kernel as kernels of their own, compiled to assembly only (tools/solana_rate.py --static-only):
// their VALU counts split the straight-line head of the kernel (the seed's draw, SHA-512) and its tail (encoding, filter), which the
// compiler interleaves in the real kernel.  Never run.
#include <hip/hip_runtime.h>

#include "../vgen_amd/csrc/core/ed25519.h"
#include "../vgen_amd/csrc/core/filter_eval.h"
#include "../vgen_amd/csrc/core/rnd.h"

using namespace vg;

extern "C" __global__ void count_draw(const RndSeed seed, u32 stream, unsigned long long first, u32 *out) {
    const u64 index = first + blockIdx.x * blockDim.x + threadIdx.x;
    u32 k[8];
    rnd_scalar(seed, stream, (u32)index, (u32)(index >> 32), k);
    for (int i = 0; i < 8; i++) out[8 * threadIdx.x + i] = k[i];
}

extern "C" __global__ void count_sha512(const u32 *in, u32 *out) {
    u32 s[8], k[8];
    for (int i = 0; i < 8; i++) s[i] = in[8 * threadIdx.x + i];
    ed_scalar_from_seed(s, k);
    for (int i = 0; i < 8; i++) out[8 * threadIdx.x + i] = k[i];
}

extern "C" __global__ void count_encode(const u32 *in, u32 *out) {
    fe25 x, y;
    for (int i = 0; i < 9; i++) {
        x.n[i] = in[18 * threadIdx.x + i];
        y.n[i] = in[18 * threadIdx.x + 9 + i];
    }
    u32 w[8];
    ed_encode(w, x, y);
    for (int i = 0; i < 8; i++) out[8 * threadIdx.x + i] = w[i];
}

extern "C" __global__ void count_filter(const DevFilter *f, const u32 *in, unsigned long long *out) {
    u32 pl[8];
    for (int i = 0; i < 8; i++) pl[i] = in[8 * threadIdx.x + i];
    const unsigned long long m = __ballot(filter_eval_sol(f, pl));
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

extern "C" __global__ void count_mul(const u32 *in, u32 *out) {
    fe25 a, b;
    for (int i = 0; i < 9; i++) {
        a.n[i] = in[18 * threadIdx.x + i];
        b.n[i] = in[18 * threadIdx.x + 9 + i];
    }
    fe25_mul(a, a, b);
    for (int i = 0; i < 9; i++) out[9 * threadIdx.x + i] = a.n[i];
}
