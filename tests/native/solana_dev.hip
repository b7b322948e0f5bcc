// solana_dev.hip — TEST-ONLY device build of the Solana format's single-source core (vgen_amd/csrc/core/fe25519.h, ed25519.h,
// filter_eval.h filter_eval_sol): the very functions ed_keys_kernel inlines, run one input per lane on the GPU and returned to the
// test-suite, so that what exists only in the hipcc build - 64-bit multiply-adds, the 64-by-32-bit remainders, the wave-uniform
// branch behind VG_ANY_LANE - is tested as compiled, on the raw scalars, field edges and filter boundaries the shipped kernel's
// own inputs (seeds through SHA-512) cannot be steered to.  The table and the filter program come from the product's host sources.
// Not part of libvgen_hip.so.  (tests/test_gpu_solana.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed25519.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/ed_host.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

// op: 0 = reduce(a), 1 = a * b, 2 = a^2, 3 = 1 / a, 4 = a + b, 5 = a - b; a, b: eight little-endian words per item (any 256-bit
// value); r: the canonical result.  RAW: a, b are nine limbs per item instead (any pattern within the function's magnitude).
template <bool RAW>
__global__ void __launch_bounds__(64) sol_fe_kernel(int op, int n, const u32 *a_in, const u32 *b_in, u32 *r_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    fe25 a, b, r;
    if (RAW) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            a.n[k] = a_in[9 * i + k];
            b.n[k] = b_in[9 * i + k];
        }
    } else {
        u32 aw[8], bw[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            aw[k] = a_in[8 * i + k];
            bw[k] = b_in[8 * i + k];
        }
        fe25_from_words(a, aw);
        fe25_from_words(b, bw);
    }
    switch (op) {
    case 1: fe25_mul(r, a, b); break;
    case 2: fe25_sqr(r, a); break;
    case 3: fe25_inv(r, a); break;
    case 4: fe25_add(r, a, b); break;
    case 5: fe25_sub<1>(r, a, b); break;
    case 6: r = a; fe25_carry(r); break;
    default: r = a; break;
    }
    fe25_reduce(r);
    u32 w[8];
    fe25_to_words(w, r);
#pragma unroll
    for (int k = 0; k < 8; k++) r_out[8 * i + k] = w[k];
}

// k * B for raw 256-bit scalars (eight little-endian words per item), encoded; an inversion per lane (a test, not the hot path)
__global__ void __launch_bounds__(64) sol_mul_kernel(int n, const u32 *table, const u32 *k_in, u32 *r_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int q = 0; q < 8; q++) k[q] = k_in[8 * i + q];
    ed_pt p;
    ed_mul_base(p, table, k);
    fe25 zi, x, y;
    fe25_inv(zi, p.Z);
    fe25_mul(x, p.X, zi);
    fe25_mul(y, p.Y, zi);
    u32 w[8];
    ed_encode(w, x, y);
#pragma unroll
    for (int q = 0; q < 8; q++) r_out[8 * i + q] = w[q];
}

__global__ void __launch_bounds__(64) sol_filter_kernel(int n, const DevFilter *f, const u32 *payloads, unsigned char *flags) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    u32 pl[8];
#pragma unroll
    for (int q = 0; q < 8; q++) pl[q] = i < n ? payloads[8 * i + q] : 0u;
    const bool hit = filter_eval_sol(f, pl);   // (every lane of the wave takes part: VG_ANY_LANE is a ballot)
    if (i < n) flags[i] = hit ? 1 : 0;
}

namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" {

int soldev_fe(int op, int raw, int n, const uint32_t *a, const uint32_t *b, uint32_t *r) {
    const size_t in_b = (size_t)n * (raw ? 9 : 8) * 4, out_b = (size_t)n * 32;
    DevBuf da, db, dr;
    CK(hipMalloc(&da.p, in_b));
    CK(hipMalloc(&db.p, in_b));
    CK(hipMalloc(&dr.p, out_b));
    CK(hipMemcpy(da.p, a, in_b, hipMemcpyHostToDevice));
    CK(hipMemcpy(db.p, b, in_b, hipMemcpyHostToDevice));
    if (raw) hipLaunchKernelGGL((sol_fe_kernel<true>), dim3((n + 63) / 64), dim3(64), 0, 0, op, n, (const u32 *)da.p, (const u32 *)db.p, (u32 *)dr.p);
    else hipLaunchKernelGGL((sol_fe_kernel<false>), dim3((n + 63) / 64), dim3(64), 0, 0, op, n, (const u32 *)da.p, (const u32 *)db.p, (u32 *)dr.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(r, dr.p, out_b, hipMemcpyDeviceToHost));
    return 0;
}

int soldev_mul(int n, const uint32_t *k, uint32_t *r) {
    DevBuf dt, dk, dr;
    CK(hipMalloc(&dt.p, ED_TABLE_WORDS * 4));
    CK(hipMalloc(&dk.p, (size_t)n * 32));
    CK(hipMalloc(&dr.p, (size_t)n * 32));
    CK(hipMemcpy(dt.p, ed_host_table(), ED_TABLE_WORDS * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dk.p, k, (size_t)n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sol_mul_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const u32 *)dt.p, (const u32 *)dk.p, (u32 *)dr.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(r, dr.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    return 0;
}

// Compiles `pattern` with the product's compiler and runs the device test on n payloads of 32 bytes.  -1 on a pattern error, -2 when
// the filter is not of kind 1, 3 or 7.  *kind receives the device kind.
int soldev_filter(const char *pattern, int ci, int n, const unsigned char *payloads, unsigned char *flags, unsigned *kind) {
    vgen_filter f;
    std::string err;
    if (!filter_compile(pattern, ci != 0, VGF_SOLANA, f, err)) return -1;
    *kind = f.dev.kind;
    if (f.dev.kind != DEVF_RANGES && f.dev.kind != DEVF_ALL && f.dev.kind != DEVF_SOL_RESIDUE) return -2;
    DevBuf df, dp, dflags;
    CK(hipMalloc(&df.p, sizeof(DevFilter)));
    CK(hipMalloc(&dp.p, (size_t)n * 32));
    CK(hipMalloc(&dflags.p, (size_t)n));
    CK(hipMemcpy(df.p, &f.dev, sizeof(DevFilter), hipMemcpyHostToDevice));
    CK(hipMemcpy(dp.p, payloads, (size_t)n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sol_filter_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const DevFilter *)df.p, (const u32 *)dp.p, (unsigned char *)dflags.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(flags, dflags.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

}
