// onion_dev.hip — TEST-ONLY device build of the onion format's single-source core (vgen_amd/csrc/core/ed_walk.h, filter_eval.h
// filter_eval_onion): the very functions onion_fwd_kernel / onion_bwd_kernel inline, run one input per lane on the GPU and returned to
// the test-suite, so that what exists only in the hipcc build is tested as compiled, on the points - the neutral element, P = +-Q, the
// points of order 2, 4 and 8 - and the filter boundaries the shipped kernels' own inputs cannot be steered to.  The filter program comes
// from the product's host sources.  Not part of libvgen_hip.so.  (tests/test_gpu_onion.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/ed_walk.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

// item i: P = (x1, y1), Q = (x2, y2), eight little-endian words each, 32 words per item; out: x(P+Q), y(P+Q), x(P-Q), y(P-Q), canonical.
__global__ void __launch_bounds__(64) onion_pair_kernel(int n, const u32 *in, u32 *out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u32 w[32];
#pragma unroll
    for (int k = 0; k < 32; k++) w[k] = in[32 * i + k];
    edw_pt p, q;
    fe25_from_words(p.x, w);
    fe25_from_words(p.y, w + 8);
    fe25_from_words(q.x, w + 16);
    fe25_from_words(q.y, w + 24);
    fe25 d;
    edw_d(d);
    fe25_mul(p.t, p.x, p.y);
    fe25_mul(p.t, p.t, d);
    fe25_mul(q.t, q.x, q.y);
    fe25 dm, dp, im, ip, r[4];
    edw_dens(dm, dp, p.t, q.t);
    fe25_carry(dm);
    fe25_carry(dp);
    fe25_inv(im, dm);
    fe25_inv(ip, dp);
    edw_pair_x(r[0], r[2], p, q, im, ip);
    edw_pair_y(r[1], r[3], p, q, im, ip);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        fe25_reduce(r[c]);
        u32 o[8];
        fe25_to_words(o, r[c]);
#pragma unroll
        for (int k = 0; k < 8; k++) out[32 * i + 8 * c + k] = o[k];
    }
}

__global__ void __launch_bounds__(64) onion_filter_kernel(int n, const DevFilter *f, const u32 *payloads, unsigned char *flags) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    u32 pl[8];
#pragma unroll
    for (int q = 0; q < 8; q++) pl[q] = i < n ? payloads[8 * i + q] : 0u;
    const bool hit = filter_eval_onion(f, pl);
    if (i < n) flags[i] = hit ? 1 : 0;
}

namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" {

int oniondev_pair(int n, const uint32_t *in, uint32_t *out) {
    const size_t b = (size_t)n * 128;
    DevBuf di, dout;
    CK(hipMalloc(&di.p, b));
    CK(hipMalloc(&dout.p, b));
    CK(hipMemcpy(di.p, in, b, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(onion_pair_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const u32 *)di.p, (u32 *)dout.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, b, hipMemcpyDeviceToHost));
    return 0;
}

// Compiles `pattern` with the product's compiler and runs the device test on n payloads of 32 bytes.  -1 on a pattern error, -2 when
// the filter is not of kind 2 or 3.  *kind receives the device kind.
int oniondev_filter(const char *pattern, int ci, int n, const unsigned char *payloads, unsigned char *flags, unsigned *kind) {
    vgen_filter f;
    std::string err;
    if (!filter_compile(pattern, ci != 0, VGF_ONION, f, err)) return -1;
    *kind = f.dev.kind;
    if (f.dev.kind != DEVF_MASKED && f.dev.kind != DEVF_ALL) return -2;
    DevBuf df, dp, dflags;
    CK(hipMalloc(&df.p, sizeof(DevFilter)));
    CK(hipMalloc(&dp.p, (size_t)n * 32));
    CK(hipMalloc(&dflags.p, (size_t)n));
    CK(hipMemcpy(df.p, &f.dev, sizeof(DevFilter), hipMemcpyHostToDevice));
    CK(hipMemcpy(dp.p, payloads, (size_t)n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(onion_filter_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const DevFilter *)df.p, (const u32 *)dp.p, (unsigned char *)dflags.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(flags, dflags.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

}
