// leanmul_dev.hip — TEST-ONLY device build of the forms of core/fe.h that exist for the sequential scan kernels' key loop, one
// input per lane (beside core_dev.hip, which runs the plain forms): the LEAN products with an addend — on the device the
// squaring's doubled limbs are a v_add_u32 written in asm, which no host build contains.  tests/test_gpu_leanmul.py.  Not part of
// libvgen_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../vgen_amd/csrc/core/fe.h"

using namespace vg;

enum { OP_MUL_ADD, OP_SQR_ADD, OP_MUL_ADD_PLAIN, OP_SQR_ADD_PLAIN };

__global__ void __launch_bounds__(64) leanmul_kernel(int op, int n, const u32 *a, const u32 *b, const u32 *c, u32 *r) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int k = i < n ? i : n - 1;
    fe x, y, z, w;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        x.n[j] = a[(size_t)k * 9 + j];
        y.n[j] = b[(size_t)k * 9 + j];
        z.n[j] = c[(size_t)k * 9 + j];
    }
    fe_set_zero(w);
    switch (op) {
    case OP_MUL_ADD: fe_mul_add<true>(w, x, y, z); break;
    case OP_SQR_ADD: fe_sqr_add<true>(w, x, z); break;
    case OP_MUL_ADD_PLAIN: fe_mul_add(w, x, y, z); break;
    case OP_SQR_ADD_PLAIN: fe_sqr_add(w, x, z); break;
    }
    if (i < n) {
#pragma unroll
        for (int j = 0; j < 9; j++) r[(size_t)i * 9 + j] = w.n[j];
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

extern "C" {

int leandev_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// a, b, c, r: n x 9 words each
int leandev_run(int op, int n, const u32 *a, const u32 *b, const u32 *c, u32 *r) {
    if (n <= 0) return 0;
    const size_t bytes = (size_t)n * 9 * sizeof(u32);
    u32 *d = nullptr;   // a | b | c | r
    CK(hipMalloc((void **)&d, 4 * bytes));
    CK(hipMemcpy(d, a, bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d + (size_t)n * 9, b, bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d + (size_t)n * 18, c, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(leanmul_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, d, d + (size_t)n * 9, d + (size_t)n * 18, d + (size_t)n * 27);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(r, d + (size_t)n * 27, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return 0;
}

}
