// match_dev.hip — TEST-ONLY device build of the two headers that decide whether a key is reported: core/filter_eval.h (the
// prefilters: hash160 ranges behind the wave-uniform VG_ANY_LANE branch, Bech32 / hex masks, the checksum through chk_lut) and
// core/dfa_eval.h (the full matcher: Base58Check with its leading-'1' run, the five-digit chunks and divmod_d5, the checksum as
// the generated base58_check_block; Bech32(m) over 5 and 8 words; hex).  One payload per thread, in the instantiations the
// product's kernels compile (MatchFmt in device/kernels.hip), on payloads the test-suite crafts, so that a range bound, a lone
// `near` lane, a long zero run or a chunk edge reaches the code as hipcc compiles it instead of waiting for a hash to land
// there.  Compiled like device/kernels.hip (same flags, VG_HASH_BLOCKS).  Not part of libvgen_hip.so.
// (tests/test_gpu_match_device.py)
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VG_HASH_BLOCKS 1   // base58_checksum runs as the scheduled block, as in the product's kernels
#include "../../vgen_amd/csrc/core/dfa_eval.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/device/device_types.h"
#include "../../vgen_amd/csrc/host/filter.h"

namespace vg {
#include "../../vgen_amd/csrc/device/hash_blocks.inc"
}

using namespace vg;

constexpr uint32_t MATCHDEV_MAX_N = 8192;   // payloads per launch

// FULL: the automaton staged into dynamic LDS exactly as payload_filter_kernel stages it, then the matcher; else the prefilter
// on a DevFilter in device memory.  Every lane of the last wave computes, on a clamped index (VG_ANY_LANE looks at all lanes);
// only threads below n store.
template <int NW, int KFMT, bool FULL>
__global__ void __launch_bounds__(256) match_kernel(const u32 *payloads, u32 n, const DevFilter *filter, const u32 *dfa_blob,
                                                    u32 dfa_bytes, int fmt, u32 *out) {
    extern __shared__ u32 dyn_lds[];
    if (FULL) {
        for (u32 i = threadIdx.x; i < dfa_bytes / 4; i += 256u) dyn_lds[i] = dfa_blob[i];
        __syncthreads();
    }
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    const u32 k = i < n ? i : n - 1;
    const u32 *p = payloads + (size_t)k * NW;
    u32 pl[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) pl[w] = p[w];
    const bool hit = FULL ? dfa_match_payload_n<NW, KFMT>(dyn_lds, fmt, pl) : filter_eval_n<NW>(filter, pl);
    if (i < n) out[i] = hit ? 1u : 0u;
}

__global__ void __launch_bounds__(256) divmod_kernel(const u32 *hi, const u32 *lo, u32 n, u32 *q, u32 *r) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u32 qq, rr;
    divmod_d5(hi[i], lo[i], qq, rr);
    q[i] = qq;
    r[i] = rr;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

namespace {

// the instantiations of the product (device/kernels.hip: MatchFmt), in the order of matchdev_run's `inst`
enum { INST_P2PKH, INST_P2SH, INST_UNCOMPRESSED, INST_ANY5, INST_ANY8, INST_COUNT };

bool inst_serves(int inst, int fmt) {
    switch (inst) {
    case INST_P2PKH: return fmt == VGF_P2PKH || fmt == VGF_P2WPKH;
    case INST_P2SH: return fmt == VGF_P2SH_P2WPKH;
    case INST_UNCOMPRESSED: return fmt == VGF_P2PKH_UNCOMPRESSED;
    case INST_ANY5: return fmt == VGF_P2PKH || fmt == VGF_P2WPKH || fmt == VGF_P2SH_P2WPKH || fmt == VGF_P2PKH_UNCOMPRESSED || fmt == VGF_ETHEREUM;
    case INST_ANY8: return fmt == VGF_P2TR;
    }
    return false;
}

template <int NW, int KFMT>
void launch(bool full, u32 n, const u32 *pay, const DevFilter *filter, const u32 *blob, u32 dfa_bytes, int fmt, u32 *out) {
    const dim3 grid((n + 255) / 256), block(256);
    if (full) hipLaunchKernelGGL((match_kernel<NW, KFMT, true>), grid, block, dfa_bytes, 0, pay, n, filter, blob, dfa_bytes, fmt, out);
    else hipLaunchKernelGGL((match_kernel<NW, KFMT, false>), grid, block, 0, 0, pay, n, filter, blob, dfa_bytes, fmt, out);
}

// The device buffers of one call: freed when the call returns, on the error paths too.
struct DevBuffers {
    void *ptr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int used = 0;
    ~DevBuffers() {
        for (int i = 0; i < used; i++) (void)hipFree(ptr[i]);
    }
    template <typename T>
    hipError_t alloc(T **d, size_t count) {
        if (used == 8) return hipErrorOutOfMemory;
        hipError_t e = hipMalloc((void **)d, count * sizeof(T));
        if (e == hipSuccess) ptr[used++] = *d;
        return e;
    }
    template <typename T>
    hipError_t copy_of(T **d, const T *h, size_t count) {
        hipError_t e = alloc(d, count);
        if (e != hipSuccess) return e;
        return hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice);
    }
};

}  // namespace

extern "C" {

int matchdev_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// What the handle holds, for the test to compare with the host build's export: kind, flags, count, witver, whether the
// filter carries chk_lut, dfa_bytes.
int matchdev_filter_info(const vgen_filter *f, uint32_t out[6]) {
    if (!f || f->list) return -1;
    out[0] = f->dev.kind;
    out[1] = f->dev.flags;
    out[2] = f->dev.count;
    out[3] = f->dev.witver;
    out[4] = f->dev.chk_lut && !f->chk_lut.empty() ? 1u : 0u;
    out[5] = f->dev.dfa_bytes;
    return 0;
}

// n payloads (n * 5 words, n * 8 for INST_ANY8; memory order) through instantiation `inst` with the filter's own format as the
// run-time fmt: the full matcher when the filter's device kind is DEVF_DFA, else the prefilter.  out: one word per payload.
// Returns 0; -1 for arguments that are not run (nothing is started); -(hipError_t) - 1000 of the first HIP call that failed: it
// returns at once then and starts nothing else.
int matchdev_run(const vgen_filter *f, const uint32_t *payloads, int inst, uint32_t n, uint32_t *out) {
    if (!f || f->list || !payloads || !out || n == 0 || n > MATCHDEV_MAX_N || inst < 0 || inst >= INST_COUNT) return -1;
    const int fmt = vgf_string_format((int)f->format);
    if (!inst_serves(inst, fmt)) return -1;
    const u32 kind = f->dev.kind;
    if (kind != DEVF_RANGES && kind != DEVF_MASKED && kind != DEVF_DFA) return -1;
    const bool full = kind == DEVF_DFA;
    if (full && (f->dev.dfa_bytes > DFA_MAX_BYTES || f->dev.dfa_bytes != f->dfa_blob.size() * 4 || f->dfa_blob.size() < DFA_HDR_WORDS)) return -1;
    if (!full && f->dev.count > DEVF_MAX_TESTS) return -1;
    const int nw = inst == INST_ANY8 ? 8 : 5;
    if (f->dev.chk_lut && f->chk_lut.size() != (size_t)nw * 4 * 256) return -1;

    u32 *d_pay = nullptr, *d_out = nullptr, *d_blob = nullptr, *d_lut = nullptr;
    DevFilter *d_filter = nullptr;
    DevBuffers bufs;
    CK(bufs.copy_of(&d_pay, payloads, (size_t)n * nw));
    CK(bufs.alloc(&d_out, n));
    CK(hipMemset(d_out, 0xA5, (size_t)n * sizeof(u32)));
    DevFilter h = f->dev;
    h.chk_lut = nullptr;
    h.dfa_blob = nullptr;
    if (f->dev.chk_lut) {
        CK(bufs.copy_of(&d_lut, f->chk_lut.data(), f->chk_lut.size()));
        h.chk_lut = d_lut;
    }
    if (full) {
        CK(bufs.copy_of(&d_blob, f->dfa_blob.data(), f->dfa_blob.size()));
        h.dfa_blob = d_blob;
    }
    CK(bufs.copy_of(&d_filter, &h, 1));
    const u32 bytes = full ? h.dfa_bytes : 0u;
    switch (inst) {
    case INST_P2PKH: launch<5, VGF_P2PKH>(full, n, d_pay, d_filter, d_blob, bytes, fmt, d_out); break;
    case INST_P2SH: launch<5, VGF_P2SH_P2WPKH>(full, n, d_pay, d_filter, d_blob, bytes, fmt, d_out); break;
    case INST_UNCOMPRESSED: launch<5, VGF_P2PKH_UNCOMPRESSED>(full, n, d_pay, d_filter, d_blob, bytes, fmt, d_out); break;
    case INST_ANY5: launch<5, -1>(full, n, d_pay, d_filter, d_blob, bytes, fmt, d_out); break;
    default: launch<8, -1>(full, n, d_pay, d_filter, d_blob, bytes, fmt, d_out); break;
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, d_out, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost));
    return 0;
}

// (hi[i], lo[i]) -> (q[i], r[i]) through divmod_d5, one input per lane.  The caller keeps hi < 58^5 (the function's domain).
int matchdev_divmod(const uint32_t *hi, const uint32_t *lo, uint32_t n, uint32_t *q, uint32_t *r) {
    if (!hi || !lo || !q || !r || n == 0 || n > MATCHDEV_MAX_N) return -1;
    for (uint32_t i = 0; i < n; i++)
        if (hi[i] >= B58_D5) return -1;
    u32 *d_hi = nullptr, *d_lo = nullptr, *d_q = nullptr, *d_r = nullptr;
    DevBuffers bufs;
    CK(bufs.copy_of(&d_hi, hi, n));
    CK(bufs.copy_of(&d_lo, lo, n));
    CK(bufs.alloc(&d_q, n));
    CK(bufs.alloc(&d_r, n));
    hipLaunchKernelGGL(divmod_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_hi, d_lo, n, d_q, d_r);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(q, d_q, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost));
    CK(hipMemcpy(r, d_r, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost));
    return 0;
}

}
