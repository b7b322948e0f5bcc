// xonly_dev.hip — TEST-ONLY driver of vg::launch_seq_fwd / vg::launch_seq_bwd for the x-only format (VGF_NOSTR): seq_fwd_kernel,
// seq_inv_kernel and xonly_bwd_kernel in its two shipped instantiations on an offset table and base points the test-suite chooses
// (tests/seq_vectors.py), so that x3 lands on the residues whose weak products need the slow path of fe_canonicalize_product.
// The twin of seq_dev.hip with this format's geometry: eight payload words per slot and three images on an endomorphism dispatch.
// Links the product's own build/lib/device/kernels.o: the kernels under test are the shipped code objects.  Not part of libvgen_hip.so.
// (tests/test_gpu_nostr.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/fe.h"
#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"

using namespace vg;

constexpr uint32_t XDEV_GUARD = 1024;           // poisoned words behind every device buffer
constexpr uint32_t XDEV_POISON = 0xA5C3A5C3u;   // what every word of the scratch, the dump, the ring and the guards starts as

// Everything the entry point reads and writes: plain pointers and sizes (mirrored field by field in the test module).
struct xdev_job {
    uint32_t lanes, s, endo, reserved;
    const uint32_t *rtab;                   // [18][lanes], limb-major: x limbs 0..8, y limbs 0..8
    const uint32_t *q;                      // s x (qx[9], qy[9]), canonical limbs
    // outputs
    int32_t launch_error;                   // hipError_t of the launcher that did not succeed (0 = both did)
    uint32_t failed_stage;                  // 1 = launch_seq_fwd, 2 = launch_seq_bwd
    uint32_t *dump_out;                     // xdev_dump_words() + XDEV_GUARD words
};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

namespace {

hipError_t poisoned(uint32_t **d, size_t words) {
    hipError_t e = hipMalloc((void **)d, words * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    return hipMemsetD32((hipDeviceptr_t)*d, (int)XDEV_POISON, words);
}

// p - a for canonical a != 0 (the test's coordinates are never 0), canonical
void canon_neg(uint32_t r[9], const uint32_t a[9]) {
    fe x, z;
    for (int i = 0; i < 9; i++) x.n[i] = a[i];
    fe_neg(z, x, 1);
    fe_normalize(z);
    for (int i = 0; i < 9; i++) r[i] = z.n[i];
}

}  // namespace

extern "C" {

int xdev_job_size() { return (int)sizeof(xdev_job); }
uint32_t xdev_guard_words() { return XDEV_GUARD; }
uint32_t xdev_poison() { return XDEV_POISON; }

// eight words per slot, 2 S lanes slots per image, three images on an endomorphism dispatch
uint64_t xdev_dump_words(uint32_t lanes, uint32_t s, uint32_t endo) { return (uint64_t)2 * s * lanes * 8 * (endo ? 3 : 1); }

// Uploads the table, fills SeqArgs as rt_dispatch does, runs launch_seq_fwd and launch_seq_bwd(VGF_NOSTR) on stream 0, synchronises
// and copies the dump back with the guard words behind it.  Returns 0, or -(hipError_t) - 1000
// of the first HIP call of the harness that failed: it returns at once then and starts nothing else.
int xdev_run(xdev_job *j) {
    if (!j || !j->rtab || !j->q || j->lanes == 0 || j->lanes % SEQ_WG != 0 || j->lanes > (1u << 16) || j->s < 2 || j->s > SEQ_MAX_S) return -1;
    if (!j->dump_out) return -1;
    const uint32_t lanes = j->lanes, S = j->s, groups = lanes / SEQ_WG;
    const uint64_t n64 = (uint64_t)2 * S * lanes;
    const size_t scratch_w = (size_t)S * 9 * lanes + (size_t)groups * 9 * SEQ_WG + (size_t)9 * groups;
    const size_t dump_w = (size_t)xdev_dump_words(lanes, S, j->endo);

    uint32_t *d_rtab = nullptr, *d_scratch = nullptr, *d_dump = nullptr;
    CK(hipMalloc((void **)&d_rtab, (size_t)18 * lanes * sizeof(uint32_t)));
    CK(hipMemcpy(d_rtab, j->rtab, (size_t)18 * lanes * sizeof(uint32_t), hipMemcpyHostToDevice));
    CK(poisoned(&d_scratch, scratch_w + XDEV_GUARD));

    SeqArgs a;
    memset(&a, 0, sizeof a);
    for (uint32_t k = 0; k < S; k++) {
        DevSeqQ &q = a.q[k];
        memcpy(q.qx, j->q + (size_t)k * 18, sizeof q.qx);
        memcpy(q.qy, j->q + (size_t)k * 18 + 9, sizeof q.qy);
        canon_neg(q.nqx, q.qx);
        canon_neg(q.nqy, q.qy);
    }
    a.rtab = d_rtab;
    a.pre = d_scratch;
    a.tree = a.pre + (size_t)S * 9 * lanes;
    a.root = a.tree + (size_t)groups * 9 * SEQ_WG;
    a.lanes = lanes;
    a.groups = groups;
    a.n = (uint32_t)n64;
    a.s = S;
    a.endo = j->endo;
    a.fmt = VGF_NOSTR;
    CK(poisoned(&d_dump, dump_w + XDEV_GUARD));
    a.dump = d_dump;
    CK(hipDeviceSynchronize());   // (the fills are done before the first kernel, whatever stream they ran on)

    j->failed_stage = 0;
    hipError_t e = launch_seq_fwd(a, 0);
    if (e != hipSuccess) {
        j->failed_stage = 1;
    } else {
        e = launch_seq_bwd(VGF_NOSTR, a, 0);
        if (e != hipSuccess) j->failed_stage = 2;
    }
    j->launch_error = (int32_t)e;
    if (e == hipSuccess) CK(hipDeviceSynchronize());

    CK(hipMemcpy(j->dump_out, d_dump, (dump_w + XDEV_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    (void)hipFree(d_rtab); (void)hipFree(d_scratch); (void)hipFree(d_dump);
    return 0;
}

}
