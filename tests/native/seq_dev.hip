// seq_dev.hip — TEST-ONLY driver of vg::launch_seq_fwd / vg::launch_seq_bwd (vgen_amd/csrc/device/kernels.hip): the sequential
// scan's kernels (seq_fwd_kernel, seq_inv_kernel, seq_bwd_kernel in its shipped instantiations, seq_hash_kernel) on an offset
// table and base points the test-suite chooses, so that the results of the affine additions land where a test puts them — on
// the residues whose weak products need the slow path of fe_canonicalize_product and the parity flip of fe_parity_weak — instead
// of where curve points happen to.  Links the product's own build/lib/device/kernels.o: the kernels under test are the shipped
// code objects, not a second compilation.  Not part of libvgen_hip.so.
// (tests/test_gpu_seq_kernels.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/fe.h"
#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"

using namespace vg;

constexpr uint32_t SEQDEV_GUARD = 1024;           // poisoned words behind every device buffer
constexpr uint32_t SEQDEV_POISON = 0xA5C3A5C3u;   // what every word of the scratch, the dump, the ring and the guards starts as

// Everything the entry point reads and writes: plain pointers and sizes (mirrored field by field in the test module).
struct seqdev_job {
    uint32_t fmt, lanes, s;
    uint32_t lone, endo, split, hash_kpl;   // split: the dispatch gets args.xs and args.hash_kpl, as a context of a split format does
    uint32_t skip_fwd;                      // launch_seq_bwd alone (for a launch it must refuse: nothing reads the scratch then)
    uint32_t match_base, match_cap;         // filter mode (filter != nullptr)
    uint32_t header_in[4];                  // DevMatchHeader on entry: count, cap, clk_cycles, clk_ticks
    const uint32_t *rtab;                   // [18][lanes], limb-major: x limbs 0..8, y limbs 0..8
    const uint32_t *q;                      // s x (qx[9], qy[9]), canonical limbs
    const DevFilter *filter;                // host copy without pointers inside (kinds 1 - 3), or nullptr = dump mode
    // outputs
    int32_t launch_error;                   // hipError_t of the launcher that did not succeed (0 = both did)
    uint32_t failed_stage;                  // 1 = launch_seq_fwd, 2 = launch_seq_bwd
    uint32_t scratch_words, dump_words;     // what the driver sized (without the guards)
    uint32_t header_out[4];
    uint32_t *scratch_out;                  // scratch_words_of() + SEQDEV_GUARD words
    uint32_t *dump_out;                     // dump mode: dump_words_of() + SEQDEV_GUARD words
    uint32_t *recs_out;                     // filter mode: (match_cap + SEQDEV_GUARD / 8) records of 10 words
};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

namespace {

hipError_t poisoned(uint32_t **d, size_t words) {
    hipError_t e = hipMalloc((void **)d, words * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    return hipMemsetD32((hipDeviceptr_t)*d, (int)SEQDEV_POISON, words);
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

// (the test module mirrors seqdev_job and DevFilter with ctypes and checks their sizes against these)
int seqdev_job_size() { return (int)sizeof(seqdev_job); }
int seqdev_filter_size() { return (int)sizeof(DevFilter); }
uint32_t seqdev_guard_words() { return SEQDEV_GUARD; }
uint32_t seqdev_poison() { return SEQDEV_POISON; }

int seqdev_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// The frame's scratch exactly as rt_dispatch lays it out (runtime.cpp: scratch_words):
//   pre [S][9][lanes] | tree [groups][9][WG] | root [9][groups] | split form: xs [9][n]
uint64_t seqdev_scratch_words(uint32_t lanes, uint32_t s, uint32_t split) {
    const uint64_t groups = lanes / SEQ_WG, n = (uint64_t)2 * s * lanes;
    return (uint64_t)s * 9 * lanes + groups * 9 * SEQ_WG + 9 * groups + (split ? 9 * n : 0);
}
uint64_t seqdev_dump_words(uint32_t lanes, uint32_t s, uint32_t endo) {
    return (uint64_t)2 * s * lanes * 5 * (endo ? 6 : 1);
}

// Uploads the table, fills SeqArgs as rt_dispatch does (the DevSeqQ with the canonical negations, the scratch regions), runs
// launch_seq_fwd and launch_seq_bwd on stream 0, synchronises and copies the scratch, the dump or the header and the records back,
// each with the guard words behind it.  Returns 0, or -(hipError_t) - 1000 of the first HIP call of the harness that failed: it
// returns at once then and starts nothing else.  A launcher that does not return hipSuccess is reported in job->launch_error:
// nothing is launched or synchronised after it, only the copies back (a refused launch must have left every buffer as it was).
int seqdev_run(seqdev_job *j) {
    if (!j || !j->rtab || !j->q || !j->scratch_out || j->lanes == 0 || j->lanes > (1u << 16) || j->s == 0 || j->s > 64) return -1;
    if (j->filter ? !j->recs_out : !j->dump_out) return -1;
    if (j->filter && (j->filter->kind < DEVF_RANGES || j->filter->kind > DEVF_ALL || j->filter->chk_lut || j->filter->count > DEVF_MAX_TESTS)) return -1;
    const uint32_t lanes = j->lanes, S = j->s, groups = lanes / SEQ_WG;
    const uint64_t n64 = (uint64_t)2 * S * lanes;
    const size_t scratch_w = (size_t)seqdev_scratch_words(lanes, S, j->split), dump_w = (size_t)seqdev_dump_words(lanes, S, j->endo);
    const size_t recs = (size_t)j->match_cap + SEQDEV_GUARD / 8, rec_w = sizeof(DevMatch) / 4, hdr_w = sizeof(DevMatchHeader) / 4;
    j->scratch_words = (uint32_t)scratch_w;
    j->dump_words = (uint32_t)dump_w;

    uint32_t *d_rtab = nullptr, *d_scratch = nullptr, *d_dump = nullptr, *d_match = nullptr;
    DevFilter *d_filter = nullptr;
    CK(hipMalloc((void **)&d_rtab, (size_t)18 * lanes * sizeof(uint32_t)));
    CK(hipMemcpy(d_rtab, j->rtab, (size_t)18 * lanes * sizeof(uint32_t), hipMemcpyHostToDevice));
    CK(poisoned(&d_scratch, scratch_w + SEQDEV_GUARD));

    SeqArgs a;
    memset(&a, 0, sizeof a);
    for (uint32_t k = 0; k < S && k < SEQ_MAX_S; k++) {
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
    if (j->split) {
        a.xs = a.root + (size_t)9 * groups;
        a.hash_kpl = j->hash_kpl;
    }
    a.lanes = lanes;
    a.groups = groups;
    a.n = (uint32_t)n64;
    a.s = S;
    a.lone = j->lone;
    a.endo = j->endo;
    a.fmt = (uint32_t)vgf_string_format((int)j->fmt);
    if (j->filter) {
        CK(poisoned(&d_match, hdr_w + recs * rec_w));
        CK(hipMemcpy(d_match, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
        CK(hipMalloc((void **)&d_filter, sizeof(DevFilter)));
        CK(hipMemcpy(d_filter, j->filter, sizeof(DevFilter), hipMemcpyHostToDevice));
        a.filter = d_filter;
        a.mhdr = reinterpret_cast<DevMatchHeader *>(d_match);
        a.mrec = reinterpret_cast<DevMatch *>(d_match + hdr_w);
        a.match_base = j->match_base;
        a.match_cap = j->match_cap;
    } else {
        CK(poisoned(&d_dump, dump_w + SEQDEV_GUARD));
        a.dump = d_dump;
    }
    CK(hipDeviceSynchronize());   // (the fills are done before the first kernel, whatever stream they ran on)

    j->launch_error = 0;
    j->failed_stage = 0;
    hipError_t e = j->skip_fwd ? hipSuccess : launch_seq_fwd(a, 0);
    if (e != hipSuccess) {
        j->failed_stage = 1;
    } else {
        e = launch_seq_bwd((int)j->fmt, a, 0);
        if (e != hipSuccess) j->failed_stage = 2;
    }
    j->launch_error = (int32_t)e;
    if (e == hipSuccess) CK(hipDeviceSynchronize());

    CK(hipMemcpy(j->scratch_out, d_scratch, (scratch_w + SEQDEV_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (j->filter) {
        CK(hipMemcpy(j->header_out, d_match, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
        CK(hipMemcpy(j->recs_out, d_match + hdr_w, recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    } else {
        CK(hipMemcpy(j->dump_out, d_dump, (dump_w + SEQDEV_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    (void)hipFree(d_rtab); (void)hipFree(d_scratch); (void)hipFree(d_dump); (void)hipFree(d_match); (void)hipFree(d_filter);
    return 0;
}

}
