// ed_keys_dev.hip — TEST-ONLY driver of vg::launch_ed_keys (vgen_amd/csrc/device/kernels.hip): ed_keys_kernel in its dump and filter
// forms and ptab_compact_kernel<8> behind the latter, on what a context never hands them - a table the test crafted (EdArgs::table
// is a plain pointer: points of small order, a point and itself, a point and its negative among the entries), one workgroup, a
// keyless wave inside a keyed workgroup, n = 1, filtered dispatches with n < batch, rings of any capacity - and every argument
// launch_ed_keys must refuse.  Links the product's own build/lib/device/kernels.o: the kernels under test are the shipped code objects,
// not a second compilation; the real table and the filter program come from the product's host sources.  Every device buffer starts
// poisoned, has EDKEYS_GUARD poisoned words behind it and is copied back whole.  No kernel is defined here.
// Not part of libvgen_hip.so.  (tests/test_gpu_ed_keys_kernel.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"
#include "../../vgen_amd/csrc/host/ed_host.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

constexpr uint32_t EDKEYS_GUARD = 1024;            // poisoned words behind every device buffer
constexpr uint32_t EDKEYS_GUARD_RECS = 128;        // ... behind the ring: whole records of ten words
constexpr uint32_t EDKEYS_POISON = 0xA5C3A5C3u;    // (no canonical limb, which is below 2^29, equals it; the tests assert that no expected payload word does)
constexpr uint32_t EDKEYS_MAX_BATCH = 4096;

// One launch_ed_keys (mirrored field by field in the test module).  The buffers are sized for alloc_batch; `batch` and `n` are what
// the launcher is told.
struct edkeys_job {
    uint32_t alloc_batch, batch, n;
    uint32_t filter_form;               // 0: dump (compact == nullptr); 1: filter form with the compaction
    uint32_t ci;                        // filter form: the pattern is case-insensitive
    // refusals, one per guard of launch_ed_keys
    uint32_t null_table, null_payloads, null_hits, null_filter;
    uint32_t other_payloads, other_hits;   // a PtabArgs naming another payload buffer / another hit mask
    uint32_t other_stride, other_images;   // PtabArgs::stride = batch - 256; PtabArgs::images = 0
    uint32_t null_mhdr, null_mrec;
    uint32_t match_base, match_cap;
    uint32_t header_in[4];              // DevMatchHeader on entry: count, cap, clk_cycles, clk_ticks
    uint32_t seed[6];                   // the stream form (seeds == nullptr): RndSeed::w, ...
    uint32_t stream;
    unsigned long long first;           // ... the stream and the index of lane 0
    const uint32_t *table;              // nullptr: ed_host_table(); else ED_TABLE_WORDS words
    const uint8_t *seeds;               // alloc_batch x 32 bytes, or nullptr for the stream form
    const char *pattern;                // filter form: compiled with filter_compile(..., VGF_SOLANA, ...)
    // outputs
    int32_t launch_error;               // hipError_t of launch_ed_keys (0 = success)
    int32_t sync_error;                 // hipError_t of the synchronisation that closes an accepted launch
    uint32_t filter_kind;               // DevFilter::kind of the compiled pattern
    uint32_t header_out[4];
    uint32_t *payloads_out;             // 8 * alloc_batch + EDKEYS_GUARD words
    uint32_t *hits_out;                 // alloc_batch / 32 + EDKEYS_GUARD words (the 64-bit mask words as pairs, low half first)
    uint32_t *recs_out;                 // filter form: (match_cap + EDKEYS_GUARD_RECS) records of 10 words
    uint32_t *table_guard_out;          // EDKEYS_GUARD words: what lies behind the uploaded table ...
    uint32_t *seeds_guard_out;          // ... and behind the uploaded seeds (untouched in the stream form)
};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

namespace {

struct DevBuf {
    uint32_t *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

hipError_t poisoned(DevBuf &d, size_t words) {
    hipError_t e = hipMalloc((void **)&d.p, words * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    return hipMemsetD32((hipDeviceptr_t)d.p, (int)EDKEYS_POISON, words);
}

// (the inputs get guard words too: a kernel that reads a little past them reads poison, not another allocation)
hipError_t uploaded(DevBuf &d, const void *src, size_t words) {
    hipError_t e = poisoned(d, words + EDKEYS_GUARD);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, src, words * sizeof(uint32_t), hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

// (the test module mirrors the job with ctypes and checks its size against this)
int edkeys_job_size() { return (int)sizeof(edkeys_job); }
uint32_t edkeys_guard_words() { return EDKEYS_GUARD; }
uint32_t edkeys_guard_records() { return EDKEYS_GUARD_RECS; }
uint32_t edkeys_poison() { return EDKEYS_POISON; }
uint32_t edkeys_table_words() { return (uint32_t)ED_TABLE_WORDS; }
uint32_t edkeys_workgroup() { return (uint32_t)ED_WG; }

int edkeys_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// Uploads the table and the seeds, fills EdArgs and PtabArgs as enqueue_ed does (runtime.cpp), calls launch_ed_keys once on stream 0,
// synchronises and copies the payloads, the hit mask, the header and the records back, each with the guard words behind it.
// Returns 0; -1 for a job the buffers could not hold whatever the launcher says (batch beyond alloc_batch, n beyond the uploaded
// seeds); -2 for a pattern that does not compile; -3 for a filter of another kind than 1, 3 or 7; -(hipError_t) - 1000 of the first
// HIP call of the harness that failed: it returns at once then and starts nothing else.  A refused launch is reported in
// job->launch_error, is not synchronised on, and must have left every buffer as it was.  An accepted one is synchronised on; a
// failure of that is reported in job->sync_error and nothing follows it.
int edkeys_run(edkeys_job *j) {
    if (!j || !j->payloads_out || !j->hits_out || !j->table_guard_out || !j->seeds_guard_out) return -1;
    if (j->alloc_batch == 0 || j->alloc_batch % ED_WG != 0 || j->alloc_batch > EDKEYS_MAX_BATCH) return -1;
    if (j->batch > j->alloc_batch || j->n > j->alloc_batch + 1) return -1;   // (n = batch + 1 is refused by the launcher; lanes stop at batch)
    if (j->filter_form && (!j->pattern || !j->recs_out)) return -1;
    if (j->other_stride && j->batch < 512) return -1;
    j->launch_error = j->sync_error = -1;
    const size_t B = j->alloc_batch;
    const size_t pay_w = 8 * B, hit_w = B / 32, seed_w = 8 * B;
    const size_t recs = (size_t)j->match_cap + EDKEYS_GUARD_RECS, rec_w = sizeof(DevMatch) / 4, hdr_w = sizeof(DevMatchHeader) / 4;

    vgen_filter f;
    if (j->filter_form) {
        std::string err;
        if (!filter_compile(j->pattern, j->ci != 0, VGF_SOLANA, f, err)) return -2;
        j->filter_kind = f.dev.kind;
        if ((f.dev.kind != DEVF_RANGES && f.dev.kind != DEVF_ALL && f.dev.kind != DEVF_SOL_RESIDUE) || f.dev.chk_lut || f.dev.dfa_blob) return -3;
    }

    DevBuf table, seeds, pay, hits, match, filter;
    CK(uploaded(table, j->table ? j->table : ed_host_table(), ED_TABLE_WORDS));
    if (j->seeds) CK(uploaded(seeds, j->seeds, seed_w));
    else CK(poisoned(seeds, EDKEYS_GUARD));
    CK(poisoned(pay, pay_w + EDKEYS_GUARD));
    CK(poisoned(hits, hit_w + EDKEYS_GUARD));

    EdArgs a;
    memset(&a, 0, sizeof a);
    a.table = j->null_table ? nullptr : table.p;
    a.seeds = j->seeds ? reinterpret_cast<const uint8_t *>(seeds.p) : nullptr;
    memcpy(a.seed, j->seed, sizeof a.seed);
    a.stream = j->stream;
    a.first = j->first;
    a.n = j->n;
    a.payloads = j->null_payloads ? nullptr : pay.p;
    PtabArgs p;
    memset(&p, 0, sizeof p);
    if (j->filter_form) {
        CK(poisoned(match, hdr_w + recs * rec_w));
        CK(hipMemcpy(match.p, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
        CK(hipMalloc((void **)&filter.p, sizeof(DevFilter)));
        CK(hipMemcpy(filter.p, &f.dev, sizeof(DevFilter), hipMemcpyHostToDevice));
        a.hits = j->null_hits ? nullptr : reinterpret_cast<unsigned long long *>(hits.p);
        a.filter = j->null_filter ? nullptr : reinterpret_cast<const DevFilter *>(filter.p);
        // (every "other" value keeps a compaction that ran all the same inside the buffers and their guards)
        p.payloads = j->other_payloads ? pay.p + 8 : pay.p;
        p.hits = reinterpret_cast<unsigned long long *>(hits.p) + (j->other_hits ? 1 : 0);
        p.mhdr = j->null_mhdr ? nullptr : reinterpret_cast<DevMatchHeader *>(match.p);
        p.mrec = j->null_mrec ? nullptr : reinterpret_cast<DevMatch *>(match.p + hdr_w);
        p.stride = j->other_stride ? j->batch - 256 : j->batch;
        p.count = j->n;
        p.images = j->other_images ? 0 : 1;
        p.match_base = j->match_base;
        p.match_cap = j->match_cap;
    }
    CK(hipDeviceSynchronize());   // (the fills are done before the first kernel)

    const hipError_t e = launch_ed_keys(a, j->batch, j->filter_form ? &p : nullptr, 0);
    j->launch_error = (int32_t)e;
    if (e == hipSuccess) {
        const hipError_t s = hipDeviceSynchronize();
        j->sync_error = (int32_t)s;
        if (s != hipSuccess) return -(int)s - 1000;
    }

    CK(hipMemcpy(j->payloads_out, pay.p, (pay_w + EDKEYS_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->hits_out, hits.p, (hit_w + EDKEYS_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->table_guard_out, table.p + ED_TABLE_WORDS, EDKEYS_GUARD * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->seeds_guard_out, seeds.p + (j->seeds ? seed_w : 0), EDKEYS_GUARD * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (j->filter_form) {
        CK(hipMemcpy(j->header_out, match.p, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
        CK(hipMemcpy(j->recs_out, match.p + hdr_w, recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    }
    return 0;
}

}
