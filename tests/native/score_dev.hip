// score_dev.hip — TEST-ONLY driver of the two score launchers of vgen_amd/csrc/device/kernels.hip.
// vg::launch_payload_score: payload_score_kernel and the compaction behind it on payloads the test-suite crafts (every digit in every
// position, zero bytes at every position, leading runs that end on and across word boundaries, the near misses of a borrowing
// zero-byte test, stale high-scoring payloads behind a ragged count) instead of where hashes happen to land.
// vg::launch_create2_score: its argument checks, and one batch held against the host's vgen_create2_address.
// Links the product's own build/lib/device/kernels.o: the kernels under test are the shipped code objects, not a second
// compilation.  Not part of libvgen_hip.so.  (tests/test_gpu_score_kernels.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/hash.h"  // (create2_message: the message words of a CREATE2 job, host side)
#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"

using namespace vg;

// Everything the first entry point reads and writes: plain pointers and sizes (mirrored field by field in the test module).
struct scoredev_job {
    uint32_t stride, count, images;
    uint32_t match_base, match_cap;
    uint32_t n_terms;
    uint32_t terms[12];                 // (metric, digit, min) x 4
    uint32_t header_in[4];              // DevMatchHeader on entry: count, cap, clk_cycles, clk_ticks
    uint32_t compact_stride;            // what the compaction is told (= stride, except where a test wants the launcher to refuse)
    const uint32_t *payloads;           // images * stride * 5 words: every slot, those at or past count included
    const uint64_t *hits_in;            // images * stride / 64 + 64 words: initial mask and the guard words behind it
    const uint32_t *recs_in;            // (match_cap + 64) records of 10 words: initial ring and the guard records behind it
    // outputs
    int32_t launch_error;               // hipError_t of launch_payload_score (0 = success)
    uint32_t header_out[4];
    uint64_t *hits_out;                 // same sizes as the inputs
    uint32_t *recs_out;
};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

extern "C" {

int scoredev_job_size() { return (int)sizeof(scoredev_job); }

int scoredev_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// Uploads the job, calls launch_payload_score once (stream 0), synchronises and copies the mask, the header and the records back.
// Returns 0, or -(hipError_t) - 1000 of the first HIP call of the harness that failed: it returns at once then and starts nothing
// else.  A launch that is refused is reported in job->launch_error: no synchronisation follows it, only the copies back (a refused
// launch must have left every buffer as it was).
int scoredev_run(scoredev_job *j) {
    if (!j || j->stride == 0 || j->images == 0 || j->images > 6) return -1;
    const size_t slots = (size_t)j->images * j->stride;
    if (slots % 64 != 0 || slots > (1u << 20)) return -1;
    const size_t words = slots / 64 + 64, recs = (size_t)j->match_cap + 64;
    uint32_t *d_pay = nullptr;
    unsigned long long *d_hits = nullptr;
    uint8_t *d_match = nullptr;   // header, then the records (the frame's layout: runtime.cpp, enqueue_ptab)
    CK(hipMalloc((void **)&d_pay, slots * 20));
    CK(hipMemcpy(d_pay, j->payloads, slots * 20, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_hits, words * 8));
    CK(hipMemcpy(d_hits, j->hits_in, words * 8, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_match, sizeof(DevMatchHeader) + recs * sizeof(DevMatch)));
    CK(hipMemcpy(d_match, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_match + sizeof(DevMatchHeader), j->recs_in, recs * sizeof(DevMatch), hipMemcpyHostToDevice));

    ScoreArgs a;
    memset(&a, 0, sizeof a);
    a.terms.n = j->n_terms;
    for (uint32_t k = 0; k < SCORE_MAX_TERMS; k++) {
        a.terms.t[k].metric = j->terms[3 * k];
        a.terms.t[k].digit = j->terms[3 * k + 1];
        a.terms.t[k].min = j->terms[3 * k + 2];
    }
    a.payloads = d_pay;
    a.hits = d_hits;
    a.stride = j->stride;
    a.count = j->count;
    a.images = j->images;
    PtabArgs p;
    memset(&p, 0, sizeof p);
    p.payloads = d_pay;
    p.hits = d_hits;
    p.mhdr = reinterpret_cast<DevMatchHeader *>(d_match);
    p.mrec = reinterpret_cast<DevMatch *>(d_match + sizeof(DevMatchHeader));
    p.stride = j->compact_stride;
    p.count = j->count;
    p.images = j->images;
    p.match_base = j->match_base;
    p.match_cap = j->match_cap;

    j->launch_error = (int32_t)launch_payload_score(a, p, 0);
    if (j->launch_error == 0) CK(hipDeviceSynchronize());
    CK(hipMemcpy(j->hits_out, d_hits, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->header_out, d_match, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->recs_out, d_match + sizeof(DevMatchHeader), recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    (void)hipFree(d_pay);
    (void)hipFree(d_hits);
    (void)hipFree(d_match);
    return 0;
}

// The same for vg::launch_create2_score: `batch` salts of the job (deployer, init_code_hash, salt_prefix || counter) from `first` on.
// payloads_in / payloads_out: batch * 5 words (only hit lanes' slots may change); the other buffers as in scoredev_job.
struct scoredev_c2job {
    uint32_t batch, compact_stride, compact_images;
    uint32_t match_base, match_cap;
    uint32_t n_terms;
    uint32_t terms[12];
    uint32_t header_in[4];
    uint8_t deployer[20], init_code_hash[32], salt_prefix[24];
    unsigned long long first;
    uint32_t alloc_slots;               // slots the buffers hold (>= batch, a multiple of 64; what a refused launch must leave alone)
    uint32_t null_out;                  // 1: pass a null payload pointer (refused)
    const uint32_t *payloads_in;
    const uint64_t *hits_in;            // alloc_slots / 64 + 64 words
    const uint32_t *recs_in;            // (match_cap + 64) records of 10 words
    int32_t launch_error;
    uint32_t header_out[4];
    uint32_t *payloads_out;
    uint64_t *hits_out;
    uint32_t *recs_out;
};

int scoredev_c2job_size() { return (int)sizeof(scoredev_c2job); }

int scoredev_run_create2(scoredev_c2job *j) {
    if (!j || j->alloc_slots == 0 || j->alloc_slots % 64 != 0 || j->alloc_slots > (1u << 20) || j->batch > j->alloc_slots) return -1;
    const size_t slots = j->alloc_slots, words = slots / 64 + 64, recs = (size_t)j->match_cap + 64;
    uint32_t *d_pay = nullptr;
    unsigned long long *d_hits = nullptr;
    uint8_t *d_match = nullptr;
    CK(hipMalloc((void **)&d_pay, slots * 20));
    CK(hipMemcpy(d_pay, j->payloads_in, slots * 20, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_hits, words * 8));
    CK(hipMemcpy(d_hits, j->hits_in, words * 8, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_match, sizeof(DevMatchHeader) + recs * sizeof(DevMatch)));
    CK(hipMemcpy(d_match, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_match + sizeof(DevMatchHeader), j->recs_in, recs * sizeof(DevMatch), hipMemcpyHostToDevice));

    Create2ScoreArgs a;
    memset(&a, 0, sizeof a);
    a.terms.n = j->n_terms;
    for (uint32_t k = 0; k < SCORE_MAX_TERMS; k++) {
        a.terms.t[k].metric = j->terms[3 * k];
        a.terms.t[k].digit = j->terms[3 * k + 1];
        a.terms.t[k].min = j->terms[3 * k + 2];
    }
    uint8_t salt[32] = {0};
    memcpy(salt, j->salt_prefix, 24);   // counter 0: the kernel places the counter
    create2_message(j->deployer, salt, j->init_code_hash, a.m);
    a.first = j->first;
    a.out = j->null_out ? nullptr : d_pay;
    a.hits = d_hits;
    PtabArgs p;
    memset(&p, 0, sizeof p);
    p.payloads = d_pay;
    p.hits = d_hits;
    p.mhdr = reinterpret_cast<DevMatchHeader *>(d_match);
    p.mrec = reinterpret_cast<DevMatch *>(d_match + sizeof(DevMatchHeader));
    p.stride = j->compact_stride;
    p.count = j->compact_stride;
    p.images = j->compact_images;
    p.match_base = j->match_base;
    p.match_cap = j->match_cap;

    j->launch_error = (int32_t)launch_create2_score(a, j->batch, p, 0);
    if (j->launch_error == 0) CK(hipDeviceSynchronize());
    CK(hipMemcpy(j->payloads_out, d_pay, slots * 20, hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->hits_out, d_hits, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->header_out, d_match, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->recs_out, d_match + sizeof(DevMatchHeader), recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    (void)hipFree(d_pay);
    (void)hipFree(d_hits);
    (void)hipFree(d_match);
    return 0;
}

}
