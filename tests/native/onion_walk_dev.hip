// onion_walk_dev.hip — TEST-ONLY driver of vg::launch_onion_points / vg::launch_onion (vgen_amd/csrc/device/kernels.hip): the onion
// walk's kernels (onion_points_kernel, onion_fwd_kernel, onion_bwd_kernel in its dump and filter forms, ptab_compact_kernel<8> behind
// the latter) on lane counts, lane tables, shared points and a zero slot the test-suite chooses - any L >= 1, not only the multiples
// of 128 a context has; points of small order, P = +-Q and the neutral element among the lane points, not only consecutive multiples
// of 8B.  Links the product's own build/lib/device/kernels.o: the kernels under test are the shipped code objects, not a second
// compilation.  Every device buffer starts poisoned, has ONIONWALK_GUARD poisoned words behind it and is copied back whole.
// Not part of libvgen_hip.so.  (tests/test_gpu_onion_kernels.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"
#include "../../vgen_amd/csrc/host/ed_host.h"

using namespace vg;

constexpr uint32_t ONIONWALK_GUARD = 1024;           // poisoned words behind every device buffer
constexpr uint32_t ONIONWALK_GUARD_RECS = 128;       // ... behind the ring: whole records of ten words
constexpr uint32_t ONIONWALK_POISON = 0xA5C3A5C3u;   // (no canonical limb, which is below 2^29, equals it)
constexpr uint32_t ONIONWALK_MAX_LANES = 4096;

// launch_onion_points: plain values and one output (mirrored field by field in the test module).
struct onionwalk_points_job {
    uint32_t start[8];                  // little-endian words
    uint32_t step, n, mul_d, wstride, istride;
    int32_t launch_error;               // hipError_t of launch_onion_points (0 = success)
    uint32_t *out;                      // 27 * n + ONIONWALK_GUARD words
};

// launch_onion.  The buffers are sized for alloc_lanes; `lanes` and `batch` are what the launcher is told (alloc_lanes and
// 64 * alloc_lanes, except where a test wants the launcher to refuse).
struct onionwalk_job {
    uint32_t alloc_lanes, lanes, batch;
    uint32_t zero_slot;
    uint32_t filter_form;               // 0: dump (compact == nullptr); 1: filter form with the compaction
    uint32_t null_pre, other_payloads;  // refusals: a null OnionArgs::pre; a PtabArgs naming another payload buffer
    uint32_t match_base, match_cap;
    uint32_t header_in[4];              // DevMatchHeader on entry: count, cap, clk_cycles, clk_ticks
    const uint32_t *lane;               // [27][alloc_lanes]: x, y, t = x y, canonical limbs
    const uint32_t *uni;                // [32][27]: x, y, e = d x y, canonical limbs
    const DevFilter *filter;            // filter form: host copy without pointers inside (kinds 2 and 3)
    // outputs
    int32_t launch_error;               // hipError_t of launch_onion (0 = success)
    uint32_t header_out[4];
    uint32_t *pre_out;                  // 18 * 32 * alloc_lanes + ONIONWALK_GUARD words
    uint32_t *inv_out;                  // 9 * alloc_lanes + ONIONWALK_GUARD words
    uint32_t *payloads_out;             // 8 * 64 * alloc_lanes + ONIONWALK_GUARD words
    uint32_t *hits_out;                 // 2 * alloc_lanes + ONIONWALK_GUARD words
    uint32_t *recs_out;                 // filter form: (match_cap + ONIONWALK_GUARD_RECS) records of 10 words
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
    return hipMemsetD32((hipDeviceptr_t)d.p, (int)ONIONWALK_POISON, words);
}

// (the lane and shared points get guard words too: a kernel that reads a little past them reads poison, not another allocation)
hipError_t uploaded(DevBuf &d, const uint32_t *src, size_t words) {
    hipError_t e = poisoned(d, words + ONIONWALK_GUARD);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, src, words * sizeof(uint32_t), hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

// (the test module mirrors the jobs and DevFilter with ctypes and checks their sizes against these)
int onionwalk_job_size() { return (int)sizeof(onionwalk_job); }
int onionwalk_points_job_size() { return (int)sizeof(onionwalk_points_job); }
int onionwalk_filter_size() { return (int)sizeof(DevFilter); }
uint32_t onionwalk_guard_words() { return ONIONWALK_GUARD; }
uint32_t onionwalk_guard_records() { return ONIONWALK_GUARD_RECS; }
uint32_t onionwalk_poison() { return ONIONWALK_POISON; }
uint32_t onionwalk_no_slot() { return ONION_NO_SLOT; }

int onionwalk_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// One launch_onion_points on stream 0 over the product's Ed25519 table into a poisoned buffer.  Returns 0, -1 for a job whose layout
// would leave the 27 n words, or -(hipError_t) - 1000 of the first HIP call of the harness that failed: it returns at once then and
// starts nothing else.  A launcher that does not return hipSuccess is reported in job->launch_error; only the copy back follows it.
int onionwalk_points(onionwalk_points_job *j) {
    if (!j || !j->out || j->n == 0 || j->n > ONIONWALK_MAX_LANES || j->wstride == 0 || j->istride == 0) return -1;
    const size_t words = (size_t)ONION_PT_WORDS * j->n;
    if ((size_t)(ONION_PT_WORDS - 1) * j->wstride + (size_t)(j->n - 1) * j->istride >= words) return -1;
    DevBuf table, out;
    CK(hipMalloc((void **)&table.p, ED_TABLE_WORDS * sizeof(uint32_t)));
    CK(hipMemcpy(table.p, ed_host_table(), ED_TABLE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
    CK(poisoned(out, words + ONIONWALK_GUARD));
    CK(hipDeviceSynchronize());   // (the fill is done before the kernel)
    OnionPointsArgs a;
    memset(&a, 0, sizeof a);
    a.table = table.p;
    memcpy(a.start, j->start, sizeof a.start);
    a.step = j->step;
    a.n = j->n;
    a.mul_d = j->mul_d;
    a.wstride = j->wstride;
    a.istride = j->istride;
    a.out = out.p;
    const hipError_t e = launch_onion_points(a, 0);
    j->launch_error = (int32_t)e;
    if (e == hipSuccess) CK(hipDeviceSynchronize());
    CK(hipMemcpy(j->out, out.p, (words + ONIONWALK_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

// Uploads the lane table and the shared points as they are (launch_onion_points is not called), fills OnionArgs and PtabArgs as
// enqueue_onion does (runtime.cpp), calls launch_onion once on stream 0, synchronises and copies pre, inv, the payloads, the hit mask,
// the header and the records back, each with the guard words behind it.  Returns as onionwalk_points does; a refused launch is
// reported in job->launch_error, is not synchronised on, and must have left every buffer as it was.
int onionwalk_run(onionwalk_job *j) {
    if (!j || !j->lane || !j->uni || !j->pre_out || !j->inv_out || !j->payloads_out || !j->hits_out) return -1;
    if (j->alloc_lanes == 0 || j->alloc_lanes > ONIONWALK_MAX_LANES || j->lanes > j->alloc_lanes) return -1;
    if (j->filter_form && (!j->filter || !j->recs_out || j->filter->chk_lut || j->filter->dfa_blob || j->filter->count > DEVF_MAX_TESTS ||
                           (j->filter->kind != DEVF_MASKED && j->filter->kind != DEVF_ALL)))
        return -1;
    const size_t L = j->alloc_lanes;
    const size_t pre_w = (size_t)2 * ONION_S * 9 * L, inv_w = 9 * L, pay_w = (size_t)2 * ONION_S * L * 8, hit_w = 2 * L;
    const size_t recs = (size_t)j->match_cap + ONIONWALK_GUARD_RECS, rec_w = sizeof(DevMatch) / 4, hdr_w = sizeof(DevMatchHeader) / 4;

    DevBuf lane, uni, pre, inv, pay, hits, match, filter;
    CK(uploaded(lane, j->lane, (size_t)ONION_PT_WORDS * L));
    CK(uploaded(uni, j->uni, (size_t)ONION_PT_WORDS * ONION_S));
    CK(poisoned(pre, pre_w + ONIONWALK_GUARD));
    CK(poisoned(inv, inv_w + ONIONWALK_GUARD));
    CK(poisoned(pay, pay_w + ONIONWALK_GUARD));
    CK(poisoned(hits, hit_w + ONIONWALK_GUARD));

    OnionArgs a;
    memset(&a, 0, sizeof a);
    a.uni = uni.p;
    a.lane = lane.p;
    a.pre = j->null_pre ? nullptr : pre.p;
    a.inv = inv.p;
    a.lanes = j->lanes;
    a.zero_slot = j->zero_slot;
    a.payloads = pay.p;
    PtabArgs p;
    memset(&p, 0, sizeof p);
    if (j->filter_form) {
        CK(poisoned(match, hdr_w + recs * rec_w));
        CK(hipMemcpy(match.p, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
        CK(hipMalloc((void **)&filter.p, sizeof(DevFilter)));
        CK(hipMemcpy(filter.p, j->filter, sizeof(DevFilter), hipMemcpyHostToDevice));
        a.hits = hits.p;
        a.filter = reinterpret_cast<const DevFilter *>(filter.p);
        p.payloads = j->other_payloads ? pay.p + 8 : pay.p;
        p.hits = reinterpret_cast<unsigned long long *>(hits.p);
        p.mhdr = reinterpret_cast<DevMatchHeader *>(match.p);
        p.mrec = reinterpret_cast<DevMatch *>(match.p + hdr_w);
        p.stride = j->batch;
        p.count = j->batch;
        p.images = 1;
        p.match_base = j->match_base;
        p.match_cap = j->match_cap;
    }
    CK(hipDeviceSynchronize());   // (the fills are done before the first kernel)

    const hipError_t e = launch_onion(a, j->batch, j->filter_form ? &p : nullptr, 0, nullptr);
    j->launch_error = (int32_t)e;
    if (e == hipSuccess) CK(hipDeviceSynchronize());

    CK(hipMemcpy(j->pre_out, pre.p, (pre_w + ONIONWALK_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->inv_out, inv.p, (inv_w + ONIONWALK_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->payloads_out, pay.p, (pay_w + ONIONWALK_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->hits_out, hits.p, (hit_w + ONIONWALK_GUARD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (j->filter_form) {
        CK(hipMemcpy(j->header_out, match.p, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
        CK(hipMemcpy(j->recs_out, match.p + hdr_w, recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    }
    return 0;
}

}
