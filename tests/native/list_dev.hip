// list_dev.hip — TEST-ONLY driver of vg::launch_ptab (vgen_amd/csrc/device/kernels.hip): the lookup / deferred-filter kernel
// and the compaction kernel of a list or contract dispatch, run on buffers the test-suite fills word by word, so that hits
// land where a test puts them (pass, wave and thread edges of the compaction, a full ring, a wrapped running count, stale
// payloads behind a ragged count) instead of where hashes happen to.  Links the product's own build/lib/device/kernels.o:
// the kernels under test are the shipped code objects, not a second compilation.  Not part of libvgen_hip.so.
// (tests/test_gpu_list_kernels.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../vgen_amd/csrc/core/rnd.h"   // (launch.h names RndSeed)
#include "../../vgen_amd/csrc/device/launch.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

// Everything the entry point reads and writes: plain pointers and sizes (mirrored field by field in the test module).
struct listdev_job {
    uint32_t payload_words, stride, count, images, repeat;
    uint32_t match_base, match_cap;
    uint32_t header_in[4];              // DevMatchHeader on entry: count, cap, clk_cycles, clk_ticks
    const uint32_t *payloads;           // images * stride * payload_words words: every slot, those at or past count included
    const uint64_t *hits_in;            // images * stride / 64 + 64 words: initial mask and the guard words behind it
    const uint32_t *recs_in;            // (match_cap + 64) records of 10 words: initial ring and the guard records behind it
    // a table (filter == nullptr) ...
    uint32_t bits, n;
    uint32_t bitmap_words, offsets_count;
    const uint32_t *bitmap, *offsets;
    const uint64_t *lo, *hi;
    // ... or a compiled filter of the public vgen_filter_compile
    const vgen_filter *filter;
    // outputs
    int32_t launch_error;               // hipError_t of the first launch_ptab that did not succeed (0 = all did)
    uint32_t header_out[4];
    uint64_t *hits_out;                 // same sizes as the inputs
    uint32_t *recs_out;
};

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -(int)e_ - 1000; } while (0)

namespace {

// (an empty array still gets an address of its own)
template <typename T>
hipError_t dev_copy_of(T **d, const T *h, size_t count) {
    const size_t bytes = count * sizeof(T);
    hipError_t e = hipMalloc((void **)d, bytes ? bytes : 256);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

// (the test module mirrors listdev_job with ctypes and checks its size against this)
int listdev_job_size() { return (int)sizeof(listdev_job); }

int listdev_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// Uploads the job, calls launch_ptab `repeat` times back to back on the same buffers (stream 0), synchronises and copies the
// mask, the header and the records back.  Returns 0, or -(hipError_t) - 1000 of the first HIP call of the harness that
// failed: it returns at once then and starts nothing else.  A launch_ptab that does not return hipSuccess is reported in
// job->launch_error: no further launch and no synchronisation follow it, only the copies back (a rejected launch must have
// left every buffer as it was).
int listdev_run(listdev_job *j) {
    if (!j || (j->payload_words != 5 && j->payload_words != 8) || j->repeat == 0) return -1;
    const size_t slots = (size_t)j->images * j->stride;
    if (slots % 64 != 0 || slots > (1u << 24)) return -1;
    const size_t words = slots / 64 + 64, recs = (size_t)j->match_cap + 64;
    if (!j->filter && (j->bits > 25 || j->bitmap_words < ((1ull << j->bits) + 31) / 32 || j->offsets_count < (1ull << j->bits) + 1)) return -1;

    uint32_t *d_pay = nullptr, *d_bitmap = nullptr, *d_offsets = nullptr, *d_blob = nullptr, *d_lut = nullptr;
    uint64_t *d_lo = nullptr, *d_hi = nullptr;
    unsigned long long *d_hits = nullptr;
    uint8_t *d_match = nullptr;   // header, then the records (the frame's layout: runtime.cpp, enqueue_ptab)
    DevFilter *d_filter = nullptr;

    CK(dev_copy_of(&d_pay, j->payloads, slots * j->payload_words));
    CK(dev_copy_of(&d_hits, reinterpret_cast<const unsigned long long *>(j->hits_in), words));
    CK(hipMalloc((void **)&d_match, sizeof(DevMatchHeader) + recs * sizeof(DevMatch)));
    CK(hipMemcpy(d_match, j->header_in, sizeof(DevMatchHeader), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_match + sizeof(DevMatchHeader), j->recs_in, recs * sizeof(DevMatch), hipMemcpyHostToDevice));

    PtabArgs p;
    memset(&p, 0, sizeof p);
    if (j->filter) {
        const vgen_filter *f = j->filter;
        DevFilter h = f->dev;
        if (f->dev.chk_lut) {
            CK(dev_copy_of(&d_lut, f->chk_lut.data(), f->chk_lut.size()));
            h.chk_lut = d_lut;
        }
        if (f->dev.kind == DEVF_DFA) {
            CK(dev_copy_of(&d_blob, f->dfa_blob.data(), f->dfa_blob.size()));
            h.dfa_blob = d_blob;
            p.dfa_blob = d_blob;
            p.dfa_bytes = h.dfa_bytes;
        }
        CK(dev_copy_of(&d_filter, &h, 1));
        p.filter = d_filter;
        p.fmt = (uint32_t)vgf_string_format((int)f->format);
    } else {
        CK(dev_copy_of(&d_bitmap, j->bitmap, j->bitmap_words));
        CK(dev_copy_of(&d_offsets, j->offsets, j->offsets_count));
        CK(dev_copy_of(&d_lo, j->lo, j->n));
        CK(dev_copy_of(&d_hi, j->hi, j->n));
        p.tab.bitmap = d_bitmap;
        p.tab.offsets = d_offsets;
        p.tab.lo = d_lo;
        p.tab.hi = d_hi;
        p.tab.bits = j->bits;
        p.tab.n = j->n;
    }
    p.payloads = d_pay;
    p.hits = d_hits;
    p.mhdr = reinterpret_cast<DevMatchHeader *>(d_match);
    p.mrec = reinterpret_cast<DevMatch *>(d_match + sizeof(DevMatchHeader));
    p.stride = j->stride;
    p.count = j->count;
    p.images = j->images;
    p.match_base = j->match_base;
    p.match_cap = j->match_cap;

    j->launch_error = 0;
    for (uint32_t r = 0; r < j->repeat; r++) {
        const hipError_t e = launch_ptab(p, (int)j->payload_words, 0);
        if (e != hipSuccess) {
            j->launch_error = (int32_t)e;
            break;
        }
    }
    if (j->launch_error == 0) CK(hipDeviceSynchronize());
    CK(hipMemcpy(j->hits_out, d_hits, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->header_out, d_match, sizeof(DevMatchHeader), hipMemcpyDeviceToHost));
    CK(hipMemcpy(j->recs_out, d_match + sizeof(DevMatchHeader), recs * sizeof(DevMatch), hipMemcpyDeviceToHost));
    (void)hipFree(d_pay); (void)hipFree(d_hits); (void)hipFree(d_match); (void)hipFree(d_bitmap); (void)hipFree(d_offsets);
    (void)hipFree(d_lo); (void)hipFree(d_hi); (void)hipFree(d_blob); (void)hipFree(d_lut); (void)hipFree(d_filter);
    return 0;
}

}
