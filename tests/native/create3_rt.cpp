// create3_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime with CREATE2 contexts and score filters (score_rt.cpp, which includes
// create2_rt.cpp and fake_rt.cpp; all three as they are) with CREATE3 jobs added, so that vgen_scan_create3 (scanner.cpp) and the
// CREATE3 entry points of cabi.cpp run under AddressSanitizer + UBSan without a device.
// The stand-in creates its format-7 contexts itself, so the driver hands each one to create3_rt_adopt, which sets
// vgen_ctx::create3_set and puts a dispatch in front of the stand-in's that serves a CREATE3 job: every salt through the
// single-source twins of the device blocks on the words the kernels form (core/hash.h), then the stand-in's emit / rt_wait like
// every other dispatch.  As in the runtime proper, either kind of job replaces the other.
// Built and run by tests/test_create3_scan_host.py; never loaded by vgen_amd.
#include "score_rt.cpp"

namespace vg {

namespace {

struct Create3State {
    int (*set2)(vgen_ctx *, const uint8_t *, const uint8_t *, const uint8_t *) = nullptr;
    int (*dispatch2)(vgen_ctx *, uint32_t, uint64_t) = nullptr;
};
std::mutex g_c3_mu;
std::map<const vgen_ctx *, Create3State> g_c3;

Create3State &c3_state(const vgen_ctx *c) {
    std::lock_guard<std::mutex> g(g_c3_mu);
    return g_c3[c];
}

int c3_set_create2(vgen_ctx *c, const uint8_t deployer[20], const uint8_t init_code_hash[32], const uint8_t salt_prefix[24]) {
    const int rc = c3_state(c).set2(c, deployer, init_code_hash, salt_prefix);
    if (rc == VGEN_OK) c->have_create3 = false;
    return rc;
}

int c3_set(vgen_ctx *c, const uint8_t factory[20], const uint8_t proxy_hash[32], const uint8_t salt_prefix[24], const uint8_t *guard, int guard_len) {
    if (guard_len < -1 || guard_len > 64 || (guard_len > 0 && !guard)) return c->fail(VGEN_E_INVALID, "vgen_set_create3: guard_len is -1 (no guard) or 0 .. 64 bytes");
    for (auto &fr : c->fr)
        if (fr.in_flight) return c->fail(VGEN_E_STATE, "vgen_set_create3 while a dispatch is in flight");
    uint8_t salt[32] = {0};
    if (guard_len < 0) memcpy(salt, salt_prefix, 24);
    create2_message(factory, salt, proxy_hash, c->create2_m);
    memset(c->create3_w, 0, sizeof c->create3_w);
    if (guard_len >= 0) create3_guard_message(guard, guard_len, salt_prefix, c->create3_w);
    c->create3_guard_len = guard_len;
    c->have_create3 = true;
    c->have_create2 = false;
    return VGEN_OK;
}

int c3_dispatch(vgen_ctx *c0, uint32_t frame, uint64_t first_counter) {
    if (!c0->have_create3) return c3_state(c0).dispatch2(c0, frame, first_counter);   // a CREATE2 job, or none yet
    FakeCtx *c = fc(c0);
    if (frame >= c->frames) return c->fail(VGEN_E_INVALID, "bad frame index");
    if (first_counter > UINT64_MAX - (c->batch - 1)) return c->fail(VGEN_E_RANGE, "vgen_dispatch_create2: the counter range passes 2^64 - 1");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    if (int rc = ensure_frame(c, frame)) return rc;
    return start_dispatch(c, frame, c->batch, [c, first_counter](FakeFrame &ff, bool dump) {
        const bool dfa = !dump && c->h_filter.kind == DEVF_DFA;
        const int guard_len = c->create3_guard_len;
        for (uint32_t i = 0; i < c->batch; i++) {
            u32 m[22], proxy[5], pl[8] = {0};
            memcpy(m, c->create2_m, sizeof m);
            if (guard_len >= 0) {
                u32 w[26], d[8];
                memcpy(w, c->create3_w, sizeof w);
                create3_guard_place_counter(w, (u32)guard_len + 24u, first_counter + i);
                keccak256_guard_digest(w, d);
                create3_place_digest(m, d);
            } else {
                create2_place_counter(m, first_counter + i);
            }
            keccak256_create2_addr(m, proxy);
            keccak256_create1_addr(proxy, pl);
            if (!dfa) {
                emit(c, ff, dump, i, pl, true);
            } else if (dfa_match_payload_n<5>(c->h_filter.dfa_blob, VGF_ETHEREUM, pl)) {
                DevMatch r;
                r.index = i;
                r.reserved = 0;
                memcpy(r.payload, pl, sizeof r.payload);
                ff.found.push_back(r);
            }
        }
    });
}

}  // namespace

}  // namespace vg

// A format-7 context of the stand-in learns CREATE3 jobs (once, right after vgen_create and before any filter is set).
extern "C" void create3_rt_adopt(vgen_ctx *c) {
    vg::Create3State &s = vg::c3_state(c);
    s.set2 = c->create2_set;
    s.dispatch2 = c->create2_dispatch;
    c->have_create3 = false;
    c->create2_set = vg::c3_set_create2;
    c->create2_dispatch = vg::c3_dispatch;
    c->create3_set = vg::c3_set;
}
