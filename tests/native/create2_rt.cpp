// create2_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime (fake_rt.cpp, included as it is) with CREATE2 contexts added, so that
// vgen_scan_create2 (scanner.cpp) and the CREATE2 entry points of cabi.cpp run under AddressSanitizer + UBSan without a device.
// A format-7 context is the stand-in's own context with the two CREATE2 entry points of vgen_ctx set; a dispatch is computed with
// the single-source twin of the device block on the message words the kernel forms (core/hash.h), and goes through the stand-in's
// emit / rt_wait like every other dispatch.  Built and run by tests/test_create2_scan_host.py; never loaded by vgen_amd.
#define rt_create rt_create_keys
#include "fake_rt.cpp"
#undef rt_create

namespace vg {

namespace {

int c2_set(vgen_ctx *c, const uint8_t deployer[20], const uint8_t init_code_hash[32], const uint8_t salt_prefix[24]) {
    for (auto &fr : c->fr)
        if (fr.in_flight) return c->fail(VGEN_E_STATE, "vgen_set_create2 while a dispatch is in flight");
    uint8_t salt[32] = {0};
    memcpy(salt, salt_prefix, 24);
    create2_message(deployer, salt, init_code_hash, c->create2_m);
    c->have_create2 = true;
    return VGEN_OK;
}

int c2_dispatch(vgen_ctx *c0, uint32_t frame, uint64_t first_counter) {
    FakeCtx *c = fc(c0);
    if (frame >= c->frames) return c->fail(VGEN_E_INVALID, "bad frame index");
    if (!c->have_create2) return c->fail(VGEN_E_STATE, "vgen_dispatch_create2 before vgen_set_create2");
    if (first_counter > UINT64_MAX - (c->batch - 1)) return c->fail(VGEN_E_RANGE, "vgen_dispatch_create2: the counter range passes 2^64 - 1");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    if (int rc = ensure_frame(c, frame)) return rc;
    return start_dispatch(c, frame, c->batch, [c, first_counter](FakeFrame &ff, bool dump) {
        const bool dfa = !dump && c->h_filter.kind == DEVF_DFA;
        for (uint32_t i = 0; i < c->batch; i++) {
            u32 m[22], pl[8] = {0};
            memcpy(m, c->create2_m, sizeof m);
            create2_place_counter(m, first_counter + i);
            keccak256_create2_addr(m, pl);
            if (!dfa) {
                emit(c, ff, dump, i, pl, true);
            } else if (dfa_match_payload_n<5>(c->h_filter.dfa_blob, VGF_ETHEREUM, pl)) {   // (the automaton judges the address STRING: Ethereum's)
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

int rt_create(const vgen_params *p_in, vgen_ctx **out, std::string &err) {
    if (!p_in || p_in->struct_size != sizeof(vgen_params) || p_in->format != VGF_ETHEREUM_CREATE2) return rt_create_keys(p_in, out, err);
    if (p_in->flags & VGEN_FLAG_ENDO) {
        err = "VGEN_FLAG_ENDO: a CREATE2 search has no curve points";
        return VGEN_E_UNSUPPORTED;
    }
    vgen_params p = *p_in;
    p.format = VGF_ETHEREUM;   // the same payload size and address strings
    if (int rc = rt_create_keys(&p, out, err)) return rc;
    (*out)->format = VGF_ETHEREUM_CREATE2;
    (*out)->create2_set = c2_set;
    (*out)->create2_dispatch = c2_dispatch;
    return VGEN_OK;
}

}  // namespace vg
