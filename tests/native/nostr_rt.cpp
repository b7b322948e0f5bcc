// nostr_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime (fake_rt.cpp, included as it is) with contexts of the Nostr format
// (VGF_NOSTR) added, so that the host scan loop (scanner.cpp) and cabi.cpp run over the format without a device: the x-only key as
// the 32-byte payload, THREE images per point on a VGEN_FLAG_ENDO context (x, beta x, beta^2 x at e * batch + i, keys_tested =
// 3 x batch), and the format's own candidate tests - the single-source core/filter_eval.h filter_eval_npub, core/dfa_eval.h
// dfa_match_npub and the list lookup the kernels run.  A Nostr context is the stand-in's own eight-word context with the format and
// the flag put back; its dispatches are computed here, one full multiplication per key, and go through the stand-in's start_dispatch /
// rt_wait like every other.  Built by tests/native/nostr.mk into libvgen_fake_nostr.so and driven through the C ABI by
// tests/test_nostr_scan_host.py; never loaded by vgen_amd.
#define rt_create rt_create_keys
#define rt_dispatch rt_dispatch_keys_walk
#define rt_dispatch_keys rt_dispatch_keys_plain
#define rt_dispatch_random rt_dispatch_random_plain
#define rt_set_match_cap rt_set_match_cap_plain
#include "fake_rt.cpp"
#undef rt_create
#undef rt_dispatch
#undef rt_dispatch_keys
#undef rt_dispatch_random
#undef rt_set_match_cap

namespace vg {

namespace {

bool is_nostr(const vgen_ctx *c) { return c->format == VGF_NOSTR; }
uint32_t images_of(const vgen_ctx *c) { return c->endo ? vgf_endo_images(VGF_NOSTR) : 1u; }

bool nostr_candidate(const FakeCtx *c, const u32 *pl) {
    if (c->h_filter.kind == DEVF_LIST) return ptab_find(c->list->view(), ptab_top64(pl)) >= 0;
    if (c->h_filter.kind == DEVF_DFA) return dfa_match_npub(c->h_filter.dfa_blob, pl);
    return filter_eval_npub(&c->h_filter, pl);
}

// key i of a dispatch under its images: one multiplication, then beta^e x - slot e * batch + i; no slot for a scalar that is no key
void emit_xonly(FakeCtx *c, FakeFrame &ff, bool dump, uint32_t i, const Scalar &k) {
    ge pt;
    if (!scalar_is_valid(k) || !host_ec_mul_gen(k, pt)) return;
    fe x = pt.x, beta;
    fe_normalize(x);
    set_beta(beta);
    for (uint32_t e = 0; e < images_of(c); e++) {
        if (e) {
            fe_mul(x, x, beta);
            fe_normalize(x);
        }
        u32 xw[8], pl[8];
        fe_to_words(x, xw);
        for (int w = 0; w < 8; w++) pl[w] = bswap32(xw[7 - w]);
        const uint32_t slot = e * c->batch + i;
        if (dump) {
            memcpy(ff.dump.data() + (size_t)slot * 32, pl, 32);
        } else if (nostr_candidate(c, pl)) {
            DevMatch m;
            m.index = slot;
            m.reserved = 0;
            memcpy(m.payload, pl, 32);
            ff.found.push_back(m);
        }
    }
}

int check_frame(FakeCtx *c, uint32_t frame) {
    if (frame >= c->frames) return c->fail(VGEN_E_INVALID, "bad frame index");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    return ensure_frame(c, frame);
}

}  // namespace

int rt_create(const vgen_params *p_in, vgen_ctx **out, std::string &err) {
    if (!p_in || p_in->struct_size != sizeof(vgen_params) || p_in->format != VGF_NOSTR) return rt_create_keys(p_in, out, err);
    vgen_params p = *p_in;
    p.format = VGF_P2TR;   // the same payload size
    if (int rc = rt_create_keys(&p, out, err)) return rc;
    (*out)->format = VGF_NOSTR;
    (*out)->endo = (p_in->flags & VGEN_FLAG_ENDO) != 0;
    return VGEN_OK;
}

int rt_set_match_cap(vgen_ctx *c, uint32_t cap) {
    if (!is_nostr(c)) return rt_set_match_cap_plain(c, cap);
    for (auto &f : c->fr)
        if (f.in_flight) return c->fail(VGEN_E_STATE, "vgen_set_match_cap while a dispatch is in flight");
    const uint64_t most = (uint64_t)c->batch * images_of(c);
    c->match_cap = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(cap, 256), most);
    return VGEN_OK;
}

int rt_dispatch(vgen_ctx *c0, uint32_t frame, const uint8_t start_key_be[32]) {
    if (!is_nostr(c0)) return rt_dispatch_keys_walk(c0, frame, start_key_be);
    FakeCtx *c = fc(c0);
    if (!start_key_be) return c->fail(VGEN_E_INVALID, "bad frame index / key");
    Scalar k0;
    scalar_from_be(k0, start_key_be);
    if (!scalar_is_valid(k0)) return c->fail(VGEN_E_RANGE, "start key is not a valid secp256k1 scalar");
    if (int rc = check_frame(c, frame)) return rc;
    c->fr[frame].start = k0;
    return start_dispatch(c, frame, (uint64_t)c->batch * images_of(c), [c, k0](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < c->batch; i++) {
            Scalar k;
            if (scalar_add_u64(k, k0, i)) memset(&k, 0, sizeof k);
            emit_xonly(c, ff, dump, i, k);
        }
    }, c->endo);
}

int rt_dispatch_keys(vgen_ctx *c0, uint32_t frame, const uint8_t *keys_be, uint32_t n) {
    if (!is_nostr(c0)) return rt_dispatch_keys_plain(c0, frame, keys_be, n);
    FakeCtx *c = fc(c0);
    if (!keys_be || n == 0 || n > c->batch) return c->fail(VGEN_E_INVALID, "vgen_dispatch_keys: bad key buffer / n");
    if (int rc = check_frame(c, frame)) return rc;
    std::vector<uint8_t> keys(keys_be, keys_be + (size_t)n * 32);
    return start_dispatch(c, frame, (uint64_t)n * images_of(c), [c, keys, n](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < n; i++) {
            Scalar k;
            scalar_from_be(k, keys.data() + (size_t)i * 32);
            emit_xonly(c, ff, dump, i, k);
        }
    }, c->endo);
}

int rt_dispatch_random(vgen_ctx *c0, uint32_t frame, const RndSeed &seed, uint32_t stream, uint64_t first_index) {
    if (!is_nostr(c0)) return rt_dispatch_random_plain(c0, frame, seed, stream, first_index);
    FakeCtx *c = fc(c0);
    if (first_index > UINT64_MAX - (c->batch - 1)) return c->fail(VGEN_E_RANGE, "vgen_dispatch_random: index range wraps 2^64");
    if (int rc = check_frame(c, frame)) return rc;
    return start_dispatch(c, frame, (uint64_t)c->batch * images_of(c), [c, seed, stream, first_index](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < c->batch; i++) {
            Scalar k;
            const uint64_t idx = first_index + i;
            rnd_scalar(seed, stream, (uint32_t)idx, (uint32_t)(idx >> 32), k.w);
            emit_xonly(c, ff, dump, i, k);
        }
    }, c->endo);
}

}  // namespace vg
