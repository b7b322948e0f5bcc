// splitkey_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime (fake_rt.cpp, included as it is) with split-key dispatches added, so
// that the host side of a split-key scan - vgen_set_base_point, the scan loop's partial keys, its re-derivation of every candidate
// from P + k*G and its refusals (scanner.cpp, cabi.cpp, host/scan_match.h) - runs without a device.  A context gets the base_set
// hook the real runtime installs; while a base is set, its dispatches are computed here: one multiplication and one complete
// addition per key through host/encode.h point_add_gen, the images (beta^e x, +-y) of the POINT at variant * batch + i, the
// payloads by payload_from_point.  Without a base every dispatch is the stand-in's own.
// splitkey_rt_corrupt(m, r) makes the stand-in LIE: the payload of every key k with k mod m == r gets its last byte flipped after
// the candidate test, as a device whose batched additions met an exceptional pair would garble it - the address still satisfies a
// prefix pattern, so only the host's re-derivation can tell.  Built by tests/native/splitkey.mk into libvgen_fake_split.so and
// driven through the C ABI by tests/test_splitkey_scan_host.py; never loaded by vgen_amd.
#define rt_create rt_create_plain
#define rt_dispatch rt_dispatch_plain
#define rt_dispatch_keys rt_dispatch_keys_plain
#define rt_dispatch_random rt_dispatch_random_plain
#include "fake_rt.cpp"
#undef rt_create
#undef rt_dispatch
#undef rt_dispatch_keys
#undef rt_dispatch_random

#include <atomic>

namespace vg {

namespace {

std::atomic<uint32_t> g_corrupt_mod{0}, g_corrupt_res{0};

int base_set(vgen_ctx *c, const ge *pt) {
    c->have_base = pt != nullptr;
    if (pt) c->base_pt = *pt;
    return VGEN_OK;
}

// key i of a dispatch under the base: the images of P + k*G, or no slot when k is no key or the sum is the point at infinity
void emit_split(FakeCtx *c, FakeFrame &ff, bool dump, const ge &base, uint32_t i, const Scalar &k) {
    ge pt;
    if (!scalar_is_valid(k) || !point_add_gen(base, k, pt)) return;
    const uint32_t images = c->endo ? vgf_endo_images((int)c->format) : 1u;
    const uint32_t m = g_corrupt_mod.load();
    const bool lie = m && k.w[0] % m == g_corrupt_res.load();
    const size_t pb = (size_t)c->payload_words * 4;
    for (uint32_t v = 0; v < images; v++) {
        ge img;
        point_image(img, pt, v);
        uint8_t out[32] = {0};
        if (!payload_from_point(c->format, img, out)) continue;
        u32 pl[8] = {0};
        memcpy(pl, out, pb);
        const uint32_t slot = v * c->batch + i;
        const bool cand = dump || candidate(c, pl);
        if (lie) reinterpret_cast<uint8_t *>(pl)[pb - 1] ^= 0x5a;
        if (dump) {
            memcpy(ff.dump.data() + (size_t)slot * pb, pl, pb);
        } else if (cand) {
            DevMatch rec;
            rec.index = slot;
            rec.reserved = 0;
            memset(rec.payload, 0, sizeof rec.payload);
            memcpy(rec.payload, pl, pb);
            ff.found.push_back(rec);
        }
    }
}

int check_frame(FakeCtx *c, uint32_t frame) {
    if (frame >= c->frames) return c->fail(VGEN_E_INVALID, "bad frame index");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    return ensure_frame(c, frame);
}

uint64_t keys_of(const FakeCtx *c, uint32_t n) { return (uint64_t)n * (c->endo ? vgf_endo_images((int)c->format) : 1u); }

}  // namespace

int rt_create(const vgen_params *p, vgen_ctx **out, std::string &err) {
    if (int rc = rt_create_plain(p, out, err)) return rc;
    (*out)->base_set = base_set;
    return VGEN_OK;
}

int rt_dispatch(vgen_ctx *c0, uint32_t frame, const uint8_t start_key_be[32]) {
    if (!c0->have_base) return rt_dispatch_plain(c0, frame, start_key_be);
    FakeCtx *c = fc(c0);
    if (!start_key_be) return c->fail(VGEN_E_INVALID, "bad frame index / key");
    Scalar k0;
    scalar_from_be(k0, start_key_be);
    if (!scalar_is_valid(k0)) return c->fail(VGEN_E_RANGE, "start key is not a valid secp256k1 scalar");
    if (int rc = check_frame(c, frame)) return rc;
    c->fr[frame].start = k0;
    const ge base = c->base_pt;
    return start_dispatch(c, frame, keys_of(c, c->batch), [c, k0, base](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < c->batch; i++) {
            Scalar k;
            if (scalar_add_u64(k, k0, i)) memset(&k, 0, sizeof k);
            emit_split(c, ff, dump, base, i, k);
        }
    }, c->endo);
}

int rt_dispatch_keys(vgen_ctx *c0, uint32_t frame, const uint8_t *keys_be, uint32_t n) {
    if (!c0->have_base) return rt_dispatch_keys_plain(c0, frame, keys_be, n);
    FakeCtx *c = fc(c0);
    if (!keys_be || n == 0 || n > c->batch) return c->fail(VGEN_E_INVALID, "vgen_dispatch_keys: bad key buffer / n");
    if (int rc = check_frame(c, frame)) return rc;
    std::vector<uint8_t> keys(keys_be, keys_be + (size_t)n * 32);
    const ge base = c->base_pt;
    return start_dispatch(c, frame, keys_of(c, n), [c, keys, n, base](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < n; i++) {
            Scalar k;
            scalar_from_be(k, keys.data() + (size_t)i * 32);
            emit_split(c, ff, dump, base, i, k);
        }
    }, c->endo);
}

int rt_dispatch_random(vgen_ctx *c0, uint32_t frame, const RndSeed &seed, uint32_t stream, uint64_t first_index) {
    if (!c0->have_base) return rt_dispatch_random_plain(c0, frame, seed, stream, first_index);
    FakeCtx *c = fc(c0);
    if (first_index > UINT64_MAX - (c->batch - 1)) return c->fail(VGEN_E_RANGE, "vgen_dispatch_random: index range wraps 2^64");
    if (int rc = check_frame(c, frame)) return rc;
    const ge base = c->base_pt;
    return start_dispatch(c, frame, keys_of(c, c->batch), [c, seed, stream, first_index, base](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < c->batch; i++) {
            Scalar k;
            const uint64_t idx = first_index + i;
            rnd_scalar(seed, stream, (uint32_t)idx, (uint32_t)(idx >> 32), k.w);
            emit_split(c, ff, dump, base, i, k);
        }
    }, c->endo);
}

}  // namespace vg

extern "C" void splitkey_rt_corrupt(uint32_t modulus, uint32_t residue) {
    vg::g_corrupt_res.store(residue);
    vg::g_corrupt_mod.store(modulus);
}
