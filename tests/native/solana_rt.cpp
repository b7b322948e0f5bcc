// solana_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime (fake_rt.cpp, included as it is) with contexts of the Solana format
// (VGF_SOLANA) added, so that the host scan loop (scanner.cpp) and cabi.cpp run over the format without a device: the Ed25519 public
// key of every seed as the 32-byte payload (the host build of core/ed25519.h, one multiplication and one inversion per seed) and the
// format's own candidate test, the single-source core/filter_eval.h filter_eval_sol the kernel runs.  A Solana context is the
// stand-in's own eight-word context with the format put back; its dispatches are computed here and go through the stand-in's
// start_dispatch / rt_wait like every other.  Built by tests/native/solana.mk into libvgen_fake_solana.so and driven through the C ABI
// by tests/test_solana.py and tests/test_solana_scan_host.py; never loaded by vgen_amd.
#define rt_create rt_create_keys
#define rt_dispatch rt_dispatch_keys_walk
#define rt_dispatch_keys rt_dispatch_keys_plain
#define rt_dispatch_random rt_dispatch_random_plain
#include "fake_rt.cpp"
#undef rt_create
#undef rt_dispatch
#undef rt_dispatch_keys
#undef rt_dispatch_random

#include "../../vgen_amd/csrc/host/ed_host.h"

namespace vg {

namespace {

bool is_solana(const vgen_ctx *c) { return c->format == VGF_SOLANA; }

// A device test may report MORE than the filter asks for (the host confirms every candidate): with `loosen` = k > 0 the stand-in also
// reports every k-th slot.  The filter compiler's selectivity estimates are exact for this format, so a scan sizes its ring right
// up front and never overflows it by itself; this is how the tests reach the scan loop's ring-overflow restart (vgen_fake_solana_loosen).
uint32_t loosen = 0;

void emit_seed(FakeCtx *c, FakeFrame &ff, bool dump, uint32_t i, const uint8_t seed[32]) {
    u32 pl[8];
    ed_public_key(seed, reinterpret_cast<uint8_t *>(pl));
    if (dump) {
        memcpy(ff.dump.data() + (size_t)i * 32, pl, 32);
    } else if (filter_eval_sol(&c->h_filter, pl) || (loosen && i % loosen == 0)) {
        DevMatch m;
        m.index = i;
        m.reserved = 0;
        memcpy(m.payload, pl, 32);
        ff.found.push_back(m);
    }
}

int check_frame(FakeCtx *c, uint32_t frame) {
    if (frame >= c->frames) return c->fail(VGEN_E_INVALID, "bad frame index");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    return ensure_frame(c, frame);
}

}  // namespace

int rt_create(const vgen_params *p_in, vgen_ctx **out, std::string &err) {
    if (!p_in || p_in->struct_size != sizeof(vgen_params) || p_in->format != VGF_SOLANA) return rt_create_keys(p_in, out, err);
    if (p_in->flags & VGEN_FLAG_ENDO) {
        err = "VGEN_FLAG_ENDO: the endomorphism images belong to secp256k1; a solana search has none";
        return VGEN_E_UNSUPPORTED;
    }
    vgen_params p = *p_in;
    p.format = VGF_P2TR;   // the same payload size
    if (int rc = rt_create_keys(&p, out, err)) return rc;
    (*out)->format = VGF_SOLANA;
    (*out)->base_set = nullptr;
    return VGEN_OK;
}

int rt_dispatch(vgen_ctx *c0, uint32_t frame, const uint8_t start_key_be[32]) {
    if (!is_solana(c0)) return rt_dispatch_keys_walk(c0, frame, start_key_be);
    return c0->fail(VGEN_E_UNSUPPORTED, "vgen_dispatch: a solana key is a seed and its scalar a hash of it - there is no walk; use vgen_dispatch_random / vgen_dispatch_keys");
}

int rt_dispatch_keys(vgen_ctx *c0, uint32_t frame, const uint8_t *keys_be, uint32_t n) {
    if (!is_solana(c0)) return rt_dispatch_keys_plain(c0, frame, keys_be, n);
    FakeCtx *c = fc(c0);
    if (!keys_be || n == 0 || n > c->batch) return c->fail(VGEN_E_INVALID, "vgen_dispatch_keys: bad key buffer / n");
    if (int rc = check_frame(c, frame)) return rc;
    std::vector<uint8_t> seeds(keys_be, keys_be + (size_t)n * 32);
    return start_dispatch(c, frame, n, [c, seeds, n](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < n; i++) emit_seed(c, ff, dump, i, seeds.data() + (size_t)i * 32);
    });
}

int rt_dispatch_random(vgen_ctx *c0, uint32_t frame, const RndSeed &seed, uint32_t stream, uint64_t first_index) {
    if (!is_solana(c0)) return rt_dispatch_random_plain(c0, frame, seed, stream, first_index);
    FakeCtx *c = fc(c0);
    if (first_index > UINT64_MAX - (c->batch - 1)) return c->fail(VGEN_E_RANGE, "vgen_dispatch_random: index range wraps 2^64");
    if (int rc = check_frame(c, frame)) return rc;
    return start_dispatch(c, frame, c->batch, [c, seed, stream, first_index](FakeFrame &ff, bool dump) {
        for (uint32_t i = 0; i < c->batch; i++) {
            const uint64_t idx = first_index + i;
            u32 d[8];
            rnd_scalar(seed, stream, (uint32_t)idx, (uint32_t)(idx >> 32), d);
            uint8_t s[32];
            for (int w = 0; w < 8; w++)
                for (int b = 0; b < 4; b++) s[4 * w + b] = (uint8_t)(d[7 - w] >> (8 * (3 - b)));
            emit_seed(c, ff, dump, i, s);
        }
    });
}

}  // namespace vg

extern "C" void vgen_fake_solana_loosen(uint32_t every) { vg::loosen = every; }
