// onion_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime (fake_rt.cpp, included as it is) with contexts of the onion format
// (VGF_ONION) added, so that the host scan loop (scanner.cpp) and cabi.cpp run over the format without a device.  A dispatch is computed
// the way the kernels compute it - the host build of core/ed_walk.h: S shared points, one table point per lane, every key one of the
// pair U_j +- R_u at the slot device_types.h gives it - and judged by the single-source core/filter_eval.h filter_eval_onion.  An onion
// context is the stand-in's own eight-word context with the format put back; its dispatches go through the stand-in's start_dispatch /
// rt_wait like every other.  Built by tests/native/onion.mk into libvgen_fake_onion.so and driven through the C ABI by
// tests/test_onion_scan_host.py; never loaded by vgen_amd.
#define rt_create rt_create_keys
#include "fake_rt.cpp"
#undef rt_create

#include "../../vgen_amd/csrc/core/ed_walk.h"
#include "../../vgen_amd/csrc/host/onion_host.h"

namespace vg {

namespace {

// (start + i step) B as an affine point with its third field: t = x y, or d x y when mul_d
void host_point(edw_pt &p, const u32 start[8], uint64_t add, bool mul_d) {
    u32 k[8];
    (void)edw_add_u64(k, start, add);
    ed_pt e;
    ed_mul_base(e, ed_host_table(), k);
    fe25 zi;
    fe25_inv(zi, e.Z);
    fe25_mul(p.x, e.X, zi);
    fe25_mul(p.y, e.Y, zi);
    fe25_mul(p.t, p.x, p.y);
    if (mul_d) {
        fe25 d;
        edw_d(d);
        fe25_mul(p.t, p.t, d);
    }
}

void emit_payload(FakeCtx *c, FakeFrame &ff, bool dump, uint32_t slot, u32 pl[8], bool no_key) {
    if (dump) {
        if (no_key) memset(pl, 0, 32);
        memcpy(ff.dump.data() + (size_t)slot * 32, pl, 32);
    } else if (!no_key && filter_eval_onion(&c->h_filter, pl)) {
        DevMatch m;
        m.index = slot;
        m.reserved = 0;
        memcpy(m.payload, pl, 32);
        ff.found.push_back(m);
    }
}

void walk_onion(FakeCtx *c, FakeFrame &ff, bool dump, const u32 first_scalar[8]) {
    const uint32_t S = ONION_S, L = c->batch / (2 * S);
    bool zero = true;
    for (int i = 0; i < 8; i++) zero = zero && first_scalar[i] == 0;
    std::vector<edw_pt> uni(S);
    for (uint32_t j = 0; j < S; j++) host_point(uni[j], first_scalar, 8ull * ((uint64_t)L * S - S / 2 + j), true);
    const u32 none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t u = 0; u < L; u++) {
        edw_pt q;
        host_point(q, none, 8ull * ((uint64_t)u * S + S / 2), false);
        for (uint32_t j = 0; j < S; j++) {
            fe25 dm, dp, im, ip, ys, yd, xs, xd;
            edw_dens(dm, dp, uni[j].t, q.t);
            fe25_carry(dm);
            fe25_carry(dp);
            fe25_inv(im, dm);
            fe25_inv(ip, dp);
            edw_pair_y(ys, yd, uni[j], q, im, ip);
            edw_pair_x(xs, xd, uni[j], q, im, ip);
            u32 ps[8], pd[8];
            edw_encode_y(ps, ys);
            edw_encode_y(pd, yd);
            ps[7] |= edw_sign(xs) << 31;
            pd[7] |= edw_sign(xd) << 31;
            const uint32_t sp = (L + u) * S + j, sm = (L - 1 - u) * S + j;
            emit_payload(c, ff, dump, sp, ps, zero && sp == 0);
            emit_payload(c, ff, dump, sm, pd, zero && sm == 0);
        }
    }
}

int fake_dispatch_onion(vgen_ctx *c0, uint32_t frame, const uint8_t base_le[32], uint64_t first) {
    FakeCtx *c = fc(c0);
    if (frame >= c->frames || !base_le) return c->fail(VGEN_E_INVALID, "bad frame index / base scalar");
    if (c->fr[frame].in_flight) return c->fail(VGEN_E_STATE, "frame already has a dispatch in flight");
    if (base_le[0] & 7) return c->fail(VGEN_E_INVALID, "vgen_dispatch_onion: the base scalar must be a multiple of 8");
    uint8_t lo[32], hi[32];
    if (first > UINT64_MAX - (c->batch - 1) || !onion_scalar_at(base_le, first, lo) || !onion_scalar_at(base_le, first + (c->batch - 1), hi))
        return c->fail(VGEN_E_RANGE, "vgen_dispatch_onion: base + 8 (first_index + batch_size - 1) reaches 2^255");
    if (int rc = ensure_frame(c, frame)) return rc;
    std::vector<u32> s(8);
    onion_words_le(lo, s.data());
    return start_dispatch(c, frame, c->batch, [c, s](FakeFrame &ff, bool dump) { walk_onion(c, ff, dump, s.data()); });
}

}  // namespace

int rt_create(const vgen_params *p_in, vgen_ctx **out, std::string &err) {
    if (!p_in || p_in->struct_size != sizeof(vgen_params) || p_in->format != VGF_ONION) return rt_create_keys(p_in, out, err);
    if (p_in->flags & VGEN_FLAG_ENDO) {
        err = "VGEN_FLAG_ENDO: the endomorphism images belong to secp256k1; an onion search has none";
        return VGEN_E_UNSUPPORTED;
    }
    vgen_params p = *p_in;
    p.format = VGF_P2TR;   // the same payload size
    if (int rc = rt_create_keys(&p, out, err)) return rc;
    (*out)->format = VGF_ONION;
    (*out)->base_set = nullptr;
    (*out)->onion_dispatch = fake_dispatch_onion;
    return VGEN_OK;
}

}  // namespace vg
