// score_rt.cpp — TEST-ONLY: the CPU stand-in of the runtime with CREATE2 contexts (create2_rt.cpp, which includes fake_rt.cpp; both as they
// are) with score filters added, so that the score path of the scan loops (scanner.cpp: VGEN_SCAN_BEST, vgen_set_score_min behind every
// improvement) and of cabi.cpp runs under AddressSanitizer + UBSan without a device.
// The stand-in's own candidate test knows nothing of device kind 6, so a score filter is installed in it as "every key is a candidate"
// and the dispatch's candidates are scored here, with the single-source core/score_eval.h the kernels compile, when the dispatch is
// waited for — against the terms as they stood when the dispatch was ENQUEUED, as on the device, where they travel in the kernel
// arguments: a vgen_set_score_min while dispatches are in flight changes later dispatches only.
// Built and run by tests/test_score_scan_host.py; never loaded by vgen_amd.
#define rt_set_filter rt_set_filter_plain
#define rt_dispatch rt_dispatch_plain
#define rt_dispatch_keys rt_dispatch_keys_plain
#define rt_dispatch_random rt_dispatch_random_plain
#define rt_wait rt_wait_plain
#include "create2_rt.cpp"
#undef rt_set_filter
#undef rt_dispatch
#undef rt_dispatch_keys
#undef rt_dispatch_random
#undef rt_wait

#include <map>

#include "../../vgen_amd/csrc/core/score_eval.h"

namespace vg {

namespace {

struct ScoreState {
    bool on = false;                          // a score filter is installed
    int (*c2_plain)(vgen_ctx *, uint32_t, uint64_t) = nullptr;
    std::map<uint32_t, ScoreTerms> sent;      // frame -> the terms its dispatch in flight was enqueued with
};
std::mutex g_mu;
std::map<const vgen_ctx *, ScoreState> g_state;   // (contexts of the driver; entries of destroyed ones are overwritten by rt_set_filter)

ScoreState &state(const vgen_ctx *c) {
    std::lock_guard<std::mutex> g(g_mu);
    return g_state[c];
}

void note_dispatch(vgen_ctx *c, uint32_t frame) {
    ScoreState &s = state(c);
    if (s.on) s.sent[frame] = c->score;
}

int c2_scored(vgen_ctx *c, uint32_t frame, uint64_t first_counter) {
    ScoreState &s = state(c);
    const int rc = s.c2_plain(c, frame, first_counter);
    if (rc == VGEN_OK) note_dispatch(c, frame);
    return rc;
}

}  // namespace

int rt_set_filter(vgen_ctx *c, const vgen_filter *f) {
    ScoreState &s = state(c);
    if (c->create2_dispatch && c->create2_dispatch != c2_scored) {   // a CREATE2 context: its dispatch notes the terms too
        s.c2_plain = c->create2_dispatch;
        c->create2_dispatch = c2_scored;
    }
    if (!f || f->dev.kind != DEVF_SCORE) {
        const int rc = rt_set_filter_plain(c, f);
        if (rc == VGEN_OK) s.on = false;
        return rc;
    }
    vgen_filter all = *f;          // what the stand-in evaluates: match-all
    all.dev.kind = DEVF_ALL;
    const int rc = rt_set_filter_plain(c, &all);
    if (rc != VGEN_OK) return rc;
    s.on = true;   // (the context's terms, c->score, are installed by vgen_set_filter in cabi.cpp behind this call)
    s.sent.clear();
    return VGEN_OK;
}

int rt_dispatch(vgen_ctx *c, uint32_t frame, const uint8_t start_key_be[32]) {
    const int rc = rt_dispatch_plain(c, frame, start_key_be);
    if (rc == VGEN_OK) note_dispatch(c, frame);
    return rc;
}

int rt_dispatch_keys(vgen_ctx *c, uint32_t frame, const uint8_t *keys_be, uint32_t n) {
    const int rc = rt_dispatch_keys_plain(c, frame, keys_be, n);
    if (rc == VGEN_OK) note_dispatch(c, frame);
    return rc;
}

int rt_dispatch_random(vgen_ctx *c, uint32_t frame, const RndSeed &seed, uint32_t stream, uint64_t first_index) {
    const int rc = rt_dispatch_random_plain(c, frame, seed, stream, first_index);
    if (rc == VGEN_OK) note_dispatch(c, frame);
    return rc;
}

int rt_wait(vgen_ctx *c0, uint32_t frame, vgen_match *out, uint32_t cap, uint32_t *n_matches, uint64_t *keys_tested) {
    ScoreState &s = state(c0);
    if (s.on && frame < c0->frames && c0->fr[frame].in_flight && !c0->fr[frame].dumped) {
        FakeCtx *c = fc(c0);
        FakeFrame &ff = c->ff[frame];
        if (ff.worker.joinable()) ff.worker.join();
        const ScoreTerms terms = s.sent[frame];
        std::vector<DevMatch> kept;
        for (const DevMatch &m : ff.found)
            if (score_eval(terms, m.payload, nullptr)) kept.push_back(m);
        ff.found.swap(kept);
    }
    return rt_wait_plain(c0, frame, out, cap, n_matches, keys_tested);
}

}  // namespace vg
