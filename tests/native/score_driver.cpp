// score_driver.cpp — score searches through the scan loops (scanner.cpp) and cabi.cpp over the CPU stand-in of the runtime (score_rt.cpp),
// built with AddressSanitizer + UBSan.  Every scan is held against a walk of the same counters / keys with vgen_create2_address /
// vgen_derive and vgen_score: a threshold scan equals the walk, VGEN_SCAN_BEST equals the walk's running maximum (strictly rising
// scores) over one context and over several, `count` cuts both, and the refusals hold.  tests/test_score_scan_host.py runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "vgen_hip.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)

static const uint32_t BATCH = 8192;
static uint8_t dep[20], ich[32], pre[24];

static vgen_ctx *mk(uint32_t fmt, uint32_t frames = 3, uint32_t cap = 4096) {
    vgen_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.batch_size = BATCH;
    p.format = fmt;
    p.frames = frames;
    p.match_cap = cap;
    vgen_ctx *c = nullptr;
    const int rc = vgen_create(&p, &c);
    if (rc) {
        printf("create %d %s\n", rc, vgen_last_error(nullptr));
        exit(2);
    }
    return c;
}

struct Hit {
    uint64_t at;      // counter, or offset from the first key
    uint32_t score;
};

// the walk: every candidate `first + i`, i < n, that the specification accepts, with its score
static std::vector<Hit> walk(uint32_t fmt, const char *spec, uint64_t first, uint64_t n) {
    vgen_filter *f = nullptr;
    if (vgen_filter_compile(spec, 0, fmt, &f)) exit(3);
    std::vector<Hit> out;
    for (uint64_t i = 0; i < n; i++) {
        char s[128];
        if (fmt == 7) {
            uint8_t salt[32], a[20];
            vgen_create2_salt(pre, first + i, salt);
            vgen_create2_address(dep, salt, ich, a);
            vgen_address_from_payload(7, a, s, sizeof s);
        } else {
            uint8_t k[32] = {0};
            const uint64_t v = first + i;
            for (int b = 0; b < 8; b++) k[24 + b] = (uint8_t)(v >> (8 * (7 - b)));
            k[0] = 0x10;   // keys 0x1000..00 + v
            if (vgen_derive(fmt, k, s, sizeof s, nullptr, 0)) exit(4);
        }
        uint32_t sc = 0;
        if (vgen_filter_matches(f, s) == 1) {
            CHECK(vgen_score(f, s, &sc) == 0);
            out.push_back({first + i, sc});
        }
    }
    vgen_filter_free(f);
    return out;
}

static std::vector<Hit> running_max(const std::vector<Hit> &w) {
    std::vector<Hit> out;
    for (const Hit &h : w)
        if (out.empty() || h.score > out.back().score) out.push_back(h);
    return out;
}

static uint64_t tail64(const uint8_t key[32]) {
    uint64_t c = 0;
    for (int b = 0; b < 8; b++) c = c << 8 | key[24 + b];
    return c;
}

static void compare(const char *what, const vgen_scan_result &res, std::vector<Hit> want, uint64_t count) {
    if (want.size() > count) want.resize(count);
    printf("%-60s %llu results, %llu ops\n", what, (unsigned long long)res.n_matches, (unsigned long long)res.operations);
    if (res.n_matches != want.size()) {
        printf("FAIL %s: %llu results, want %zu\n", what, (unsigned long long)res.n_matches, want.size());
        fails++;
        return;
    }
    for (size_t i = 0; i < want.size(); i++)
        if (tail64(res.matches[i].key) != want[i].at) {
            printf("FAIL %s: result %zu is %llu, want %llu\n", what, i, (unsigned long long)tail64(res.matches[i].key), (unsigned long long)want[i].at);
            fails++;
            return;
        }
}

// What a count cut over SEVERAL contexts promises without a ledger: the shards take matches against a shared counter as their batches
// finish, so which `count` of the walk's hits are kept depends on which context finishes first; the result is then sorted by key.
// -> exactly `count` results, each one a hit of the walk, in ascending key order.  (VGEN_SCAN_BEST goes through the ledger in global
// batch order and is held to the exact sequence, like every scan on one context.)
static void compare_any_of(const char *what, const vgen_scan_result &res, const std::vector<Hit> &walked, uint64_t count) {
    printf("%-60s %llu results, %llu ops\n", what, (unsigned long long)res.n_matches, (unsigned long long)res.operations);
    CHECK(walked.size() >= count && res.n_matches == count);
    size_t w = 0;
    for (uint64_t i = 0; i < res.n_matches; i++) {
        const uint64_t at = tail64(res.matches[i].key);
        while (w < walked.size() && walked[w].at < at) w++;   // (ascending on both sides: one pass)
        if (w == walked.size() || walked[w].at != at) {
            printf("FAIL %s: result %llu (%llu) is no hit of the walk, or out of order\n", what, (unsigned long long)i, (unsigned long long)at);
            fails++;
            return;
        }
        w++;
    }
}

static vgen_scan_config config(uint32_t fmt, uint64_t count, uint64_t maxb, uint32_t flags) {
    vgen_scan_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.format = fmt;
    c.count = count;
    c.max_batches = maxb;
    c.flags = flags;
    return c;
}

int main() {
    for (int i = 0; i < 20; i++) dep[i] = 1 + i;
    for (int i = 0; i < 32; i++) ich[i] = 0x20 + i;
    for (int i = 0; i < 24; i++) pre[i] = 0x80 + i;

    // ---- CREATE2: threshold scans and VGEN_SCAN_BEST over 1, 2 and 3 contexts ----
    struct C2 { const char *spec; uint64_t first; uint64_t batches; uint32_t nctx; uint64_t count; uint32_t flags; uint32_t cap; };
    const C2 c2[] = {
        {"score:zero-bytes>=2", 0, 3, 1, UINT64_MAX, 0, 4096},
        {"score:zero-bytes>=1", 77, 4, 2, UINT64_MAX, 0, 256},          // (rings overflow: the context starts the batch again with larger ones)
        {"score:leading:0>=1&count:0>=4", 5, 3, 3, UINT64_MAX, 0, 4096},
        {"score:count:0>=3", 0, 4, 1, 7, 0, 4096},                       // a count cut
        {"score:count:0>=1", 0, 4, 1, UINT64_MAX, VGEN_SCAN_BEST, 4096},
        {"score:count:0>=1", 0, 6, 2, UINT64_MAX, VGEN_SCAN_BEST, 4096},
        {"score:count:0>=1", 0, 6, 3, UINT64_MAX, VGEN_SCAN_BEST, 256},
        {"score:zero-bytes>=1&count:f>=2", 1000, 4, 2, UINT64_MAX, VGEN_SCAN_BEST, 4096},
        {"score:count:a>=2", 0, 4, 2, 3, VGEN_SCAN_BEST, 4096},          // a count cut: the first three improvements
        {"score:leading:0>=1", 0, 3, 1, UINT64_MAX, VGEN_SCAN_BEST, 4096},
    };
    for (const C2 &cs : c2) {
        std::vector<vgen_ctx *> ctxs;
        for (uint32_t i = 0; i < cs.nctx; i++) ctxs.push_back(mk(7, 3, cs.cap));
        // max_batches is per context: batches that are a multiple of the contexts, so that the scan covers exactly `batches` of them
        const uint64_t per_ctx = (cs.batches + cs.nctx - 1) / cs.nctx, covered = per_ctx * cs.nctx;
        vgen_scan_config cfg = config(7, cs.count, per_ctx, cs.flags);
        vgen_scan_result res;
        const int rc = vgen_scan_create2(ctxs.data(), cs.nctx, cs.spec, dep, ich, pre, cs.first, &cfg, nullptr, nullptr, nullptr, &res);
        if (rc) printf("rc %d %s\n", rc, vgen_last_error(ctxs[0]));
        CHECK(rc == 0);
        std::vector<Hit> w = walk(7, cs.spec, cs.first, covered * BATCH);
        CHECK(!w.empty() && w.size() < covered * BATCH);   // the reference has hits and misses
        if (cs.flags & VGEN_SCAN_BEST) w = running_max(w);
        const std::string what = std::string("create2 ") + cs.spec + (cs.flags ? " best" : "") + " ctx " + std::to_string(cs.nctx);
        compare(what.c_str(), res, w, cs.count);
        if (cs.count == UINT64_MAX) CHECK(res.operations == covered * BATCH);
        if (cs.flags & VGEN_SCAN_BEST)
            for (uint64_t i = 1; i < res.n_matches; i++) CHECK(tail64(res.matches[i].key) > tail64(res.matches[i - 1].key));
        vgen_scan_result_free(&res);
        for (auto *c : ctxs) vgen_destroy(c);
    }

    // ---- key walks (format 5; the stand-in has no contract format): vgen_scan and vgen_scan_multi from a start key ----
    struct KS { uint32_t fmt; const char *spec; uint64_t first; uint64_t batches; uint32_t nctx; uint64_t count; uint32_t flags; };
    const KS ks[] = {
        {5, "score:zero-bytes>=1", 1, 1, 1, UINT64_MAX, 0},
        {5, "score:count:0>=4", 1, 2, 2, 9, 0},                          // several contexts, a count cut: any nine hits of the walk, ascending
        {5, "score:count:0>=4", 1, 2, 1, 9, 0},                          // one context: the first nine
        {5, "score:count:0>=1", 1, 2, 1, UINT64_MAX, VGEN_SCAN_BEST},
        {5, "score:count:f>=1", 1, 2, 2, UINT64_MAX, VGEN_SCAN_BEST},
        {5, "score:zero-bytes>=0&count:0>=1", 9, 3, 3, 2, VGEN_SCAN_BEST},
    };
    for (const KS &cs : ks) {
        std::vector<vgen_ctx *> ctxs;
        for (uint32_t i = 0; i < cs.nctx; i++) ctxs.push_back(mk(cs.fmt));
        const uint64_t per_ctx = (cs.batches + cs.nctx - 1) / cs.nctx, covered = per_ctx * cs.nctx;
        vgen_scan_config cfg = config(cs.fmt, cs.count, per_ctx, cs.flags);
        cfg.has_start = 1;
        cfg.start[0] = 0x10;
        for (int b = 0; b < 8; b++) cfg.start[24 + b] = (uint8_t)(cs.first >> (8 * (7 - b)));
        vgen_scan_result res;
        const int rc = cs.nctx == 1 ? vgen_scan(ctxs[0], cs.spec, &cfg, nullptr, nullptr, nullptr, &res)
                                    : vgen_scan_multi(ctxs.data(), cs.nctx, cs.spec, &cfg, nullptr, nullptr, nullptr, &res);
        if (rc) printf("rc %d %s\n", rc, vgen_last_error(ctxs[0]));
        CHECK(rc == 0);
        std::vector<Hit> w = walk(cs.fmt, cs.spec, cs.first, covered * BATCH);
        CHECK(!w.empty() && w.size() < covered * BATCH);
        if (cs.flags & VGEN_SCAN_BEST) w = running_max(w);
        const std::string what = std::string("format ") + std::to_string(cs.fmt) + " " + cs.spec + (cs.flags ? " best" : "") + " ctx " + std::to_string(cs.nctx);
        if (cs.nctx > 1 && !(cs.flags & VGEN_SCAN_BEST) && cs.count != UINT64_MAX) compare_any_of(what.c_str(), res, w, cs.count);
        else compare(what.c_str(), res, w, cs.count);
        vgen_scan_result_free(&res);
        for (auto *c : ctxs) vgen_destroy(c);
    }

    // ---- vgen_set_score_min: later dispatches only; vgen_set_filter resets it; the refusals ----
    {
        vgen_ctx *c = mk(7);
        vgen_filter *f = nullptr, *plain = nullptr;
        CHECK(vgen_filter_compile("score:count:0>=4&zero-bytes>=0", 0, 7, &f) == 0);
        CHECK(vgen_filter_compile("^0x00", 0, 7, &plain) == 0);
        CHECK(vgen_set_score_min(c, 5) == VGEN_E_STATE);           // dump mode
        CHECK(vgen_set_filter(c, plain) == 0 && vgen_set_score_min(c, 5) == VGEN_E_STATE);
        CHECK(vgen_set_create2(c, dep, ich, pre) == 0 && vgen_set_filter(c, f) == 0);
        CHECK(vgen_set_score_min(c, 41) == VGEN_E_PATTERN && vgen_set_score_min(c, 40) == 0 && vgen_set_score_min(c, 4) == 0);
        std::vector<vgen_match> r0(BATCH), r1(BATCH), r2(BATCH);
        uint32_t n0 = 0, n1 = 0, n2 = 0;
        CHECK(vgen_dispatch_create2(c, 0, 0) == 0);
        CHECK(vgen_set_score_min(c, 6) == 0);                      // while frame 0 is in flight
        CHECK(vgen_dispatch_create2(c, 1, 0) == 0);
        CHECK(vgen_wait(c, 0, r0.data(), BATCH, &n0, nullptr) == 0 && vgen_wait(c, 1, r1.data(), BATCH, &n1, nullptr) == 0);
        CHECK(vgen_set_filter(c, f) == 0 && vgen_dispatch_create2(c, 2, 0) == 0 && vgen_wait(c, 2, r2.data(), BATCH, &n2, nullptr) == 0);
        const std::vector<Hit> w4 = walk(7, "score:count:0>=4", 0, BATCH), w6 = walk(7, "score:count:0>=6", 0, BATCH);
        CHECK(n0 == w4.size() && n1 == w6.size() && n2 == w4.size() && w6.size() < w4.size() && !w6.empty());
        for (uint32_t i = 0; i < n1 && i < w6.size(); i++) CHECK(r1[i].index == w6[i].at);
        for (uint32_t i = 0; i < n0 && i < w4.size(); i++) CHECK(r0[i].index == w4[i].at && r2[i].index == w4[i].at);
        // VGEN_SCAN_BEST: score specifications only, and not with a checkpoint
        vgen_scan_result res;
        vgen_scan_config cfg = config(7, 1, 1, VGEN_SCAN_BEST);
        CHECK(vgen_scan_create2(&c, 1, "^0x00", dep, ich, pre, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
        cfg.checkpoint_path = "/tmp/score_driver_never_written.ckpt";
        CHECK(vgen_scan_create2(&c, 1, "score:count:0>=1", dep, ich, pre, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        CHECK(strstr(vgen_last_error(c), "checkpoint") != nullptr);
        cfg.checkpoint_path = nullptr;
        cfg.flags = VGEN_SCAN_BEST | VGEN_SCAN_RANDOM_KEYS;
        CHECK(vgen_scan_create2(&c, 1, "score:count:0>=1", dep, ich, pre, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        vgen_filter_free(f);
        vgen_filter_free(plain);
        vgen_destroy(c);

        vgen_ctx *k = mk(5);
        vgen_scan_config kc = config(5, 1, 1, VGEN_SCAN_BEST);
        kc.seed = 3;
        CHECK(vgen_scan(k, "^0x00", &kc, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
        CHECK(vgen_scan_multi(&k, 1, "^0x00", &kc, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
        kc.checkpoint_path = "/tmp/score_driver_never_written.ckpt";
        CHECK(vgen_scan(k, "score:count:0>=1", &kc, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED && strstr(vgen_last_error(k), "checkpoint") != nullptr);
        CHECK(vgen_scan_multi(&k, 1, "score:count:0>=1", &kc, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        vgen_destroy(k);
        // a score specification on a format without hex digits: unsupported, from the scans as from vgen_filter_compile
        vgen_ctx *b = mk(0);
        vgen_scan_config bc = config(0, 1, 1, 0);
        bc.seed = 3;
        vgen_filter *nf = nullptr;
        CHECK(vgen_filter_compile("score:zero-bytes>=1", 0, 0, &nf) == VGEN_E_UNSUPPORTED);
        CHECK(vgen_scan(b, "score:zero-bytes>=1", &bc, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        CHECK(vgen_scan_multi(&b, 1, "score:zero-bytes>=1", &bc, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        CHECK(vgen_scan(b, "score:bogus", &bc, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
        vgen_destroy(b);
    }
    printf(fails ? "FAILED %d\n" : "all ok\n", fails);
    return fails != 0;
}
