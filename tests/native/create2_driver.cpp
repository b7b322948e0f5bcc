// create2_driver.cpp — vgen_scan_create2 (scanner.cpp) over the CPU stand-in of the runtime (create2_rt.cpp), built with AddressSanitizer + UBSan:
// every scan is held against a walk of the same counters with vgen_create2_address and the exact automaton.  Scenarios: one and several
// contexts, count cuts, max_batches, rings that overflow (the context starts the batch again with larger ones), an on-device automaton,
// host filtering from dumps (-i), the end of the 64-bit counter space, and the refusals.  tests/test_create2_scan_host.py runs it.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include <string>
#include "vgen_hip.h"
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
int main() {
    uint8_t dep[20], h[32], pre[24];
    for (int i = 0; i < 20; i++) dep[i] = 1 + i;
    for (int i = 0; i < 32; i++) h[i] = 0x20 + i;
    for (int i = 0; i < 24; i++) pre[i] = 0x80 + i;
    auto mk = [&](uint32_t cap) { vgen_params p; memset(&p, 0, sizeof p); p.struct_size = sizeof p; p.batch_size = 8192; p.format = 7; p.frames = 3; p.match_cap = cap; vgen_ctx *c = nullptr; int rc = vgen_create(&p, &c); if (rc) { printf("create %d %s\n", rc, vgen_last_error(nullptr)); exit(2); } return c; };
    auto addr0 = [&](uint64_t c) { uint8_t s[32], a[20]; vgen_create2_salt(pre, c, s); vgen_create2_address(dep, s, h, a); return std::vector<uint8_t>(a, a + 20); };
    struct Case { const char *pat; int ci; uint64_t count; uint64_t first; uint64_t maxb; uint32_t nctx; uint32_t cap; };
    Case cases[] = {{"^0x00", 0, 5, 0, 0, 1, 4096}, {"^0x00", 0, 5, 0, 0, 2, 4096}, {"^0x0", 0, UINT64_MAX, 123, 3, 1, 256}, {"^0x0", 0, UINT64_MAX, 123, 2, 3, 256},
                    {"ab", 0, 40, 0xFFFFFFFFull - 100, 0, 2, 4096}, {"^0x0A", 1, 7, 0, 0, 1, 4096}, {"^0x", 0, UINT64_MAX, UINT64_MAX - 3 * 8192 - 4, 0, 2, 4096},
                    {"[0-9]a$", 0, 9, 5, 0, 2, 4096}};
    for (auto &cs : cases) {
        std::vector<vgen_ctx *> ctxs;
        for (uint32_t i = 0; i < cs.nctx; i++) ctxs.push_back(mk(cs.cap));
        vgen_scan_config cfg; memset(&cfg, 0, sizeof cfg); cfg.struct_size = sizeof cfg; cfg.format = 7; cfg.count = cs.count; cfg.case_insensitive = cs.ci; cfg.max_batches = cs.maxb;
        vgen_scan_result res;
        int rc = vgen_scan_create2(ctxs.data(), cs.nctx, cs.pat, dep, h, pre, cs.first, &cfg, nullptr, nullptr, nullptr, &res);
        if (rc) printf("rc %d %s\n", rc, vgen_last_error(ctxs[0]));
        CHECK(rc == 0);
        vgen_filter *f = nullptr; vgen_filter_compile(cs.pat, cs.ci, 7, &f);
        // expected: walk the counters the scan covered
        std::vector<uint64_t> want;
        uint64_t nb = res.operations / 8192;
        for (uint64_t c = 0; c < nb * 8192 && want.size() < cs.count; c++) {
            auto a = addr0(cs.first + c); char s[128]; vgen_address_from_payload(7, a.data(), s, sizeof s);
            if (vgen_filter_matches(f, s) == 1) want.push_back(cs.first + c);
        }
        CHECK(res.n_matches == want.size());
        for (uint64_t i = 0; i < res.n_matches && i < want.size(); i++) {
            uint64_t c = 0; for (int b = 0; b < 8; b++) c = c << 8 | res.matches[i].key[24 + b];
            if (c != want[i]) { printf("  %s: match %llu counter %llx want %llx\n", cs.pat, (unsigned long long)i, (unsigned long long)c, (unsigned long long)want[i]); fails++; break; }
            CHECK(memcmp(res.matches[i].key, pre, 24) == 0 && res.matches[i].format == 7 && !strcmp(res.matches[i].wif, res.matches[i].hex) && !strncmp(res.matches[i].hex, "0x80", 4));
        }
        printf("%-8s ctx %u: %llu matches, %llu ops, complete %d\n", cs.pat, cs.nctx, (unsigned long long)res.n_matches, (unsigned long long)res.operations, res.complete);
        if (cs.maxb) CHECK(res.operations == cs.maxb * cs.nctx * 8192);
        vgen_scan_result_free(&res); vgen_filter_free(f);
        for (auto *c : ctxs) vgen_destroy(c);
    }
    // refusals
    vgen_ctx *c = mk(4096); vgen_scan_config cfg; memset(&cfg, 0, sizeof cfg); cfg.struct_size = sizeof cfg; cfg.format = 7; cfg.count = 1; vgen_scan_result res;
    CHECK(vgen_scan(c, "^0x00", &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    CHECK(vgen_scan_multi(&c, 1, "^0x00", &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    cfg.seed = 4; CHECK(vgen_scan_create2(&c, 1, "^0x00", dep, h, pre, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    cfg.seed = 0; cfg.checkpoint_path = "/tmp/x.ckpt"; CHECK(vgen_scan_create2(&c, 1, "^0x00", dep, h, pre, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    vgen_destroy(c);
    printf(fails ? "FAILED %d\n" : "all ok\n", fails);
    return fails != 0;
}
