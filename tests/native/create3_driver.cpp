// create3_driver.cpp — vgen_scan_create3 (scanner.cpp) over the CPU stand-in of the runtime (create3_rt.cpp), built with AddressSanitizer +
// UBSan: every scan is held against a plain walk of the same counters with vgen_create3_address and the exact automaton or the
// score.  Scenarios: no guard and guards of several lengths, regex and score patterns, VGEN_SCAN_BEST, count cuts, max_batches, one
// and two contexts, rings that overflow, the end of the counter space, the refusals, and a CREATE2 scan on contexts that a
// CREATE3 scan used before.  tests/test_create3_scan_host.py runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vgen_hip.h"

extern "C" void create3_rt_adopt(vgen_ctx *c);

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static const uint32_t BATCH = 8192;

static uint8_t fac[20], ph[32], pre[24], guard[64];

static vgen_ctx *mk(uint32_t cap) {
    vgen_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.batch_size = BATCH;
    p.format = 7;
    p.frames = 3;
    p.match_cap = cap;
    vgen_ctx *c = nullptr;
    const int rc = vgen_create(&p, &c);
    if (rc) {
        printf("create %d %s\n", rc, vgen_last_error(nullptr));
        exit(2);
    }
    create3_rt_adopt(c);
    return c;
}

static std::string addr3(int guard_len, uint64_t counter) {
    uint8_t s[32], a[20];
    char str[128];
    vgen_create2_salt(pre, counter, s);
    if (vgen_create3_address(fac, s, ph, guard, guard_len, nullptr, a) != VGEN_OK) exit(3);
    vgen_address_from_payload(7, a, str, sizeof str);
    return str;
}

static uint64_t counter_of(const vgen_generated &g) {
    uint64_t c = 0;
    for (int b = 0; b < 8; b++) c = c << 8 | g.key[24 + b];
    return c;
}

static vgen_scan_config config(uint64_t count, int ci, uint64_t maxb, uint32_t flags) {
    vgen_scan_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.format = 7;
    cfg.count = count;
    cfg.case_insensitive = ci;
    cfg.max_batches = maxb;
    cfg.flags = flags;
    return cfg;
}

int main() {
    for (int i = 0; i < 20; i++) fac[i] = (uint8_t)(1 + i);
    for (int i = 0; i < 32; i++) ph[i] = (uint8_t)(0x20 + i);
    for (int i = 0; i < 24; i++) pre[i] = (uint8_t)(0x80 + i);
    for (int i = 0; i < 64; i++) guard[i] = (uint8_t)(0xA0 + i);

    // the stand-in's dispatch is the host function, salt by salt (both built on core/hash.h, through different entry points)
    struct Case { const char *pat; int guard_len; int ci; uint64_t count; uint64_t first; uint64_t maxb; uint32_t nctx; uint32_t cap; uint32_t flags; };
    const Case cases[] = {
        {"^0x00", -1, 0, 5, 0, 0, 1, 4096, 0}, {"^0x00", -1, 0, 5, 0, 0, 2, 4096, 0}, {"^0x00", 0, 0, 5, 0, 0, 1, 4096, 0}, {"^0x00", 20, 0, 5, 0, 0, 2, 4096, 0},
        {"^0x0", 64, 0, UINT64_MAX, 123, 3, 1, 256, 0},                              // rings overflow; max_batches
        {"^0x0", 3, 0, UINT64_MAX, 123, 2, 2, 256, 0},
        {"ab", 32, 0, 40, 0xFFFFFFFFull - 100, 0, 2, 4096, 0},                       // an on-device automaton across 2^32
        {"^0x0A", 1, 1, 7, 0, 0, 1, 4096, 0},                                        // host filtering from dumps
        {"^0x", 63, 0, UINT64_MAX, UINT64_MAX - 3 * BATCH - 4, 0, 2, 4096, 0},       // the end of the counter space
        {"score:zero-bytes>=2", -1, 0, UINT64_MAX, 0, 2, 1, 4096, 0}, {"score:zero-bytes>=2", 20, 0, UINT64_MAX, 7, 1, 2, 4096, 0},
        {"score:count:0>=1", 20, 0, UINT64_MAX, 0, 2, 1, 4096, VGEN_SCAN_BEST}, {"score:count:0>=1", -1, 0, UINT64_MAX, 0, 1, 2, 4096, VGEN_SCAN_BEST},
        {"score:count:0>=1", 52, 0, 3, 0, 0, 2, 4096, VGEN_SCAN_BEST},               // --best with a count: the first three improvements
    };
    int n_cases = 0, n_complete = 0;
    for (const Case &cs : cases) {
        std::vector<vgen_ctx *> ctxs;
        for (uint32_t i = 0; i < cs.nctx; i++) ctxs.push_back(mk(cs.cap));
        vgen_scan_config cfg = config(cs.count, cs.ci, cs.maxb, cs.flags);
        vgen_scan_result res;
        const int rc = vgen_scan_create3(ctxs.data(), cs.nctx, cs.pat, fac, ph, pre, guard, cs.guard_len, cs.first, &cfg, nullptr, nullptr, nullptr, &res);
        if (rc) printf("rc %d %s\n", rc, vgen_last_error(ctxs[0]));
        CHECK(rc == 0);
        vgen_filter *f = nullptr;
        CHECK(vgen_filter_compile(cs.pat, cs.ci, 7, &f) == VGEN_OK);
        const bool best = (cs.flags & VGEN_SCAN_BEST) != 0;
        // expected: a plain walk of the counters the scan covered
        std::vector<uint64_t> want;
        int64_t top = -1;
        const uint64_t nb = res.operations / BATCH;
        for (uint64_t c = 0; c < nb * BATCH && want.size() < cs.count; c++) {
            const std::string a = addr3(cs.guard_len, cs.first + c);
            if (vgen_filter_matches(f, a.c_str()) != 1) continue;
            if (best) {
                uint32_t s = 0;
                CHECK(vgen_score(f, a.c_str(), &s) == VGEN_OK);
                if ((int64_t)s <= top) continue;
                top = s;
            }
            want.push_back(cs.first + c);
        }
        CHECK(!want.empty());                       // no comparison is empty
        CHECK(res.n_matches == want.size());
        uint32_t last_score = 0;
        for (uint64_t i = 0; i < res.n_matches && i < want.size(); i++) {
            const vgen_generated &g = res.matches[i];
            if (counter_of(g) != want[i]) {
                printf("  %s: match %llu counter %llx want %llx\n", cs.pat, (unsigned long long)i, (unsigned long long)counter_of(g), (unsigned long long)want[i]);
                fails++;
                break;
            }
            CHECK(memcmp(g.key, pre, 24) == 0 && g.format == 7 && !strcmp(g.wif, g.hex) && !strncmp(g.hex, "0x80", 4) && strlen(g.hex) == 66);
            CHECK(addr3(cs.guard_len, want[i]) == g.address);
            if (best) {
                uint32_t s = 0;
                CHECK(vgen_score(f, g.address, &s) == VGEN_OK && (i == 0 || s > last_score));   // strictly rising
                last_score = s;
            }
        }
        printf("%-20s guard %2d ctx %u: %llu matches, %llu ops, complete %d\n", cs.pat, cs.guard_len, cs.nctx, (unsigned long long)res.n_matches,
               (unsigned long long)res.operations, res.complete);
        if (cs.maxb) CHECK(res.operations == cs.maxb * cs.nctx * BATCH);
        n_cases++;
        n_complete += res.complete;
        vgen_scan_result_free(&res);
        vgen_filter_free(f);
        for (auto *c : ctxs) vgen_destroy(c);
    }
    CHECK(n_complete == 1);

    // a guard of length 0 is not "no guard", and the guard's bytes matter
    CHECK(addr3(-1, 5) != addr3(0, 5) && addr3(20, 5) != addr3(21, 5));

    // CREATE3, then CREATE2 on the same contexts: the second scan is CREATE2's, and a CREATE3 scan after it is CREATE3's again
    {
        std::vector<vgen_ctx *> ctxs = {mk(4096), mk(4096)};
        vgen_scan_config cfg = config(6, 0, 0, 0);
        vgen_filter *f = nullptr;
        vgen_filter_compile("^0x00", 0, 7, &f);
        for (int round = 0; round < 3; round++) {
            const bool c3 = round != 1;
            vgen_scan_result res;
            const int rc = c3 ? vgen_scan_create3(ctxs.data(), 2, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res)
                              : vgen_scan_create2(ctxs.data(), 2, "^0x00", fac, ph, pre, 0, &cfg, nullptr, nullptr, nullptr, &res);
            CHECK(rc == 0 && res.n_matches == 6);
            std::vector<uint64_t> want;
            for (uint64_t c = 0; want.size() < 6 && c < 40 * BATCH; c++) {
                std::string a;
                if (c3) {
                    a = addr3(20, c);
                } else {
                    uint8_t s[32], b[20];
                    char str[128];
                    vgen_create2_salt(pre, c, s);
                    vgen_create2_address(fac, s, ph, b);
                    vgen_address_from_payload(7, b, str, sizeof str);
                    a = str;
                }
                if (vgen_filter_matches(f, a.c_str()) == 1) want.push_back(c);
            }
            for (uint64_t i = 0; i < res.n_matches && i < want.size(); i++) CHECK(counter_of(res.matches[i]) == want[i]);
            printf("round %d (%s): first counter %llu\n", round, c3 ? "create3" : "create2", (unsigned long long)(res.n_matches ? counter_of(res.matches[0]) : 0));
            vgen_scan_result_free(&res);
        }
        vgen_filter_free(f);
        for (auto *c : ctxs) vgen_destroy(c);
    }

    // refusals: those of vgen_scan_create2, and the guard's length
    vgen_ctx *c = mk(4096);
    vgen_scan_config cfg = config(1, 0, 0, 0);
    vgen_scan_result res;
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 65, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, -2, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, nullptr, 1, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    CHECK(vgen_scan_create3(&c, 1, "^0x00", nullptr, ph, pre, nullptr, -1, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, nullptr, 0, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_OK && res.n_matches == 1);
    vgen_scan_result_free(&res);
    cfg.seed = 4;
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    CHECK(strstr(vgen_last_error(c), "vgen_scan_create3") != nullptr);
    cfg.seed = 0;
    cfg.checkpoint_path = "/tmp/x.ckpt";
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    cfg.checkpoint_path = nullptr;
    cfg.has_start = 1;
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_UNSUPPORTED);
    cfg.has_start = 0;
    cfg.flags = VGEN_SCAN_BEST;   // --best needs a score specification
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    cfg.flags = 0;
    cfg.format = 5;
    CHECK(vgen_scan_create3(&c, 1, "^0x00", fac, ph, pre, guard, 20, 0, &cfg, nullptr, nullptr, nullptr, &res) == VGEN_E_INVALID);
    CHECK(vgen_set_create3(c, fac, ph, pre, guard, 65) == VGEN_E_INVALID && vgen_set_create3(c, fac, ph, pre, nullptr, 3) == VGEN_E_INVALID);
    CHECK(vgen_set_create3(c, fac, ph, pre, nullptr, -1) == VGEN_OK);
    vgen_destroy(c);
    // a context that is not format 7, and one of the stand-in that nobody taught CREATE3 jobs: no entry point, VGEN_E_INVALID
    {
        vgen_params p;
        memset(&p, 0, sizeof p);
        p.struct_size = sizeof p;
        p.batch_size = BATCH;
        p.format = 7;
        p.frames = 2;
        vgen_ctx *plain = nullptr;
        CHECK(vgen_create(&p, &plain) == VGEN_OK);
        CHECK(vgen_set_create3(plain, fac, ph, pre, nullptr, -1) == VGEN_E_INVALID);
        vgen_destroy(plain);
        p.format = 5;
        CHECK(vgen_create(&p, &plain) == VGEN_OK);
        CHECK(vgen_set_create3(plain, fac, ph, pre, nullptr, -1) == VGEN_E_INVALID);
        vgen_destroy(plain);
    }
    printf("cases %d\n", n_cases);
    printf(fails ? "FAILED %d\n" : "all ok\n", fails);
    return fails != 0;
}
