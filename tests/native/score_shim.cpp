// score_shim.cpp — TEST-ONLY: the g++ build of core/score_eval.h behind two C entry points, for tests/test_score.py (the very
// source hipcc compiles into payload_score_kernel and create2_score_kernel).  Built by the test itself; never loaded by vgen_amd.
#include <string.h>

#include "../../vgen_amd/csrc/core/score_eval.h"

extern "C" {

// value of one metric on a 20-byte payload
uint32_t score_shim_metric(uint32_t metric, uint32_t digit, const uint8_t payload[20]) {
    vg::u32 w[5], H[5];
    memcpy(w, payload, 20);
    for (int i = 0; i < 5; i++) H[i] = vg::bswap32(w[i]);
    return vg::score_metric(metric, digit, H);
}

// n terms (metric, digit, min) x n -> 1 when every term holds; *score = the first term's value
int score_shim_eval(uint32_t n, const uint32_t *terms, const uint8_t payload[20], uint32_t *score) {
    vg::ScoreTerms t;
    memset(&t, 0, sizeof t);
    t.n = n;
    for (uint32_t k = 0; k < n && k < vg::SCORE_MAX_TERMS; k++) {
        t.t[k].metric = terms[3 * k];
        t.t[k].digit = terms[3 * k + 1];
        t.t[k].min = terms[3 * k + 2];
    }
    vg::u32 w[5];
    memcpy(w, payload, 20);
    return vg::score_eval(t, w, score) ? 1 : 0;
}

// many payloads at once: out[i] = the metric's value on payloads[20 i ..]
void score_shim_metric_many(uint32_t metric, uint32_t digit, const uint8_t *payloads, uint32_t count, uint32_t *out) {
    for (uint32_t i = 0; i < count; i++) out[i] = score_shim_metric(metric, digit, payloads + (size_t)20 * i);
}
}
