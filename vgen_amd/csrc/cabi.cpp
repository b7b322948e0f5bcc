// cabi.cpp — the extern "C" surface declared in include/vgen_hip.h.
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <string>
#include <vector>

#include "../../include/vgen_hip.h"
#include "host/ed_host.h"
#include "host/onion_host.h"
#include "host/encode.h"
#include "host/filter.h"
#include "host/pattern_info.h"
#include "host/provider.h"
#include "core/hash.h"
#include "host/scalar.h"
#include "runtime.h"

namespace {
thread_local std::string g_last_error;

// (No load-time side effects: the library neither sets nor needs GPU_MAX_HW_QUEUES.  A context drives every frame
// through a stream of its own, spread over the runtime's stream priority levels so that each owns a hardware queue —
// runtime.cpp: create_stream.)

int copy_out(const std::string &s, char *out, size_t cap) {
    if (!out || cap < s.size() + 1) return VGEN_E_INVALID;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}
}  // namespace

extern "C" {

int vgen_abi_version(void) { return VGEN_ABI_VERSION; }

int vgen_device_count(int *n) {
    if (!n) return VGEN_E_INVALID;
    return vg::rt_device_count(n, g_last_error);
}

int vgen_device_name(int device, char *buf, size_t cap) {
    if (!buf || cap == 0) return VGEN_E_INVALID;
    std::string s;
    if (int rc = vg::rt_device_name(device, s, g_last_error)) return rc;
    strncpy(buf, s.c_str(), cap - 1);
    buf[cap - 1] = 0;
    return VGEN_OK;
}

int vgen_create(const vgen_params *p, vgen_ctx **out) {
    std::string err;
    int rc = vg::rt_create(p, out, err);
    if (rc != VGEN_OK) g_last_error = err;
    return rc;
}

void vgen_destroy(vgen_ctx *ctx) { vg::rt_destroy(ctx); }

const char *vgen_last_error(const vgen_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int vgen_get_info(const vgen_ctx *ctx, uint32_t *batch_size, uint32_t *frames, uint32_t *match_cap) {
    if (!ctx) return VGEN_E_INVALID;
    if (batch_size) *batch_size = ctx->batch;
    if (frames) *frames = ctx->frames;
    if (match_cap) *match_cap = ctx->match_cap;
    return VGEN_OK;
}

int vgen_get_resources(const vgen_ctx *ctx, uint32_t *dump_frames, uint32_t *table_bits, uint32_t *table_bits_wanted, char *note, size_t note_cap) {
    if (!ctx) return VGEN_E_INVALID;
    std::string why;
    const int rc = vg::rt_get_resources(ctx, dump_frames, table_bits, table_bits_wanted, &why);
    if (note && note_cap) {
        strncpy(note, why.c_str(), note_cap - 1);
        note[note_cap - 1] = 0;
    }
    return rc;
}

int vgen_get_memory(const vgen_ctx *ctx, vgen_memory_info *out) {
    if (!ctx || !out) return VGEN_E_INVALID;
    return vg::rt_get_memory(ctx, out);
}

int vgen_filter_compile(const char *pattern, int case_insensitive, uint32_t format, vgen_filter **out) {
    if (!pattern || !out) return VGEN_E_INVALID;
    if (vg::score_spec_unsupported(pattern, format)) {
        g_last_error = vg::SCORE_FORMATS_MESSAGE;
        return VGEN_E_UNSUPPORTED;
    }
    vgen_filter *f = new vgen_filter();
    std::string err;
    if (!vg::filter_compile(pattern, case_insensitive != 0, format, *f, err)) {
        g_last_error = err;
        delete f;
        return VGEN_E_PATTERN;
    }
    *out = f;
    return VGEN_OK;
}

void vgen_filter_free(vgen_filter *f) { delete f; }

int vgen_filter_matches(const vgen_filter *f, const char *address) {
    if (!f || !address) return VGEN_E_INVALID;
    if (f->list || f->score.n) return vg::filter_accepts(*f, address, nullptr) ? 1 : 0;
    return f->dfa.is_match(address) ? 1 : 0;
}

int vgen_filter_compile_list(const char *patterns, int case_insensitive, uint32_t format, vgen_filter **out) {
    if (!patterns || !out) return VGEN_E_INVALID;
    if (format == vg::VGF_SOLANA) {
        g_last_error = "pattern lists are not provided for the solana format (12): a list's table holds intervals of 64 payload bits, Base58 of 32 bytes needs all 256";
        return VGEN_E_UNSUPPORTED;
    }
    if (format == vg::VGF_ONION) {
        g_last_error = "pattern lists are not provided for the onion format (13)";
        return VGEN_E_UNSUPPORTED;
    }
    vgen_filter *f = new vgen_filter();
    std::string err;
    if (!vg::filter_compile_list(patterns, case_insensitive != 0, format, *f, err)) {
        g_last_error = err;
        delete f;
        return VGEN_E_PATTERN;
    }
    *out = f;
    return VGEN_OK;
}

int vgen_filter_pattern_count(const vgen_filter *f, uint32_t *n) {
    if (!f || !n) return VGEN_E_INVALID;
    *n = f->list ? (uint32_t)f->list->patterns.size() : 1u;
    return VGEN_OK;
}

int vgen_filter_pattern(const vgen_filter *f, uint32_t index, char *out, size_t cap) {
    if (!f) return VGEN_E_INVALID;
    if (f->list ? index >= f->list->patterns.size() : index != 0) return VGEN_E_INVALID;
    return copy_out(f->list ? f->list->patterns[index] : f->pattern, out, cap);
}

int vgen_filter_which(const vgen_filter *f, const char *address, uint32_t *indices, uint32_t cap, uint32_t *n) {
    if (!f || !address || !n || (cap && !indices)) return VGEN_E_INVALID;
    std::vector<uint32_t> w;
    vg::filter_which(*f, address, nullptr, w);
    *n = (uint32_t)w.size();
    for (uint32_t i = 0; i < w.size() && i < cap; i++) indices[i] = w[i];
    return VGEN_OK;
}

int vgen_filter_device_kind(const vgen_filter *f) { return f ? (int)f->dev.kind : VGEN_E_INVALID; }

int vgen_filter_dfa_bytes(const vgen_filter *f) { return f ? (f->dev.kind == vg::DEVF_DFA ? (int)f->dev.dfa_bytes : 0) : VGEN_E_INVALID; }

int vgen_pattern_invalid_chars(const char *pattern, int case_insensitive, uint32_t format, char *out, size_t cap,
                               size_t *n) {
    if (!pattern || !n || !vg::format_charset_name(format)) return VGEN_E_INVALID;
    const std::string bad = vg::pattern_invalid_chars(pattern, case_insensitive != 0, format);
    *n = bad.size();
    if (out && cap) {
        const size_t m = bad.size() < cap - 1 ? bad.size() : cap - 1;
        memcpy(out, bad.data(), m);
        out[m] = 0;
    }
    return VGEN_OK;
}

int vgen_pattern_difficulty(const char *pattern, int case_insensitive, uint32_t format, uint64_t *out) {
    if (!pattern || !out || !vg::format_charset_name(format)) return VGEN_E_INVALID;
    *out = vg::pattern_difficulty(pattern, case_insensitive != 0, format);
    return VGEN_OK;
}

const char *vgen_format_charset_name(uint32_t format) { return vg::format_charset_name(format); }

int vgen_provider_resolve(const char *pattern, const char *table_path, char *address, size_t acap, uint32_t *format,
                          int32_t *has_range, uint8_t start_be[32], uint8_t end_be[32]) {
    if (!pattern || !address || !format || !has_range || !start_be || !end_be) return VGEN_E_INVALID;
    vg::ProviderResult r;
    std::string err;
    const int rc = vg::provider_resolve(pattern, table_path, r, err);
    if (rc < 0) {
        g_last_error = err;
        return VGEN_E_INVALID;
    }
    if (rc == 0) return 0;
    if (r.address.size() + 1 > acap) return VGEN_E_INVALID;
    memcpy(address, r.address.c_str(), r.address.size() + 1);
    *format = r.format;
    *has_range = r.has_range ? 1 : 0;
    memcpy(start_be, r.start, 32);
    memcpy(end_be, r.end, 32);
    return 1;
}

int vgen_provider_build_pattern(const char *address, uint32_t prefix_length, char *out, size_t cap) {
    if (!address || !out) return VGEN_E_INVALID;
    const std::string p = prefix_length ? vg::provider_build_pattern(address, prefix_length) : vg::provider_build_exact_pattern(address);
    if (p.size() + 1 > cap) return VGEN_E_INVALID;
    memcpy(out, p.c_str(), p.size() + 1);
    return VGEN_OK;
}

int vgen_clock_probe_start(vgen_ctx *ctx, uint32_t duration_ms) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_clock_probe_start(ctx, duration_ms);
}

int vgen_clock_probe_read(vgen_ctx *ctx, double *mhz) {
    if (!ctx || !mhz) return VGEN_E_INVALID;
    return vg::rt_clock_probe_read(ctx, mhz);
}

int vgen_set_match_cap(vgen_ctx *ctx, uint32_t match_cap) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_set_match_cap(ctx, match_cap);
}

int vgen_set_filter(vgen_ctx *ctx, const vgen_filter *f) {
    if (!ctx) return VGEN_E_INVALID;
    const int rc = vg::rt_set_filter(ctx, f);
    if (rc != VGEN_OK) return rc;
    // a score filter's terms (n = 0 for every other filter): the runtime installs them itself; repeated here so that a stand-in of the
    // runtime that knows nothing of score filters (tests/native) leaves the context in the same state
    if (f) ctx->score = f->score;
    else memset(&ctx->score, 0, sizeof ctx->score);
    return VGEN_OK;
}

int vgen_set_score_min(vgen_ctx *ctx, uint32_t min) {
    if (!ctx) return VGEN_E_INVALID;
    if (!ctx->have_filter || ctx->score.n == 0)   // (the terms are installed by vgen_set_filter, for a score filter only)
        return ctx->fail(VGEN_E_STATE, "vgen_set_score_min: the installed filter is not a score filter");
    if (min > vg::score_metric_max(ctx->score.t[0].metric))
        return ctx->fail(VGEN_E_PATTERN, "vgen_set_score_min: the first term's metric is at most " + std::to_string(vg::score_metric_max(ctx->score.t[0].metric)));
    ctx->score.t[0].min = min;
    return VGEN_OK;
}

int vgen_score(const vgen_filter *f, const char *address, uint32_t *score) {
    if (!f || !address || !score || f->score.n == 0) return VGEN_E_INVALID;
    return vg::score_of(*f, address, nullptr, score, nullptr) ? VGEN_OK : VGEN_E_INVALID;
}

// An onion context walks Ed25519 scalars in steps of 8 from a base: the secp256k1 dispatches refuse it.
static int refuse_onion(vgen_ctx *c, const char *what) {
    return c->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": an onion context walks Ed25519 scalars a + 8 i - use vgen_dispatch_onion");
}

int vgen_dispatch(vgen_ctx *ctx, uint32_t frame, const uint8_t start_key_be[32]) {
    if (!ctx) return VGEN_E_INVALID;
    if (ctx->format == vg::VGF_ONION) return refuse_onion(ctx, "vgen_dispatch");
    return vg::rt_dispatch(ctx, frame, start_key_be);
}

int vgen_dispatch_keys(vgen_ctx *ctx, uint32_t frame, const uint8_t *keys_be, uint32_t n) {
    if (!ctx) return VGEN_E_INVALID;
    if (ctx->format == vg::VGF_ONION) return refuse_onion(ctx, "vgen_dispatch_keys");
    return vg::rt_dispatch_keys(ctx, frame, keys_be, n);
}

#ifdef VGEN_TEST_HOOKS
// Fault injection: only in the test build of the library (tests/native/libvgen_hip_hooks.so, tests/native/vgen_hip_hooks.h).
extern "C" int vgen_debug_fail_after(vgen_ctx *ctx, uint64_t after_dispatches) {
    if (!ctx) return VGEN_E_INVALID;
    ctx->fail_after = after_dispatches;
    return VGEN_OK;
}
#endif

int vgen_dispatch_random(vgen_ctx *ctx, uint32_t frame, uint64_t seed, uint32_t stream, uint64_t first_index) {
    if (!ctx) return VGEN_E_INVALID;
    if (ctx->format == vg::VGF_ONION) return refuse_onion(ctx, "vgen_dispatch_random");
    return vg::rt_dispatch_random(ctx, frame, vg::rnd_seed_from_u64(seed), stream, first_index);
}

int vgen_dispatch_random_seed(vgen_ctx *ctx, uint32_t frame, const uint8_t seed[24], uint32_t stream, uint64_t first_index) {
    if (!ctx || !seed) return VGEN_E_INVALID;
    if (ctx->format == vg::VGF_ONION) return refuse_onion(ctx, "vgen_dispatch_random_seed");
    return vg::rt_dispatch_random(ctx, frame, vg::rnd_seed_from_bytes(seed), stream, first_index);
}

int vgen_random_key(uint64_t seed, uint32_t stream, uint64_t index, uint8_t key_be[32]) {
    if (!key_be) return VGEN_E_INVALID;
    return vg::random_key_be(vg::rnd_seed_from_u64(seed), stream, index, key_be) ? VGEN_OK : VGEN_E_RANGE;
}

int vgen_random_key_seed(const uint8_t seed[24], uint32_t stream, uint64_t index, uint8_t key_be[32]) {
    if (!seed || !key_be) return VGEN_E_INVALID;
    return vg::random_key_be(vg::rnd_seed_from_bytes(seed), stream, index, key_be) ? VGEN_OK : VGEN_E_RANGE;
}

int vgen_wait(vgen_ctx *ctx, uint32_t frame, vgen_match *out, uint32_t cap, uint32_t *n_matches,
              uint64_t *keys_tested) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_wait(ctx, frame, out, cap, n_matches, keys_tested);
}

int vgen_read_dump(vgen_ctx *ctx, uint32_t frame, uint8_t *out, size_t out_len) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_read_dump(ctx, frame, out, out_len);
}

int vgen_dump_view(vgen_ctx *ctx, uint32_t frame, const uint8_t **ptr, size_t *len) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_dump_view(ctx, frame, ptr, len);
}

int vgen_get_topology(const vgen_ctx *ctx, uint32_t *streams, uint32_t *hw_queues, uint32_t *priority_levels,
                      int32_t *oversubscribed) {
    if (!ctx) return VGEN_E_INVALID;
    if (streams) *streams = ctx->frames;
    if (hw_queues) *hw_queues = ctx->hw_queues;
    if (priority_levels) *priority_levels = ctx->prio_levels;
    if (oversubscribed) *oversubscribed = vg::rt_oversubscribed(ctx) ? 1 : 0;
    return VGEN_OK;
}

int vgen_frame_kernel_ms(vgen_ctx *ctx, uint32_t frame, float *ms) {
    if (!ctx || !ms) return VGEN_E_INVALID;
    return vg::rt_frame_times(ctx, frame, ms, nullptr);
}

int vgen_frame_clock(vgen_ctx *ctx, uint32_t frame, uint32_t *cycles, uint32_t *ticks_100mhz) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_frame_clock(ctx, frame, cycles, ticks_100mhz);
}

int vgen_frame_dispatch_ms(vgen_ctx *ctx, uint32_t frame, float *ms) {
    if (!ctx || !ms) return VGEN_E_INVALID;
    return vg::rt_frame_times(ctx, frame, nullptr, ms);
}

int vgen_address_from_payload(uint32_t format, const uint8_t *payload, char *out, size_t cap) {
    if (!payload) return VGEN_E_INVALID;
    std::string s = vg::address_from_payload(format, payload);
    if (s.empty()) return VGEN_E_UNSUPPORTED;
    return copy_out(s, out, cap);
}

int vgen_key_to_wif(uint32_t format, const uint8_t key_be[32], char *out, size_t cap) {
    if (!key_be) return VGEN_E_INVALID;
    if (format == vg::VGF_SOLANA) return copy_out(vg::key_to_wif(format, key_be), out, cap);   // a seed: any 32 bytes
    if (format == vg::VGF_ONION) return copy_out(vg::key_to_wif(format, key_be), out, cap);    // an Ed25519 scalar, little-endian
    vg::Scalar k;
    vg::scalar_from_be(k, key_be);
    if (!vg::scalar_is_valid(k)) return VGEN_E_RANGE;
    return copy_out(vg::key_to_wif(format, key_be), out, cap);
}

int vgen_key_add(const uint8_t key_be[32], uint64_t amount, uint8_t out_be[32]) {
    if (!key_be || !out_be) return VGEN_E_INVALID;
    vg::Scalar k, r;
    vg::scalar_from_be(k, key_be);
    uint32_t carry = vg::scalar_add_u64(r, k, amount);
    vg::scalar_to_be(r, out_be);
    return (carry || !vg::scalar_is_valid(r)) ? VGEN_E_RANGE : VGEN_OK;
}

int vgen_key_variant(const uint8_t key_be[32], uint32_t variant, uint8_t out_be[32]) {
    if (!key_be || !out_be || variant >= 6) return VGEN_E_INVALID;
    vg::Scalar k, r;
    vg::scalar_from_be(k, key_be);
    if (!vg::scalar_is_valid(k)) return VGEN_E_RANGE;
    vg::scalar_variant(r, k, variant);
    vg::scalar_to_be(r, out_be);
    return VGEN_OK;
}

int vgen_nostr_encode(uint32_t kind, const uint8_t data[32], char *out, size_t cap) {
    if (!data || kind > 1) return VGEN_E_INVALID;
    return copy_out(vg::nip19_encode(kind ? "nsec" : "npub", data), out, cap);
}

int vgen_nostr_decode(const char *text, uint32_t *kind, uint8_t out[32]) {
    if (!text || !kind || !out) return VGEN_E_INVALID;
    const std::string s(text);
    for (uint32_t k = 0; k < 2; k++)
        if (vg::nip19_decode(k ? "nsec" : "npub", s, out)) {
            *kind = k;
            return VGEN_OK;
        }
    return VGEN_E_INVALID;
}

int vgen_derive(uint32_t format, const uint8_t key_be[32], char *address, size_t acap, char *wif, size_t wcap) {
    if (!key_be) return VGEN_E_INVALID;
    uint8_t payload[32];
    int n = vg::payload_from_key(format, key_be, payload);
    if (n == 0) {
        vg::Scalar k;
        vg::scalar_from_be(k, key_be);
        return vg::scalar_is_valid(k) ? VGEN_E_UNSUPPORTED : VGEN_E_RANGE;
    }
    if (address) {
        int rc = copy_out(vg::address_from_payload(format, payload), address, acap);
        if (rc < 0) return rc;
    }
    if (wif) {
        int rc = copy_out(vg::key_to_wif(format, key_be), wif, wcap);
        if (rc < 0) return rc;
    }
    return VGEN_OK;
}

int vgen_contract_address(const uint8_t deployer[20], uint64_t nonce, uint8_t out[20]) {
    if (!deployer || !out) return VGEN_E_INVALID;
    // rlp([deployer, nonce]): list header, 0x94 + the 20 address bytes, the nonce as a big-endian integer without leading zeros
    uint8_t msg[1 + 21 + 9], h[32];
    size_t n = 1;
    msg[n++] = 0x94;
    memcpy(msg + n, deployer, 20);
    n += 20;
    if (nonce == 0) {
        msg[n++] = 0x80;
    } else if (nonce < 0x80) {
        msg[n++] = (uint8_t)nonce;
    } else {
        int len = 0;
        for (uint64_t v = nonce; v; v >>= 8) len++;
        msg[n++] = (uint8_t)(0x80 + len);
        for (int i = len - 1; i >= 0; i--) msg[n++] = (uint8_t)(nonce >> (8 * i));
    }
    msg[0] = (uint8_t)(0xc0 + (n - 1));   // payload of at most 30 bytes: short list
    vg::host_keccak256(msg, n, h);
    memcpy(out, h + 12, 20);
    return VGEN_OK;
}

int vgen_keccak256(const uint8_t *data, size_t len, uint8_t out[32]) {
    if ((!data && len) || !out) return VGEN_E_INVALID;
    vg::host_keccak256(data, len, out);
    return VGEN_OK;
}

int vgen_create2_address(const uint8_t deployer[20], const uint8_t salt[32], const uint8_t init_code_hash[32], uint8_t out[20]) {
    if (!deployer || !salt || !init_code_hash || !out) return VGEN_E_INVALID;
    // through the single-source twin of the device block (core/hash.h), on the 22 message words the kernel hashes
    vg::u32 m[22], a[5];
    vg::create2_message(deployer, salt, init_code_hash, m);
    vg::keccak256_create2_addr(m, a);
    memcpy(out, a, 20);
    return VGEN_OK;
}

int vgen_create2_salt(const uint8_t salt_prefix[24], uint64_t counter, uint8_t salt[32]) {
    if (!salt_prefix || !salt) return VGEN_E_INVALID;
    memcpy(salt, salt_prefix, 24);
    for (int i = 0; i < 8; i++) salt[24 + i] = (uint8_t)(counter >> (8 * (7 - i)));
    return VGEN_OK;
}

int vgen_set_create2(vgen_ctx *ctx, const uint8_t deployer[20], const uint8_t init_code_hash[32], const uint8_t salt_prefix[24]) {
    if (!ctx) return VGEN_E_INVALID;
    if (!deployer || !init_code_hash || !salt_prefix) return ctx->fail(VGEN_E_INVALID, "vgen_set_create2: null job field");
    return vg::rt_set_create2(ctx, deployer, init_code_hash, salt_prefix);
}

int vgen_dispatch_create2(vgen_ctx *ctx, uint32_t frame, uint64_t first_counter) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_dispatch_create2(ctx, frame, first_counter);
}

int vgen_create3_proxy_hash(uint8_t out[32]) {
    if (!out) return VGEN_E_INVALID;
    // the 16-byte proxy Solmate / Solady CREATE3 and CreateX deploy; hashed here, not stored
    static const uint8_t proxy[16] = {0x67, 0x36, 0x3d, 0x3d, 0x37, 0x36, 0x3d, 0x34, 0xf0, 0x3d, 0x52, 0x60, 0x08, 0x60, 0x18, 0xf3};
    vg::host_keccak256(proxy, sizeof proxy, out);
    return VGEN_OK;
}

int vgen_create3_address(const uint8_t factory[20], const uint8_t salt[32], const uint8_t proxy_init_code_hash[32], const uint8_t *guard,
                         int32_t guard_len, uint8_t proxy_out[20], uint8_t out[20]) {
    if (!factory || !salt || !proxy_init_code_hash || !out || guard_len < -1 || guard_len > 64 || (guard_len > 0 && !guard)) return VGEN_E_INVALID;
    // through the single-source twins of the device blocks and the message builders the kernels use (core/hash.h)
    vg::u32 proxy[5], a[5];
    vg::create3_address(factory, salt, proxy_init_code_hash, guard, guard_len, proxy, a);
    if (proxy_out) memcpy(proxy_out, proxy, 20);
    memcpy(out, a, 20);
    return VGEN_OK;
}

int vgen_set_create3(vgen_ctx *ctx, const uint8_t factory[20], const uint8_t proxy_init_code_hash[32], const uint8_t salt_prefix[24],
                     const uint8_t *guard, int32_t guard_len) {
    if (!ctx) return VGEN_E_INVALID;
    if (!factory || !proxy_init_code_hash || !salt_prefix) return ctx->fail(VGEN_E_INVALID, "vgen_set_create3: null job field");
    if (guard_len < -1 || guard_len > 64 || (guard_len > 0 && !guard)) return ctx->fail(VGEN_E_INVALID, "vgen_set_create3: guard_len is -1 (no guard) or 0 .. 64 bytes");
    return vg::rt_set_create3(ctx, factory, proxy_init_code_hash, salt_prefix, guard, guard_len);
}

// ---- split-key search ----

int vgen_set_base_point(vgen_ctx *ctx, const uint8_t *pub, size_t len) {
    if (!ctx) return VGEN_E_INVALID;
    if (ctx->format == vg::VGF_ETHEREUM_CREATE2)
        return ctx->fail(VGEN_E_UNSUPPORTED, "vgen_set_base_point: an ethereum-create2 context tests salts - there is no key to split");
    if (ctx->format == vg::VGF_SOLANA)
        return ctx->fail(VGEN_E_UNSUPPORTED, "vgen_set_base_point: a solana key is a seed whose scalar is its hash - partial keys cannot be added");
    if (ctx->format == vg::VGF_ONION)
        return ctx->fail(VGEN_E_UNSUPPORTED, "vgen_set_base_point: split keys are not provided for the onion format");
    if (!ctx->base_set) return ctx->fail(VGEN_E_UNSUPPORTED, "vgen_set_base_point: this runtime does not serve split-key dispatches");
    const bool clear = !pub && len == 0;
    vg::ge pt;
    if (!clear && !vg::point_from_sec1(pub, len, pt))
        return ctx->fail(VGEN_E_INVALID, "vgen_set_base_point: not a secp256k1 public key (33 bytes 02 / 03 + x or 65 bytes 04 + x + y, coordinates "
                                         "below p, on the curve)");
    for (auto &f : ctx->fr)
        if (f.in_flight) return ctx->fail(VGEN_E_STATE, "vgen_set_base_point while a dispatch is in flight");
    return ctx->base_set(ctx, clear ? nullptr : &pt);
}

int vgen_get_base_point(const vgen_ctx *ctx, uint8_t out65[65], int32_t *is_set) {
    if (!ctx || !is_set) return VGEN_E_INVALID;
    *is_set = ctx->have_base ? 1 : 0;
    if (ctx->have_base && out65) vg::point_to_sec1(ctx->base_pt, out65);
    return VGEN_OK;
}

int vgen_split_dropped(const vgen_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return VGEN_E_INVALID;
    *n = ctx->split_dropped.load(std::memory_order_relaxed);
    return VGEN_OK;
}

int vgen_split_derive(uint32_t format, const uint8_t *pub, size_t len, const uint8_t partial_be[32], uint32_t variant, char *address, size_t cap) {
    if (!pub || !partial_be || !address) return VGEN_E_INVALID;
    if (!vg::format_charset_name(format) || format == vg::VGF_ETHEREUM_CREATE2 || vg::vgf_is_ed((int)format)) return VGEN_E_UNSUPPORTED;
    vg::ge base, pt, img;
    if (variant >= vg::vgf_endo_images((int)format) || !vg::point_from_sec1(pub, len, base)) return VGEN_E_INVALID;
    vg::Scalar k;
    vg::scalar_from_be(k, partial_be);
    if (vg::scalar_cmp_words(k.w, vg::SCALAR_N) >= 0) return VGEN_E_RANGE;
    if (!vg::point_add_gen(base, k, pt)) return VGEN_E_RANGE;
    vg::point_image(img, pt, variant);
    uint8_t payload[32];
    if (!vg::payload_from_point(format, img, payload)) return VGEN_E_UNSUPPORTED;
    return copy_out(vg::address_from_payload(format, payload), address, cap);
}

int vgen_split_combine(uint32_t format, const uint8_t secret_be[32], const uint8_t partial_be[32], const char *address, uint8_t final_be[32],
                       uint32_t *variant) {
    if (!secret_be || !partial_be || !address || !final_be) return VGEN_E_INVALID;
    if (!vg::format_charset_name(format) || format == vg::VGF_ETHEREUM_CREATE2 || vg::vgf_is_ed((int)format)) return VGEN_E_UNSUPPORTED;
    vg::Scalar s, k, sum;
    vg::scalar_from_be(s, secret_be);
    vg::scalar_from_be(k, partial_be);
    if (!vg::scalar_is_valid(s) || vg::scalar_cmp_words(k.w, vg::SCALAR_N) >= 0) return VGEN_E_RANGE;
    // (s + k) mod n: both below n, so one conditional subtraction
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)s.w[i] + k.w[i];
        sum.w[i] = (uint32_t)c;
        c >>= 32;
    }
    if (c || vg::scalar_cmp_words(sum.w, vg::SCALAR_N) >= 0) {
        int64_t b = 0;
        for (int i = 0; i < 8; i++) {
            const int64_t d = (int64_t)sum.w[i] - vg::SCALAR_N[i] + b;
            sum.w[i] = (uint32_t)d;
            b = d >> 32;
        }
    }
    if (vg::scalar_is_zero(sum)) return VGEN_E_RANGE;
    const std::string want(address);
    for (uint32_t v = 0; v < vg::vgf_endo_images((int)format); v++) {
        vg::Scalar kv;
        vg::scalar_variant(kv, sum, v);
        uint8_t kb[32], payload[32];
        vg::scalar_to_be(kv, kb);
        if (!vg::payload_from_key(format, kb, payload)) continue;
        const std::string got = vg::address_from_payload(format, payload);
        // (hex addresses: the EIP-55 casing is a checksum, not part of the address)
        if (vg::vgf_is_hex((int)format) ? got.size() == want.size() && strcasecmp(got.c_str(), want.c_str()) == 0 : got == want) {
            memcpy(final_be, kb, 32);
            if (variant) *variant = v;
            return VGEN_OK;
        }
    }
    return VGEN_E_INVALID;
}

// ---- Solana ----

int vgen_solana_seed(const uint8_t seed[24], uint32_t stream, uint64_t index, uint8_t out[32]) {
    if (!seed || !out) return VGEN_E_INVALID;
    // the digest core/rnd.h draws, in its natural byte order: what vgen_random_key_seed returns, without its range test
    vg::u32 k[8];
    vg::rnd_scalar(vg::rnd_seed_from_bytes(seed), stream, (vg::u32)index, (vg::u32)(index >> 32), k);
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(k[7 - i] >> (8 * (3 - b)));
    return VGEN_OK;
}

int vgen_solana_public_key(const uint8_t seed[32], uint8_t pub[32]) {
    if (!seed || !pub) return VGEN_E_INVALID;
    vg::ed_public_key(seed, pub);
    return VGEN_OK;
}

int vgen_solana_keypair_base58(const uint8_t seed[32], char *out, size_t cap) {
    if (!seed || !out || cap < 89) return VGEN_E_INVALID;
    return copy_out(vg::solana_keypair_base58(seed), out, cap);
}

int vgen_solana_decode(const char *address, uint8_t pub[32]) {
    if (!address || !pub) return VGEN_E_INVALID;
    return vg::solana_decode(address, pub) ? VGEN_OK : VGEN_E_INVALID;
}

// ---- Tor v3 onion addresses ----

int vgen_onion_encode(const uint8_t pub[32], char *out, size_t cap) {
    if (!pub || !out) return VGEN_E_INVALID;
    return copy_out(vg::onion_encode(pub), out, cap);
}

int vgen_onion_decode(const char *address, uint8_t pub[32]) {
    if (!address || !pub) return VGEN_E_INVALID;
    return vg::onion_decode(address, pub) ? VGEN_OK : VGEN_E_INVALID;
}

int vgen_onion_expand(const uint8_t scalar_le[32], uint8_t out[64]) {
    if (!scalar_le || !out) return VGEN_E_INVALID;
    vg::onion_expand(scalar_le, out);
    return VGEN_OK;
}

int vgen_onion_base(const uint8_t seed[24], uint32_t stream, uint8_t scalar_le[32]) {
    if (!seed || !scalar_le) return VGEN_E_INVALID;
    vg::onion_base(vg::rnd_seed_from_bytes(seed), stream, scalar_le);
    return VGEN_OK;
}

int vgen_dispatch_onion(vgen_ctx *ctx, uint32_t frame, const uint8_t base_scalar_le[32], uint64_t first_index) {
    if (!ctx) return VGEN_E_INVALID;
    return vg::rt_dispatch_onion(ctx, frame, base_scalar_le, first_index);
}

}  // extern "C"
