// scan_match.h — a confirmed match as the scan loop carries it (scanner.cpp): from a candidate to the private key and the
// address, the list the matches are collected in, and their rendering for the caller.
#pragma once
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../../include/vgen_hip.h"
#include "ed_host.h"
#include "onion_host.h"
#include "encode.h"
#include "filter.h"
#include "scalar.h"

namespace vg {

// `images`: 1, or 6 when the dispatch tested the endomorphism / negation images of every point: index is then
// variant * batch + i and the key is variant `index / batch` of batch_start + i (host/scalar.h).
// How a batch's candidate index maps to its private key: batch_start + index (the walk), or the counter-based stream.
struct BatchKeys {
    uint64_t batch_no = 0;   // this shard's batch number (checkpointed batches included)
    Scalar start{};
    bool random = false;
    RndSeed seed{};
    uint64_t first_index = 0;
    uint32_t stream = 0;
    // split-key scans (a context with a base point): the base P the batch was dispatched under, and where refused candidates are counted
    const ge *base = nullptr;
    std::atomic<uint64_t> *dropped = nullptr;
};

// A confirmed match as the scan loop carries it: the private key and the address string.  WIF and hex are rendered when
// the match is handed to the caller (finish_result), in parallel and only for the matches that survive `count` — the
// reference, too, builds its WIF per MATCH, not per candidate (src/gpu.rs:1080-1088).  [Round 3 carried the 276-byte ABI
// record with everything rendered: on a permissive pattern (`^1C`: one key in 23) more than half of a scan was the serial
// hand-over of those records and their second Base58Check, profiles/r04_permissive.txt.]
struct LiteMatch {
    uint8_t key[32];
    char address[64];     // NUL-terminated (longest: a 62-character bech32m address)
};

// The matches of a scan in hand-over order, kept as the BLOCKS they arrive in (the worker threads' per-batch results, moved in whole): a
// permissive pattern yields millions, and copying them into one growing vector — reallocations and first-touch page faults, all on the
// scanning thread — was a third of such a scan even after the records had shrunk to 96 bytes (profiles/r04_permissive.txt).
class MatchList {
public:
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    void push_back(const LiteMatch &m) {
        if (blocks_.empty() || blocks_.back().size() == blocks_.back().capacity()) {
            blocks_.emplace_back();
            blocks_.back().reserve(1024);
        }
        blocks_.back().push_back(m);
        n_++;
    }
    // the first k entries of v, without copying them
    void take(std::vector<LiteMatch> &&v, size_t k) {
        if (k == 0) return;
        if (k < v.size()) v.resize(k);
        n_ += v.size();
        blocks_.push_back(std::move(v));
    }
    void append_copy(const std::vector<LiteMatch> &v) {
        if (v.empty()) return;
        n_ += v.size();
        blocks_.push_back(v);
    }
    void append(MatchList &&o) {
        for (auto &b : o.blocks_) {
            n_ += b.size();
            blocks_.push_back(std::move(b));
        }
        o.blocks_.clear();
        o.n_ = 0;
    }
    void truncate(size_t n) {   // keep the first n
        while (n_ > n) {
            auto &b = blocks_.back();
            const size_t drop = std::min(n_ - n, b.size());
            b.resize(b.size() - drop);
            n_ -= drop;
            if (b.empty()) blocks_.pop_back();
        }
    }
    std::vector<LiteMatch> flatten() const {
        std::vector<LiteMatch> out;
        out.reserve(n_);
        for (auto &b : blocks_) out.insert(out.end(), b.begin(), b.end());
        return out;
    }
    const std::vector<std::vector<LiteMatch>> &blocks() const { return blocks_; }

private:
    std::vector<std::vector<LiteMatch>> blocks_;
    size_t n_ = 0;
};

inline bool make_match(const vgen_filter &flt, uint32_t format, const BatchKeys &bk, uint32_t index,
                const uint8_t *payload, const Scalar *end, LiteMatch &g, uint32_t batch = 0, uint32_t images = 1) {
    std::string addr = address_from_payload(format, payload);
    if (addr.empty() || addr.size() >= sizeof g.address || !filter_accepts(flt, addr, payload)) return false;   // pattern.matches, gpu.rs:1069
    if (format == VGF_SOLANA) {
        // The key is the SEED the stream drew for this candidate (every draw is one: no range test).  Its public key is re-derived here
        // with the host build of the device's headers, and a candidate whose payload differs is dropped: one multiplication per MATCH.
        if (!bk.random) return false;   // (nothing walks this format)
        const uint64_t at = bk.first_index + index;
        u32 d[8];
        rnd_scalar(bk.seed, bk.stream, (u32)at, (u32)(at >> 32), d);
        uint8_t mine[32];
        for (int i = 0; i < 8; i++)
            for (int b = 0; b < 4; b++) g.key[4 * i + b] = (uint8_t)(d[7 - i] >> (8 * (3 - b)));
        ed_public_key(g.key, mine);
        if (memcmp(mine, payload, 32) != 0) {
            if (bk.dropped) bk.dropped->fetch_add(1, std::memory_order_relaxed);
            return false;
        }
        memcpy(g.address, addr.c_str(), addr.size() + 1);
        return true;
    }
    if (format == VGF_ONION) {
        // The key is the scalar base(seed, stream) + 8 (first_index + index), little-endian.  Its public key is re-derived here (scalar x B
        // with the host build of the device's headers) and a candidate whose payload differs is dropped: one multiplication per MATCH.
        if (!bk.random) return false;   // (the scan loop names every batch by its stream and first index)
        uint8_t base[32], mine[32];
        onion_base(bk.seed, bk.stream, base);
        if (!onion_scalar_at(base, bk.first_index + index, g.key)) return false;
        onion_public_key(g.key, mine);
        if (memcmp(mine, payload, 32) != 0) {
            if (bk.dropped) bk.dropped->fetch_add(1, std::memory_order_relaxed);
            return false;
        }
        memcpy(g.address, addr.c_str(), addr.size() + 1);
        return true;
    }
    Scalar k;
    const uint32_t variant = images > 1 ? index / batch : 0;
    if (images > 1) index %= batch;
    if (bk.random) {
        uint8_t rk[32];
        if (!random_key_be(bk.seed, bk.stream, bk.first_index + index, rk)) return false;   // not a valid draw: no key
        scalar_from_be(k, rk);
    } else if (scalar_add_u64(k, bk.start, index) || !scalar_is_valid(k)) {
        return false;                                                   // increment_key -> None
    }
    if (bk.base) {
        // Split-key scan: the result is the PARTIAL key as walked (no image applied: the address is image `variant` of the point
        // P + k*G, and only the requester can apply it to s + k).  The payload is re-derived here from P + k*G with the host's
        // complete addition and the single-source hashes, and a candidate whose payload differs from the device's is dropped and
        // counted: the walk's "no exceptional cases because k0 + N + S < n" is a statement about the effective scalar s + k,
        // which the host does not know - a crafted P makes one workgroup's batched additions meet Q_j = +/-R_u and garbles its
        // payloads.  One point operation per MATCH, not per key.
        ge pt, img;
        uint8_t mine[32] = {0};
        bool same = scalar_is_valid(k) && point_add_gen(*bk.base, k, pt);
        if (same) {
            point_image(img, pt, variant);
            const int len = payload_from_point(format, img, mine);
            same = len != 0 && memcmp(mine, payload, (size_t)len) == 0;
        }
        if (!same) {
            if (bk.dropped) bk.dropped->fetch_add(1, std::memory_order_relaxed);
            return false;
        }
        scalar_to_be(k, g.key);
        memcpy(g.address, addr.c_str(), addr.size() + 1);
        return true;
    }
    if (variant) {
        Scalar kv;
        scalar_variant(kv, k, variant);
        k = kv;
    }
    if (end && scalar_cmp(k, *end) > 0) return false;                   // gpu.rs:1074-1078
    scalar_to_be(k, g.key);
    memcpy(g.address, addr.c_str(), addr.size() + 1);
    return true;
}

// GeneratedAddress (src/address.rs:63-72) of a match: address, WIF (src/gpu.rs:1080-1088), hex, format, key.
// `partial` (split-key scans): the key is a partial key - hex = wif = "0x" + its lowercase hex, the CREATE2 convention, never a WIF: a
// partial key must not look importable.
inline void render_match(uint32_t format, const LiteMatch &m, vgen_generated &g, bool partial = false) {
    memset(&g, 0, sizeof g);
    const std::string hex = (partial ? "0x" : "") + hex_lower(m.key, 32), wif = partial ? hex : key_to_wif(format, m.key);
    strncpy(g.address, m.address, sizeof g.address - 1);
    strncpy(g.wif, wif.c_str(), sizeof g.wif - 1);
    strncpy(g.hex, hex.c_str(), sizeof g.hex - 1);
    g.format = format;
    memcpy(g.key, m.key, 32);
}

// a recorded match (checkpoint file: keys only) back into the loop's form
inline bool lite_from_key(uint32_t format, const uint8_t kb[32], LiteMatch &g) {
    uint8_t payload[32];
    if (!payload_from_key(format, kb, payload)) return false;
    const std::string addr = address_from_payload(format, payload);
    if (addr.empty() || addr.size() >= sizeof g.address) return false;
    memcpy(g.key, kb, 32);
    memcpy(g.address, addr.c_str(), addr.size() + 1);
    return true;
}

}  // namespace vg
