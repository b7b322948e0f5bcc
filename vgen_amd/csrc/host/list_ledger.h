// list_ledger.h — which confirmed keys of a pattern-list scan are its results (vgen_scan_list, scanner.cpp).
#pragma once
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#include "filter.h"
#include "scan_match.h"

namespace vg {

// The per-pattern bookkeeping of a pattern-list scan (vgen_scan_list).  Shards hand in the confirmed matches of every batch
// they commit, keyed by the batch's GLOBAL number (batch * shards + shard); the ledger applies them in that order — what
// vgen_scan's order is on one context — so that "the first per_pattern keys of the walk that satisfy pattern i" does not
// depend on which context finished first.  A match is taken when it satisfies a pattern that still wants matches; it then
// counts toward every pattern it satisfies.
struct ListLedger {
    const vgen_filter *flt = nullptr;
    uint64_t per_pattern = 0, count = UINT64_MAX;
    uint32_t shards = 1;
    std::vector<uint64_t> recorded;       // per shard: batches a resumed checkpoint already holds (applied up front)
    std::mutex mu;
    std::vector<uint64_t> got;            // matches taken per pattern
    uint64_t unsatisfied = 0;             // patterns below per_pattern (per_pattern > 0)
    std::map<uint64_t, std::vector<LiteMatch>> pending;   // committed batches waiting for the ones before them
    uint64_t next = 0;                    // global batch applied next
    std::vector<LiteMatch> accepted;
    std::atomic<bool> done{false};
    std::atomic<uint64_t> n_accepted{0};
    bool arrival = false;                 // contexts that walk from bases of their own (VGEN_FLAG_ENDO): no global order to keep

    void init(const vgen_filter *f, uint64_t pp, uint64_t cnt, uint32_t n_shards) {
        flt = f;
        per_pattern = pp;
        count = cnt;
        shards = std::max(1u, n_shards);
        got.assign(f->list->patterns.size(), 0);
        unsatisfied = pp ? got.size() : 0;
        recorded.assign(shards, 0);
        done = count == 0;
    }
    // (under mu)
    void apply(const std::vector<LiteMatch> &v) {
        std::vector<uint32_t> which;
        for (const LiteMatch &m : v) {
            if (done) return;
            filter_which(*flt, m.address, nullptr, which);
            bool want = per_pattern == 0 && !which.empty();
            for (uint32_t i : which) want = want || got[i] < per_pattern;
            if (!want) continue;
            for (uint32_t i : which)
                if (++got[i] == per_pattern && per_pattern) unsatisfied--;
            accepted.push_back(m);
            n_accepted.store(accepted.size(), std::memory_order_relaxed);
            if (accepted.size() >= count || (per_pattern && unsatisfied == 0)) done = true;
        }
    }
    bool is_recorded(uint64_t g) const { return g / shards < recorded[g % shards]; }
    void submit(uint64_t g, std::vector<LiteMatch> &&v) {
        std::lock_guard<std::mutex> lk(mu);
        if (arrival) {
            apply(v);
            return;
        }
        pending[g] = std::move(v);
        for (;;) {
            auto it = pending.find(next);
            if (it != pending.end()) {
                apply(it->second);
                pending.erase(it);
            } else if (!is_recorded(next)) {
                break;
            }
            next++;
        }
    }
    // the scan is over: batches still waiting behind a gap (a failed context's that nobody took over) in their order
    void flush() {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : pending) apply(kv.second);
        pending.clear();
    }
};

}  // namespace vg
