// best_ledger.h — which confirmed candidates of a VGEN_SCAN_BEST scan are its results (scanner.cpp).
#pragma once
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#include "filter.h"
#include "scan_match.h"

namespace vg {

// "Report only improvements": shards hand in the confirmed matches of every batch they commit, keyed by the batch's GLOBAL number,
// and the ledger applies the batches in that order (as ListLedger does for a pattern list): a match is a result only if its score is
// strictly higher than the score of every result before it.  The order — batches in order, keys ascending within a batch — does not
// depend on which context finished first, so a seeded or range scan is reproducible.  `best` is what the shards read to raise
// their contexts' threshold (vgen_set_score_min(best + 1)): an optimisation only, the rule is applied here.
struct BestLedger {
    const vgen_filter *flt = nullptr;
    uint64_t count = UINT64_MAX;
    std::mutex mu;
    std::map<uint64_t, std::vector<LiteMatch>> pending;   // committed batches waiting for the ones before them
    uint64_t next = 0;                                    // global batch applied next
    std::vector<LiteMatch> accepted;
    std::atomic<bool> done{false};
    std::atomic<uint64_t> n_accepted{0};
    std::atomic<int64_t> best{-1};                        // score of the last result; -1: none yet
    bool arrival = false;                                 // contexts that walk from bases of their own: no global order to keep

    void init(const vgen_filter *f, uint64_t cnt) {
        flt = f;
        count = cnt;
        done = count == 0;
    }
    uint32_t max_score() const { return score_metric_max(flt->score.t[0].metric); }
    // (under mu)
    void apply(const std::vector<LiteMatch> &v) {
        for (const LiteMatch &m : v) {
            if (done) return;
            uint32_t sc = 0;
            bool ok = false;
            if (!score_of(*flt, m.address, nullptr, &sc, &ok) || !ok || (int64_t)sc <= best.load(std::memory_order_relaxed)) continue;
            best.store(sc, std::memory_order_relaxed);
            accepted.push_back(m);
            n_accepted.store(accepted.size(), std::memory_order_relaxed);
            if (accepted.size() >= count || sc >= max_score()) done = true;   // (nothing scores higher than the metric's range)
        }
    }
    void submit(uint64_t g, std::vector<LiteMatch> &&v) {
        std::lock_guard<std::mutex> lk(mu);
        if (arrival) {
            apply(v);
            return;
        }
        pending[g] = std::move(v);
        for (auto it = pending.find(next); it != pending.end(); it = pending.find(next)) {
            apply(it->second);
            pending.erase(it);
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
