// scanner.cpp — vgen_scan: the host loop of the GPU scan, mirroring scan_gpu_with_runner
// (reference src/gpu.rs:920-1125) above the C ABI.
//
// Same control flow as the reference: pick the base key (config.start, or a random valid scalar —
// gpu.rs:933-945), prime every frame (gpu.rs:973-995), then round-robin: await a frame, immediately
// re-dispatch it with the next batch (gpu.rs:1003-1028), turn that frame's results into matches
// (gpu.rs:1030-1104), add batch_size to the operation count and call the progress callback
// (gpu.rs:1106-1109); stop when `count` matches exist and nothing more was dispatched (gpu.rs:1111).
// Differences, all on the host side of the boundary: candidates arrive pre-filtered by the device and
// are confirmed with the exact DFA (the reference encodes and regex-matches all batch_size hashes on
// rayon); the base key can be seeded; batches can be striped over several contexts (multi-GPU).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../../include/vgen_hip.h"
#include "host/checkpoint.h"
#include "host/encode.h"
#include "host/filter.h"
#include "host/host_pool.h"
#include "host/best_ledger.h"
#include "host/list_ledger.h"
#include "host/scalar.h"
#include "host/scan_match.h"
#include "runtime.h"

// -DVGEN_SCAN_PROFILE (tools/permissive_probe.py, profiles/r04_permissive.txt): seconds the scanning thread spends in vgen_wait, in the
// worker pool's confirmation pass, in the hand-over of the workers' matches and in dispatch calls, printed when a shard ends.
#ifdef VGEN_SCAN_PROFILE
static inline double prof_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define PROF(var, stmt) { const double t_ = prof_now(); stmt; var += prof_now() - t_; }
#else
#define PROF(var, stmt) { stmt; }
#endif

namespace vg {

// k0(seed, shard) = SHA-256("vgen-mi355x" || u64le(seed) || u32le(shard)) mod n, re-drawn if 0
// (BASELINE.md §4).
void seed_key(uint64_t seed, uint32_t shard, Scalar &out) {
    uint32_t redraw = 0;
    for (;;) {
        uint8_t buf[11 + 8 + 4 + 4];
        size_t n = 11;
        memcpy(buf, "vgen-mi355x", 11);
        for (int i = 0; i < 8; i++) buf[n++] = (uint8_t)(seed >> (8 * i));
        for (int i = 0; i < 4; i++) buf[n++] = (uint8_t)(shard >> (8 * i));
        if (redraw)
            for (int i = 0; i < 4; i++) buf[n++] = (uint8_t)(redraw >> (8 * i));
        uint8_t d[32];
        host_sha256(buf, n, d);
        scalar_from_be(out, d);
        if (scalar_cmp_words(out.w, SCALAR_N) >= 0) {
            // digest < 2^256 < 2n: one subtraction reduces it
            int64_t b = 0;
            for (int i = 0; i < 8; i++) {
                int64_t t = (int64_t)out.w[i] - SCALAR_N[i] + b;
                out.w[i] = (uint32_t)t;
                b = t >> 32;
            }
        }
        if (!scalar_is_zero(out)) return;
        redraw++;
    }
}

namespace {

void random_valid_key(Scalar &k) {
    std::random_device rd;
    for (;;) {
        for (int i = 0; i < 8; i++) k.w[i] = rd();
        if (scalar_is_valid(k)) return;   // rejection sampling, gpu.rs:938-944
    }
}

// The seed of a random-key scan (core/rnd.h): the caller's 64-bit one — reproducible runs and tests, NOT for keys that will
// hold value — or, unseeded, 192 bits of OS entropy (every key the mode returns is a function of seed, stream and index:
// the seed is all the secret there is; the reference seeds a 256-bit StdRng from the OS, src/scanner.rs:144).
RndSeed scan_rnd_seed(uint64_t cfg_seed) {
    if (cfg_seed) return rnd_seed_from_u64(cfg_seed);
    std::random_device rd;   // (getrandom / /dev/urandom on this platform)
    RndSeed s;
    for (int i = 0; i < 6; i++) s.w[i] = rd();
    return s;
}

}  // namespace
}  // namespace vg

using namespace vg;

namespace {

// Where a shard (slot of the batch striping) stands: batches committed so far, in dispatch order.  A multi-device scan
// keeps one per slot so that a surviving context can take over the slot of a failed one exactly where it stopped
// (with a checkpoint the ledger's done[] is the same number and wins).
struct SlotProgress {
    std::atomic<uint64_t> done{0};
};

// Where the confirmed matches of one shard go, and with that how much of a batch has to be examined.  Three policies, by
// the optional parts that are set:
//   plain count (neither `ck` nor `ll`): matches are taken while `count` has room — the shard's own count, or the counter the
//       shards of a multi-device scan share — and dropped after that; a batch is examined only as far as there is room.
//   checkpoint (`ck`, this shard being its slot `ck_slot`): every candidate of a batch is examined and the batch is committed with
//       ALL of its matches, also those beyond `count`: the file stays a consistent prefix of the scan whatever count a later run asks for.
//   list ledger (`ll`): every candidate is examined and the ledger decides, in global batch order, which matches are results.
// `slot` (optional): the slot's progress, for a context that takes the slot over after this one failed.
struct ResultSink {
    explicit ResultSink(uint64_t count_, std::atomic<uint64_t> *shared_found_ = nullptr) : count(count_), shared_found(shared_found_) {}

    MatchList matches;                   // what this shard took (a checkpointed vgen_scan starts with the earlier runs' matches)
    Checkpoint *ck = nullptr;
    uint32_t ck_slot = 0;
    SlotProgress *slot = nullptr;
    ListLedger *ll = nullptr;
    BestLedger *best = nullptr;          // VGEN_SCAN_BEST: like a list's ledger, it decides in global batch order what is a result

    // does every candidate of a batch have to be examined?
    bool examine_all() const { return ck != nullptr || ll != nullptr || best != nullptr; }
    uint64_t found() const {
        if (best) return best->n_accepted.load(std::memory_order_relaxed);
        if (ll) return ll->n_accepted.load(std::memory_order_relaxed);
        return shared_found ? shared_found->load(std::memory_order_relaxed) : matches.size();
    }
    // matches `count` still has room for
    uint64_t room() const {
        const uint64_t have = found();
        return have < count ? count - have : 0;
    }
    // is there a reason to examine another candidate of the batch in hand?
    bool wants_more() const { return examine_all() || room() > 0; }
    // the scan has what it was asked for (a pattern-list scan: when its ledger says so — every pattern has its matches, or `count`)
    bool done() const { return best ? best->done.load(std::memory_order_relaxed) : ll ? ll->done.load(std::memory_order_relaxed) : found() >= count; }
    // batches of this slot that are finished already: recorded in the checkpoint, or committed by the context that owned
    // the slot before it failed; and those of them that count against max_batches (the slot's budget; a checkpoint's is per call)
    uint64_t batches_done() const { return ck ? ck->done[ck_slot] : slot ? slot->done.load() : 0; }
    uint64_t batches_taken_over() const { return slot && !ck ? slot->done.load() : 0; }

    // A confirmed match: into the result while `count` has room (a list's results are the ledger's business), and into the
    // batch's record when there is one.
    void add(const LiteMatch &g) {
        if (examine_all()) batch.push_back(g);
        if (ll || best || room() == 0) return;
        matches.push_back(g);
        taken_uncommitted++;
        if (shared_found) shared_found->fetch_add(1, std::memory_order_relaxed);
    }
    // The workers' confirmed matches of one batch (index order: part 0, part 1, ...), handed over in bulk.  Returns true when
    // some were dropped.
    bool add_parts(std::vector<std::vector<LiteMatch>> &part) {
        size_t total = 0;
        for (auto &p : part) total += p.size();
        size_t take = ll || best ? 0 : (size_t)std::min<uint64_t>(total, room());
        const size_t taken = take;
        for (auto &p : part) {
            if (examine_all()) batch.insert(batch.end(), p.begin(), p.end());
            const size_t k = std::min(take, p.size());
            matches.take(std::move(p), k);     // the worker's vector itself becomes a block of the result: nothing is copied
            take -= k;
        }
        taken_uncommitted += taken;
        if (shared_found && taken) shared_found->fetch_add(taken, std::memory_order_relaxed);
        return taken < total && !examine_all();
    }
    // The batch in hand is finished: global batch `batch_no` of the scan, `tested` keys.
    void commit(uint64_t batch_no, uint64_t tested) {
        if (ck) ck->commit(ck_slot, batch, tested);
        if (ll) ll->submit(batch_no, std::move(batch));
        if (best) best->submit(batch_no, std::move(batch));
        batch.clear();
        if (slot) slot->done.fetch_add(1);
        taken_uncommitted = 0;
    }
    // A scan that fails between examining a batch and committing it (in dump mode the host filter runs BEFORE the frame is
    // dispatched again, and that dispatch is where a dead device shows) must not keep that batch's matches: the batch is not
    // counted as done, so whoever resumes or takes over the slot will produce them again.
    void rollback() {
        matches.truncate(matches.size() - (size_t)taken_uncommitted);
        if (shared_found) shared_found->fetch_sub(taken_uncommitted, std::memory_order_relaxed);
        taken_uncommitted = 0;
    }

private:
    uint64_t count;
    std::atomic<uint64_t> *shared_found;
    std::vector<LiteMatch> batch;                // checkpoint / list: every confirmed match of the batch in hand (the commit unit)
    uint64_t taken_uncommitted = 0;              // matches taken from the batch in hand, not yet committed
};

// What one shard is asked to do, and what it reports back.
struct ScanJob {
    const vgen_scan_config *cfg = nullptr;
    vgen_progress_cb cb = nullptr;
    void *user = nullptr;
    const volatile int32_t *stop = nullptr;
    std::atomic<uint64_t> *shared_ops = nullptr;   // multi-device: the wrapper's callback adds each batch to it, so `cb` gets the batch's keys
    const RndSeed *scan_seed = nullptr;            // random keys: the seed of the whole scan when the caller resolved one
    uint64_t operations = 0;                       // out: keys tested by this call
    bool range_done = false;                       // out: the shard stopped because its range ran out
};

// The candidates of one dispatch as the confirmation pass sees them — the payloads of a dump (candidate i is key index i)
// or the records of the match ring — with what turns one into a match.
struct Candidates {
    const vgen_filter &flt;
    uint32_t format;
    const BatchKeys &keys;
    const Scalar *end;
    uint32_t batch, images;
    const uint8_t *dump;        // payload of index i at dump + i * stride, or
    size_t stride;
    const vgen_match *recs;     // records (index, payload)

    // Confirms candidates lo .. hi-1 in order, as long as more() says so, and hands every match to take().  Returns the
    // first candidate it did not examine.
    template <class More, class Take>
    uint32_t confirm(uint32_t lo, uint32_t hi, More more, Take take) const {
        LiteMatch g;
        for (; lo < hi && more(); lo++) {
            const bool ok = recs ? make_match(flt, format, keys, recs[lo].index, recs[lo].payload, end, g, batch, images)
                                 : make_match(flt, format, keys, lo, dump + (size_t)lo * stride, end, g, batch, images);
            if (ok) take(g);
        }
        return lo;
    }
    void confirm_into(uint32_t lo, uint32_t hi, std::vector<LiteMatch> &out) const {
        confirm(lo, hi, []() { return true; }, [&out](const LiteMatch &g) { out.push_back(g); });
    }
};

// One shard of a scan on one context: what to scan in `job`, where the matches go in `sink`.
int scan_shard(vgen_ctx *ctx, const vgen_filter &flt, ScanJob &job, ResultSink &sink) {
    const vgen_scan_config *cfg = job.cfg;
    if (cfg->format != ctx->format) return ctx->fail(VGEN_E_INVALID, "scan format differs from the context's format");
    const bool random_keys = (cfg->flags & VGEN_SCAN_RANDOM_KEYS) != 0;
    if (ctx->endo && !random_keys && (cfg->has_start || cfg->has_end || cfg->seed || cfg->n_shards > 1 || cfg->checkpoint_path))
        return ctx->fail(VGEN_E_INVALID, "a VGEN_FLAG_ENDO context tests six images of every point (three for x-only keys), not a contiguous key range: "
                                         "it serves unseeded random scans only (no start / end / seed / shards / checkpoint)");
    // (random keys on an endomorphism context: six keys per draw — the candidate and its lambda / negation images; seeds and
    //  shards keep their meaning there, they name streams of candidates, not ranges)
    if (random_keys && (cfg->has_start || cfg->has_end))
        return ctx->fail(VGEN_E_INVALID, "VGEN_SCAN_RANDOM_KEYS draws an independent key per candidate: no start / end");
    if (random_keys && sink.ck && !job.scan_seed) return ctx->fail(VGEN_E_INVALID, "a checkpointed random-key scan needs its seed (open_checkpoint sets it)");

    const uint32_t N = ctx->batch;
    const size_t pbytes = (size_t)ctx->payload_words * 4;
    const uint32_t shards = cfg->n_shards > 1 ? cfg->n_shards : 1;
    const uint32_t shard = cfg->n_shards > 1 ? cfg->shard : 0;
    if (shard >= shards) return ctx->fail(VGEN_E_INVALID, "shard >= n_shards");

    // Device filter or host filtering of full dumps.  A prefilter whose expected candidates per batch do not fit the
    // match ring does not fall back to the reference's mode (every hash to the host): the ring GROWS to four times
    // the expectation, as long as that stays below half a record per key (beyond that nearly every key is a match
    // and the 20 B/key dump is the cheaper transfer).  A DEVF_DFA filter has no selectivity estimate: it starts on
    // the device with the ring it finds and adapts on overflow (below).
    auto next_pow2 = [](uint64_t v) {
        uint64_t p = 256;
        while (p < v) p <<= 1;
        return p;
    };
    bool host_all = flt.dev.kind == DEVF_HOST_ALL;
    const double keys_per_dispatch = (double)N * rt_images(ctx);
    if (!host_all && flt.selectivity >= 0 && flt.selectivity * keys_per_dispatch * 4 > (double)ctx->match_cap) {
        const uint64_t want = next_pow2((uint64_t)(flt.selectivity * keys_per_dispatch * 4));
        if (want <= N / 2) {
            int rc = vgen_set_match_cap(ctx, (uint32_t)want);
            if (rc != VGEN_OK) return rc;
        } else {
            host_all = true;
        }
    }
    int rc = vgen_set_filter(ctx, host_all ? nullptr : &flt);
    if (rc != VGEN_OK) return rc;
    // VGEN_SCAN_BEST: the device's threshold follows the best score so far (a context that joins or takes a slot over starts from it).
    // An optimisation only: the ledger applies the rule, and dispatches in flight under an older threshold deliver extras it discards.
    int64_t best_sent = -1;
    auto follow_best = [&]() {
        if (!sink.best || host_all || !ctx->have_filter) return;
        const int64_t b = sink.best->best.load(std::memory_order_relaxed);
        if (b <= best_sent || b + 1 > (int64_t)sink.best->max_score() || (uint32_t)(b + 1) <= flt.score.t[0].min) return;
        if (vgen_set_score_min(ctx, (uint32_t)(b + 1)) == VGEN_OK) best_sent = b;
    };
    follow_best();

    // Scans that multiply a scalar per key (random keys, taproot): how wide a generator table is this scan worth?  The default
    // 24-bit table (10 additions per multiplication) is there in 30 ms; the 27-bit signed one (9 additions, +5 %) in 60 ms and
    // 21.5 GB; the 29-bit signed one (8 additions, +12.5 %) takes 0.7 - 2.3 s and 138 of the device's 288 GB (profiles/r04_gtab_signed.txt):
    // from 3 s of expected scanning the first pays for itself several times over, from 30 s the second.
    // From the keys the scan can expect to test — the range, max_batches, or count / the filter's selectivity — at the path's rate.
    // This is a PREFERENCE: the caller bounds it (cfg->table_bits_max, vgen_params.table_bits / device_mem_budget_bytes), the runtime
    // checks it against the device's free memory, builds the wider table in the background while this loop dispatches on the one
    // it has, and takes it into use when it is complete (runtime.cpp) — the scan never waits for a table.
    if ((random_keys || ctx->format == VGF_P2TR) && !vgf_is_ed((int)ctx->format)) {   // (a Solana or onion context has no generator table to widen)
        // (a count-limited scan whose pattern has no selectivity estimate — the whole DFA on the device — is taken for short)
        double keys = cfg->count == UINT64_MAX ? 1e30 : 0.0;
        if (!host_all && flt.selectivity > 0 && cfg->count != UINT64_MAX) keys = (double)cfg->count / flt.selectivity;
        if (host_all && cfg->count != UINT64_MAX) keys = (double)cfg->count * 64.0;   // (nearly every key matches)
        if (cfg->max_batches) keys = std::min(keys, (double)cfg->max_batches * keys_per_dispatch);
        if (cfg->has_end && cfg->has_start) {
            Scalar a, b;
            scalar_from_be(a, cfg->start);
            scalar_from_be(b, cfg->end);
            bool small = true;     // the range fits 64 bits of distance?
            for (int i = 2; i < 8; i++) small = small && a.w[i] == b.w[i];
            if (small) {
                const uint64_t lo = (uint64_t)a.w[1] << 32 | a.w[0], hi = (uint64_t)b.w[1] << 32 | b.w[0];
                if (hi >= lo) keys = std::min(keys, (double)(hi - lo) + 1.0);
            }
        }
        const double seconds = keys / (random_keys && ctx->endo ? 5.5e9 : 1.35e9) / (double)shards;
        rt_prefer_table_bits(ctx, seconds >= 30.0 ? 29u : seconds >= 3.0 ? 27u : 0u, cfg->table_bits_max);
    }

    // independent random keys: candidate index = batch number x N within stream `shard` of the seed
    // (the seed of the whole scan when the caller resolved one — all shards of a multi-device scan and a resumed checkpoint
    //  share it —, else this call's own)
    const RndSeed rnd_seed = !random_keys ? RndSeed{} : job.scan_seed ? *job.scan_seed : scan_rnd_seed(cfg->seed);
    Scalar current;
    if (random_keys) {
        memset(&current, 0, sizeof current);
        current.w[0] = 1;   // (unused: keeps the range bookkeeping below on valid ground)
    } else if (cfg->has_start) {
        scalar_from_be(current, cfg->start);
    } else if (cfg->seed) {
        seed_key(cfg->seed, 0, current);   // one base; shards stripe it (deterministic multi-GPU)
    } else {
        random_valid_key(current);
    }
    if (!scalar_is_valid(current)) return ctx->fail(VGEN_E_RANGE, "start key is not a valid secp256k1 scalar");
    Scalar end_key;
    const Scalar *end = nullptr;
    if (cfg->has_end) {
        scalar_from_be(end_key, cfg->end);
        end = &end_key;
    }
    // batch striping: this context takes global batches shard, shard + shards, ...
    bool exhausted = false;
    if (shard && !random_keys) exhausted = scalar_add_u64(current, current, (uint64_t)shard * N) || !scalar_is_valid(current);
    const uint64_t stride = (uint64_t)shards * N;
    // resume / take-over: this shard's first `skipped` batches are already in the checkpoint, or were committed by the
    // context that owned the slot before it failed
    const uint64_t skipped = sink.batches_done();
    const uint64_t taken_over = sink.batches_taken_over();   // counts against max_batches: the slot's budget, not the context's
    if (skipped && !exhausted && !random_keys) {
        uint64_t skip = skipped;
        while (skip && !exhausted) {
            const uint64_t step = std::min<uint64_t>(skip, UINT64_MAX / stride);
            exhausted = scalar_add_u64(current, current, step * stride) || !scalar_is_valid(current);
            skip -= step;
        }
    }

    uint64_t dispatched = 0;
    uint64_t total_ops = 0;
    // frames this scan drives: all of them, or — filtering full dumps on the host — those that have a dump buffer
    // (runtime.cpp: ensure_dump_slab bounds the pinned memory; the host filter is the bottleneck there anyway)
    uint32_t nf = ctx->frames;
    if (host_all && ctx->dump_frames) nf = std::min(nf, ctx->dump_frames);
    std::vector<BatchKeys> pend(ctx->frames);
    uint32_t in_flight = 0;
    int status = VGEN_OK;

    // (the host's stop flag is written by another thread: an atomic read, src/gpu.rs:980-984 reads its AtomicBool Relaxed)
    auto stopped = [&]() { return job.stop && __atomic_load_n(const_cast<const int32_t *>(job.stop), __ATOMIC_RELAXED) != 0; };
    auto in_range = [&]() { return !exhausted && (!end || scalar_cmp(current, *end) <= 0); };
    auto can_dispatch = [&]() { return in_range() && (!cfg->max_batches || dispatched + taken_over < cfg->max_batches); };
    // a batch dispatched under a base point: its candidates are re-derived from that point (make_match) and yield partial keys
    auto mark_split = [&](BatchKeys &bk) {
        if (!ctx->have_base) return;
        bk.base = &ctx->base_pt;
        bk.dropped = &ctx->split_dropped;
    };
    auto dispatch = [&](uint32_t frame) -> int {
        if (random_keys) {
            // every shard owns a stream of its own and walks its candidates in order (the oracle's worker thread, oracle/vo_scan.c)
            const uint64_t batch_no = skipped + dispatched;
            const uint64_t first = batch_no * (uint64_t)N;
            if (first / N != batch_no || first > UINT64_MAX - (N - 1)) {
                exhausted = true;
                return ctx->fail(VGEN_E_RANGE, "random-key stream exhausted (2^64 candidates)");
            }
            uint8_t sb[24];
            rnd_seed_to_bytes(rnd_seed, sb);
            int r;
            if (ctx->format == VGF_ONION) {   // the walk: batch b of shard s is candidates b N .. of the base scalar of stream s
                uint8_t base[32];
                onion_base(rnd_seed, shard, base);
                r = vgen_dispatch_onion(ctx, frame, base, first);   // (VGEN_E_RANGE, probability ~2^-187, ends the scan)
            } else {
                r = vgen_dispatch_random_seed(ctx, frame, sb, shard, first);
            }
            if (r != VGEN_OK) return r;
            pend[frame] = BatchKeys{};
            pend[frame].batch_no = batch_no;
            pend[frame].random = true;
            pend[frame].seed = rnd_seed;
            pend[frame].stream = shard;
            pend[frame].first_index = first;
            mark_split(pend[frame]);
            dispatched++;
            return VGEN_OK;
        }
        uint8_t kb[32];
        scalar_to_be(current, kb);
        int r = vgen_dispatch(ctx, frame, kb);
        if (r != VGEN_OK) return r;
        pend[frame] = BatchKeys{};
        pend[frame].batch_no = skipped + dispatched;
        pend[frame].start = current;
        mark_split(pend[frame]);
        dispatched++;
        Scalar nx;
        if (scalar_add_u64(nx, current, stride) || !scalar_is_valid(nx)) exhausted = true;   // key space exhausted
        else current = nx;
        return VGEN_OK;
    };

    // Frames in flight, in dispatch order (results are consumed in that order, so matches stay in ascending batch
    // order).  The scan starts with two frames and activates one more per completed batch: with all frames primed
    // at once the first result would wait for its share of a device busy with sixteen dispatches (2.3 ms to the
    // first match instead of ~0.3 ms); a long scan reaches the full depth after `frames` batches.
    std::deque<uint32_t> order;
    uint32_t active = 0;   // frames 0 .. active-1 have been put to use
    auto launch = [&](uint32_t f) -> bool {
        if ((status = dispatch(f)) != VGEN_OK) return false;
        order.push_back(f);
        in_flight++;
        return true;
    };
    // A scan of the scalar-multiplication paths that turns out LONG although nothing said so up front (no selectivity estimate, a
    // count that keeps not being reached): after 5 s it asks for the 29-bit signed table (+12.5 % once it is there) and simply goes
    // on — the runtime builds it behind the dispatches (round 4 drained the frames and paused 0.7 - 2.3 s here).
    const bool table_path = (random_keys || ctx->format == VGF_P2TR) && !vgf_is_ed((int)ctx->format);
    const auto scan_t0 = std::chrono::steady_clock::now();
    bool upgrade_asked = false;
    auto may_launch = [&]() { return can_dispatch() && !stopped() && !sink.done(); };
    // (a frame's stream — a hardware queue of its own — is created at its first dispatch and takes ~8 ms: a fresh context
    // starts on frame 0 alone, so that an easy pattern's first match does not wait for a second queue it never needs)
    auto prime = [&]() {
        while (active < std::min<uint32_t>(nf, 2) && may_launch()) {
            if (active >= 1 && !rt_frame_ready(ctx, active)) break;
            if (!launch(active++)) break;
        }
    };
    prime();

    std::vector<vgen_match> recs(ctx->match_cap);   // (after the ring has its size for this scan)
    std::unique_ptr<HostFilterPool> pool;   // created with the first dumped batch / the first batch with thousands of candidates
    bool cut_any = false;      // (no checkpoint) some batch had matches beyond `count` dropped: the range was not covered

#ifdef VGEN_SCAN_PROFILE
    double prof_wait = 0, prof_pool = 0, prof_merge = 0, prof_dispatch = 0;
    uint64_t prof_cand = 0;
#endif
    while (status == VGEN_OK && !order.empty()) {
        const uint32_t frame = order.front();
        order.pop_front();
        uint32_t n_found = 0;
        uint64_t tested = 0;
        PROF(prof_wait, status = vgen_wait(ctx, frame, recs.data(), (uint32_t)recs.size(), &n_found, &tested));
        if (status != VGEN_OK) break;
        in_flight--;
        const BatchKeys batch_start = pend[frame];
        const bool dumped = ctx->fr[frame].dumped;
        const uint32_t images = tested > N ? (uint32_t)(tested / N) : 1;   // 6 for an endomorphism dispatch
        bool cut = false;      // this batch: a confirmed (or unexamined) match was dropped because `count` was reached

        if (dumped) {
            // Host filtering of the whole batch (the reference's only mode, gpu.rs:1030-1093) straight from the
            // pinned buffer the dispatch copied itself into — hence BEFORE the frame is dispatched again —, in
            // parallel index ranges, results kept in ascending index order.  The device is not the bottleneck
            // here (encoding and matching 2^20 addresses takes the host tens of milliseconds).
            const uint8_t *dump = nullptr;
            if ((status = vgen_dump_view(ctx, frame, &dump, nullptr)) != VGEN_OK) break;
            // A scan that wants few matches of a pattern nearly every key satisfies (the reference's default `range
            // --puzzle N`: pattern ".", count 1, src/lib.rs:519) must not encode a million addresses to return the first:
            // the dump is examined in index order in growing pieces — a first short one on this thread — until `count` is
            // reached; what is left unexamined counts as cut.  With a checkpoint the whole batch is examined (a committed
            // batch is recorded with every match it holds).
            const uint32_t total = (uint32_t)tested;   // N, or 6 N for an endomorphism dispatch
            const Candidates cand{flt, cfg->format, batch_start, end, N, images, dump, pbytes, nullptr};
            uint32_t pos = 0;
            for (unsigned round = 0; pos < total && sink.wants_more(); round++) {
                const uint64_t need = sink.examine_all() ? total : sink.room();
                uint64_t len = total - pos;
                if (!sink.examine_all() && need < total / 8) len = std::min<uint64_t>(len, std::max<uint64_t>(need * 4, 64) << std::min(2 * round, 24u));
                if (len < 1024) {
                    pos = cand.confirm(pos, pos + (uint32_t)len, [&]() { return sink.wants_more(); }, [&](const LiteMatch &g) { sink.add(g); });
                    continue;
                }
                if (!pool) pool.reset(new HostFilterPool(host_threads()));
                const unsigned nt = pool->size();
                std::vector<std::vector<LiteMatch>> part(nt);
                const uint32_t base = pos, span = (uint32_t)len;
                pool->run([&](unsigned t) {
                    cand.confirm_into(base + (uint32_t)((uint64_t)span * t / nt), base + (uint32_t)((uint64_t)span * (t + 1) / nt), part[t]);
                });
                if (sink.add_parts(part)) cut = true;
                pos += span;
            }
            if (pos < total) cut = true;   // keys left unexamined (conservative: they may not all be matches)
        }

        bool dispatched_next = false;
        bool ramp_later = false;
        if (may_launch()) {
            bool ok_launch = true;
            PROF(prof_dispatch, ok_launch = launch(frame));
            if (!ok_launch) break;
            dispatched_next = true;
            // ramp up: one more frame per batch — at once when its stream exists; frames that still need their stream
            // (a hardware queue, ~8 ms to create) join as a helper thread gets the streams made, which is asked for
            // after this batch's candidates have been examined and only if the scan goes on
            if (active < nf && may_launch()) {
                if (!rt_frame_ready(ctx, active)) ramp_later = true;
                else if (!launch(active++)) break;
            }
        }

        if (!dumped) {
            if (n_found > recs.size()) {
                // More candidates than the ring holds (a permissive pattern): nothing may be dropped, so drain
                // what is in flight, grow the ring (x4, at least twice what this batch produced) — or, once a ring
                // would need more than half a record per key, switch to host filtering of full dumps, the
                // reference's mode — and redo from this batch.
                for (uint32_t f = 0; f < ctx->frames; f++)
                    if (ctx->fr[f].in_flight) (void)vgen_wait(ctx, f, nullptr, 0, nullptr, nullptr);
                const uint64_t want = next_pow2(std::max<uint64_t>((uint64_t)recs.size() * 4, (uint64_t)n_found * 2));
                if (want <= N / 2) {
                    if ((status = vgen_set_match_cap(ctx, (uint32_t)want)) != VGEN_OK) break;
                    recs.resize(ctx->match_cap);
                } else if ((status = vgen_set_filter(ctx, nullptr)) != VGEN_OK) {
                    break;
                } else if (ctx->dump_frames) {
                    nf = std::min(nf, ctx->dump_frames);
                }
                dispatched -= 1 + in_flight;
                in_flight = 0;
                order.clear();
                active = 0;
                if (!random_keys) current = batch_start.start;
                exhausted = false;
                prime();
                continue;
            }
            const Candidates cand{flt, cfg->format, batch_start, end, N, images, nullptr, 0, recs.data()};
            if (n_found >= 2048) {
                // many candidates (a permissive pattern on a grown ring): confirm them on the worker pool, in index order
                if (!pool) pool.reset(new HostFilterPool(host_threads()));
                const unsigned nt = pool->size();
                std::vector<std::vector<LiteMatch>> part(nt);
                PROF(prof_pool, pool->run([&](unsigned t) {
                    cand.confirm_into((uint32_t)((uint64_t)n_found * t / nt), (uint32_t)((uint64_t)n_found * (t + 1) / nt), part[t]);
                }));
                PROF(prof_merge, if (sink.add_parts(part)) cut = true;);
#ifdef VGEN_SCAN_PROFILE
                prof_cand += n_found;
#endif
            } else {
                // candidates left unexamined count as cut (conservative: they may not all be matches)
                cut = cand.confirm(0, n_found, [&]() { return sink.wants_more(); }, [&](const LiteMatch &g) { sink.add(g); }) < n_found;
            }
        }

        total_ops += tested;                         // gpu.rs:1106 (batch_size; six times that for an endomorphism dispatch)
        cut_any = cut_any || cut;
        sink.commit(batch_start.batch_no * shards + shard, tested);
        follow_best();
        if (job.cb) job.cb(job.shared_ops ? tested : total_ops, job.user);   // multi-device: the wrapper adds N to the shared count under its lock
        if (sink.done() && !dispatched_next) break;   // gpu.rs:1111
        if (table_path && !upgrade_asked && std::chrono::duration<double>(std::chrono::steady_clock::now() - scan_t0).count() >= 5.0) {
            rt_prefer_table_bits(ctx, 29, cfg->table_bits_max);   // taken into use when it is complete; nothing waits
            upgrade_asked = true;
        }
        if (ramp_later && active < nf && may_launch()) {
            // not ready and no helper for this stream kind: create it here and now, as before
            if (!rt_frame_ready(ctx, active) && rt_prepare_streams(ctx)) continue;
            if (!launch(active++)) break;
        }
    }
#ifdef VGEN_SCAN_PROFILE
    fprintf(stderr, "[scan profile] wait %.3f s  pool %.3f s  merge %.3f s  dispatch %.3f s  candidates %llu  matches %zu  ops %llu\n", prof_wait, prof_pool,
            prof_merge, prof_dispatch, (unsigned long long)prof_cand, sink.matches.size(), (unsigned long long)total_ops);
#endif
    if (status != VGEN_OK) sink.rollback();   // the batch in hand was not committed
    // drain anything still in flight (the reference drops its runner; we must not leave frames busy)
    const bool all_processed = order.empty() && !cut_any;   // no dispatched batch was left unread or cut short
    for (uint32_t f = 0; f < ctx->frames; f++)
        if (ctx->fr[f].in_flight) (void)vgen_wait(ctx, f, nullptr, 0, nullptr, nullptr);
    job.operations = total_ops;
    job.range_done = status == VGEN_OK && !in_range() && all_processed;
    return status;
}

// The base key of a scan without config.start: seeded or drawn from OS entropy.
void resolve_base(vgen_scan_config &c) {
    if (c.has_start) return;
    Scalar k;
    if (c.seed) seed_key(c.seed, 0, k);
    else random_valid_key(k);
    scalar_to_be(k, c.start);
    c.has_start = 1;
}

// Sets up the checkpoint of a scan over `slots` shards starting at shard `first_shard`; resumes from the
// file when there is one (adopting its base key for an unseeded random scan).  VGEN_OK / error.
int open_checkpoint(vgen_ctx *ctx, Checkpoint &ck, const char *pattern, vgen_scan_config &c, uint32_t batch, uint32_t n_shards,
                    uint32_t first_shard, uint32_t slots, RndSeed &rnd_seed) {
    const bool random_keys = (c.flags & VGEN_SCAN_RANDOM_KEYS) != 0;
    const bool pin_base = c.has_start || c.seed;
    if (random_keys) {
        // the scan is named by its seed (OS entropy when the caller gave none: the file then carries it to the next run);
        // `done` counts the batches of each stream
        rnd_seed = scan_rnd_seed(c.seed);
        memset(c.start, 0, 32);
        rnd_seed_to_bytes(rnd_seed, c.start + 8);
    } else {
        resolve_base(c);
    }
    ck.random = random_keys;
    ck.path = c.checkpoint_path;
    ck.pattern = pattern;
    ck.ci = c.case_insensitive != 0;
    ck.format = c.format;
    ck.batch = batch;
    ck.n_shards = n_shards;
    ck.first_shard = first_shard;
    memcpy(ck.base, c.start, 32);
    ck.has_end = c.has_end != 0;
    if (ck.has_end) memcpy(ck.end, c.end, 32);
    if (c.checkpoint_interval_ms) ck.interval_s = c.checkpoint_interval_ms / 1000.0;
    ck.done.assign(slots, 0);
    const int r = ck.load(pin_base);
    if (r < 0) return ctx->fail(VGEN_E_INVALID, ck.error);
    memcpy(c.start, ck.base, 32);
    if (random_keys) {   // (the file's seed when the caller gave none)
        rnd_seed = rnd_seed_from_bytes(ck.base + 8);
        memset(c.start, 0, 32);
    }
    return VGEN_OK;
}

// Hands the matches to the caller as GeneratedAddress records: this is where WIF and hex are rendered — for the matches that
// survived `count`, straight into the result array, on several threads when there are thousands.
// (`partial`: a split-key scan's keys are partial keys and are rendered as such, render_match)
int finish_result(vgen_ctx *ctx, uint32_t format, const MatchList &matches, uint64_t ops, double secs, vgen_scan_result *out, bool partial = false) {
    out->n_matches = matches.size();
    out->operations = ops;
    if (!matches.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        out->matches = (vgen_generated *)malloc(matches.size() * sizeof(vgen_generated));
        if (!out->matches) return ctx->fail(VGEN_E_NOMEM, "out of memory");
        const size_t n = matches.size();
        const unsigned nt = n >= 4096 ? host_threads() : 1;
        const auto &blocks = matches.blocks();
        auto work = [&](unsigned t) {
            // entries [lo, hi) of the list, walked block by block
            const size_t lo = n * t / nt, hi = n * (t + 1) / nt;
            size_t base = 0;
            for (auto &b : blocks) {
                const size_t from = std::max(lo, base), to = std::min(hi, base + b.size());
                for (size_t i = from; i < to; i++) render_match(format, b[i - base], out->matches[i], partial);
                base += b.size();
                if (base >= hi) break;
            }
        };
        if (nt == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
            work(0);
            for (auto &x : th) x.join();
        }
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();   // rendering is part of the scan's time
    }
    out->elapsed_secs = secs;
    return VGEN_OK;
}

}  // namespace

// The key-walking scans do not serve a CREATE2 context or configuration: its candidates are salts.
static int refuse_create2(vgen_ctx *ctx, const char *what) {
    return ctx->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": the ethereum-create2 format is searched by salt - use vgen_scan_create2");
}
static bool any_create2(vgen_ctx **ctxs, uint32_t n_ctx, const vgen_scan_config &cfg) {
    bool any = cfg.format == VGF_ETHEREUM_CREATE2;
    for (uint32_t i = 0; i < n_ctx; i++) any = any || ctxs[i]->format == VGF_ETHEREUM_CREATE2;
    return any;
}

// Solana scans (VGF_SOLANA, context or configuration): a seed has no neighbour, so the scan IS the random-key loop - the flag is implied -
// and there is no range to start or end; checkpoints are not provided yet.  VGEN_OK, or the refusal.
static int solana_scan_rules(vgen_ctx **ctxs, uint32_t n_ctx, vgen_scan_config &c, const char *what) {
    bool any = c.format == VGF_SOLANA;
    for (uint32_t i = 0; i < n_ctx; i++) any = any || ctxs[i]->format == VGF_SOLANA;
    if (!any) return VGEN_OK;
    vgen_ctx *c0 = ctxs[0];
    // (all or none: the flag below must not reach a context of another format, nor a Solana context a scan of another)
    for (uint32_t i = 0; i < n_ctx; i++)
        if (ctxs[i]->format != VGF_SOLANA || c.format != VGF_SOLANA)
            return c0->fail(VGEN_E_INVALID, std::string(what) + ": a solana scan needs the solana format (12) in the configuration and on every context");
    if (c.has_start || c.has_end)
        return c0->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": a solana key is a seed and its scalar a hash of it - there is no key range (has_start / has_end)");
    if (c.checkpoint_path) return c0->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": checkpoints are not provided for the solana format");
    c.flags |= VGEN_SCAN_RANDOM_KEYS;
    return VGEN_OK;
}

// Onion scans (VGF_ONION, context or configuration): every shard walks a + 8 i from the base scalar of its own stream of the seed, so
// the scan runs the stream loop (the flag is implied: a batch is named by stream and first index, not by a secp256k1 start key); a
// key range and checkpoints are not provided.  VGEN_OK, or the refusal.
static int onion_scan_rules(vgen_ctx **ctxs, uint32_t n_ctx, vgen_scan_config &c, const char *what) {
    bool any = c.format == VGF_ONION;
    for (uint32_t i = 0; i < n_ctx; i++) any = any || ctxs[i]->format == VGF_ONION;
    if (!any) return VGEN_OK;
    vgen_ctx *c0 = ctxs[0];
    for (uint32_t i = 0; i < n_ctx; i++)
        if (ctxs[i]->format != VGF_ONION || c.format != VGF_ONION)
            return c0->fail(VGEN_E_INVALID, std::string(what) + ": an onion scan needs the onion format (13) in the configuration and on every context");
    if (c.has_start || c.has_end)
        return c0->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": an onion scan walks from the base scalar of its seed - there is no key range (has_start / has_end)");
    if (c.checkpoint_path) return c0->fail(VGEN_E_UNSUPPORTED, std::string(what) + ": checkpoints are not provided for the onion format");
    c.flags |= VGEN_SCAN_RANDOM_KEYS;
    return VGEN_OK;
}

// ABI 4's vgen_scan_config, or ABI 3's 136 bytes (no table_bits_max: no cap): -> the full structure, fields beyond the caller's zero.
static bool normalise_scan_config(const vgen_scan_config *in, vgen_scan_config &full) {
    constexpr uint32_t CONFIG_ABI3 = 136;
    if (!in || (in->struct_size != sizeof(vgen_scan_config) && in->struct_size != CONFIG_ABI3)) return false;
    memset(&full, 0, sizeof full);
    memcpy(&full, in, in->struct_size);
    full.struct_size = sizeof full;
    return true;
}

// VGEN_SCAN_BEST is for score specifications, and not for checkpointed scans (the rule needs the scores of everything reported before).
static int check_best(vgen_ctx *ctx, const vgen_scan_config &c, const vgen_filter &flt) {
    if (!(c.flags & VGEN_SCAN_BEST)) return VGEN_OK;
    if (flt.score.n == 0) return ctx->fail(VGEN_E_INVALID, "the scan flag `best` (vgen_scan_config.flags = 2) needs a score specification ('score:...') as the pattern");
    if (c.checkpoint_path) return ctx->fail(VGEN_E_UNSUPPORTED, "the scan flag `best` (vgen_scan_config.flags = 2) together with checkpoint_path is not supported: a resumed scan would not know the scores reported before");
    return VGEN_OK;
}

// Split-key scans (contexts with a base point, vgen_set_base_point): one base for all contexts of the scan, and none of what stores
// keys and re-derives addresses from them - a partial key alone derives nothing.  *split receives whether the scan is one.
static int check_split(vgen_ctx **ctxs, uint32_t n_ctx, const vgen_scan_config &c, bool list, bool *split) {
    bool any = false;
    for (uint32_t i = 0; i < n_ctx; i++) any = any || ctxs[i]->have_base;
    *split = any;
    if (!any) return VGEN_OK;
    vgen_ctx *c0 = ctxs[0];
    for (uint32_t i = 0; i < n_ctx; i++)
        if (!ctxs[i]->have_base || !fe_equal_canonical(ctxs[i]->base_pt.x, c0->base_pt.x) || !fe_equal_canonical(ctxs[i]->base_pt.y, c0->base_pt.y))
            return c0->fail(VGEN_E_INVALID, "split-key scan: all contexts must have the same base point (vgen_set_base_point)");
    if (list) return c0->fail(VGEN_E_UNSUPPORTED, "vgen_scan_list is not supported on contexts with a base point (split-key): lists work per dispatch there");
    if (c.checkpoint_path)
        return c0->fail(VGEN_E_UNSUPPORTED, "checkpoint_path is not supported on contexts with a base point (split-key): a checkpoint stores keys and "
                                            "re-derives addresses from them, and a partial key derives nothing");
    if (c.has_end) return c0->fail(VGEN_E_UNSUPPORTED, "key ranges (has_end) are not supported on contexts with a base point (split-key)");
    return VGEN_OK;
}

extern "C" int vgen_scan(vgen_ctx *ctx, const char *pattern, const vgen_scan_config *cfg_in, vgen_progress_cb cb,
                         void *user, const volatile int32_t *stop, vgen_scan_result *out) {
    vgen_scan_config c;   // (a checkpoint may give it the file's base key)
    if (!ctx || !pattern || !out || !normalise_scan_config(cfg_in, c)) return VGEN_E_INVALID;
    memset(out, 0, sizeof *out);
    if (ctx->format == VGF_ETHEREUM_CREATE2 || c.format == VGF_ETHEREUM_CREATE2) return refuse_create2(ctx, "vgen_scan");
    if (int rc = solana_scan_rules(&ctx, 1, c, "vgen_scan")) return rc;
    if (int rc = onion_scan_rules(&ctx, 1, c, "vgen_scan")) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    vgen_filter flt;
    std::string err;
    if (score_spec_unsupported(pattern, c.format)) return ctx->fail(VGEN_E_UNSUPPORTED, SCORE_FORMATS_MESSAGE);
    if (!filter_compile(pattern, c.case_insensitive != 0, c.format, flt, err))
        return ctx->fail(VGEN_E_PATTERN, err);
    // One flow, with or without a checkpoint.  With one, what earlier runs found counts towards `count` (committed batches keep
    // all their matches), and nothing is dispatched when the file says the scan is complete or already holds `count` matches.
    // While the shard runs, its matches stay the first `count` of the checkpoint's record: they serve every way out.
    if (int rc = check_best(ctx, c, flt)) return rc;
    bool split = false;
    if (int rc = check_split(&ctx, 1, c, false, &split)) return rc;
    std::unique_ptr<Checkpoint> ck;
    RndSeed rnd_seed{};
    ResultSink sink(c.count);
    BestLedger bl;
    if (c.flags & VGEN_SCAN_BEST) {
        bl.init(&flt, c.count);
        bl.arrival = true;   // one context: its batches are committed in the scan's order (whatever stripe of a sharding it walks)
        sink.best = &bl;
    }
    if (c.checkpoint_path) {
        ck.reset(new Checkpoint);
        const uint32_t shards = c.n_shards > 1 ? c.n_shards : 1;
        int rc = open_checkpoint(ctx, *ck, pattern, c, ctx->batch, shards, c.n_shards > 1 ? c.shard : 0, 1, rnd_seed);
        if (rc != VGEN_OK) return rc;
        sink.ck = ck.get();
        sink.matches.append_copy(ck->ledger);
        if (sink.matches.size() > c.count) sink.matches.truncate((size_t)c.count);
    }
    ScanJob job;
    job.cfg = &c;
    job.cb = cb;
    job.user = user;
    job.stop = stop;
    job.scan_seed = ck ? &rnd_seed : nullptr;
    int rc = VGEN_OK;
    if (!ck || (!ck->complete && sink.matches.size() < c.count)) rc = scan_shard(ctx, flt, job, sink);
    if (ck) {
        std::lock_guard<std::mutex> g(ck->mu);
        ck->complete = ck->complete || (rc == VGEN_OK && job.range_done);
        if (!ck->write_locked() && rc == VGEN_OK) rc = ctx->fail(VGEN_E_INVALID, "cannot write checkpoint file '" + ck->path + "'");
        out->resumed_operations = ck->resumed_operations;
    }
    // On an error: the error, AND what the batches finished before it had found (complete = 0; with a checkpoint, earlier
    // runs included — the file holds the same): a host that falls back to another backend (the reference's run_search does,
    // src/lib.rs:727-746,1185-1198) keeps those matches
    const std::string why = ctx->err;
    if (sink.best) sink.matches.take(std::vector<LiteMatch>(bl.accepted), bl.accepted.size());
    const int frc = finish_result(ctx, c.format, sink.matches, job.operations, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), out, split);
    if (rc != VGEN_OK) {
        out->failed_shards = 1;
        ctx->err = why;
        return rc;
    }
    out->complete = ck ? ck->complete : job.range_done;
    return frc;
}

// Multi-device scan: one host thread per context, batches striped over the contexts (context i takes
// global batches b = i mod n), a shared match counter and stop flag, results merged in ascending key
// order and truncated to `count` (no collective, host-side aggregation only).
// The body of vgen_scan_multi for a compiled filter; `pattern` names the scan in a checkpoint.  With `ll` (vgen_scan_list)
// the shards hand their confirmed matches to the list's ledger, which decides what the scan returns.
static int scan_multi_run(vgen_ctx **ctxs, uint32_t n_ctx, const vgen_filter &flt, const char *pattern, const vgen_scan_config *cfg,
                          vgen_progress_cb cb, void *user, const volatile int32_t *stop, vgen_scan_result *out, ListLedger *ll) {
    if (int rc = check_best(ctxs[0], *cfg, flt)) return rc;
    bool split = false;
    if (int rc = check_split(ctxs, n_ctx, *cfg, ll != nullptr, &split)) return rc;
    BestLedger best_ledger;
    BestLedger *bl = (cfg->flags & VGEN_SCAN_BEST) ? &best_ledger : nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    vgen_scan_config base = *cfg;
    Checkpoint ck;
    Checkpoint *ckp = nullptr;
    // Endomorphism contexts test images of points, not a range to stripe: every device walks from a random base of its
    // own (disjoint with overwhelming probability, SURVEY.md 8(e) "random mode"), sharing the match counter.
    bool endo = false;
    for (uint32_t i = 0; i < n_ctx; i++) endo = endo || ctxs[i]->endo;
    const bool random_keys = (cfg->flags & VGEN_SCAN_RANDOM_KEYS) != 0;
    if (endo) {
        for (uint32_t i = 0; i < n_ctx; i++)
            if (!ctxs[i]->endo) return ctxs[0]->fail(VGEN_E_INVALID, "vgen_scan_multi: VGEN_FLAG_ENDO must be set on all contexts or on none");
        if (!random_keys && (cfg->has_start || cfg->has_end || cfg->seed || cfg->checkpoint_path))
            return ctxs[0]->fail(VGEN_E_INVALID, "VGEN_FLAG_ENDO contexts serve unseeded random scans only (no start / end / seed / checkpoint)");
    }
    // the walk of an endomorphism context starts from a random base of its own per device; random-key scans stripe by
    // stream (shard i walks stream i) whatever the context
    const bool own_bases = endo && !random_keys;   // no slots to stripe or adopt: every context walks from its own random base
    if (bl) {
        bl->init(&flt, cfg->count);
        bl->arrival = own_bases && n_ctx > 1;
    }
    RndSeed rnd_seed{};   // random-key scans: one seed for all streams (shard i walks stream i of it)
    if (cfg->checkpoint_path) {
        int rc = open_checkpoint(ctxs[0], ck, pattern, base, ctxs[0]->batch, n_ctx, 0, n_ctx, rnd_seed);
        if (rc != VGEN_OK) return rc;
        ckp = &ck;
    } else if (random_keys) {
        rnd_seed = scan_rnd_seed(cfg->seed);
    } else if (!own_bases) {
        resolve_base(base);   // all shards must walk the same base key
    }
    std::atomic<uint64_t> found{0}, ops_shared{0};
    if (ckp) found = ck.ledger.size();
    if (ll) {
        ll->arrival = own_bases && n_ctx > 1;
        if (ckp) {   // what earlier runs confirmed counts first, in the order it was recorded
            std::lock_guard<std::mutex> g(ll->mu);
            ll->recorded = ck.done;
            ll->apply(ck.ledger);
            while (ll->is_recorded(ll->next)) ll->next++;
        }
    }
    const bool skip_all = ckp && (ck.complete || (ll ? ll->done.load() : ck.ledger.size() >= cfg->count));
    // Per SLOT of the striping (slot i starts on context i): matches, operations, progress, whether its range ran out.
    // Per CONTEXT: the status of its last scan_shard.  A context that fails retires; its slot is left where its last
    // committed batch put it, and a context that has finished its own slot takes it over from there (the reference has one
    // adapter and falls back to its CPU path instead, src/lib.rs:727-746,1185-1198; SURVEY.md 5: "per-GPU worker failure =>
    // re-queue its range on surviving GPUs").  Batches in flight on the failed context were never committed: the adopter
    // redoes them.  Contexts that finish while others are still running wait for a possible orphan instead of exiting.
    std::vector<MatchList> part(n_ctx);
    std::vector<uint64_t> ops(n_ctx, 0);
    std::vector<int> rcs(n_ctx, VGEN_OK);
    std::vector<char> range_done(n_ctx, 0), slot_finished(n_ctx, 0);
    std::vector<SlotProgress> progress(n_ctx);
    std::mutex cb_mu, q_mu;
    std::condition_variable q_cv;
    std::deque<uint32_t> orphans;
    uint32_t running = skip_all ? 0 : n_ctx;   // threads still inside a scan_shard call
    uint32_t failed_ctx = 0;
    // one callback per finished batch of any shard, with the cumulative count of all shards: the increment and
    // the call share a lock, so the host sees strictly increasing multiples of the batch size (gpu.rs:1106-1109)
    struct CbCtx { vgen_progress_cb cb; void *user; std::mutex *mu; std::atomic<uint64_t> *ops; } cbc{cb, user, &cb_mu, &ops_shared};
    auto locked_cb = [](uint64_t delta, void *u) {
        CbCtx *c = (CbCtx *)u;
        std::lock_guard<std::mutex> g(*c->mu);
        c->cb(c->ops->fetch_add(delta) + delta, c->user);
    };
    auto scan_over = [&]() {
        return (stop && __atomic_load_n(const_cast<const int32_t *>(stop), __ATOMIC_RELAXED) != 0) ||
               (bl ? bl->done.load() : ll ? ll->done.load() : found.load() >= cfg->count);
    };
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n_ctx && !skip_all; i++)
        th.emplace_back([&, i]() {
            uint32_t slot = i;
            for (;;) {
                vgen_scan_config c = base;
                c.shard = own_bases ? 0 : slot;
                c.n_shards = own_bases ? 0 : n_ctx;
                ScanJob job;
                job.cfg = &c;
                job.cb = cb ? (vgen_progress_cb)locked_cb : nullptr;
                job.user = &cbc;
                job.stop = stop;
                job.shared_ops = &ops_shared;
                job.scan_seed = random_keys ? &rnd_seed : nullptr;
                ResultSink sink(c.count, &found);
                sink.ck = ckp;
                sink.ck_slot = slot;
                sink.slot = own_bases ? nullptr : &progress[slot];
                sink.ll = ll;
                sink.best = bl;
                const int rc = scan_shard(ctxs[i], flt, job, sink);
                std::unique_lock<std::mutex> lk(q_mu);
                part[slot].append(std::move(sink.matches));
                ops[slot] += job.operations;
                if (rc != VGEN_OK) {
                    // this context retires; the slot it was working on is up for adoption (never for endomorphism contexts:
                    // they walk from random bases of their own, there is no range to complete)
                    rcs[i] = rc;
                    failed_ctx++;
                    running--;
                    if (!own_bases) orphans.push_back(slot);
                    q_cv.notify_all();
                    return;
                }
                range_done[slot] = job.range_done;
                slot_finished[slot] = 1;
                // finished a slot: adopt an orphan if the scan still wants keys, else wait while anybody may still fail
                running--;
                q_cv.notify_all();
                q_cv.wait(lk, [&]() { return !orphans.empty() || running == 0 || scan_over(); });
                if (orphans.empty() || scan_over()) return;
                slot = orphans.front();
                orphans.pop_front();
                running++;
            }
        });
    for (auto &x : th) x.join();
    bool all_done = !skip_all;
    for (uint32_t i = 0; i < n_ctx; i++) all_done = all_done && slot_finished[i] && range_done[i];
    int first_err = VGEN_OK;
    uint32_t first_err_ctx = 0;
    for (uint32_t i = 0; i < n_ctx; i++)
        if (rcs[i] != VGEN_OK && first_err == VGEN_OK) {
            first_err = rcs[i];
            first_err_ctx = i;
        }
    // Every slot covered (by its own context or an adopter), or the scan ended because `count` / the stop flag said so:
    // the failures were absorbed.  Otherwise (no context left to adopt a slot) the scan is incomplete and the call fails —
    // still handing over everything the committed batches found.
    bool uncovered = false;
    for (uint32_t i = 0; i < n_ctx && !skip_all; i++) uncovered = uncovered || !slot_finished[i];
    const bool absorbed = first_err != VGEN_OK && (!uncovered || scan_over() || own_bases) && failed_ctx < n_ctx;
    if (ckp) {
        std::lock_guard<std::mutex> g(ck.mu);
        ck.complete = ck.complete || all_done;
        if (!ck.write_locked() && first_err == VGEN_OK) {
            first_err = ctxs[0]->fail(VGEN_E_INVALID, "cannot write checkpoint file '" + ck.path + "'");
            first_err_ctx = 0;
        }
        out->resumed_operations = ck.resumed_operations;
    }
    out->complete = ckp ? ck.complete : all_done;
    out->failed_shards = (int32_t)failed_ctx;
    // The results: a list's are its ledger's, in the scan's order; else what the checkpoint recorded (earlier runs' matches +
    // every batch committed by this one) or what the shards took, in ascending key order
    std::vector<LiteMatch> all;
    if (bl) {
        bl->flush();
        all = bl->accepted;
    } else if (ll) {
        ll->flush();
        all = ll->accepted;
    } else if (ckp) {
        all = ck.ledger;
    } else {
        for (auto &p : part) {
            const std::vector<LiteMatch> flat = p.flatten();
            all.insert(all.end(), flat.begin(), flat.end());
        }
    }
    if (!ll && !bl) std::sort(all.begin(), all.end(), [](const LiteMatch &a, const LiteMatch &b) { return memcmp(a.key, b.key, 32) < 0; });
    uint64_t total = 0;
    for (uint64_t o : ops) total += o;
    MatchList result;
    result.take(std::move(all), (size_t)std::min<uint64_t>(all.size(), cfg->count));
    const std::string why = first_err != VGEN_OK ? ctxs[first_err_ctx]->err : std::string();
    const int frc = finish_result(ctxs[0], cfg->format, result, total, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), out, split);
    if (first_err != VGEN_OK && !absorbed) {
        out->complete = 0;
        ctxs[first_err_ctx]->err = why;
        if (first_err_ctx != 0) ctxs[0]->err = "context " + std::to_string(first_err_ctx) + ": " + why;
        return first_err;
    }
    if (first_err != VGEN_OK) ctxs[first_err_ctx]->err = why;   // absorbed: still readable through vgen_last_error(ctxs[i])
    return frc;
}

// The arguments vgen_scan_multi and vgen_scan_list share: contexts of one batch size, a configuration, a result to fill (zeroed here).
static bool multi_args(vgen_ctx **ctxs, uint32_t n_ctx, const vgen_scan_config *cfg_in, vgen_scan_config &full, vgen_scan_result *out) {
    if (!ctxs || n_ctx == 0 || !out || !normalise_scan_config(cfg_in, full)) return false;
    for (uint32_t i = 0; i < n_ctx; i++)
        if (!ctxs[i] || ctxs[i]->batch != ctxs[0]->batch) return false;
    memset(out, 0, sizeof *out);
    return true;
}

extern "C" int vgen_scan_multi(vgen_ctx **ctxs, uint32_t n_ctx, const char *pattern, const vgen_scan_config *cfg_in,
                               vgen_progress_cb cb, void *user, const volatile int32_t *stop, vgen_scan_result *out) {
    vgen_scan_config cfg_full;
    if (!pattern || !multi_args(ctxs, n_ctx, cfg_in, cfg_full, out)) return VGEN_E_INVALID;
    if (any_create2(ctxs, n_ctx, cfg_full)) return refuse_create2(ctxs[0], "vgen_scan_multi");
    if (int rc = solana_scan_rules(ctxs, n_ctx, cfg_full, "vgen_scan_multi")) return rc;
    if (int rc = onion_scan_rules(ctxs, n_ctx, cfg_full, "vgen_scan_multi")) return rc;
    const vgen_scan_config *cfg = &cfg_full;
    vgen_filter flt;
    std::string err;
    if (score_spec_unsupported(pattern, cfg->format)) return ctxs[0]->fail(VGEN_E_UNSUPPORTED, SCORE_FORMATS_MESSAGE);
    if (!filter_compile(pattern, cfg->case_insensitive != 0, cfg->format, flt, err))
        return ctxs[0]->fail(VGEN_E_PATTERN, err);
    return scan_multi_run(ctxs, n_ctx, flt, pattern, cfg, cb, user, stop, out, nullptr);
}

// A pattern list over one or several contexts: vgen_scan_multi's loop (one context: vgen_scan's) with the list as the filter
// and its ledger deciding which confirmed keys are results.  The checkpoint names the scan by the list's digest.
extern "C" int vgen_scan_list(vgen_ctx **ctxs, uint32_t n_ctx, const vgen_filter *list, uint64_t per_pattern,
                              const vgen_scan_config *cfg_in, vgen_progress_cb cb, void *user, const volatile int32_t *stop,
                              vgen_scan_result *out) {
    vgen_scan_config cfg_full;
    if (!list || !multi_args(ctxs, n_ctx, cfg_in, cfg_full, out)) return VGEN_E_INVALID;
    if (any_create2(ctxs, n_ctx, cfg_full)) return refuse_create2(ctxs[0], "vgen_scan_list");
    if (cfg_full.format == VGF_SOLANA || list->format == VGF_SOLANA || ctxs[0]->format == VGF_SOLANA)
        return ctxs[0]->fail(VGEN_E_UNSUPPORTED, "vgen_scan_list: pattern lists are not provided for the solana format");
    if (cfg_full.format == VGF_ONION || list->format == VGF_ONION || ctxs[0]->format == VGF_ONION)
        return ctxs[0]->fail(VGEN_E_UNSUPPORTED, "vgen_scan_list: pattern lists are not provided for the onion format");
    if (!list->list) return ctxs[0]->fail(VGEN_E_INVALID, "vgen_scan_list needs a pattern list (vgen_filter_compile_list)");
    if (cfg_full.format != list->format) return ctxs[0]->fail(VGEN_E_INVALID, "scan format differs from the pattern list's format");
    cfg_full.case_insensitive = list->case_insensitive ? 1 : 0;   // the list carries it
    cfg_full.n_shards = 0;
    cfg_full.shard = 0;
    const std::string id = "pattern-list:" + hex_lower(list->list->digest, 32);
    const bool own_bases = ctxs[0]->endo && !(cfg_full.flags & VGEN_SCAN_RANDOM_KEYS);
    ListLedger ll;
    ll.init(list, per_pattern, cfg_full.count, own_bases ? 1 : n_ctx);
    return scan_multi_run(ctxs, n_ctx, *list, id.c_str(), &cfg_full, cb, user, stop, out, &ll);
}

// ---- CREATE2: a search over salts (VGEN_FMT_ETHEREUM_CREATE2) --------------------------------------------------------------
// A loop of its own, on the calling thread: global batch b = counters first_counter + b * batch .. goes to context b mod n_ctx, every
// context keeps its frames full in dispatch order, and the batches are waited for and confirmed in global order, so the results
// come in ascending counter order by construction.  No key arithmetic, no checkpoint, no take-over of a failed context.
namespace {

struct Create2Lane {
    vgen_ctx *ctx = nullptr;
    uint32_t nframes = 0;                 // frames driven: all of them, or those dump mode serves
    uint32_t next_frame = 0;
    uint64_t next = 0;                    // next global batch this context dispatches
    uint64_t issued = 0;                  // batches dispatched and not abandoned: what max_batches counts
    std::vector<std::pair<uint32_t, uint64_t>> fl;   // (frame, global batch) in flight, oldest first
};

// waits for everything the lane has in flight and forgets it (the scan is over, or the lane starts again from a batch)
void create2_drain(Create2Lane &l) {
    for (auto &fb : l.fl) (void)rt_wait(l.ctx, fb.first, nullptr, 0, nullptr, nullptr);
    l.fl.clear();
}

}  // namespace

// The salt scan of both kinds of job: `what` names the entry point in messages, `install` puts the job on a context, `salt_prefix`
// is the caller's part of the raw salt, which is what a result's key holds.
static int salt_scan_run(const char *what, const std::function<int(vgen_ctx *)> &install, vgen_ctx **ctxs, uint32_t n_ctx, const char *pattern,
                         const uint8_t salt_prefix[24], uint64_t first_counter, const vgen_scan_config *cfg_in, vgen_progress_cb cb,
                         void *user, const volatile int32_t *stop, vgen_scan_result *out) {
    vgen_scan_config c;
    if (!pattern || !salt_prefix || !multi_args(ctxs, n_ctx, cfg_in, c, out)) return VGEN_E_INVALID;
    vgen_ctx *c0 = ctxs[0];
    const std::string name = what;
    if (c.format != VGF_ETHEREUM_CREATE2) return c0->fail(VGEN_E_INVALID, name + ": the scan format must be ethereum-create2 (7)");
    for (uint32_t i = 0; i < n_ctx; i++) {
        if (ctxs[i]->format != VGF_ETHEREUM_CREATE2) return c0->fail(VGEN_E_INVALID, name + ": a context was not created for the ethereum-create2 format (7)");
        for (auto &f : ctxs[i]->fr)
            if (f.in_flight) return c0->fail(VGEN_E_STATE, name + " while a dispatch is in flight");
    }
    if ((c.flags & VGEN_SCAN_BEST) && c.checkpoint_path)
        return c0->fail(VGEN_E_UNSUPPORTED, "the scan flag `best` (vgen_scan_config.flags = 2) together with checkpoint_path is not supported: a resumed scan would not know the scores reported before");
    if (c.has_start || c.has_end || c.seed || c.shard || c.n_shards > 1 || c.checkpoint_path || (c.flags & ~VGEN_SCAN_BEST))
        return c0->fail(VGEN_E_UNSUPPORTED, name + " reads format, count, case_insensitive, max_batches and the scan flag `best` (2): start / end, seed, shards, checkpoints and other flags do not apply to a salt search");
    const auto t0 = std::chrono::steady_clock::now();
    vgen_filter flt;
    std::string err;
    if (score_spec_unsupported(pattern, c.format)) return c0->fail(VGEN_E_UNSUPPORTED, SCORE_FORMATS_MESSAGE);
    if (!filter_compile(pattern, c.case_insensitive != 0, c.format, flt, err)) return c0->fail(VGEN_E_PATTERN, err);
    if (int brc = check_best(c0, c, flt)) return brc;
    const bool dump = flt.dev.kind == DEVF_HOST_ALL;   // no device filter: every payload comes back and the host filters
    const uint32_t batch = c0->batch;
    // whole batches the counter space holds from first_counter on (a tail shorter than a batch is not tested)
    const uint64_t n_batches = first_counter > UINT64_MAX - (batch - 1) ? 0 : (UINT64_MAX - (batch - 1) - first_counter) / batch + 1;
    std::vector<Create2Lane> lanes(n_ctx);
    int rc = VGEN_OK;
    for (uint32_t i = 0; i < n_ctx && rc == VGEN_OK; i++) {
        Create2Lane &l = lanes[i];
        l.ctx = ctxs[i];
        l.next = i;
        l.nframes = l.ctx->frames;
        if ((rc = install(l.ctx)) != VGEN_OK) break;
        if ((rc = vgen_set_filter(l.ctx, &flt)) != VGEN_OK) break;   // (through the C entry point: it also installs a score filter's terms)
        if (dump) {
            uint32_t df = 0;
            if ((rc = rt_get_resources(l.ctx, &df, nullptr, nullptr, nullptr)) != VGEN_OK) break;
            l.nframes = std::max(1u, std::min(l.nframes, df));
        }
    }
    if (rc != VGEN_OK) {
        if (c0->err.empty()) c0->err = name + ": a context refused the job or the filter (vgen_last_error of that context)";
        return rc;
    }
    auto stopped = [&]() { return stop && __atomic_load_n(const_cast<const int32_t *>(stop), __ATOMIC_RELAXED) != 0; };
    ResultSink sink(c.count);
    BestLedger bl;
    int64_t best_sent = -1;   // VGEN_SCAN_BEST: the best score the contexts' thresholds follow
    if (c.flags & VGEN_SCAN_BEST) {
        bl.init(&flt, c.count);
        sink.best = &bl;
    }
    std::vector<vgen_match> recs;
    uint64_t ops = 0, g = 0;   // g: the next global batch to finish
    bool complete = false;
    vgen_ctx *failed = nullptr;
    auto fill = [&](Create2Lane &l) -> int {
        while (l.fl.size() < l.nframes && l.next < n_batches && (c.max_batches == 0 || l.issued < c.max_batches)) {
            if (int r = rt_dispatch_create2(l.ctx, l.next_frame, first_counter + l.next * batch)) return r;
            l.fl.emplace_back(l.next_frame, l.next);
            l.next_frame = (l.next_frame + 1) % l.nframes;
            l.next += n_ctx;
            l.issued++;
        }
        return VGEN_OK;
    };
    while (rc == VGEN_OK && !sink.done() && !stopped()) {
        for (auto &l : lanes)
            if ((rc = fill(l)) != VGEN_OK) {
                failed = l.ctx;
                break;
            }
        if (rc != VGEN_OK) break;
        Create2Lane &l = lanes[g % n_ctx];
        if (l.fl.empty()) {   // this context has nothing left to do: the counter space or its max_batches ran out
            complete = g >= n_batches;
            break;
        }
        const uint32_t frame = l.fl.front().first;
        const uint64_t base = first_counter + g * batch;
        uint32_t found = 0;
        uint64_t tested = 0;
        recs.resize(dump ? 0 : l.ctx->match_cap);
        if ((rc = rt_wait(l.ctx, frame, recs.data(), (uint32_t)recs.size(), &found, &tested)) != VGEN_OK) {
            l.fl.erase(l.fl.begin());
            failed = l.ctx;
            break;
        }
        l.fl.erase(l.fl.begin());
        if (!dump && found > l.ctx->match_cap) {
            // more candidates than the ring holds: this context starts again from batch g with rings for a whole batch
            l.issued -= l.fl.size() + 1;
            create2_drain(l);
            l.next = g;
            l.next_frame = 0;
            if ((rc = rt_set_match_cap(l.ctx, batch)) != VGEN_OK) failed = l.ctx;
            continue;
        }
        const uint8_t *view = nullptr;
        if (dump && (rc = rt_dump_view(l.ctx, frame, &view, nullptr)) != VGEN_OK) {
            failed = l.ctx;
            break;
        }
        const uint32_t n = dump ? batch : found;
        for (uint32_t k = 0; k < n && sink.wants_more(); k++) {
            const uint32_t index = dump ? k : recs[k].index;
            const uint8_t *payload = dump ? view + (size_t)k * 20 : reinterpret_cast<const uint8_t *>(recs[k].payload);
            const std::string addr = address_from_payload(c.format, payload);
            LiteMatch m;
            if (addr.empty() || addr.size() >= sizeof m.address || !filter_accepts(flt, addr, payload)) continue;
            memcpy(m.key, salt_prefix, 24);   // the "key" of a result is the (raw) salt
            const uint64_t counter = base + index;
            for (int b = 0; b < 8; b++) m.key[24 + b] = (uint8_t)(counter >> (8 * (7 - b)));
            memcpy(m.address, addr.c_str(), addr.size() + 1);
            sink.add(m);
        }
        sink.commit(g, tested);
        if (sink.best && bl.best.load() > best_sent && bl.best.load() + 1 <= (int64_t)bl.max_score()) {
            // an improvement: later dispatches of every context report only what beats it (those in flight still deliver extras, discarded above)
            best_sent = bl.best.load();
            if ((uint32_t)(best_sent + 1) > flt.score.t[0].min)
                for (auto &ln : lanes) (void)vgen_set_score_min(ln.ctx, (uint32_t)(best_sent + 1));
        }
        ops += tested;
        g++;
        if (cb) cb(ops, user);
    }
    for (auto &l : lanes) create2_drain(l);
    const std::string why = failed ? failed->err : std::string();
    if (sink.best) sink.matches.take(std::vector<LiteMatch>(bl.accepted), bl.accepted.size());
    out->n_matches = sink.matches.size();
    out->operations = ops;
    if (!sink.matches.empty()) {
        out->matches = (vgen_generated *)malloc(sink.matches.size() * sizeof(vgen_generated));
        if (!out->matches) return c0->fail(VGEN_E_NOMEM, "out of memory");
        size_t i = 0;
        for (auto &blk : sink.matches.blocks())
            for (const LiteMatch &m : blk) {
                vgen_generated &r = out->matches[i++];
                memset(&r, 0, sizeof r);
                const std::string hex = "0x" + hex_lower(m.key, 32);
                strncpy(r.address, m.address, sizeof r.address - 1);
                strncpy(r.wif, hex.c_str(), sizeof r.wif - 1);
                strncpy(r.hex, hex.c_str(), sizeof r.hex - 1);
                r.format = c.format;
                memcpy(r.key, m.key, 32);
            }
    }
    out->elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != VGEN_OK) {
        out->failed_shards = 1;
        c0->err = why;
        return rc;
    }
    out->complete = complete ? 1 : 0;
    return VGEN_OK;
}

extern "C" int vgen_scan_create2(vgen_ctx **ctxs, uint32_t n_ctx, const char *pattern, const uint8_t deployer[20], const uint8_t init_code_hash[32],
                                 const uint8_t salt_prefix[24], uint64_t first_counter, const vgen_scan_config *cfg_in, vgen_progress_cb cb,
                                 void *user, const volatile int32_t *stop, vgen_scan_result *out) {
    if (!deployer || !init_code_hash || !salt_prefix) return VGEN_E_INVALID;
    return salt_scan_run("vgen_scan_create2", [&](vgen_ctx *ctx) { return rt_set_create2(ctx, deployer, init_code_hash, salt_prefix); }, ctxs, n_ctx,
                         pattern, salt_prefix, first_counter, cfg_in, cb, user, stop, out);
}

// The same loop over a CREATE3 job: the device reports the contract's address, a result's key is the raw salt the caller passes
// to the factory (the guarded salt and the proxy are recomputed by whoever prints them: vgen_create3_address).
extern "C" int vgen_scan_create3(vgen_ctx **ctxs, uint32_t n_ctx, const char *pattern, const uint8_t factory[20], const uint8_t proxy_init_code_hash[32],
                                 const uint8_t salt_prefix[24], const uint8_t *guard, int32_t guard_len, uint64_t first_counter,
                                 const vgen_scan_config *cfg_in, vgen_progress_cb cb, void *user, const volatile int32_t *stop, vgen_scan_result *out) {
    if (!factory || !proxy_init_code_hash || !salt_prefix || guard_len < -1 || guard_len > 64 || (guard_len > 0 && !guard)) return VGEN_E_INVALID;
    return salt_scan_run("vgen_scan_create3", [&](vgen_ctx *ctx) { return rt_set_create3(ctx, factory, proxy_init_code_hash, salt_prefix, guard, guard_len); },
                         ctxs, n_ctx, pattern, salt_prefix, first_counter, cfg_in, cb, user, stop, out);
}

extern "C" void vgen_scan_result_free(vgen_scan_result *r) {
    if (!r) return;
    free(r->matches);
    memset(r, 0, sizeof *r);
}
