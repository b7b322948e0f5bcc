// checkpoint.h — the checkpoint file of a scan (scanner.cpp): finished batches per shard and their matches.
#pragma once
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "encode.h"
#include "scan_match.h"

namespace vg {

// Checkpoint of one scan (the reference has none): which batches of every shard are
// finished, and the matches found in them, so that an interrupted range / seeded scan resumes where it
// stopped instead of from its first key.  A batch is committed — its matches appended and its shard's
// counter advanced — under one lock, so every file written is a consistent prefix of the scan.  Shards
// process their batches in dispatch order, so "batches done" is a single number per shard.
//
// File (text, mode 0600 — it holds the private keys of the matches; rewritten atomically through <path>.tmp,
// fsync, rename):
//   vgen-hip checkpoint v1 / pattern_hex= / case_insensitive= / format= / batch_size= / n_shards= /
//   first_shard= / base= / end= / operations= / done=<per slot> / complete= / mode=range|random-seed24 / match=<key hex> ...
struct Checkpoint {
    std::string path;
    std::string pattern;
    int ci = 0;
    uint32_t format = 0, batch = 0, n_shards = 1, first_shard = 0;
    uint8_t base[32] = {0}, end[32] = {0};
    bool has_end = false;
    bool random = false;                   // a random-key scan: `base` holds its 24-byte seed (bytes 8..31), done[] counts batches of the streams
    double interval_s = 10.0;

    std::mutex mu;
    std::vector<uint64_t> done;            // per slot (slot = shard - first_shard)
    std::vector<LiteMatch> ledger;         // matches of committed batches, commit order
    uint64_t operations = 0;               // over all runs
    uint64_t resumed_operations = 0;       // as loaded
    bool complete = false;
    std::chrono::steady_clock::time_point last_write = std::chrono::steady_clock::now();
    std::string error;

    static std::string hex(const uint8_t *p, size_t n) { return hex_lower(p, n); }
    static bool unhex(const std::string &s, std::vector<uint8_t> &out) {
        if (s.size() % 2) return false;
        out.clear();
        for (size_t i = 0; i < s.size(); i += 2) {
            unsigned v;
            if (!isxdigit((unsigned char)s[i]) || !isxdigit((unsigned char)s[i + 1]) || sscanf(s.c_str() + i, "%2x", &v) != 1)
                return false;
            out.push_back((uint8_t)v);
        }
        return true;
    }

    // Loads `path` when it exists and checks that it describes this very scan.  `pin_base`: the caller
    // fixed the base key (config.start or a seed); otherwise the file's base key is adopted.
    // returns 1 = resumed, 0 = no file (fresh scan), -1 = error (see `error`).
    int load(bool pin_base) {
        FILE *f = fopen(path.c_str(), "r");
        if (!f) return 0;
        std::vector<std::pair<std::string, std::string>> kv;
        char line[4096];
        bool header = false;
        while (fgets(line, sizeof line, f)) {
            std::string s(line);
            while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
            if (!header) {
                if (s != "vgen-hip checkpoint v1") break;
                header = true;
                continue;
            }
            size_t eq = s.find('=');
            if (eq != std::string::npos) kv.emplace_back(s.substr(0, eq), s.substr(eq + 1));
        }
        fclose(f);
        if (!header) return bad("not a vgen-hip checkpoint file");
        auto get = [&](const char *k) -> const std::string * {
            for (auto &e : kv)
                if (e.first == k) return &e.second;
            return nullptr;
        };
        auto differs = [&](const char *k, const std::string &want) {
            const std::string *v = get(k);
            return !v || *v != want;
        };
        if (differs("pattern_hex", hex((const uint8_t *)pattern.data(), pattern.size()))) return bad("pattern");
        if (differs("case_insensitive", std::to_string(ci))) return bad("case_insensitive");
        if (differs("format", std::to_string(format))) return bad("format");
        if (differs("batch_size", std::to_string(batch))) return bad("batch_size");
        if (differs("n_shards", std::to_string(n_shards))) return bad("n_shards");
        if (differs("first_shard", std::to_string(first_shard))) return bad("first_shard");
        if (differs("end", has_end ? hex(end, 32) : "none")) return bad("end");
        {
            const std::string *m = get("mode");   // (files written before the field existed are key-range scans')
            // ("random" without the suffix: a file of round 3's 64-bit-seeded stream function, which no longer exists)
            if ((m ? *m : std::string("range")) != (random ? "random-seed24" : "range")) return bad("mode");
        }
        std::vector<uint8_t> b;
        const std::string *bs = get("base");
        if (!bs || !unhex(*bs, b) || b.size() != 32) return bad("base");
        if (pin_base && memcmp(b.data(), base, 32) != 0) return bad("base");
        memcpy(base, b.data(), 32);
        const std::string *d = get("done"), *o = get("operations"), *c = get("complete");
        if (!d || !o || !c) return bad("done/operations/complete");
        std::vector<uint64_t> dn;
        const char *p = d->c_str();
        while (*p) {
            char *e;
            dn.push_back(strtoull(p, &e, 10));
            if (e == p) return bad("done");
            p = e;
            while (*p == ' ') p++;
        }
        if (dn.size() != done.size()) return bad("done (slot count)");
        done = dn;
        operations = resumed_operations = strtoull(o->c_str(), nullptr, 10);
        complete = *c == "1";
        for (auto &e : kv) {
            if (e.first != "match") continue;
            LiteMatch g;
            if (!unhex(e.second, b) || b.size() != 32 || !lite_from_key(format, b.data(), g)) return bad("match");
            ledger.push_back(g);
        }
        return 1;
    }
    int bad(const char *field) {
        error = "checkpoint file '" + path + "' does not belong to this scan (" + field + ")";
        return -1;
    }

    // caller holds mu.  The file lists private keys (match=...): it is created 0600, never through a symlink,
    // and reaches the disk (fsync) before it replaces the previous checkpoint.
    bool write_locked() {
        const std::string tmp = path + ".tmp";
        const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_NOFOLLOW | O_CLOEXEC, 0600);
        if (fd < 0) return false;
        (void)fchmod(fd, 0600);   // an older .tmp may have been left with wider permissions
        FILE *f = fdopen(fd, "w");
        if (!f) {
            close(fd);
            return false;
        }
        fprintf(f, "vgen-hip checkpoint v1\npattern_hex=%s\ncase_insensitive=%d\nformat=%u\nbatch_size=%u\nn_shards=%u\n"
                   "first_shard=%u\nbase=%s\nend=%s\noperations=%llu\ndone=",
                hex((const uint8_t *)pattern.data(), pattern.size()).c_str(), ci, format, batch, n_shards, first_shard,
                hex(base, 32).c_str(), has_end ? hex(end, 32).c_str() : "none", (unsigned long long)operations);
        for (size_t i = 0; i < done.size(); i++) fprintf(f, "%s%llu", i ? " " : "", (unsigned long long)done[i]);
        fprintf(f, "\ncomplete=%d\nmode=%s\n", complete ? 1 : 0, random ? "random-seed24" : "range");
        for (auto &g : ledger) fprintf(f, "match=%s\n", hex(g.key, 32).c_str());
        bool ok = fflush(f) == 0 && fsync(fd) == 0;
        ok = (fclose(f) == 0) && ok;
        ok = ok && rename(tmp.c_str(), path.c_str()) == 0;
        last_write = std::chrono::steady_clock::now();
        return ok;
    }

    // One finished batch of `slot`: its matches and the shard's counter move together.
    void commit(uint32_t slot, const std::vector<LiteMatch> &batch_matches, uint64_t ops) {
        std::lock_guard<std::mutex> g(mu);
        ledger.insert(ledger.end(), batch_matches.begin(), batch_matches.end());
        done[slot]++;
        operations += ops;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - last_write).count() >= interval_s)
            (void)write_locked();
    }
};

}  // namespace vg
