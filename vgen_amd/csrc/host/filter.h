// filter.h — vgen_filter: a compiled pattern = exact DFA (host confirmation) + device prefilter.
//
// The reference evaluates Pattern::matches on the host for every key of every batch
// (src/gpu.rs:1030-1093).  Here the pattern is analysed once: from its DFA we derive a NECESSARY
// condition on the 20-byte payload that the kernel can test in a few instructions —
//   Base58 formats : the accepted address prefixes become hash160 ranges (big-integer bounds of
//                    "prefix * 58^k" for every feasible address length),
//   Bech32 / hex   : accepted leading symbols and required trailing symbols become bit masks over
//                    the payload (and over the Bech32 checksum, which the kernel recomputes),
// and every candidate the device reports is confirmed on the host with the exact DFA over the
// encoded address string, so results equal the reference's host-side filter bit for bit.
#pragma once
#include <stdint.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../device/device_types.h"
#include "regex_dfa.h"

namespace vg {

// A compiled pattern list (vgen_filter_compile_list; device kind DEVF_LIST).  Every pattern is a start-anchored prefix
// whose matches are ranges of the big-endian payload; the ranges of all patterns, cut to the top 64 bits, are split into
// disjoint sorted intervals, each naming the patterns it can satisfy.  The device looks candidates up in the interval
// table (core/ptab_eval.h); the host confirms each with the exact automata of its interval's patterns, built at first use.
struct PatternList {
    std::vector<std::string> patterns;     // pattern i = the i-th pattern line
    std::vector<uint64_t> lo, hi;          // disjoint intervals of the top 64 payload bits, sorted
    std::vector<uint32_t> pat_off;         // patterns of interval j: pat_idx[pat_off[j] .. pat_off[j + 1]), ascending
    std::vector<uint32_t> pat_idx;
    uint32_t bits = 16;                    // first level: buckets of the top `bits` bits
    std::vector<uint32_t> bitmap, offsets; // (core/ptab_eval.h)
    uint8_t digest[32] = {0};              // SHA-256 over the pattern texts, the case flag and the format (checkpoints)
    // pattern i's exact automaton, compiled at first use: built under mu, published through the atomic pointer, then read
    // without a lock (every candidate of every confirming thread looks one up)
    mutable std::mutex mu;
    mutable std::unique_ptr<std::atomic<const Dfa *>[]> dfa;
    ~PatternList();
    DevPtab view() const;                  // host pointers into the vectors above
    const Dfa &dfa_of(uint32_t i, bool case_insensitive) const;
};

}  // namespace vg

struct vgen_filter {
    std::string pattern;
    bool case_insensitive = false;
    uint32_t format = 0;
    vg::Dfa dfa;            // decides Pattern::matches exactly
    vg::DevFilter dev{};    // device prefilter (superset)
    double selectivity = 1.0;   // estimated fraction of keys the device reports
    std::vector<uint32_t> chk_lut;   // Bech32 checksum tables (20 x 256) when the prefilter tests the checksum
    std::vector<uint32_t> dfa_blob;  // DEVF_DFA: the DFA in device layout (core/dfa_eval.h)
    std::shared_ptr<vg::PatternList> list;   // DEVF_LIST: the pattern list (dfa above stays empty)
    vg::ScoreTerms score{};                  // DEVF_SCORE: the terms of a score specification (n = 0: not one; dfa stays empty)
};

namespace vg {

// Compiles pattern + derives the device prefilter for `format`. false + err on invalid patterns.
bool filter_compile(const std::string &pattern, bool case_insensitive, uint32_t format, vgen_filter &out,
                    std::string &err);

// Score specifications ("score:" + 1 - 4 terms `<metric>>=<n>` joined by '&'; metrics zero-bytes, leading-zero-bytes, leading:<h>,
// count:<h> on the 40 hex digits of the address; include/vgen_hip.h).  The prefix is reserved: ':' is in no address alphabet, so
// as a regular expression such a string could never match.  filter_compile takes one for the hex formats (device kind DEVF_SCORE).
bool is_score_spec(const std::string &pattern);
// ... on any other format it is VGEN_E_UNSUPPORTED, in vgen_filter_compile and in every scan alike
inline bool score_spec_unsupported(const std::string &pattern, uint32_t format) { return is_score_spec(pattern) && !vgf_is_hex((int)format); }
constexpr const char *SCORE_FORMATS_MESSAGE =
    "a score specification scores the hex digits of an address: formats 5 (ethereum), 6 (ethereum-contract) and 7 (ethereum-create2) only";
bool score_parse(const std::string &spec, ScoreTerms &out, std::string &err);
// Fraction of uniformly random payloads a specification accepts, and its reciprocal rounded down (saturating): exact for one term
// (binomial tail with (20, 1/256) or (40, 1/16); 256^-n or 16^-n for the leading runs).  For several terms the smallest single-term
// probability: an UPPER bound on the hit rate, a LOWER bound on the difficulty.
void score_odds(const ScoreTerms &s, double *selectivity, uint64_t *difficulty);
// The score of `address` under a score filter (the value of the first term's metric); false when the filter is no score filter or
// the string is no address of its format.  `payload` (optional) spares the decode.  *accepted: every term holds.
bool score_of(const vgen_filter &f, const std::string &address, const uint8_t *payload, uint32_t *score, bool *accepted);

// Hard limit on the patterns of one list (vgen_hip.h: vgen_filter_compile_list).
constexpr uint32_t LIST_MAX_PATTERNS = 1u << 20;
// Compiles a pattern list (one pattern per line; empty lines and lines starting with '#' skipped) for `format`.  false +
// err ("line N: reason") when a line is not a start-anchored prefix, matches every address or none, repeats an earlier
// line, or the list is empty.
bool filter_compile_list(const std::string &text, bool case_insensitive, uint32_t format, vgen_filter &out, std::string &err);
// The payload of an address of `format` (Base58Check / Bech32 / Bech32m / hex decoded and checked); false when the string
// is not such an address.  out: 20 bytes, 32 for P2TR.
bool payload_from_address(uint32_t format, const std::string &address, uint8_t out[32]);
// Pattern indices the address satisfies, ascending: a list's through its interval table and the automata of the interval's
// patterns; a single pattern's {0} or {}.  `payload` (optional) spares the decode when the caller has it.
void filter_which(const vgen_filter &f, const std::string &address, const uint8_t *payload, std::vector<uint32_t> &out);
// Pattern::matches for either kind of filter (a list: any of its patterns).
bool filter_accepts(const vgen_filter &f, const std::string &address, const uint8_t *payload);

}  // namespace vg
