// filter.cpp — see filter.h.
#include "filter.h"

#include "../core/dfa_eval.h"
#include "../core/filter_eval.h"
#include "../core/ptab_eval.h"
#include "../core/score_eval.h"
#include "ed_host.h"
#include "onion_host.h"
#include "encode.h"

#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>

namespace vg {

namespace {

// ---- tiny 256-bit unsigned integer (address payloads are 200 bits) ------------------------------------

struct U256 {
    uint64_t w[4] = {0, 0, 0, 0};
    static U256 from_u64(uint64_t v) {
        U256 r;
        r.w[0] = v;
        return r;
    }
    static U256 pow2(unsigned e) {
        U256 r;
        r.w[e >> 6] = 1ull << (e & 63);
        return r;
    }
};

int cmp(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; i--) {
        if (a.w[i] < b.w[i]) return -1;
        if (a.w[i] > b.w[i]) return 1;
    }
    return 0;
}

U256 add(const U256 &a, const U256 &b) {
    U256 r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}

U256 sub(const U256 &a, const U256 &b) {   // a >= b
    U256 r;
    unsigned __int128 bw = 0;
    for (int i = 0; i < 4; i++) {
        unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - (uint64_t)bw;
        r.w[i] = (uint64_t)d;
        bw = (d >> 64) & 1;
    }
    return r;
}

U256 mul_small(const U256 &a, uint32_t m) {
    U256 r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] * m;
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}

U256 shr32(const U256 &a) {
    U256 r;
    for (int i = 0; i < 4; i++) r.w[i] = (a.w[i] >> 32) | (i < 3 ? a.w[i + 1] << 32 : 0);
    return r;
}

U256 umax(const U256 &a, const U256 &b) { return cmp(a, b) >= 0 ? a : b; }
U256 umin(const U256 &a, const U256 &b) { return cmp(a, b) <= 0 ? a : b; }

void to_be_words160(const U256 &a, uint32_t out[5]) {
    // a < 2^160
    out[4] = (uint32_t)a.w[0];
    out[3] = (uint32_t)(a.w[0] >> 32);
    out[2] = (uint32_t)a.w[1];
    out[1] = (uint32_t)(a.w[1] >> 32);
    out[0] = (uint32_t)a.w[2];
}

double to_double(const U256 &a) {
    double r = 0;
    for (int i = 3; i >= 0; i--) r = r * 18446744073709551616.0 + (double)a.w[i];
    return r;
}

const char B58[] = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
const char BECH32[] = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";
const char HEXL[] = "0123456789abcdef";

int b58_digit(char c) {
    const char *p = strchr(B58, c);
    return p && c ? (int)(p - B58) : -1;
}

uint32_t step(const Dfa &d, uint32_t s, unsigned char c) { return d.trans[(size_t)s * d.n_cls + d.cls[c]]; }

// Enumerates the address prefixes (over `alphabet`) from DFA state `from` that can still lead to a
// match: a branch ends when the state is absorbing (match_now: every extension matches), dead, or
// `max_depth` symbols long.  Returns false when the search exceeds its budget (pattern does not
// constrain prefixes usefully).
struct Prefix {
    std::string s;
    bool absorbing;
};

bool enumerate_prefixes(const Dfa &d, uint32_t from, const char *alphabet, size_t max_depth, size_t budget,
                        std::vector<Prefix> &out) {
    out.clear();
    struct Item {
        uint32_t state;
        std::string s;
    };
    std::vector<Item> stack;
    stack.push_back({from, ""});
    size_t visited = 0;
    while (!stack.empty()) {
        Item it = stack.back();
        stack.pop_back();
        if (++visited > budget) return false;
        if (d.dead[it.state]) continue;
        if (d.match_now[it.state]) {
            out.push_back({it.s, true});
            continue;
        }
        if (it.s.size() >= max_depth) {
            out.push_back({it.s, false});
            continue;
        }
        for (const char *a = alphabet; *a; a++) stack.push_back({step(d, it.state, (unsigned char)*a), it.s + *a});
    }
    return true;
}

// ---- Base58 (P2PKH / P2SH) ----------------------------------------------------------------------------------

struct Range {
    U256 lo, hi;   // inclusive, as 160-bit hash160 values
};

// Ranges of the 25-byte payload integer V whose Base58Check string starts with `p`.
void prefix_to_ranges(const std::string &p, uint8_t version, std::vector<Range> &out) {
    // a = leading '1's of the prefix, q = the rest
    size_t a = 0;
    while (a < p.size() && p[a] == '1') a++;
    const std::string q = p.substr(a);
    U256 vlo, vhi;   // payload-integer window the version byte allows
    if (version == 0x00) {
        if (a == 0 && !q.empty()) return;   // P2PKH addresses start with '1'
    } else {
        if (a > 0) return;                   // a P2SH payload has no leading zero byte
    }
    std::vector<std::pair<U256, U256>> v;    // payload integer ranges
    const U256 one = U256::from_u64(1);
    if (version == 0x00) {
        if (a > 25) return;
        if (q.empty()) {
            // at least a leading zero bytes: V < 256^(25-a)
            if (a == 0) v.push_back({U256(), sub(U256::pow2(192), one)});
            else v.push_back({U256(), sub(U256::pow2(8 * (25 - (unsigned)a)), one)});
        } else {
            if (a > 24) return;
            // exactly a leading zero bytes
            vlo = U256::pow2(8 * (24 - (unsigned)a));
            vhi = sub(U256::pow2(8 * (25 - (unsigned)a)), one);
        }
    } else {
        vlo = mul_small(U256::pow2(192), version);
        vhi = sub(mul_small(U256::pow2(192), (uint32_t)version + 1), one);
    }
    if (!q.empty()) {
        U256 qv;
        for (char c : q) {
            int dg = b58_digit(c);
            if (dg < 0) return;
            qv = add(mul_small(qv, 58), U256::from_u64((uint64_t)dg));
        }
        U256 lo = qv, hi = qv;   // m = |q| digits: exactly the value q
        // grow the digit count; 35 digits cover 2^200
        for (size_t m = q.size(); m <= 35; m++) {
            U256 l = umax(lo, vlo), h = umin(hi, vhi);
            if (cmp(l, h) <= 0) v.push_back({l, h});
            if (cmp(lo, vhi) > 0) break;
            // next m: [lo*58, hi*58 + 57]; stop before overflowing 256 bits
            if (lo.w[3] >> 56) break;
            lo = mul_small(lo, 58);
            hi = add(mul_small(hi, 58), U256::from_u64(57));
        }
    }
    for (auto &r : v) {
        U256 l = r.first, h = r.second;
        if (version != 0x00) {
            const U256 base = mul_small(U256::pow2(192), version);
            l = sub(l, base);
            h = sub(h, base);
        }
        out.push_back({shr32(l), shr32(h)});   // drop the 4 checksum bytes: superset on the edges
    }
}

void merge_ranges(std::vector<Range> &r) {
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return cmp(a.lo, b.lo) < 0; });
    std::vector<Range> out;
    const U256 one = U256::from_u64(1);
    for (auto &x : r) {
        if (!out.empty() && cmp(x.lo, add(out.back().hi, one)) <= 0) {
            out.back().hi = umax(out.back().hi, x.hi);
        } else {
            out.push_back(x);
        }
    }
    r.swap(out);
}

void derive_base58(const Dfa &d, uint8_t version, DevFilter &dev, double &sel) {
    dev.kind = DEVF_HOST_ALL;
    dev.count = 0;
    sel = 1.0;
    if (d.match_now[0]) {
        dev.kind = DEVF_ALL;
        return;
    }
    for (size_t depth = 12; depth >= 1; depth--) {
        std::vector<Prefix> prefixes;
        if (!enumerate_prefixes(d, 0, B58, depth, 200000, prefixes)) continue;
        std::vector<Range> ranges;
        for (auto &p : prefixes) prefix_to_ranges(p.s, version, ranges);
        merge_ranges(ranges);
        if (ranges.size() > DEVF_MAX_TESTS) continue;
        double total = 0;
        for (auto &r : ranges) total += to_double(sub(r.hi, r.lo)) + 1.0;
        sel = total / 1.4615016373309029e48;   // 2^160
        if (sel > 0.999999) {
            // everything is a candidate: exact "match all" only if no branch was cut at the depth limit
            bool exact = true;
            for (auto &p : prefixes) exact = exact && p.absorbing;
            dev.kind = exact ? DEVF_ALL : DEVF_HOST_ALL;
            return;
        }
        if (sel > 0.2) {   // ranges that cover most of the space are no prefilter
            bool exact = true;
            for (auto &p : prefixes) exact = exact && p.absorbing;
            if (!exact) {
                dev.kind = DEVF_HOST_ALL;
                sel = 1.0;
                return;
            }
        }
        dev.kind = DEVF_RANGES;
        dev.count = (uint32_t)ranges.size();
        for (size_t i = 0; i < ranges.size(); i++) {
            to_be_words160(ranges[i].lo, dev.tests[i].a);
            to_be_words160(ranges[i].hi, dev.tests[i].b);
        }
        return;
    }
}

// ---- Solana: Base58 of the 32-byte public key read as one big-endian number N, no version byte, no checksum ---------------

struct Range256 {
    U256 lo, hi;   // inclusive
};

// a * 58 + d; false when the result passes 2^256 - 1
bool mul58_add(U256 &a, uint32_t d) {
    unsigned __int128 c = d;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] * 58u;
        a.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return c == 0;
}

void to_be_words256(const U256 &a, uint32_t out[8]) {
    for (int i = 0; i < 4; i++) {
        out[7 - 2 * i] = (uint32_t)a.w[i];
        out[6 - 2 * i] = (uint32_t)(a.w[i] >> 32);
    }
}

// The exact ranges of N whose address starts with `p`: z leading '1's are z leading zero bytes, and what follows them are the
// leading digits of a number of exactly 32 - z bytes - one range per digit count that fits (two at most: 58^d grows by 5.86 bits).
void sol_prefix_ranges(const std::string &p, std::vector<Range256> &out) {
    size_t z = 0;
    while (z < p.size() && p[z] == '1') z++;
    const std::string q = p.substr(z);
    auto below_pow2 = [&](unsigned e) {   // 2^e - 1, e <= 256
        U256 r;
        for (int i = 0; i < 4; i++) r.w[i] = e >= 64u * (i + 1) ? ~0ull : e > 64u * i ? (1ull << (e - 64u * i)) - 1 : 0;
        return r;
    };
    if (z > 32 || (z == 32 && !q.empty())) return;
    if (q.empty()) {   // at least z leading zero bytes
        out.push_back({U256(), below_pow2(8 * (32 - (unsigned)z))});
        return;
    }
    const U256 vlo = U256::pow2(8 * (31 - (unsigned)z)), vhi = below_pow2(8 * (32 - (unsigned)z));
    U256 lo, hi;
    bool hi_sat = false;
    for (char c : q) {
        const int dg = b58_digit(c);
        if (dg < 0 || !mul58_add(lo, (uint32_t)dg)) return;
    }
    hi = lo;
    for (size_t m = q.size(); m <= 44; m++) {
        const U256 l = umax(lo, vlo), h = umin(hi_sat ? vhi : hi, vhi);
        if (cmp(l, h) <= 0) out.push_back({l, h});
        if (cmp(lo, vhi) > 0) break;
        if (!mul58_add(lo, 0)) break;   // from here on every candidate passes 2^256
        if (!hi_sat && !mul58_add(hi, 57)) hi_sat = true;
    }
}

void merge_ranges256(std::vector<Range256> &r) {
    std::sort(r.begin(), r.end(), [](const Range256 &a, const Range256 &b) { return cmp(a.lo, b.lo) < 0; });
    std::vector<Range256> out;
    const U256 one = U256::from_u64(1);
    for (auto &x : r) {
        const bool top = !out.empty() && (~out.back().hi.w[0] | ~out.back().hi.w[1] | ~out.back().hi.w[2] | ~out.back().hi.w[3]) == 0;
        if (!out.empty() && (top || cmp(x.lo, add(out.back().hi, one)) <= 0)) out.back().hi = umax(out.back().hi, x.hi);
        else out.push_back(x);
    }
    r.swap(out);
}

// The device test of a Solana pattern: ranges of N from the accepted prefixes, residues of N modulo 58^k (k <= 5) from the accepted
// last k characters, both when the pattern constrains both ends.  Always a superset: when the exact prefixes need more than
// DEVF_MAX_TESTS ranges (classes, -i) the enumeration stops at the deepest level that fits, and the suffixes are those acceptable from ANY
// reachable state (an address has 32 to 44 characters: where its last k begin is not known).
void derive_solana(const Dfa &d, DevFilter &dev, double &sel) {
    dev.kind = DEVF_HOST_ALL;
    dev.count = 0;
    sel = 1.0;
    if (d.match_now[0]) {
        dev.kind = DEVF_ALL;
        return;
    }
    // (1) prefixes -> ranges, the deepest enumeration that fits
    std::vector<Range256> ranges;
    double prefix_sel = 1.0;
    bool prefix_exact = false;
    for (size_t depth = 1; depth <= 12; depth++) {   // (ascending: an unanchored pattern gives up after three levels, not after twelve)
        std::vector<Prefix> prefixes;
        if (!enumerate_prefixes(d, 0, B58, depth, 200000, prefixes)) break;
        std::vector<Range256> r;
        for (auto &p : prefixes) sol_prefix_ranges(p.s, r);
        merge_ranges256(r);
        if (r.size() > DEVF_MAX_TESTS) break;
        double total = 0;
        for (auto &x : r) total += to_double(sub(x.hi, x.lo)) + 1.0;
        prefix_sel = total / 1.157920892373162e77;   // 2^256
        prefix_exact = true;
        for (auto &p : prefixes) prefix_exact = prefix_exact && p.absorbing;
        ranges.swap(r);
        if (prefix_exact) break;   // nothing deeper to learn
    }
    if (prefix_sel > 0.999999 && prefix_exact && ranges.size() == 1) {   // every address, decided by the prefixes alone
        dev.kind = DEVF_ALL;
        return;
    }
    const bool prefix_constrains = prefix_sel <= 0.2 || (prefix_exact && prefix_sel < 0.999999);

    // (2) suffixes of k = 1 .. 5 characters -> residues mod 58^k
    std::vector<uint32_t> all;
    {
        std::vector<uint8_t> seen(d.n_states, 0);
        std::vector<uint32_t> stack{0};
        seen[0] = 1;
        while (!stack.empty()) {
            const uint32_t st = stack.back();
            stack.pop_back();
            if (d.dead[st]) continue;
            all.push_back(st);
            if (d.match_now[st]) continue;
            for (const char *a = B58; *a; a++) {
                const uint32_t n = step(d, st, (unsigned char)*a);
                if (!seen[n]) {
                    seen[n] = 1;
                    stack.push_back(n);
                }
            }
        }
        std::sort(all.begin(), all.end());
    }
    struct SuffixSet {
        unsigned k = 0;
        std::vector<uint32_t> residues;
        double sel = 1.0;
    };
    std::vector<SuffixSet> sets;
    // viable[r][s]: from state s some string of exactly r more characters ends in acceptance - prunes the enumeration
    std::vector<std::vector<uint8_t>> viable(6, std::vector<uint8_t>(d.n_states, 0));
    for (uint32_t st = 0; st < d.n_states; st++) viable[0][st] = d.match_now[st] || d.match_at_end[st];
    for (unsigned r = 1; r <= 5; r++)
        for (uint32_t st = 0; st < d.n_states; st++) {
            if (d.match_now[st]) {
                viable[r][st] = 1;
                continue;
            }
            for (const char *a = B58; *a && !viable[r][st]; a++) viable[r][st] = viable[r - 1][step(d, st, (unsigned char)*a)];
        }
    for (unsigned k = 1; k <= 5; k++) {
        struct Item {
            std::vector<uint32_t> states;
            uint32_t v;
            unsigned len;
        };
        std::vector<Item> stack;
        stack.push_back({all, 0, 0});
        SuffixSet ss;
        ss.k = k;
        size_t visited = 0;
        bool overflow = false;
        while (!stack.empty() && !overflow) {
            Item it = std::move(stack.back());
            stack.pop_back();
            if (++visited > 400000) overflow = true;
            if (it.len == k) {
                bool ok = false;
                for (uint32_t st : it.states) ok = ok || d.match_now[st] || d.match_at_end[st];
                if (ok) {
                    ss.residues.push_back(it.v);
                    if (ss.residues.size() > DEVF_MAX_TESTS) overflow = true;
                }
                continue;
            }
            for (uint32_t a = 0; a < 58; a++) {
                std::vector<uint32_t> nxt;
                for (uint32_t st : it.states) {
                    const uint32_t n = d.match_now[st] ? st : step(d, st, (unsigned char)B58[a]);
                    if (!d.dead[n] && viable[k - it.len - 1][n]) nxt.push_back(n);
                }
                if (nxt.empty()) continue;
                std::sort(nxt.begin(), nxt.end());
                nxt.erase(std::unique(nxt.begin(), nxt.end()), nxt.end());
                stack.push_back({std::move(nxt), it.v * 58u + a, it.len + 1});
            }
        }
        if (overflow) break;
        ss.sel = (double)ss.residues.size();
        for (unsigned i = 0; i < k; i++) ss.sel /= 58.0;
        std::sort(ss.residues.begin(), ss.residues.end());
        sets.push_back(std::move(ss));
    }
    // the most selective suffix set that leaves room for the ranges; without room for both, the better end alone
    const SuffixSet *best = nullptr, *best_alone = nullptr;
    for (auto &ss : sets) {
        if (ss.sel > 0.2) continue;
        if (!best_alone || ss.sel < best_alone->sel * (1.0 - 1e-9)) best_alone = &ss;   // (the shortest suffix of a selectivity)
        if (prefix_constrains && ranges.size() + ss.residues.size() <= DEVF_MAX_TESTS && (!best || ss.sel < best->sel * (1.0 - 1e-9))) best = &ss;
    }
    const SuffixSet *use_s = nullptr;
    bool use_p = prefix_constrains;
    if (prefix_constrains && best) use_s = best;
    else if (best_alone && (!prefix_constrains || best_alone->sel < prefix_sel)) {
        use_s = best_alone;
        use_p = false;
    }
    if (!use_p && !use_s) return;   // DEVF_HOST_ALL: correct and slow
    uint32_t n = 0;
    if (use_p)
        for (auto &x : ranges) {
            to_be_words256(x.lo, dev.tests[n].a);
            to_be_words256(x.hi, dev.tests[n].b);
            n++;
        }
    sel = use_p ? prefix_sel : 1.0;
    if (use_s) {
        dev.kind = DEVF_SOL_RESIDUE;
        dev.chk_base = n;
        uint32_t m = 1;
        for (unsigned i = 0; i < use_s->k; i++) m *= 58u;
        dev.witver = m;
        for (uint32_t r : use_s->residues) dev.tests[n++].a[0] = r;
        sel *= use_s->sel;
    } else {
        dev.kind = DEVF_RANGES;
    }
    dev.count = n;
}

// ---- fixed-length symbol strings (Bech32 P2WPKH, hex Ethereum) ---------------------------------------------

struct SymSpec {
    const char *header;     // literal address head fed to the DFA first
    const char *alphabet;   // symbol -> character
    unsigned bits;          // bits per symbol
    unsigned n_data;        // symbols that come from the payload
    unsigned n_chk;         // trailing checksum symbols (Bech32)
    unsigned payload_bits;  // 160, or 256 for P2TR (the last data symbol is then zero-padded)
    unsigned max_prefix = 12;   // deepest prefix enumeration tried (Nostr keys: all 52 data symbols, so that a long literal prefix is
                                // a mask over all of its bits - the kernel's compare is eight words wide whatever the depth)
};

int sym_index(const SymSpec &sp, char c) {
    const char *p = strchr(sp.alphabet, c);
    return p && c ? (int)(p - sp.alphabet) : -1;
}

// Writes symbol `v` at position `pos` (0 = first data symbol) into a test's mask/value.  Returns false
// when the symbol cannot occur there (a set bit in the zero padding of the last data symbol).
bool set_symbol(const SymSpec &sp, DevFilterTest &t, unsigned pos, unsigned v) {
    if (pos < sp.n_data) {
        const unsigned bit = pos * sp.bits;   // from the most significant bit of the payload
        for (unsigned k = 0; k < sp.bits; k++) {
            const unsigned b = bit + k, w = b >> 5, o = 31 - (b & 31);
            const bool one = (v >> (sp.bits - 1 - k)) & 1;
            if (b >= sp.payload_bits) {
                if (one) return false;
                continue;
            }
            t.a[w] |= 1u << o;
            if (one) t.b[w] |= 1u << o;
        }
    } else {
        const unsigned c = pos - sp.n_data;   // checksum symbol c in bits (29 - 5c) .. (25 - 5c)
        const unsigned sh = 25 - 5 * c;
        t.chk_mask |= 31u << sh;
        t.chk_value |= (v & 31u) << sh;
    }
    return true;
}

void derive_symbols(const Dfa &d, const SymSpec &sp, DevFilter &dev, double &sel) {
    dev.kind = DEVF_HOST_ALL;
    dev.count = 0;
    dev.flags = 0;
    sel = 1.0;
    uint32_t s = 0;
    for (const char *h = sp.header; *h; h++) {
        if (d.match_now[s]) break;
        s = step(d, s, (unsigned char)*h);
    }
    if (d.match_now[s]) {
        dev.kind = DEVF_ALL;
        return;
    }
    const unsigned n_total = sp.n_data + sp.n_chk;
    const size_t A = strlen(sp.alphabet);

    // (1) accepted prefixes over the data symbols
    // the shallowest depth that reaches the best selectivity: deeper enumerations of the same language
    // (e.g. "q" + any symbol for ^bc1qq.*) only multiply the tests
    std::vector<Prefix> prefixes;
    size_t pdepth = 0;
    double prefix_sel = 1.0;
    for (size_t depth = 1; depth <= std::min<size_t>(sp.max_prefix, sp.n_data); depth++) {
        std::vector<Prefix> p;
        if (!enumerate_prefixes(d, s, sp.alphabet, depth, 100000, p) || p.size() > DEVF_MAX_TESTS) break;
        double sel_d = 0;
        for (auto &q : p) {
            double f = 1.0;
            for (size_t i = 0; i < q.s.size(); i++) f /= (double)A;
            sel_d += f;
        }
        if (pdepth == 0 || sel_d < prefix_sel * (1.0 - 1e-9)) {
            prefixes.swap(p);
            pdepth = depth;
            prefix_sel = sel_d;
        }
    }
    // prefixes that together cover every string (e.g. the 32 one-symbol prefixes of an unanchored or
    // suffix-only pattern) constrain nothing: crossing them with the suffixes would only multiply tests
    bool prefix_constrains = pdepth > 0 && prefix_sel < 0.999999;

    // (2) required suffixes: states reachable after t symbols, then suffixes that can accept
    std::vector<std::set<uint32_t>> reach(n_total + 1);
    reach[0].insert(s);
    for (unsigned t = 0; t < n_total; t++)
        for (uint32_t st : reach[t]) {
            if (d.dead[st]) continue;
            for (size_t a = 0; a < A; a++) reach[t + 1].insert(d.match_now[st] ? st : step(d, st, (unsigned char)sp.alphabet[a]));
        }
    std::vector<std::string> best_suffixes;
    double suffix_sel = 1.0;
    const unsigned kmax = std::min<unsigned>(8, n_total);
    // viable[r][s]: from DFA state s some string of exactly r more symbols ends in acceptance — prunes
    // the suffix enumeration to branches that can still succeed
    std::vector<std::vector<uint8_t>> viable(kmax + 1, std::vector<uint8_t>(d.n_states, 0));
    for (uint32_t st = 0; st < d.n_states; st++) viable[0][st] = d.match_now[st] || d.match_at_end[st];
    for (unsigned r = 1; r <= kmax; r++)
        for (uint32_t st = 0; st < d.n_states; st++) {
            if (d.match_now[st]) {
                viable[r][st] = 1;
                continue;
            }
            for (size_t a = 0; a < A && !viable[r][st]; a++)
                viable[r][st] = viable[r - 1][step(d, st, (unsigned char)sp.alphabet[a])];
        }
    for (unsigned k = 1; k <= kmax; k++) {
        // DFS over suffix strings with state sets
        struct Item {
            std::vector<uint32_t> states;
            std::string s;
        };
        std::vector<std::string> acc;
        std::vector<Item> stack;
        stack.push_back({std::vector<uint32_t>(reach[n_total - k].begin(), reach[n_total - k].end()), ""});
        size_t visited = 0;
        bool overflow = false;
        while (!stack.empty() && !overflow) {
            Item it = std::move(stack.back());
            stack.pop_back();
            if (++visited > 400000) {
                overflow = true;
                break;
            }
            if (it.s.size() == k) {
                bool ok = false;
                for (uint32_t st : it.states) ok = ok || d.match_now[st] || d.match_at_end[st];
                if (ok) {
                    acc.push_back(it.s);
                    if (acc.size() > DEVF_MAX_TESTS) overflow = true;
                }
                continue;
            }
            for (size_t a = 0; a < A; a++) {
                std::vector<uint32_t> nxt;
                const unsigned remaining = k - (unsigned)it.s.size() - 1;
                for (uint32_t st : it.states) {
                    uint32_t n = d.match_now[st] ? st : step(d, st, (unsigned char)sp.alphabet[a]);
                    if (!d.dead[n] && viable[remaining][n]) nxt.push_back(n);
                }
                if (nxt.empty()) continue;
                std::sort(nxt.begin(), nxt.end());
                nxt.erase(std::unique(nxt.begin(), nxt.end()), nxt.end());
                stack.push_back({std::move(nxt), it.s + sp.alphabet[a]});
            }
        }
        if (overflow) break;
        double f = (double)acc.size();
        for (unsigned i = 0; i < k; i++) f /= (double)A;
        if (f < suffix_sel) {
            suffix_sel = f;
            best_suffixes = acc;
        }
    }
    const bool suffix_constrains = suffix_sel < 0.999999;

    if (!prefix_constrains && !suffix_constrains) return;   // DEVF_HOST_ALL
    std::vector<Prefix> use_p;
    std::vector<std::string> use_s;
    if (prefix_constrains && suffix_constrains && prefixes.size() * best_suffixes.size() <= DEVF_MAX_TESTS) {
        use_p = prefixes;
        use_s = best_suffixes;
        sel = prefix_sel * suffix_sel;
    } else if (prefix_constrains && (!suffix_constrains || prefix_sel <= suffix_sel)) {
        use_p = prefixes;
        use_s.push_back("");
        sel = prefix_sel;
    } else {
        use_p.push_back({"", false});
        use_s = best_suffixes;
        sel = suffix_sel;
    }
    if (sel > 0.2) {   // not a useful necessary condition: leave it to the full match (DEVF_DFA) / host
        sel = 1.0;
        return;
    }
    dev.kind = DEVF_MASKED;
    dev.count = 0;
    for (auto &p : use_p)
        for (auto &sx : use_s) {
            DevFilterTest t;
            memset(&t, 0, sizeof t);
            bool possible = true;
            for (size_t i = 0; i < p.s.size(); i++)
                possible = set_symbol(sp, t, (unsigned)i, (unsigned)sym_index(sp, p.s[i])) && possible;
            for (size_t i = 0; i < sx.size(); i++)
                possible = set_symbol(sp, t, n_total - (unsigned)sx.size() + (unsigned)i, (unsigned)sym_index(sp, sx[i])) && possible;
            if (!possible) continue;
            if (t.chk_mask) dev.flags |= DEVF_FLAG_BECH32_CHK;
            dev.tests[dev.count++] = t;
        }
    // count == 0 means nothing can match: the kernel then reports no candidates
}

// ---- Tor v3 onion addresses: 56 Base32 characters of key || checksum || version --------------------------------------------------
// Characters 0 .. 48 are bits 0 .. 244 of the key's byte stream - y alone; the sign of x is stream bit 248, the checksum a SHA3-256
// the device does not compute.  So the device test is the masked compare of a START-ANCHORED prefix (classes and -i included: up to
// DEVF_MAX_TESTS accepted prefixes, the shallowest enumeration of the best selectivity, no deeper than 49 characters) and nothing
// else: suffixes, unanchored patterns and whatever constrains later characters only are DEVF_HOST_ALL.  Always a superset.
const char B32[] = "abcdefghijklmnopqrstuvwxyz234567";

void derive_onion(const Dfa &d, DevFilter &dev, double &sel) {
    dev.kind = DEVF_HOST_ALL;
    dev.count = 0;
    dev.flags = 0;
    sel = 1.0;
    if (d.match_now[0]) {
        dev.kind = DEVF_ALL;
        return;
    }
    const SymSpec sp = {"", B32, 5, 49, 0, 256, 49};
    std::vector<Prefix> prefixes;
    double prefix_sel = 1.0;
    bool have = false;
    for (size_t depth = 1; depth <= 49; depth++) {
        std::vector<Prefix> p;
        if (!enumerate_prefixes(d, 0, B32, depth, 100000, p) || p.size() > DEVF_MAX_TESTS) break;
        double sel_d = 0;
        bool exact = true;
        for (auto &q : p) {
            double f = 1.0;
            for (size_t i = 0; i < q.s.size(); i++) f /= 32.0;
            sel_d += f;
            exact = exact && q.absorbing;
        }
        if (!have || sel_d < prefix_sel * (1.0 - 1e-9)) {
            prefixes.swap(p);
            prefix_sel = sel_d;
            have = true;
        }
        if (exact) {        // nothing deeper to learn
            if (sel_d > 0.999999) {   // every string of this depth is accepted whatever follows: every address matches
                dev.kind = DEVF_ALL;
                return;
            }
            break;
        }
    }
    if (!have || prefix_sel > 0.2) return;   // not a useful necessary condition: the host filters
    dev.kind = DEVF_MASKED;
    sel = prefix_sel;
    for (auto &p : prefixes) {
        DevFilterTest t;
        memset(&t, 0, sizeof t);
        for (size_t i = 0; i < p.s.size(); i++) (void)set_symbol(sp, t, (unsigned)i, (unsigned)sym_index(sp, p.s[i]));
        dev.tests[dev.count++] = t;
    }
}

// Packs `d` into the device layout of core/dfa_eval.h.  `head` is the literal every address of the format
// starts with and that the device does not re-walk; `alphabet` maps symbol index -> character.
// Returns false when the automaton does not fit the LDS budget (or 16-bit state numbers).
bool build_dfa_blob(const Dfa &d, const char *head, const char *alphabet, std::vector<uint32_t> &blob) {
    if (d.n_states > 65535) return false;
    uint32_t s = 0;
    for (const char *h = head; *h; h++) s = d.match_now[s] ? s : step(d, s, (unsigned char)*h);
    const size_t flags_off = DFA_HDR_WORDS * 4;
    const size_t trans_off = (flags_off + d.n_states + 3) & ~(size_t)3;
    const size_t total = (trans_off + (size_t)d.n_states * d.n_cls * 2 + 3) & ~(size_t)3;
    if (total > DFA_MAX_BYTES) return false;
    blob.assign(total / 4, 0);
    blob[0] = d.n_states;
    blob[1] = d.n_cls;
    blob[2] = s;
    blob[3] = (uint32_t)flags_off;
    blob[4] = (uint32_t)trans_off;
    blob[5] = (uint32_t)total;
    uint8_t *b = reinterpret_cast<uint8_t *>(blob.data());
    for (size_t i = 0; alphabet[i]; i++) b[8 * 4 + i] = d.cls[(unsigned char)alphabet[i]];
    for (uint32_t st = 0; st < d.n_states; st++)
        b[flags_off + st] = (uint8_t)((d.match_now[st] ? 1 : 0) | (d.match_at_end[st] ? 2 : 0) | (d.dead[st] ? 4 : 0));
    uint16_t *t = reinterpret_cast<uint16_t *>(b + trans_off);
    for (size_t i = 0; i < (size_t)d.n_states * d.n_cls; i++) t[i] = (uint16_t)d.trans[i];
    return true;
}

}  // namespace

// ---- score specifications -----------------------------------------------------------------------------------------

bool is_score_spec(const std::string &pattern) { return pattern.compare(0, 6, "score:") == 0; }

bool score_parse(const std::string &spec, ScoreTerms &out, std::string &err) {
    memset(&out, 0, sizeof out);
    if (!is_score_spec(spec)) {
        err = "a score specification starts with 'score:'";
        return false;
    }
    size_t pos = 6;
    for (;;) {
        size_t e = spec.find('&', pos);
        if (e == std::string::npos) e = spec.size();
        const std::string term = spec.substr(pos, e - pos);
        const std::string at = "score term " + std::to_string(out.n + 1) + ": ";
        if (term.empty()) {
            err = at + "empty (terms are '<metric>>=<n>' joined by '&')";
            return false;
        }
        if (out.n == SCORE_MAX_TERMS) {
            err = "a score specification has at most " + std::to_string(SCORE_MAX_TERMS) + " terms";
            return false;
        }
        const size_t ge = term.find(">=");
        if (ge == std::string::npos || ge == 0) {
            err = at + "'" + term + "' is not '<metric>>=<n>'";
            return false;
        }
        const std::string metric = term.substr(0, ge), num = term.substr(ge + 2);
        auto &t = out.t[out.n];
        auto hex_digit = [](char c) -> int {
            const char *q = c ? strchr(HEXL, (char)tolower((unsigned char)c)) : nullptr;
            return q ? (int)(q - HEXL) : -1;
        };
        if (metric == "zero-bytes") {
            t.metric = SCORE_ZERO_BYTES;
        } else if (metric == "leading-zero-bytes") {
            t.metric = SCORE_LEADING_ZERO_BYTES;
        } else if ((metric.compare(0, 8, "leading:") == 0 && metric.size() == 9 && hex_digit(metric[8]) >= 0) ||
                   (metric.compare(0, 6, "count:") == 0 && metric.size() == 7 && hex_digit(metric[6]) >= 0)) {
            t.metric = metric[0] == 'l' ? SCORE_LEADING_DIGIT : SCORE_COUNT_DIGIT;
            t.digit = (uint32_t)hex_digit(metric.back());
        } else {
            err = at + "unknown metric '" + metric + "' (zero-bytes, leading-zero-bytes, leading:<hex digit>, count:<hex digit>)";
            return false;
        }
        if (num.empty() || num.size() > 3 || num.find_first_not_of("0123456789") != std::string::npos) {
            err = at + "'" + num + "' is not a number";
            return false;
        }
        t.min = (uint32_t)atoi(num.c_str());
        if (t.min > score_metric_max(t.metric)) {
            err = at + "'" + metric + "' is at most " + std::to_string(score_metric_max(t.metric));
            return false;
        }
        out.n++;
        if (e == spec.size()) break;
        pos = e + 1;
    }
    return true;
}

namespace {

U256 div_small(const U256 &a, uint32_t d) {   // exact or rounded down
    U256 r;
    unsigned __int128 rem = 0;
    for (int i = 3; i >= 0; i--) {
        const unsigned __int128 cur = (rem << 64) | a.w[i];
        r.w[i] = (uint64_t)(cur / d);
        rem = cur % d;
    }
    return r;
}

// payloads (of 2^160) on which one term holds
U256 score_term_payloads(uint32_t metric, uint32_t min) {
    const bool bytes = metric == SCORE_ZERO_BYTES || metric == SCORE_LEADING_ZERO_BYTES;
    const uint32_t N = bytes ? 20 : 40, other = bytes ? 255 : 15, bits = bytes ? 8 : 4;
    if (metric == SCORE_LEADING_ZERO_BYTES || metric == SCORE_LEADING_DIGIT) return U256::pow2(160 - bits * min);
    // sum over k = min .. N of C(N, k) * other^(N - k):  term_N = 1, term_(k-1) = term_k * other * k / (N - k + 1)
    U256 term = U256::from_u64(1), sum;
    for (uint32_t k = N;; k--) {
        if (k >= min) sum = add(sum, term);
        if (k == 0 || k <= min) break;
        term = div_small(mul_small(term, other * k), N - k + 1);
    }
    return sum;
}

}  // namespace

void score_odds(const ScoreTerms &s, double *selectivity, uint64_t *difficulty) {
    U256 t = U256::pow2(160);
    for (uint32_t k = 0; k < s.n && k < SCORE_MAX_TERMS; k++) t = umin(t, score_term_payloads(s.t[k].metric, s.t[k].min));
    if (selectivity) *selectivity = to_double(t) / 1461501637330902918203684832716283019655932542976.0;   // 2^160
    if (!difficulty) return;
    // floor(2^160 / t) by long division, saturating
    unsigned __int128 q = 0;
    U256 r;
    for (int bit = 160; bit >= 0; bit--) {
        r = add(r, r);
        if (bit == 160) r.w[0] |= 1;
        q <<= 1;
        if (cmp(r, t) >= 0) {
            r = sub(r, t);
            q |= 1;
        }
        if (q >> 64) break;
    }
    *difficulty = (q >> 64) ? UINT64_MAX : (uint64_t)q;
}

bool score_of(const vgen_filter &f, const std::string &address, const uint8_t *payload, uint32_t *score, bool *accepted) {
    if (f.score.n == 0) return false;
    uint8_t buf[32];
    if (!payload) {
        if (!payload_from_address(f.format, address, buf)) return false;
        payload = buf;
    }
    u32 w[5];
    memcpy(w, payload, 20);
    u32 sc = 0;
    const bool ok = score_eval(f.score, w, &sc);
    if (score) *score = sc;
    if (accepted) *accepted = ok;
    return true;
}

bool filter_compile(const std::string &pattern, bool case_insensitive, uint32_t format, vgen_filter &out,
                    std::string &err) {
    out.pattern = pattern;
    out.case_insensitive = case_insensitive;
    out.format = format;
    memset(&out.dev, 0, sizeof out.dev);
    memset(&out.score, 0, sizeof out.score);
    if (is_score_spec(pattern)) {   // (the reserved prefix: case_insensitive plays no part)
        if (!vgf_is_hex((int)format)) {
            err = "a score specification scores the hex digits of an address: ethereum, ethereum-contract and ethereum-create2 only";
            return false;
        }
        if (!score_parse(pattern, out.score, err)) return false;
        out.dev.kind = DEVF_SCORE;
        score_odds(out.score, &out.selectivity, nullptr);
        return true;
    }
    if (!regex_compile(pattern, case_insensitive, out.dfa, err)) return false;
    if (out.dfa.lazy) {
        // no DFA tables (regex_dfa.h): nothing to derive a device test from — the reference's mode, every key to the host
        out.dev.kind = DEVF_HOST_ALL;
        out.selectivity = 1.0;
        return true;
    }
    switch (format) {
    case VGF_P2PKH:
    case VGF_P2PKH_UNCOMPRESSED:
        derive_base58(out.dfa, 0x00, out.dev, out.selectivity);
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(out.dfa, "", B58, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    case VGF_P2SH_P2WPKH:
        derive_base58(out.dfa, 0x05, out.dev, out.selectivity);
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(out.dfa, "", B58, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    case VGF_P2WPKH: {
        const SymSpec sp = {"bc1q", BECH32, 5, 32, 6, 160};
        derive_symbols(out.dfa, sp, out.dev, out.selectivity);
        out.dev.witver = 0;
        if (out.dev.flags & DEVF_FLAG_BECH32_CHK) {
            // chk(H) = chk(0) ^ XOR_i (chk(only byte i set to b) ^ chk(0)): the polymod is linear over GF(2)
            const u32 zero[5] = {0, 0, 0, 0, 0};
            const u32 base = bech32_checksum_bc20(zero, 0);
            out.chk_lut.assign(20 * 256, 0);
            for (int i = 0; i < 20; i++)
                for (u32 b = 0; b < 256; b++) {
                    u32 H[5] = {0, 0, 0, 0, 0};
                    H[i / 4] = b << (24 - 8 * (i % 4));
                    out.chk_lut[(size_t)i * 256 + b] = bech32_checksum_bc20(H, 0) ^ base;
                }
            out.dev.chk_base = base;
            out.dev.chk_lut = out.chk_lut.data();   // host pointer; the runtime swaps in the device copy
        }
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(out.dfa, "bc1q", BECH32, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    }
    case VGF_ETHEREUM:
    case VGF_ETHEREUM_CONTRACT:
    case VGF_ETHEREUM_CREATE2: {   // (a contract address is an address string like the account's)
        // EIP-55 casing depends on a second Keccak the kernel does not compute: derive the device
        // test from the case-insensitive language (a superset); the host confirms with the exact DFA.
        Dfa folded;
        std::string e2;
        if (!regex_compile(pattern, true, folded, e2)) {
            err = e2;
            return false;
        }
        if (folded.lazy) {
            out.dev.kind = DEVF_HOST_ALL;
            out.selectivity = 1.0;
            return true;
        }
        const SymSpec sp = {"0x", HEXL, 4, 40, 0, 160};
        derive_symbols(folded, sp, out.dev, out.selectivity);
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(folded, "0x", HEXL, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    }
    case VGF_NOSTR: {
        // npub1 + 52 data symbols (256 key bits + 4 pad bits: the last data symbol is q or s) + 6 Bech32 checksum symbols
        const SymSpec sp = {"npub1", BECH32, 5, 52, 6, 256, 52};
        derive_symbols(out.dfa, sp, out.dev, out.selectivity);
        out.dev.witver = 0;
        if (out.dev.flags & DEVF_FLAG_BECH32_CHK) {   // the checksum as an affine map of the 32 key bytes, as for P2TR
            const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const u32 base = bech32_checksum_npub(zero);
            out.chk_lut.assign(32 * 256, 0);
            for (int i = 0; i < 32; i++)
                for (u32 b = 0; b < 256; b++) {
                    u32 H[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    H[i / 4] = b << (24 - 8 * (i % 4));
                    out.chk_lut[(size_t)i * 256 + b] = bech32_checksum_npub(H) ^ base;
                }
            out.dev.chk_base = base;
            out.dev.chk_lut = out.chk_lut.data();
        }
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(out.dfa, "npub1", BECH32, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    }
    case VGF_SOLANA:
        derive_solana(out.dfa, out.dev, out.selectivity);
        break;
    case VGF_ONION:
        derive_onion(out.dfa, out.dev, out.selectivity);
        break;
    case VGF_P2TR: {
        // bc1p + 52 data symbols (256 bits + 4 pad bits) + 6 Bech32m checksum symbols
        const SymSpec sp = {"bc1p", BECH32, 5, 52, 6, 256};
        derive_symbols(out.dfa, sp, out.dev, out.selectivity);
        out.dev.witver = 1;
        if (out.dev.flags & DEVF_FLAG_BECH32_CHK) {
            const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const u32 base = bech32_checksum_bc<8>(zero, 1);
            out.chk_lut.assign(32 * 256, 0);
            for (int i = 0; i < 32; i++)
                for (u32 b = 0; b < 256; b++) {
                    u32 H[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    H[i / 4] = b << (24 - 8 * (i % 4));
                    out.chk_lut[(size_t)i * 256 + b] = bech32_checksum_bc<8>(H, 1) ^ base;
                }
            out.dev.chk_base = base;
            out.dev.chk_lut = out.chk_lut.data();
        }
        if (out.dev.kind == DEVF_HOST_ALL && build_dfa_blob(out.dfa, "bc1p", BECH32, out.dfa_blob)) out.dev.kind = DEVF_DFA;
        break;
    }
    default:
        out.dev.kind = DEVF_HOST_ALL;
        out.selectivity = 1.0;
        break;
    }
    if (out.dev.kind == DEVF_DFA) {
        out.dev.dfa_blob = out.dfa_blob.data();   // host pointer; the runtime swaps in the device copy
        out.dev.dfa_bytes = (uint32_t)(out.dfa_blob.size() * 4);
        out.selectivity = -1.0;                   // unknown: the scanner adapts (ring overflow -> host filtering)
    }
    return true;
}

// ---- pattern lists ------------------------------------------------------------------------------------------------

namespace {

constexpr size_t LIST_MAX_RANGES = 4096;   // payload ranges of one pattern (a single pattern's prefilter takes DEVF_MAX_TESTS)

struct Range64 {
    uint64_t lo, hi;
    uint32_t pat;
};

// top 64 bits of a 160-bit value held in a U256
uint64_t top64_of160(const U256 &a) { return (a.w[1] >> 32) | (a.w[2] << 32); }

const char *const NOT_PREFIX =
    "is not a start-anchored prefix (a list takes patterns whose matches are ranges of the payload: suffixes, unanchored "
    "patterns and constraints on later symbols or the checksum run alone through vgen_filter_compile)";

// The top-64-bit ranges of one pattern, or a reason why it has none a list can use.
bool list_ranges(const std::string &pattern, bool ci, uint32_t format, uint32_t index, std::vector<Range64> &out, std::string &why) {
    Dfa d;
    std::string err;
    // Ethereum: the device sees the payload, not the EIP-55 casing: ranges of the case-folded language (the host confirms)
    if (!regex_compile(pattern, ci || vgf_is_hex((int)format), d, err)) {
        why = err;
        return false;
    }
    if (d.lazy) {
        why = NOT_PREFIX;
        return false;
    }
    const size_t first = out.size();
    if (format == VGF_P2PKH || format == VGF_P2PKH_UNCOMPRESSED || format == VGF_P2SH_P2WPKH) {
        if (d.match_now[0]) {
            why = "matches every address";
            return false;
        }
        std::vector<Prefix> prefixes;
        if (!enumerate_prefixes(d, 0, B58, 40, 200000, prefixes)) {
            why = NOT_PREFIX;
            return false;
        }
        for (auto &p : prefixes)
            if (!p.absorbing) {
                why = NOT_PREFIX;
                return false;
            }
        std::vector<Range> ranges;
        for (auto &p : prefixes) prefix_to_ranges(p.s, format == VGF_P2SH_P2WPKH ? 0x05 : 0x00, ranges);
        merge_ranges(ranges);
        if (ranges.size() > LIST_MAX_RANGES) {
            why = "needs more than " + std::to_string(LIST_MAX_RANGES) + " payload ranges";
            return false;
        }
        double total = 0;
        for (auto &r : ranges) total += to_double(sub(r.hi, r.lo)) + 1.0;
        if (total / 1.4615016373309029e48 > 0.999999) {
            why = "matches every address";
            return false;
        }
        for (auto &r : ranges) out.push_back({top64_of160(r.lo), top64_of160(r.hi), index});
    } else if (format == VGF_P2WPKH || format == VGF_P2TR || format == VGF_NOSTR || vgf_is_hex((int)format)) {
        const bool eth = vgf_is_hex((int)format);
        const char *head = eth ? "0x" : format == VGF_NOSTR ? "npub1" : format == VGF_P2TR ? "bc1p" : "bc1q";
        const char *alphabet = eth ? HEXL : BECH32;
        const unsigned bits = eth ? 4 : 5, n_data = eth ? 40 : (format == VGF_P2TR || format == VGF_NOSTR) ? 52 : 32;
        uint32_t st = 0;
        for (const char *h = head; *h && !d.match_now[st]; h++) st = step(d, st, (unsigned char)*h);
        if (d.match_now[st]) {
            why = "matches every address";
            return false;
        }
        std::vector<Prefix> prefixes;
        if (!enumerate_prefixes(d, st, alphabet, n_data, 200000, prefixes)) {
            why = NOT_PREFIX;
            return false;
        }
        for (auto &p : prefixes)
            if (!p.absorbing) {
                why = NOT_PREFIX;
                return false;
            }
        if (prefixes.size() > LIST_MAX_RANGES) {
            why = "needs more than " + std::to_string(LIST_MAX_RANGES) + " payload ranges";
            return false;
        }
        for (auto &p : prefixes) {
            // a top-aligned bit prefix: the symbols' bits from the payload's most significant bit on, cut at 64
            uint64_t v = 0;
            unsigned pos = 0;
            for (char c : p.s) {
                const unsigned sym = (unsigned)(strchr(alphabet, c) - alphabet);
                for (int k = (int)bits - 1; k >= 0; k--, pos++)
                    if (pos < 64 && ((sym >> k) & 1)) v |= 1ull << (63 - pos);
            }
            const uint64_t low = pos >= 64 ? 0 : (pos == 0 ? ~0ull : (1ull << (64 - pos)) - 1);
            if (pos == 0) {
                why = "matches every address";
                return false;
            }
            out.push_back({v, v | low, index});
        }
    } else {
        why = "unknown address format";
        return false;
    }
    if (out.size() == first) {
        why = "matches no address of this format";
        return false;
    }
    return true;
}

}  // namespace

DevPtab PatternList::view() const {
    DevPtab t;
    t.bitmap = bitmap.data();
    t.offsets = offsets.data();
    t.lo = lo.data();
    t.hi = hi.data();
    t.bits = bits;
    t.n = (uint32_t)lo.size();
    return t;
}

const Dfa &PatternList::dfa_of(uint32_t i, bool case_insensitive) const {
    if (const Dfa *d = dfa[i].load(std::memory_order_acquire)) return *d;
    std::lock_guard<std::mutex> g(mu);
    if (const Dfa *d = dfa[i].load(std::memory_order_relaxed)) return *d;
    Dfa *d = new Dfa();
    std::string err;
    (void)regex_compile(patterns[i], case_insensitive, *d, err);   // compiled once already (filter_compile_list)
    dfa[i].store(d, std::memory_order_release);
    return *d;
}

PatternList::~PatternList() {
    if (dfa)
        for (size_t i = 0; i < patterns.size(); i++) delete dfa[i].load(std::memory_order_relaxed);
}

bool filter_compile_list(const std::string &text, bool case_insensitive, uint32_t format, vgen_filter &out, std::string &err) {
    std::shared_ptr<PatternList> L = std::make_shared<PatternList>();
    std::vector<Range64> ranges;
    std::unordered_map<std::string, uint32_t> seen;   // pattern -> its line
    size_t pos = 0;
    uint32_t line = 0;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string p = text.substr(pos, e - pos);
        pos = e + 1;
        line++;
        if (!p.empty() && p.back() == '\r') p.pop_back();
        if (p.empty() || p[0] == '#') continue;
        const std::string at = "line " + std::to_string(line) + ": ";
        auto dup = seen.find(p);
        if (dup != seen.end()) {
            err = at + "duplicate of line " + std::to_string(dup->second);
            return false;
        }
        if (L->patterns.size() >= LIST_MAX_PATTERNS) {
            err = at + "more than " + std::to_string(LIST_MAX_PATTERNS) + " patterns";
            return false;
        }
        std::string why;
        if (!list_ranges(p, case_insensitive, format, (uint32_t)L->patterns.size(), ranges, why)) {
            err = at + "'" + p + "' " + why;
            return false;
        }
        seen.emplace(p, line);
        L->patterns.push_back(p);
    }
    if (L->patterns.empty()) {
        err = "the pattern list is empty";
        return false;
    }
    // disjoint intervals: sweep the range boundaries; between two boundaries the set of covering patterns is constant
    struct Ev {
        uint64_t at;    // first value of the piece the event opens / closes before
        bool open;
        bool past_end;  // a close at 2^64 (hi = 2^64 - 1)
        uint32_t pat;
    };
    std::vector<Ev> ev;
    ev.reserve(ranges.size() * 2);
    for (auto &r : ranges) {
        ev.push_back({r.lo, true, false, r.pat});
        ev.push_back({r.hi + 1, false, r.hi == ~0ull, r.pat});
    }
    std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) {
        if (a.past_end != b.past_end) return !a.past_end;
        return a.at < b.at;
    });
    std::map<uint32_t, uint32_t> active;   // pattern -> ranges of it covering the current point
    L->pat_off.push_back(0);
    size_t k = 0;
    while (k < ev.size()) {
        const uint64_t at = ev[k].at;
        const bool end = ev[k].past_end;
        while (k < ev.size() && ev[k].at == at && ev[k].past_end == end) {
            if (ev[k].open) active[ev[k].pat]++;
            else if (--active[ev[k].pat] == 0) active.erase(ev[k].pat);
            k++;
        }
        if (active.empty() || end) continue;
        // the piece [at, next boundary - 1]
        const uint64_t hi = k < ev.size() && !ev[k].past_end ? ev[k].at - 1 : ~0ull;
        L->lo.push_back(at);
        L->hi.push_back(hi);
        for (auto &a : active) L->pat_idx.push_back(a.first);
        L->pat_off.push_back((uint32_t)L->pat_idx.size());
    }
    // first level: about two buckets per interval, 16 .. 24 bits
    const size_t n = L->lo.size();
    unsigned b = 16;
    while (b < 24 && ((size_t)1 << b) < 2 * n) b++;
    L->bits = b;
    const uint64_t nb = 1ull << b;
    L->bitmap.assign((size_t)(nb / 32), 0);
    L->offsets.assign((size_t)nb + 1, (uint32_t)n);
    double covered = 0;
    size_t j = 0;
    for (uint64_t q = 0; q < nb; q++) {
        const uint64_t first = q << (64 - b), last = first | ((1ull << (64 - b)) - 1);
        while (j < n && L->hi[j] < first) j++;
        L->offsets[q] = (uint32_t)j;
        if (j < n && L->lo[j] <= last) L->bitmap[q >> 5] |= 1u << (q & 31);
    }
    for (size_t i = 0; i < n; i++) covered += (double)(L->hi[i] - L->lo[i]) + 1.0;
    L->dfa.reset(new std::atomic<const Dfa *>[L->patterns.size()]);
    for (size_t i = 0; i < L->patterns.size(); i++) L->dfa[i].store(nullptr, std::memory_order_relaxed);
    // the list's identity: pattern texts, case flag, format
    std::string id;
    for (auto &p : L->patterns) {
        id += p;
        id.push_back('\n');
    }
    id += case_insensitive ? "i" : "-";
    id += std::to_string(format);
    host_sha256((const uint8_t *)id.data(), id.size(), L->digest);

    out.pattern.clear();
    out.case_insensitive = case_insensitive;
    out.format = format;
    memset(&out.dev, 0, sizeof out.dev);
    out.dev.kind = DEVF_LIST;
    out.selectivity = covered / 18446744073709551616.0;
    out.list = L;
    return true;
}

bool payload_from_address(uint32_t format, const std::string &address, uint8_t out[32]) {
    std::string a = address;
    if (format == VGF_P2PKH || format == VGF_P2PKH_UNCOMPRESSED || format == VGF_P2SH_P2WPKH) {
        if (a.empty() || a.size() > 40) return false;
        uint8_t v[25] = {0};   // the 25-byte payload integer, big-endian
        for (char c : a) {
            const int dg = b58_digit(c);
            if (dg < 0) return false;
            unsigned carry = (unsigned)dg;
            for (int i = 24; i >= 0; i--) {
                carry += 58u * v[i];
                v[i] = (uint8_t)carry;
                carry >>= 8;
            }
            if (carry) return false;
        }
        memcpy(out, v + 1, 20);
    } else if (vgf_is_hex((int)format)) {
        if (a.size() != 42 || a[0] != '0' || (a[1] != 'x' && a[1] != 'X')) return false;
        for (int i = 0; i < 20; i++) {
            int hv[2];
            for (int h = 0; h < 2; h++) {
                const char c = (char)tolower((unsigned char)a[2 + 2 * i + h]);
                const char *q = c ? strchr(HEXL, c) : nullptr;
                if (!q) return false;
                hv[h] = (int)(q - HEXL);
            }
            out[i] = (uint8_t)(hv[0] << 4 | hv[1]);
        }
        return true;   // any casing decodes; the patterns' automata judge the string itself
    } else if (format == VGF_NOSTR) {
        return nip19_decode("npub", a, out);   // (strict: header, length, case, pad bits, checksum)
    } else if (format == VGF_SOLANA) {
        return solana_decode(a, out);          // (strict: the alphabet, exactly 32 bytes)
    } else if (format == VGF_ONION) {
        return onion_decode(a, out);           // (strict: length, lower case, the alphabet, version, checksum)
    } else if (format == VGF_P2WPKH || format == VGF_P2TR) {
        const size_t n_data = format == VGF_P2TR ? 52 : 32, len = 4 + n_data + 6;
        if (a.size() != len) return false;
        for (auto &c : a) c = (char)tolower((unsigned char)c);
        uint32_t acc = 0;
        int bits = 0;
        size_t o = 0;
        for (size_t i = 4; i < 4 + n_data; i++) {
            const char *q = a[i] ? strchr(BECH32, a[i]) : nullptr;
            if (!q) return false;
            acc = (acc << 5) | (uint32_t)(q - BECH32);
            bits += 5;
            if (bits >= 8) {
                bits -= 8;
                out[o++] = (uint8_t)(acc >> bits);
            }
        }
        // (the re-encoding below checks the header, the padding and the checksum; a mixed-case string is no address)
        bool lower = false, upper = false;
        for (char c : address) {
            lower = lower || (c >= 'a' && c <= 'z');
            upper = upper || (c >= 'A' && c <= 'Z');
        }
        if (lower && upper) return false;
    } else {
        return false;
    }
    // exact: the string must be the encoding of the payload it decodes to (version byte, checksum, padding)
    return address_from_payload(format, out) == a;
}

void filter_which(const vgen_filter &f, const std::string &address, const uint8_t *payload, std::vector<uint32_t> &out) {
    out.clear();
    if (f.score.n) {
        bool ok = false;
        if (score_of(f, address, payload, nullptr, &ok) && ok) out.push_back(0);
        return;
    }
    if (!f.list) {
        if (f.dfa.is_match(address)) out.push_back(0);
        return;
    }
    uint8_t buf[32];
    if (!payload) {
        if (!payload_from_address(f.format, address, buf)) return;
        payload = buf;
    }
    u32 w[2];
    memcpy(w, payload, 8);
    const PatternList &L = *f.list;
    const int j = ptab_find(L.view(), ptab_top64(w));
    if (j < 0) return;
    for (uint32_t k = L.pat_off[j]; k < L.pat_off[j + 1]; k++)
        if (L.dfa_of(L.pat_idx[k], f.case_insensitive).is_match(address)) out.push_back(L.pat_idx[k]);
}

bool filter_accepts(const vgen_filter &f, const std::string &address, const uint8_t *payload) {
    if (f.score.n) {
        bool ok = false;
        return score_of(f, address, payload, nullptr, &ok) && ok;
    }
    if (!f.list) return f.dfa.is_match(address);
    std::vector<uint32_t> w;
    filter_which(f, address, payload, w);
    return !w.empty();
}

}  // namespace vg
