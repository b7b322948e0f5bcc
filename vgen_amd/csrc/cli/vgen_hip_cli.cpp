// vgen_hip_cli.cpp — `vgen-hip`: a thin command line over the C ABI of libvgen_hip.so, reproducing the
// flag set, defaults and result writers of the reference's `generate` / `range` / `list-gpus` /
// `verify` commands (src/lib.rs:44-211 flags, :642-663 range parsing, :524 count 0 = unbounded,
// :825-865 --repeat, :879-974 writers, :1038-1086 formatting helpers).  SURVEY.md §8(f) item 1.
//
// `estimate` (lib.rs:345-375) reports the device rate.  Provider patterns resolve against a static table (host/provider.cpp), not the boha crate.  Deliberately absent: the TUI and any CPU scan path (`--no-gpu` is an
// error here: this build has no CPU backend).  Added: --seed (the reference seeds from OS entropy
// only), --devices (batch-striped multi-GPU scan), --frames, --checkpoint (resumable scans).
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/vgen_hip.h"

namespace {

volatile int32_t g_stop = 0;

void on_sigint(int) {
    if (g_stop) _exit(130);   // second Ctrl-C exits (lib.rs:1088-1097)
    g_stop = 1;
}

struct Opts {
    std::string cmd, pattern, format = "p2pkh", output = "text", file, range, key, address, devices = "0", checkpoint, provider_table;
    bool has_pattern = false, ignore_case = false, quiet = false, json = false, no_gpu = false;
    uint64_t count = 1, repeat = 1, seed = 0;
    std::string patterns_file;                // --patterns-file: one pattern per line, one scan (vgen_scan_list)
    bool has_patterns_file = false, count_given = false;
    uint64_t per_pattern = 1;                 // --per-pattern (0 = unbounded)
    bool no_endo = false;
    bool random_keys = false;
    bool best = false;                        // --best (score specifications): VGEN_SCAN_BEST
    uint32_t batch = 1u << 20, frames = 12;   // twelve frames own twelve hardware queues (runtime.cpp)
    uint32_t table_bits_max = 0;              // vgen_scan_config.table_bits_max (0 = the context's memory policy decides)
    uint64_t mem_budget = 0;                  // vgen_params.device_mem_budget_bytes (0 = automatic)
    int puzzle = 0;
    long prefix_length = -1;   // -l / --prefix-length (provider patterns)
    // -f ethereum-create2: the job of the salt search
    std::string deployer, init_code_hash, init_code_file, salt_prefix, salt_start;
    bool has_deployer = false, has_init_code_hash = false, has_init_code_file = false, has_salt_prefix = false, has_salt_start = false;
    // -f ethereum-create3: the same salt search through a CREATE3 factory (--deployer is the factory)
    std::string proxy_hash, salt_guard;
    bool has_proxy_hash = false, has_salt_guard = false, salt_guard_hash = false;
    // split-key search: --base-pubkey (generate), and the requester's `combine`
    std::string base_pubkey, secret_file, partial;
    std::string keypair_dir;                  // -f solana: one <address>.json per result, the 64-number array solana-keygen reads
    std::string key_dir;                      // -f onion: one directory <address>.onion per result, the three files Tor reads (mkp224o's layout)
    bool has_base = false;
    bool create3() const { return format == "ethereum-create3"; }
    bool any_create3_option() const { return has_proxy_hash || has_salt_guard || salt_guard_hash; }
    bool any_create2_option() const { return has_deployer || has_init_code_hash || has_init_code_file || has_salt_prefix || has_salt_start; }
};

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "Error: %s\n", msg.c_str());
    exit(1);
}

int format_id(const std::string &f) {
    if (f == "p2pkh") return VGEN_FMT_P2PKH;
    if (f == "p2wpkh") return VGEN_FMT_P2WPKH;
    if (f == "p2sh-p2wpkh" || f == "p2sh-p2-wpkh" || f == "p2shp2wpkh") return VGEN_FMT_P2SH_P2WPKH;
    if (f == "p2tr") return VGEN_FMT_P2TR;
    if (f == "ethereum") return VGEN_FMT_ETHEREUM;
    if (f == "ethereum-contract") return VGEN_FMT_ETHEREUM_CONTRACT;
    if (f == "ethereum-create2") return VGEN_FMT_ETHEREUM_CREATE2;
    if (f == "ethereum-create3") return VGEN_FMT_ETHEREUM_CREATE2;   // no format of its own: a CREATE3 job on a format-7 context (Opts::create3)
    if (f == "p2pkh-uncompressed") return VGEN_FMT_P2PKH_UNCOMPRESSED;
    if (f == "nostr") return VGEN_FMT_NOSTR;
    if (f == "solana") return VGEN_FMT_SOLANA;
    if (f == "onion") return VGEN_FMT_ONION;
    die("invalid value '" + f + "' for '--format' (p2pkh, p2wpkh, p2sh-p2wpkh, p2tr, ethereum, ethereum-contract, ethereum-create2, ethereum-create3, nostr, solana, onion)");
}

const char *format_display(int id) {   // Display for AddressFormat, src/address.rs:48-58
    switch (id) {
    case VGEN_FMT_P2PKH: return "P2PKH";
    case VGEN_FMT_P2PKH_UNCOMPRESSED: return "P2PKH (Uncompressed)";
    case VGEN_FMT_P2WPKH: return "P2WPKH";
    case VGEN_FMT_P2SH_P2WPKH: return "P2SH-P2WPKH";
    case VGEN_FMT_P2TR: return "P2TR";
    case VGEN_FMT_ETHEREUM_CONTRACT: return "Ethereum contract (nonce 0)";   // (no comma: the csv writer keeps eight plain columns)
    case VGEN_FMT_ETHEREUM_CREATE2: return "Ethereum contract (CREATE2)";
    case VGEN_FMT_NOSTR: return "Nostr (npub)";
    case VGEN_FMT_SOLANA: return "Solana";
    case VGEN_FMT_ONION: return "Tor v3 onion";
    default: return "Ethereum";
    }
}

std::string format_duration(double secs) {   // lib.rs:1038-1052
    char b[64];
    if (secs < 1.0) snprintf(b, sizeof b, "%.0fms", secs * 1000.0);
    else if (secs < 60.0) snprintf(b, sizeof b, "%.1fs", secs);
    else if (secs < 3600.0) snprintf(b, sizeof b, "%.1fm", secs / 60.0);
    else if (secs < 86400.0) snprintf(b, sizeof b, "%.1fh", secs / 3600.0);
    else if (secs < 31536000.0) snprintf(b, sizeof b, "%.1fd", secs / 86400.0);
    else snprintf(b, sizeof b, "%.1fy", secs / 31536000.0);
    return b;
}

std::string with_commas(uint64_t n) {   // lib.rs:1075-1086
    std::string s = std::to_string(n), out;
    for (size_t i = 0; i < s.size(); i++) {
        if (i != 0 && (s.size() - i) % 3 == 0) out.push_back(',');
        out.push_back(s[i]);
    }
    return out;
}

std::string csv_escape(const std::string &f) {   // lib.rs:1058-1073
    if (f.find_first_of(",\"\n\r") == std::string::npos) return f;
    std::string out = "\"";
    for (char c : f) {
        if (c == '"') out.push_back('"');
        out.push_back(c);
    }
    return out + "\"";
}

std::string json_str(const std::string &s) {
    std::string o = "\"";
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') {
            o.push_back('\\');
            o.push_back((char)c);
        } else if (c < 0x20) {
            char b[8];
            snprintf(b, sizeof b, "\\u%04x", c);
            o += b;
        } else {
            o.push_back((char)c);
        }
    }
    return o + "\"";
}

std::string json_f64(double v) {
    char b[64];
    snprintf(b, sizeof b, "%.17g", v);
    double back = strtod(b, nullptr);
    for (int prec = 1; prec < 17; prec++) {   // shortest representation that round-trips
        char t[64];
        snprintf(t, sizeof t, "%.*g", prec, v);
        if (strtod(t, nullptr) == back) {
            snprintf(b, sizeof b, "%s", t);
            break;
        }
    }
    std::string s = b;
    if (s.find_first_of(".eE") == std::string::npos) s += ".0";
    return s;
}

bool parse_hex_key(const std::string &hex, uint8_t out[32]) {
    if (hex.empty() || hex.size() > 64) return false;
    memset(out, 0, 32);
    std::string h(64 - hex.size(), '0');
    h += hex;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return false;
        for (int j = 0; j < 2; j++) {
            char c = h[2 * i + j];
            if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'))) return false;
        }
        out[i] = (uint8_t)v;
    }
    return true;
}

// A mainnet WIF string (Base58Check of 0x80 | key [| 0x01]) taken apart WITHOUT its checksum being verified (the caller
// re-encodes the key and compares strings): the 32 key bytes, and whether the string claims a compressed public key.
bool parse_wif(const std::string &s, uint8_t key[32], bool *compressed) {
    static const char *alphabet = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
    if (s.size() < 50 || s.size() > 53) return false;
    std::vector<uint8_t> num;   // big-endian base-256 digits
    for (char ch : s) {
        const char *q = strchr(alphabet, ch);
        if (!q || !ch) return false;
        unsigned carry = (unsigned)(q - alphabet);
        for (size_t i = num.size(); i-- > 0;) {
            carry += 58u * num[i];
            num[i] = (uint8_t)carry;
            carry >>= 8;
        }
        while (carry) {
            num.insert(num.begin(), (uint8_t)carry);
            carry >>= 8;
        }
    }
    if ((num.size() != 37 && num.size() != 38) || num[0] != 0x80) return false;
    if (num.size() == 38 && num[33] != 0x01) return false;
    memcpy(key, num.data() + 1, 32);
    if (compressed) *compressed = num.size() == 38;
    return true;
}

void usage() {
    fprintf(stderr,
            "vgen-hip — MI355X scan engine for the vgen hot path\n\n"
            "  FORMAT: p2pkh (default), p2wpkh, p2sh-p2wpkh, p2tr, p2pkh-uncompressed, ethereum, ethereum-contract (the address of the\n"
            "          contract the key's account creates with its FIRST transaction, nonce 0; results carry that account as `deployer`),\n"
            "          nostr (the Nostr public key npub1... of NIP-19: Bech32 of the BIP-340 x-only key; results carry the nsec1... secret key\n"
            "          as `wif` and the key's 32 bytes as `public_key_hex`; unseeded searches test three keys per curve point),\n"
            "          solana, onion (see below)\n"
            "  vgen-hip generate -p PATTERN [-f FORMAT] [-i] [-c COUNT] [-o text|json|jsonl|csv|minimal] [--file PATH]\n"
            "                    [--gpu-batch-size N] [--repeat N] [-q] [--seed S] [--devices 0,1,..|all] [--frames F]\n"
            "                    [--frames F]          (dispatches in flight, default 12; several searches on ONE device share it\n"
            "                                           evenly as long as their frames add up to twenty or fewer: 2 x 8, 3 x 6 ...)\n"
            "                    [--seed S]            (a reproducible search: base key / candidate stream derived from the 64-bit S —\n"
            "                                           for tests and benchmarks; keys found this way are only as secret as S)\n"
            "                    [--checkpoint FILE]   (resume an interrupted scan from FILE; written as the scan runs)\n"
            "                    [--mem-budget-gib G]  (device memory each context may hold; default: its frames, and no generator table\n"
            "                                           larger than half of the device's free memory)\n"
            "                    [--table-bits-max B]  (P2TR / --random-keys: the widest generator table a long scan may move to —\n"
            "                                           24: 11.8 GB, 27: 21.5 GB, 29: 138 GB (+12.5 %%); built behind the scan, never waited for)\n"
            "                    [--no-endo]           (unseeded searches, any format but P2TR, test six keys per curve\n"
            "                                           point — k, lambda k, lambda^2 k and their negations; this walks k0 + i only)\n"
            "                    [--random-keys]       (an independent random key per candidate, drawn on the device — the shape of\n"
            "                                           the reference's CPU path, src/scanner.rs:118-169 —, six keys per draw unless\n"
            "                                           --no-endo; ~3x slower than the walk)\n"
            "                    PATTERN may be a provider pattern boha:b1000:N [-l PREFIX_LENGTH] [--provider-table CSV]\n"
            "  vgen-hip generate -f ethereum-create2 -p PATTERN --deployer 0xADDR (--init-code-hash 0xHASH | --init-code-file FILE)\n"
            "                    [--salt-prefix 0xHEX] [--salt-start N] [-c COUNT] [-i] [--devices ..] [-o ..]   (CREATE2, EIP-1014: searches the\n"
            "                    SALT salt_prefix (up to 24 bytes, zero padded) || 8-byte counter from N on; the printed key is the salt, and the\n"
            "                    address exists only when exactly this deployer runs CREATE2 with exactly this init code)\n"
            "  vgen-hip generate -f ethereum|ethereum-contract|ethereum-create2 -p 'score:TERM[&TERM..]' [--best] ...   (rank hex addresses: up to\n"
            "                    four terms METRIC>=N with the metrics zero-bytes, leading-zero-bytes, leading:H and count:H (H a hex digit);\n"
            "                    results carry a score, the value of the first term's metric.  --best reports only results that beat every\n"
            "                    score before them, -c then bounds the number of improvements.  range and estimate take such a pattern too)\n"
            "  vgen-hip generate -f ethereum-create3 -p PATTERN --deployer 0xFACTORY [--proxy-init-code-hash 0xHASH] [--salt-guard 0xHEX | --salt-guard-hash]\n"
            "                    [--salt-prefix 0xHEX] [--salt-start N] [-c COUNT] [-i] [--devices ..] [-o ..]   (CREATE3: the contract the factory's\n"
            "                    proxy deploys, whatever its init code; searches the RAW salt as above.  --salt-guard: the 0 - 64 bytes the factory\n"
            "                    hashes in front of the salt, e.g. the sender's 20 bytes; --salt-guard-hash: it hashes the salt alone)\n"
            "  vgen-hip generate -p PATTERN --base-pubkey HEX [-f FORMAT] ...   (split-key search for somebody else: HEX is the requester's public\n"
            "                    key, 33 or 65 bytes; the search walks P + k*G and prints the PARTIAL key k - not a key to anything by itself,\n"
            "                    never a WIF.  Only the holder of the secret behind HEX can form the final key: `combine`.  Every key-owned\n"
            "                    format; with --no-endo, --seed, --random-keys, --devices, -c, score: patterns and every writer.  Not with\n"
            "                    --checkpoint, --patterns-file or range: unsupported for split-key searches)\n"
            "  vgen-hip combine --secret-file PATH --partial HEX --address ADDR [-f FORMAT]   (the requester's side: PATH holds the secret, 32\n"
            "                    bytes or 64 hex digits - never on the command line; prints the final key (secret + partial) mod n, under the\n"
            "                    image that gives ADDR, as the format prints keys; fails if no image of the sum has that address)\n"
            "  vgen-hip generate -f solana -p PATTERN [-i] [-c COUNT] [-o ..] [--devices ..] [--seed S] [--keypair-dir DIR]   (Solana addresses:\n"
            "                    Base58 of an Ed25519 public key.  The key is the 32-byte SEED; every candidate is an independent draw (--random-keys\n"
            "                    and --no-endo are accepted and change nothing).  Results carry the seed in hex and the keypair string wallets\n"
            "                    import; --keypair-dir writes DIR/<address>.json, the 64-number array solana-keygen reads, mode 0600.  --seed makes\n"
            "                    the keys guessable.  estimate takes the format; range, --checkpoint, --patterns-file and --base-pubkey do not)\n"
            "  vgen-hip generate -f onion -p PATTERN [-i] [-c COUNT] [-o ..] [--devices ..] [--seed S] [--key-dir DIR]   (Tor v3 onion addresses:\n"
            "                    56 Base32 characters a-z2-7, printed with .onion.  The key is the Ed25519 SCALAR and the search walks a, a + 8,\n"
            "                    a + 16, ...: THE KEYS OF ONE RUN ARE NEIGHBOURS - whoever learns one of them and the run's other addresses can\n"
            "                    derive the others, so keys for different parties come from different runs.  Results carry the 64-byte expanded\n"
            "                    secret key in hex; --key-dir writes DIR/<address>.onion/ with hs_ed25519_secret_key, hs_ed25519_public_key and\n"
            "                    hostname, modes 0700 / 0600.  --random-keys and --no-endo are accepted and change nothing; --seed makes the keys\n"
            "                    guessable.  estimate takes the format; range, --checkpoint, --patterns-file, --base-pubkey and verify do not)\n"
            "  vgen-hip generate --patterns-file FILE [--per-pattern N] ...   (instead of -p: one start-anchored prefix per line,\n"
            "                    one scan; N results per pattern (default 1, 0 = unbounded), -c caps the total (default: none);\n"
            "                    each result's pattern field is the lowest-index line it satisfies.  range takes it too)\n"
            "  vgen-hip range (--range START:END | --puzzle P) [-p PATTERN] [-f FORMAT] [-c COUNT (0 = whole range)] ...\n"
            "  vgen-hip estimate -p PATTERN [-f FORMAT] [-i]\n"
            "  vgen-hip verify -k WIF_OR_HEX [-a ADDRESS]\n"
            "  vgen-hip list-gpus [--json]\n");
}

Opts parse(int argc, char **argv) {
    Opts o;
    if (argc < 2) {
        usage();
        exit(2);
    }
    o.cmd = argv[1];
    if (o.cmd == "range") o.count = 1;
    // clap's spellings of one argument: --name=value, -nVALUE, and boolean shorts run together (-iq) — split up front.  Only
    // words in OPTION position are reinterpreted: the word after an option that takes a value is that value, verbatim, whatever
    // it starts with (`-p -abc` is the pattern "-abc", not three flags).
    static const char *const long_with_value[] = {"--pattern", "--format", "--count", "--output", "--file", "--gpu-batch-size", "--repeat",
                                                  "--seed", "--devices", "--frames", "--checkpoint", "--range", "--puzzle", "--key", "--address",
                                                  "--prefix-length", "--provider-table", "--threads", "--backend", "--cpu-batch-size", "--table-bits-max",
                                                  "--mem-budget-gib", "--patterns-file", "--per-pattern", "--deployer", "--init-code-hash", "--init-code-file",
                                                  "--salt-prefix", "--salt-start", "--proxy-init-code-hash", "--salt-guard", "--base-pubkey", "--secret-file", "--partial", "--keypair-dir", "--key-dir"};
    static const char short_with_value[] = "pfcorkaltT";
    std::vector<std::string> args;
    bool next_is_value = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (next_is_value) {
            args.push_back(a);
            next_is_value = false;
            continue;
        }
        const size_t eq = a.find('=');
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            if (eq != std::string::npos) {
                args.push_back(a.substr(0, eq));
                args.push_back(a.substr(eq + 1));
            } else {
                args.push_back(a);
                for (const char *name : long_with_value) next_is_value = next_is_value || a == name;
            }
        } else if (a.size() >= 2 && a[0] == '-' && a[1] != '-') {
            for (size_t k = 1; k < a.size(); k++) {
                const char ch = a[k];
                args.push_back(std::string("-") + ch);
                if (strchr(short_with_value, ch)) {   // takes a value: the rest of the word (after an optional '=') is it, else the next word
                    std::string rest = a.substr(k + 1);
                    if (!rest.empty() && rest[0] == '=') rest = rest.substr(1);
                    if (!rest.empty()) args.push_back(rest);
                    else next_is_value = true;
                    break;
                }
            }
        } else {
            args.push_back(a);
        }
    }
    for (size_t i = 0; i < args.size(); i++) {
        const std::string a = args[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= args.size()) die("a value is required for '" + a + "'");
            return args[++i];
        };
        if (a == "-p" || a == "--pattern") { o.pattern = val(); o.has_pattern = true; }
        else if (a == "-f" || a == "--format") o.format = val();
        else if (a == "-i" || a == "--ignore-case") o.ignore_case = true;
        else if (a == "-c" || a == "--count") { o.count = strtoull(val().c_str(), nullptr, 10); o.count_given = true; }
        else if (a == "--patterns-file") { o.patterns_file = val(); o.has_patterns_file = true; }
        else if (a == "--per-pattern") o.per_pattern = strtoull(val().c_str(), nullptr, 10);
        else if (a == "-o" || a == "--output") o.output = val();
        else if (a == "--file") o.file = val();
        else if (a == "--gpu-batch-size") o.batch = (uint32_t)strtoul(val().c_str(), nullptr, 10);
        else if (a == "--repeat") o.repeat = strtoull(val().c_str(), nullptr, 10);
        else if (a == "-q" || a == "--quiet") o.quiet = true;
        else if (a == "--seed") o.seed = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--devices") o.devices = val();
        else if (a == "--frames") o.frames = (uint32_t)strtoul(val().c_str(), nullptr, 10);
        else if (a == "--checkpoint") o.checkpoint = val();
        else if (a == "--table-bits-max") o.table_bits_max = (uint32_t)strtoul(val().c_str(), nullptr, 10);
        else if (a == "--mem-budget-gib") o.mem_budget = (uint64_t)(strtod(val().c_str(), nullptr) * 1073741824.0);
        else if (a == "-r" || a == "--range") o.range = val();
        else if (a == "--puzzle") o.puzzle = atoi(val().c_str());
        else if (a == "-k" || a == "--key") o.key = val();
        else if (a == "-a" || a == "--address") o.address = val();
        else if (a == "--json") o.json = true;
        else if (a == "--no-gpu") o.no_gpu = true;
        else if (a == "--no-endo") o.no_endo = true;
        else if (a == "--random-keys") o.random_keys = true;
        else if (a == "--best") o.best = true;
        else if (a == "--no-tui" || a == "--tui") {}                                   // no TUI in this build
        else if (a == "-l" || a == "--prefix-length") o.prefix_length = strtol(val().c_str(), nullptr, 10);
        else if (a == "--provider-table") o.provider_table = val();
        else if (a == "--deployer") { o.deployer = val(); o.has_deployer = true; }
        else if (a == "--init-code-hash") { o.init_code_hash = val(); o.has_init_code_hash = true; }
        else if (a == "--init-code-file") { o.init_code_file = val(); o.has_init_code_file = true; }
        else if (a == "--salt-prefix") { o.salt_prefix = val(); o.has_salt_prefix = true; }
        else if (a == "--salt-start") { o.salt_start = val(); o.has_salt_start = true; }
        else if (a == "--proxy-init-code-hash") { o.proxy_hash = val(); o.has_proxy_hash = true; }
        else if (a == "--salt-guard") { o.salt_guard = val(); o.has_salt_guard = true; }
        else if (a == "--salt-guard-hash") o.salt_guard_hash = true;
        else if (a == "--base-pubkey") { o.base_pubkey = val(); o.has_base = true; }
        else if (a == "--secret-file") o.secret_file = val();
        else if (a == "--partial") o.partial = val();
        else if (a == "--keypair-dir") o.keypair_dir = val();
        else if (a == "--key-dir") o.key_dir = val();
        else if (a == "-t" || a == "--threads" || a == "--backend" || a == "--cpu-batch-size") (void)val();   // accepted, not applicable
        else if (a == "-h" || a == "--help") { usage(); exit(0); }
        else die("unexpected argument '" + a + "'");
    }
    return o;
}

std::vector<int> parse_devices(const std::string &s) {
    int n = 0;
    if (vgen_device_count(&n) != VGEN_OK || n <= 0) die("no HIP device available (this build has no CPU backend)");
    std::vector<int> out;
    if (s == "all") {
        for (int i = 0; i < n; i++) out.push_back(i);
        return out;
    }
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t c = s.find(',', pos);
        std::string t = s.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        if (t.empty()) die("bad --devices list");
        int d = atoi(t.c_str());
        if (d < 0 || d >= n) die("device " + t + " out of range (" + std::to_string(n) + " device(s))");
        out.push_back(d);
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    return out;
}

// resolve_pattern_and_format / the provider half of resolve_range_params (src/lib.rs:563-590,599-631):
// a "boha:..." pattern becomes the exact (or, with -l, prefix) pattern of the puzzle's address, selects the
// address format and, for `range` without an explicit range, supplies the key range.
struct Resolved {
    std::string pattern;
    bool from_provider = false, has_range = false;
    uint8_t start[32], end[32];
};

Resolved resolve_provider(Opts &o, bool for_range) {
    Resolved r;
    r.pattern = o.pattern;
    char addr[128];
    uint32_t fmt = 0;
    int32_t has_range = 0;
    const char *table = !o.provider_table.empty() ? o.provider_table.c_str() : getenv("VGEN_PROVIDER_TABLE");
    const int rc = vgen_provider_resolve(o.pattern.c_str(), table, addr, sizeof addr, &fmt, &has_range, r.start, r.end);
    if (rc < 0) die(vgen_last_error(nullptr));
    if (rc == 0) {
        if (o.prefix_length >= 0 && !for_range) fprintf(stderr, "Warning: --prefix-length is ignored for regex patterns\n");
        return r;
    }
    if (o.prefix_length == 0) die("--prefix-length must be at least 1 for provider patterns");
    char pat[300];
    vgen_provider_build_pattern(addr, o.prefix_length > 0 ? (uint32_t)o.prefix_length : 0, pat, sizeof pat);
    if (o.prefix_length > 0 || !for_range) fprintf(stderr, "Provider: %s → %s → pattern '%s'\n", o.pattern.c_str(), addr, pat);
    else fprintf(stderr, "Provider: %s → %s → exact match\n", o.pattern.c_str(), addr);
    static const char *names[] = {"p2pkh", "p2wpkh", "p2sh-p2wpkh", "p2tr", "p2pkh-uncompressed", "ethereum", "ethereum-contract", "ethereum-create2"};
    o.format = names[fmt];
    r.pattern = pat;
    r.from_provider = true;
    r.has_range = has_range != 0;
    return r;
}

// Warning for patterns that can never match (src/lib.rs:684-706).
void warn_impossible_pattern(const std::string &pattern, bool ignore_case, int fmt) {
    char bad[260];
    size_t n = 0;
    if (vgen_pattern_invalid_chars(pattern.c_str(), ignore_case, (uint32_t)fmt, bad, sizeof bad, &n) != VGEN_OK || n == 0) return;
    const char *cs = vgen_format_charset_name((uint32_t)fmt);
    fprintf(stderr, "Warning: Pattern contains characters not valid in %s addresses: '%s'\n", cs, bad);
    fprintf(stderr, "  %s alphabet excludes these characters - pattern will NEVER match!\n", cs);
    if (strcmp(cs, "Base58") == 0)
        fprintf(stderr, "  Base58 excludes: 0 (zero), O (uppercase o), I (uppercase i), l (lowercase L)\n");
    fprintf(stderr, "\n");
}

// -f ethereum-create2: the job of the salt search from the command line, checked before any device is opened.
struct Create2Job {
    uint8_t deployer[20] = {0}, init_code_hash[32] = {0}, salt_prefix[24] = {0};
    uint64_t first = 0;
};

// "0x" + hex digits (the 0x optional) -> at most `cap` bytes; the number of bytes, or -1
int parse_hex_bytes(const std::string &s, uint8_t *out, size_t cap) {
    const std::string h = s.compare(0, 2, "0x") == 0 || s.compare(0, 2, "0X") == 0 ? s.substr(2) : s;
    if (h.size() % 2 != 0 || h.size() / 2 > cap) return -1;
    for (size_t i = 0; i < h.size(); i++)
        if (!isxdigit((unsigned char)h[i])) return -1;
    for (size_t i = 0; i < h.size() / 2; i++) out[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    return (int)(h.size() / 2);
}

void salt_options(const Opts &o, uint8_t salt_prefix[24], uint64_t &first);   // --salt-prefix and --salt-start, below

Create2Job create2_job(const Opts &o, bool has_range, bool list) {
    if (o.cmd != "generate" || has_range) die("'-f ethereum-create2' searches salts: use it with 'generate' (no key range)");
    if (o.seed) die("the argument '--seed' cannot be used with '-f ethereum-create2' (the search walks salt counters from --salt-start)");
    if (o.random_keys) die("the argument '--random-keys' cannot be used with '-f ethereum-create2' (there are no keys)");
    if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f ethereum-create2'");
    if (list) die("the argument '--patterns-file' cannot be used with '-f ethereum-create2'");
    Create2Job j;
    if (!o.has_deployer) die("the following required arguments were not provided for '-f ethereum-create2': --deployer <0xADDRESS>");
    if (parse_hex_bytes(o.deployer, j.deployer, 20) != 20) die("--deployer must be an address of 20 bytes in hex");
    if (o.has_init_code_hash == o.has_init_code_file) die("exactly one of '--init-code-hash' and '--init-code-file' is required for '-f ethereum-create2'");
    if (o.has_init_code_hash) {
        if (parse_hex_bytes(o.init_code_hash, j.init_code_hash, 32) != 32) die("--init-code-hash must be 32 bytes in hex");
    } else {
        FILE *f = fopen(o.init_code_file.c_str(), "rb");
        if (!f) die("cannot read init code file '" + o.init_code_file + "'");
        std::string code;
        char buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) code.append(buf, n);
        fclose(f);
        vgen_keccak256(reinterpret_cast<const uint8_t *>(code.data()), code.size(), j.init_code_hash);   // the file's bytes as they are
    }
    salt_options(o, j.salt_prefix, j.first);
    return j;
}

// -f ethereum-create3: the job from the command line, checked before any device is opened.
struct Create3Job {
    uint8_t factory[20] = {0}, proxy_hash[32] = {0}, salt_prefix[24] = {0}, guard[64] = {0};
    int guard_len = -1;   // -1: the factory uses the raw salt
    uint64_t first = 0;
};

// --salt-guard / --salt-guard-hash -> the guard's length (-1: none); the bytes into guard[64]
int salt_guard(const Opts &o, uint8_t guard[64]) {
    if (o.has_salt_guard && o.salt_guard_hash) die("the argument '--salt-guard' cannot be used with '--salt-guard-hash' ('-f ethereum-create3')");
    if (o.salt_guard_hash) return 0;
    if (!o.has_salt_guard) return -1;
    const int n = parse_hex_bytes(o.salt_guard, guard, 64);
    if (n < 0) die("--salt-guard takes 0 to 64 bytes in hex ('-f ethereum-create3')");
    return n;
}

Create3Job create3_job(const Opts &o, bool has_range, bool list) {
    if (o.cmd != "generate" || has_range) die("'-f ethereum-create3' searches salts: use it with 'generate' (no key range)");
    if (o.seed) die("the argument '--seed' cannot be used with '-f ethereum-create3' (the search walks salt counters from --salt-start)");
    if (o.random_keys) die("the argument '--random-keys' cannot be used with '-f ethereum-create3' (there are no keys)");
    if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f ethereum-create3'");
    if (list) die("the argument '--patterns-file' cannot be used with '-f ethereum-create3'");
    if (o.has_init_code_file || o.has_init_code_hash)
        die("the arguments '--init-code-file' and '--init-code-hash' cannot be used with '-f ethereum-create3' (the address does not depend on the init code; see --proxy-init-code-hash)");
    Create3Job j;
    if (!o.has_deployer) die("the following required arguments were not provided for '-f ethereum-create3': --deployer <0xFACTORY>");
    if (parse_hex_bytes(o.deployer, j.factory, 20) != 20) die("--deployer must be an address of 20 bytes in hex");
    if (!o.has_proxy_hash) vgen_create3_proxy_hash(j.proxy_hash);
    else if (parse_hex_bytes(o.proxy_hash, j.proxy_hash, 32) != 32) die("--proxy-init-code-hash must be 32 bytes in hex");
    j.guard_len = salt_guard(o, j.guard);
    salt_options(o, j.salt_prefix, j.first);
    return j;
}

// (the tail of the CREATE2 job's parser, kept where it stood)
void salt_options(const Opts &o, uint8_t salt_prefix[24], uint64_t &first) {
    if (o.has_salt_prefix) {
        uint8_t pre[25];
        const std::string h = o.salt_prefix.compare(0, 2, "0x") == 0 || o.salt_prefix.compare(0, 2, "0X") == 0 ? o.salt_prefix.substr(2) : o.salt_prefix;
        if (h.size() > 48) die("--salt-prefix takes at most 24 bytes (the last 8 bytes of the salt are the counter)");
        const int n = parse_hex_bytes(o.salt_prefix, pre, 24);
        if (n < 0) die("--salt-prefix must be hex");
        memcpy(salt_prefix, pre, (size_t)n);   // left-aligned, zero padded
    }
    if (o.has_salt_start) {
        char *end = nullptr;
        errno = 0;
        first = strtoull(o.salt_start.c_str(), &end, 0);
        if (errno || !end || *end || o.salt_start.empty() || o.salt_start[0] == '-') die("--salt-start must be a counter below 2^64");
    }
}

std::string hex0x(const uint8_t *b, size_t n) {
    std::string s = "0x";
    char t[3];
    for (size_t i = 0; i < n; i++) {
        snprintf(t, sizeof t, "%02x", b[i]);
        s += t;
    }
    return s;
}

// `estimate` (src/lib.rs:345-375): difficulty heuristic over a measured rate.  The reference times its CPU
// generator (scanner.rs:333-346); here the rate is that of this pattern's scan on the device, over a
// bounded number of dispatches.
int run_estimate(Opts &o) {
    o.pattern = resolve_provider(o, false).pattern;
    const int fmt = format_id(o.format);
    vgen_filter *probe = nullptr;
    if (vgen_filter_compile(o.pattern.c_str(), o.ignore_case, (uint32_t)fmt, &probe) != VGEN_OK) die(vgen_last_error(nullptr));
    vgen_filter_free(probe);
    uint64_t difficulty = 0;
    vgen_pattern_difficulty(o.pattern.c_str(), o.ignore_case, (uint32_t)fmt, &difficulty);

    std::vector<int> devs = parse_devices(o.devices);
    vgen_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.device = devs[0];
    p.batch_size = o.batch;
    p.format = (uint32_t)fmt;
    p.frames = o.frames;
    vgen_ctx *c = nullptr;
    if (vgen_create(&p, &c) != VGEN_OK) die(std::string("GPU initialization failed: ") + vgen_last_error(nullptr));
    vgen_scan_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.format = (uint32_t)fmt;
    cfg.count = UINT64_MAX;
    cfg.case_insensitive = o.ignore_case;
    cfg.seed = fmt == VGEN_FMT_ETHEREUM_CREATE2 ? 0 : o.seed;
    uint8_t guard[64] = {0};
    const int guard_len = o.create3() ? salt_guard(o, guard) : -1;   // ethereum-create3: a guard costs a third block per salt
    double rate = 0;
    for (int pass = 0; pass < 2; pass++) {   // first pass warms the device up
        cfg.max_batches = pass ? 96 : 12;
        vgen_scan_result res;
        const uint8_t zero[32] = {0};   // ethereum-create2: the rate does not depend on the job
        const int rc = o.create3() ? vgen_scan_create3(&c, 1, o.pattern.c_str(), zero, zero, zero, guard, guard_len, 0, &cfg, nullptr, nullptr, &g_stop, &res)
                       : fmt == VGEN_FMT_ETHEREUM_CREATE2 ? vgen_scan_create2(&c, 1, o.pattern.c_str(), zero, zero, zero, 0, &cfg, nullptr, nullptr, &g_stop, &res)
                                                        : vgen_scan(c, o.pattern.c_str(), &cfg, nullptr, nullptr, &g_stop, &res);
        if (rc != VGEN_OK) die(vgen_last_error(c));
        rate = res.elapsed_secs > 0 ? (double)res.operations / res.elapsed_secs : 0.0;
        vgen_scan_result_free(&res);
    }
    vgen_destroy(c);
    printf("Pattern: %s\nFormat: %s\nCase insensitive: %s\n\n", o.pattern.c_str(), o.create3() ? "Ethereum contract (CREATE3)" : format_display(fmt),
           o.ignore_case ? "true" : "false");
    printf("Estimated difficulty: 1 in %llu\n", (unsigned long long)difficulty);
    printf("Benchmark rate: %.0f addr/sec\n", rate);
    printf("Expected time: %s\n", format_duration(rate > 0 ? (double)difficulty / rate : 0.0).c_str());
    return 0;
}

// The reference's spinner line (src/lib.rs:783-805: "[elapsed] Checked N addresses", hidden when stderr is not a terminal and
// with --quiet): redrawn at most ten times a second from the scan's progress callback.
struct Progress {
    uint64_t base = 0;      // operations of the finished --repeat rounds
    double last = 0, t0 = 0;
    bool shown = false;
};
double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
void progress_cb(uint64_t ops, void *user) {
    Progress *p = static_cast<Progress *>(user);
    const double t = now_s();
    if (t - p->last < 0.1) return;
    p->last = t;
    p->shown = true;
    const unsigned secs = (unsigned)(t - p->t0);
    fprintf(stderr, "\r[%02u:%02u:%02u] Checked %s addresses\x1b[K", secs / 3600, secs / 60 % 60, secs % 60, with_commas(p->base + ops).c_str());
    fflush(stderr);
}
void progress_clear(Progress &p) {
    if (p.shown) fprintf(stderr, "\r\x1b[K");
    p.shown = false;
}

// --patterns-file: the list, compiled before any device is opened.  A provider pattern or an invalid line ends the program
// (status 1) with its line number.
vgen_filter *load_pattern_list(const Opts &o, int fmt) {
    FILE *f = fopen(o.patterns_file.c_str(), "rb");
    if (!f) die("cannot read patterns file '" + o.patterns_file + "'");
    std::string text;
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    size_t pos = 0;
    for (unsigned line = 1; pos < text.size(); line++) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        if (text.compare(pos, 5, "boha:") == 0)
            die(o.patterns_file + ": line " + std::to_string(line) + ": provider patterns (boha:) cannot be part of a pattern list");
        pos = e + 1;
    }
    vgen_filter *list = nullptr;
    if (vgen_filter_compile_list(text.c_str(), o.ignore_case, (uint32_t)fmt, &list) != VGEN_OK)
        die(o.patterns_file + ": " + vgen_last_error(nullptr));
    return list;
}

// The text of the lowest-index pattern of `list` that `address` satisfies (a result's `pattern` field).
// -f solana --keypair-dir: DIR/<address>.json holds the 64 bytes seed || public key as a JSON array of numbers, the file
// `solana-keygen` and `solana config set --keypair` read; created with mode 0600 (a private key).
void write_keypair_file(const std::string &dir, const vgen_generated &g) {
    uint8_t kp[64];
    memcpy(kp, g.key, 32);
    if (vgen_solana_public_key(g.key, kp + 32) != VGEN_OK) die("a result of a solana search has no public key");
    const std::string path = dir + "/" + g.address + ".json";
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    if (fd < 0 || fchmod(fd, 0600) != 0) die("cannot write keypair file '" + path + "'");
    std::string text = "[";
    for (int i = 0; i < 64; i++) text += (i ? "," : "") + std::to_string(kp[i]);
    text += "]\n";
    const bool ok = write(fd, text.data(), text.size()) == (ssize_t)text.size();
    if (close(fd) != 0 || !ok) die("cannot write keypair file '" + path + "'");
}

// -f onion --key-dir: DIR/<address>.onion/ (mode 0700) with the three files of a Tor hidden-service directory, mode 0600 - mkp224o's layout.
void write_onion_dir(const std::string &dir, const vgen_generated &g, const uint8_t expanded[64], const uint8_t pub[32]) {
    const std::string d = dir + "/" + g.address + ".onion";
    if (mkdir(d.c_str(), 0700) != 0 && errno != EEXIST) die("cannot create key directory '" + d + "'");
    if (chmod(d.c_str(), 0700) != 0) die("cannot set the mode of key directory '" + d + "'");
    auto put = [&](const char *name, const std::string &body) {
        const std::string path = d + "/" + name;
        const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
        if (fd < 0 || fchmod(fd, 0600) != 0) die("cannot write key file '" + path + "'");
        const bool ok = write(fd, body.data(), body.size()) == (ssize_t)body.size();
        if (close(fd) != 0 || !ok) die("cannot write key file '" + path + "'");
    };
    put("hs_ed25519_secret_key", std::string("== ed25519v1-secret: type0 ==") + std::string(3, '\0') + std::string((const char *)expanded, 64));
    put("hs_ed25519_public_key", std::string("== ed25519v1-public: type0 ==") + std::string(3, '\0') + std::string((const char *)pub, 32));
    put("hostname", std::string(g.address) + ".onion\n");
}

std::string list_pattern_of(const vgen_filter *list, const char *address) {
    uint32_t idx = 0, n = 0;
    if (vgen_filter_which(list, address, &idx, 1, &n) != VGEN_OK || n == 0) return std::string();
    char buf[4096];
    return vgen_filter_pattern(list, idx, buf, sizeof buf) >= 0 ? std::string(buf) : std::string();
}

int run_search(const Opts &o, const std::string &pattern_arg, bool has_range, const uint8_t start[32], const uint8_t end[32],
               const vgen_filter *list = nullptr) {
    const std::string &pattern = pattern_arg;
    if (o.no_gpu) die("--no-gpu: this build has no CPU scan path (the MI355X engine is the only backend)");
    const int fmt = format_id(o.format);
    const bool create2 = fmt == VGEN_FMT_ETHEREUM_CREATE2;
    const bool create3 = o.create3();   // (then `create2` holds as well: the same context, scan loop and outputs, another job)
    if (!create2 && o.any_create2_option())
        die("'--deployer', '--init-code-hash', '--init-code-file', '--salt-prefix' and '--salt-start' belong to '-f ethereum-create2'");
    if (!create3 && o.any_create3_option())
        die("'--proxy-init-code-hash', '--salt-guard' and '--salt-guard-hash' belong to '-f ethereum-create3'");
    const bool solana = fmt == VGEN_FMT_SOLANA;
    if (solana) {   // a seed has no neighbour: nothing walks, nothing resumes, nothing splits
        if (has_range) die("'-f solana' cannot be used with 'range': a solana key is a seed whose scalar is its hash - there is no key range");
        if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f solana': checkpoints are not provided for this format");
        if (list) die("the argument '--patterns-file' cannot be used with '-f solana': pattern lists are not provided for this format");
        if (o.has_base) die("the argument '--base-pubkey' cannot be used with '-f solana': a seed cannot be split");
    } else if (!o.keypair_dir.empty()) die("the argument '--keypair-dir' belongs to '-f solana'");
    const bool onion = fmt == VGEN_FMT_ONION;
    if (onion) {   // the walk starts at the base scalar of the run's seed: no range, nothing resumes, no lists, nothing splits
        if (has_range) die("'-f onion' cannot be used with 'range': an onion search walks from the base scalar of its seed - there is no key range");
        if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f onion': checkpoints are not provided for this format");
        if (list) die("the argument '--patterns-file' cannot be used with '-f onion': pattern lists are not provided for this format");
        if (o.has_base) die("the argument '--base-pubkey' cannot be used with '-f onion': split keys are not provided for this format");
    } else if (!o.key_dir.empty()) die("the argument '--key-dir' belongs to '-f onion'");
    Create2Job job;
    Create3Job job3;
    if (create3) job3 = create3_job(o, has_range, list != nullptr);
    else if (create2) job = create2_job(o, has_range, list != nullptr);
    // surface pattern errors before touching the device (Pattern::new, pattern.rs:21-33)
    if (!list) {
        vgen_filter *probe = nullptr;
        if (vgen_filter_compile(pattern.c_str(), o.ignore_case, (uint32_t)fmt, &probe) != VGEN_OK) die(vgen_last_error(nullptr));
        vgen_filter_free(probe);
        warn_impossible_pattern(pattern, o.ignore_case, fmt);
    }

    // --base-pubkey: a split-key search, checked before any device is opened
    uint8_t base_pub[65];
    int base_len = 0;
    if (o.has_base) {
        if (create2) die("the argument '--base-pubkey' cannot be used with '-f " + o.format + "' (a salt search has no key to split)");
        if (has_range) die("the argument '--base-pubkey' cannot be used with 'range': key ranges are not supported for split-key searches");
        if (!o.checkpoint.empty()) die("the argument '--base-pubkey' cannot be used with '--checkpoint': checkpoints are not supported for split-key searches");
        if (list) die("the argument '--base-pubkey' cannot be used with '--patterns-file': pattern lists are not supported for split-key searches");
        base_len = parse_hex_bytes(o.base_pubkey, base_pub, sizeof base_pub);
        char probe[128];
        const uint8_t zero[32] = {0};
        if ((base_len != 33 && base_len != 65) || vgen_split_derive((uint32_t)fmt, base_pub, (size_t)base_len, zero, 0, probe, sizeof probe) < 0)
            die("--base-pubkey must be a secp256k1 public key in hex: 33 bytes (02 / 03 ..) or 65 bytes (04 ..)");
    }

    std::vector<int> devs = parse_devices(o.devices);
    std::vector<vgen_ctx *> ctxs;
    for (int d : devs) {
        vgen_params p;
        memset(&p, 0, sizeof p);
        p.struct_size = sizeof p;
        p.device = d;
        p.batch_size = o.batch;
        p.format = (uint32_t)fmt;
        p.frames = o.frames;
        p.device_mem_budget_bytes = o.mem_budget;
        // a vanity search proper — random base, no range, no seed, no checkpoint — may test any keys it likes:
        // six images per curve point (VGEN_FLAG_ENDO, +30 % keys per second); everything else walks k0 + i
        // (--random-keys: six keys per draw; seeds name candidate streams there, so they do not rule it out)
        if (!o.no_endo && fmt != 3 && !create2 && !solana && !onion && (o.random_keys || (!has_range && !o.seed && o.checkpoint.empty()))) p.flags |= VGEN_FLAG_ENDO;
        vgen_ctx *c = nullptr;
        if (vgen_create(&p, &c) != VGEN_OK) die(std::string("GPU initialization failed: ") + vgen_last_error(nullptr));
        if (o.has_base && vgen_set_base_point(c, base_pub, (size_t)base_len) != VGEN_OK) die(vgen_last_error(c));
        ctxs.push_back(c);
    }
    std::string base_hex;   // (as given, lower case)
    for (int i = 0; i < base_len; i++) {
        char t[3];
        snprintf(t, sizeof t, "%02x", base_pub[i]);
        base_hex += t;
    }

    vgen_scan_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.format = (uint32_t)fmt;
    cfg.count = o.count == 0 ? UINT64_MAX : o.count;   // lib.rs:524
    if (list && !o.count_given) cfg.count = UINT64_MAX;   // a list is bounded per pattern (--per-pattern); -c stays the total cap
    cfg.case_insensitive = o.ignore_case;
    cfg.seed = o.seed;
    cfg.table_bits_max = o.table_bits_max;
    // every key a seeded search returns is a function of the 64-bit seed and a small counter: whoever learns the address can
    // replay the search (unseeded searches draw 256 / 192 bits from the OS, as the reference does: src/gpu.rs:936-945, scanner.rs:144)
    if (o.seed && !has_range && !o.quiet)
        fprintf(stderr, "Warning: --seed makes this search reproducible and its keys guessable (64 bits of secret): do not fund what it finds\n");
    if (has_range) {
        cfg.has_start = cfg.has_end = 1;
        memcpy(cfg.start, start, 32);
        memcpy(cfg.end, end, 32);
    }
    if (!o.checkpoint.empty()) cfg.checkpoint_path = o.checkpoint.c_str();   // resumable scan (not in the reference)
    if (o.random_keys) {
        if (has_range) die("--random-keys draws an independent key per candidate: no range");
        cfg.flags |= VGEN_SCAN_RANDOM_KEYS;
    }
    // -p 'score:...': results carry their score; --best reports every new best score as it turns up (-c bounds the number of
    // improvements; without -c the search runs to the end of its range, a score that cannot be beaten, or Ctrl-C)
    vgen_filter *score_flt = nullptr;
    if (!list && pattern.compare(0, 6, "score:") == 0 && vgen_filter_compile(pattern.c_str(), 0, (uint32_t)fmt, &score_flt) != VGEN_OK) die(vgen_last_error(nullptr));
    if (o.best) {
        if (!score_flt) die("the argument '--best' needs a score specification as the pattern (-p 'score:zero-bytes>=1')");
        if (!o.checkpoint.empty()) die("the argument '--best' cannot be used with '--checkpoint'");
        cfg.flags |= VGEN_SCAN_BEST;
        if (!o.count_given) cfg.count = UINT64_MAX;
    }

    std::vector<vgen_generated> all;
    uint64_t total_ops = 0;
    double total_secs = 0;
    Progress prog;
    prog.t0 = now_s();
    const bool show_progress = !o.quiet && (isatty(2) || getenv("VGEN_PROGRESS") != nullptr);   // (VGEN_PROGRESS=1: also into a pipe or a log)
    for (uint64_t rep = 0; rep < (o.repeat ? o.repeat : 1) && !g_stop; rep++) {   // lib.rs:825-865
        vgen_scan_result res;
        prog.base = total_ops;
        int rc = create3 ? vgen_scan_create3(ctxs.data(), (uint32_t)ctxs.size(), pattern.c_str(), job3.factory, job3.proxy_hash, job3.salt_prefix, job3.guard,
                                             job3.guard_len, job3.first, &cfg, show_progress ? progress_cb : nullptr, &prog, &g_stop, &res)
                 : create2 ? vgen_scan_create2(ctxs.data(), (uint32_t)ctxs.size(), pattern.c_str(), job.deployer, job.init_code_hash, job.salt_prefix, job.first, &cfg,
                                             show_progress ? progress_cb : nullptr, &prog, &g_stop, &res)
                 : list ? vgen_scan_list(ctxs.data(), (uint32_t)ctxs.size(), list, o.per_pattern, &cfg, show_progress ? progress_cb : nullptr,
                                       &prog, &g_stop, &res)
                 : ctxs.size() == 1 ? vgen_scan(ctxs[0], pattern.c_str(), &cfg, show_progress ? progress_cb : nullptr, &prog, &g_stop, &res)
                                    : vgen_scan_multi(ctxs.data(), (uint32_t)ctxs.size(), pattern.c_str(), &cfg, show_progress ? progress_cb : nullptr,
                                                      &prog, &g_stop, &res);
        progress_clear(prog);
        if (rc != VGEN_OK) die(vgen_last_error(ctxs[0]));
        // what the scan absorbed must not pass unseen: a device that failed (the others took its ranges over), a generator
        // table that could not be had (the scan went on with the small one, at a third of the rate)
        if (res.failed_shards > 0)
            fprintf(stderr, "Warning: %d of %zu devices failed during the scan; the remaining ones took their ranges over\n", res.failed_shards, ctxs.size());
        for (size_t i = 0; i < ctxs.size() && rep == 0; i++) {
            uint32_t bits = 0, wanted = 0;
            char note[256] = "";
            // (a note exists only for a table the context could NOT have: widths are not comparable as numbers — 27 signed bits beat 26)
            if (vgen_get_resources(ctxs[i], nullptr, &bits, &wanted, note, sizeof note) == VGEN_OK && bits && bits != wanted && note[0])
                fprintf(stderr, "Warning: device %zu: %s\n", i, note);
        }
        for (uint64_t i = 0; i < res.n_matches; i++) all.push_back(res.matches[i]);
        total_ops += res.operations;
        total_secs += res.elapsed_secs;
        vgen_scan_result_free(&res);
    }
    for (auto *c : ctxs) vgen_destroy(c);

    FILE *w = stdout;
    if (!o.file.empty() && !(w = fopen(o.file.c_str(), "w"))) die("Failed to create output file");
    const double rate = total_secs > 0 ? (double)total_ops / total_secs : 0.0;
    const std::string fmt_name = create3 ? "Ethereum contract (CREATE3)" : format_display(fmt);
    if (o.output == "csv" && !all.empty())
        fprintf(w, "address,wif,private_key_hex,format,pattern,operations,elapsed_secs,rate%s\n", score_flt ? ",score" : "");
    for (size_t idx = 0; idx < all.size(); idx++) {
        const vgen_generated &g = all[idx];
        const std::string pattern = list ? list_pattern_of(list, g.address) : pattern_arg;
        // ethereum-contract: the address found is the contract's; the key controls the account that has to deploy it
        char deployer[128] = "";
        // split-key search: the key is the partial key as walked; which image of P + k*G has the address is found here
        int variant = -1;
        if (o.has_base) {
            char a[128];
            for (uint32_t v = 0; v < (fmt == VGEN_FMT_NOSTR ? 3u : 6u) && variant < 0; v++)
                if (vgen_split_derive((uint32_t)fmt, base_pub, (size_t)base_len, g.key, v, a, sizeof a) > 0 && strcmp(a, g.address) == 0) variant = (int)v;
            if (variant < 0) die("a result of a split-key search is no image of its point");
            // (ethereum-contract: the deploying account is the one of the FINAL key - the same image of the point)
            if (fmt == VGEN_FMT_ETHEREUM_CONTRACT && vgen_split_derive(VGEN_FMT_ETHEREUM, base_pub, (size_t)base_len, g.key, (uint32_t)variant, deployer, sizeof deployer) < 0)
                die("a result of a split-key search has no account");
        } else
        if (fmt == VGEN_FMT_ETHEREUM_CONTRACT && vgen_derive(VGEN_FMT_ETHEREUM, g.key, deployer, sizeof deployer, nullptr, 0) != VGEN_OK)
            die("malformed or out-of-range secret key");
        // ethereum-create2: the "key" is the salt; the address exists only for this deployer and this init code
        std::string c2_hash;
        if (create2 && !create3) {
            snprintf(deployer, sizeof deployer, "%s", hex0x(job.deployer, 20).c_str());
            c2_hash = hex0x(job.init_code_hash, 32);
        }
        // ethereum-create3: the salt is the raw one the factory is called with; the proxy and the hashed salt are recomputed here
        std::string c3_proxy, c3_hash, c3_guarded;
        if (create3) {
            uint8_t proxy[20], contract[20], gs[32];
            if (vgen_create3_address(job3.factory, g.key, job3.proxy_hash, job3.guard, job3.guard_len, proxy, contract) != VGEN_OK) die("malformed CREATE3 job");
            snprintf(deployer, sizeof deployer, "%s", hex0x(job3.factory, 20).c_str());
            c3_proxy = hex0x(proxy, 20);
            c3_hash = hex0x(job3.proxy_hash, 32);
            if (job3.guard_len >= 0) {
                uint8_t msg[96];
                memcpy(msg, job3.guard, (size_t)job3.guard_len);
                memcpy(msg + job3.guard_len, g.key, 32);
                vgen_keccak256(msg, (size_t)job3.guard_len + 32, gs);
                c3_guarded = hex0x(gs, 32);
            }
        }
        // solana: the key is the seed; the keypair string is what wallets import, the address's 32 bytes are the public key
        std::string keypair;
        if (solana) {
            char kp[96];
            if (vgen_solana_keypair_base58(g.key, kp, sizeof kp) < 0) die("a result of a solana search has no keypair string");
            keypair = kp;
            if (!o.keypair_dir.empty()) write_keypair_file(o.keypair_dir, g);
        }
        // nostr: the address is the Bech32 of the x-only public key; its 32 bytes in hex beside it
        std::string pub_hex;
        // onion: the key is the scalar; what Tor loads are the 64 expanded bytes, the address's 32 bytes are the public key
        std::string expanded_hex;
        if (onion) {
            uint8_t ex[64], pub[32];
            if (vgen_onion_expand(g.key, ex) != VGEN_OK || vgen_onion_decode(g.address, pub) != VGEN_OK) die("a result of an onion search is no address");
            static const char HX[] = "0123456789abcdef";
            for (int i = 0; i < 64; i++) {
                expanded_hex.push_back(HX[ex[i] >> 4]);
                expanded_hex.push_back(HX[ex[i] & 15]);
            }
            for (int i = 0; i < 32; i++) {
                pub_hex.push_back(HX[pub[i] >> 4]);
                pub_hex.push_back(HX[pub[i] & 15]);
            }
            if (!o.key_dir.empty()) write_onion_dir(o.key_dir, g, ex, pub);
        }
        if (solana) {
            uint8_t pub[32];
            if (vgen_solana_decode(g.address, pub) != VGEN_OK) die("a result of a solana search is no address");
            static const char HX[] = "0123456789abcdef";
            for (int i = 0; i < 32; i++) {
                pub_hex.push_back(HX[pub[i] >> 4]);
                pub_hex.push_back(HX[pub[i] & 15]);
            }
        }
        if (fmt == VGEN_FMT_NOSTR) {
            uint32_t kind = 0;
            uint8_t pub[32];
            if (vgen_nostr_decode(g.address, &kind, pub) != VGEN_OK || kind != 0) die("a result of a nostr search is no npub");
            static const char HX[] = "0123456789abcdef";
            for (int i = 0; i < 32; i++) {
                pub_hex.push_back(HX[pub[i] >> 4]);
                pub_hex.push_back(HX[pub[i] & 15]);
            }
        }
        uint32_t score = 0;   // (score searches only: every other output stays byte for byte what it was)
        if (score_flt && vgen_score(score_flt, g.address, &score) != VGEN_OK) die("a result of a score search has no score");
        if (o.output == "text") {
            fprintf(w, "=== Match %zu of %zu ===\n", idx + 1, all.size());
            if (create2) fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s\nSalt    : %s\n", pattern.c_str(), fmt_name.c_str(), g.address, g.hex);
            else if (onion) fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s.onion\nSecret key : %s\nPubkey  : %s\n", pattern.c_str(), fmt_name.c_str(), g.address, expanded_hex.c_str(), pub_hex.c_str());
            else if (solana) fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s\nSeed    : %s\nKeypair : %s\n", pattern.c_str(), fmt_name.c_str(), g.address, g.hex, keypair.c_str());
            else if (o.has_base) {
                // a partial key: no key to anything without the secret behind the base public key (vgen-hip combine)
                fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s\nPartial key : %s\nBase pubkey : %s\nVariant : %d\n", pattern.c_str(), fmt_name.c_str(),
                        g.address, g.hex, base_hex.c_str(), variant);
                if (!pub_hex.empty()) fprintf(w, "Pubkey  : %s\n", pub_hex.c_str());
            } else if (!pub_hex.empty()) fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s\nNsec    : %s\nHex     : %s\nPubkey  : %s\n", pattern.c_str(),
                                               fmt_name.c_str(), g.address, g.wif, g.hex, pub_hex.c_str());
            else fprintf(w, "Pattern : %s\nFormat  : %s\nAddress : %s\nWIF     : %s\nHex     : %s\n", pattern.c_str(),
                         fmt_name.c_str(), g.address, g.wif, g.hex);
            if (create3) {
                fprintf(w, "Deployer: %s  (the CREATE3 factory that must be called with the salt above)\nProxy   : %s\nProxyHash: %s\n", deployer, c3_proxy.c_str(), c3_hash.c_str());
                if (!c3_guarded.empty()) fprintf(w, "GuardedSalt: %s\n", c3_guarded.c_str());
            } else if (create2) fprintf(w, "Deployer: %s  (the factory that must run CREATE2 with the salt above)\nInitHash: %s\n", deployer, c2_hash.c_str());
            else if (deployer[0]) fprintf(w, "Deployer: %s  (the account of this key; its first transaction must create the contract)\n", deployer);
            if (score_flt) fprintf(w, "Score   : %u\n", score);
            if (!o.quiet) {
                fprintf(w, "Ops     : %s (%.0f/sec)\n", with_commas(total_ops).c_str(), rate);
                fprintf(w, "Time    : %s\n", format_duration(total_secs).c_str());
            }
            fprintf(w, "\n");
        } else if (o.output == "json" || o.output == "jsonl") {
            const bool pretty = o.output == "json";
            const char *nl = pretty ? "\n  " : "", *sp = pretty ? " " : "";
            fprintf(w, "{%s\"address\":%s%s,", nl, sp, json_str(g.address).c_str());
            if (deployer[0]) fprintf(w, "%s\"deployer\":%s%s,", nl, sp, json_str(deployer).c_str());
            if (create3) {
                fprintf(w, "%s\"proxy\":%s%s,%s\"proxy_init_code_hash\":%s%s,", nl, sp, json_str(c3_proxy).c_str(), nl, sp, json_str(c3_hash).c_str());
                if (!c3_guarded.empty()) fprintf(w, "%s\"guarded_salt\":%s%s,", nl, sp, json_str(c3_guarded).c_str());
            } else if (create2) fprintf(w, "%s\"init_code_hash\":%s%s,", nl, sp, json_str(c2_hash).c_str());
            if (score_flt) fprintf(w, "%s\"score\":%s%u,", nl, sp, score);
            if (!pub_hex.empty()) fprintf(w, "%s\"public_key_hex\":%s%s,", nl, sp, json_str(pub_hex).c_str());
            // split-key search: the partial key, the base it belongs to and the image - and no wif: a partial key is not importable
            if (solana) fprintf(w, "%s\"seed_hex\":%s%s,%s\"keypair_base58\":%s%s,", nl, sp, json_str(g.hex).c_str(), nl, sp, json_str(keypair).c_str());   // (no wif)
            else if (onion) fprintf(w, "%s\"secret_key_hex\":%s%s,", nl, sp, json_str(expanded_hex).c_str());   // (the 64 expanded bytes; no wif)
            else if (o.has_base) fprintf(w, "%s\"partial_key_hex\":%s%s,%s\"base_public_key\":%s%s,%s\"variant\":%s%d,", nl, sp, json_str(g.hex + 2).c_str(), nl, sp,
                                    json_str(base_hex).c_str(), nl, sp, variant);
            else fprintf(w, "%s\"wif\":%s%s,%s\"private_key_hex\":%s%s,", nl, sp, json_str(g.wif).c_str(), nl, sp, json_str(g.hex).c_str());
            fprintf(w, "%s\"format\":%s%s,%s\"pattern\":%s%s,%s"
                       "\"operations\":%s%llu,%s\"elapsed_secs\":%s%s,%s\"rate\":%s%s%s}\n",
                    nl,
                    sp, json_str(fmt_name).c_str(), nl, sp, json_str(pattern).c_str(), nl, sp,
                    (unsigned long long)total_ops, nl, sp, json_f64(total_secs).c_str(), nl, sp, json_f64(rate).c_str(),
                    pretty ? "\n" : "");
        } else if (o.output == "csv") {
            fprintf(w, "%s,%s,%s,%s,%s,%llu,%s,%s", csv_escape(g.address).c_str(), csv_escape(g.wif).c_str(),
                    csv_escape(g.hex).c_str(), csv_escape(fmt_name).c_str(), csv_escape(pattern).c_str(),
                    (unsigned long long)total_ops, json_f64(total_secs).c_str(), json_f64(rate).c_str());
            if (score_flt) fprintf(w, ",%u", score);
            fprintf(w, "\n");
        } else if (o.output == "minimal") {
            fprintf(w, "%s\n", g.wif);
        } else {
            die("invalid value '" + o.output + "' for '--output'");
        }
    }
    vgen_filter_free(score_flt);
    if (w != stdout) {
        fclose(w);
        if (!all.empty() && !o.quiet) fprintf(stderr, "Wrote %zu result(s) to %s\n", all.size(), o.file.c_str());
    }
    if (all.empty() && !o.quiet)
        fprintf(stderr, "No match found after %s operations (%s)\n", with_commas(total_ops).c_str(),
                format_duration(total_secs).c_str());
    return 0;
}

}  // namespace

const char *argv_pattern(int argc, char **argv) {
    for (int i = 2; i + 1 < argc; i++)
        if (!strcmp(argv[i], "-p") || !strcmp(argv[i], "--pattern")) return argv[i + 1];
    return "";
}

int main(int argc, char **argv) {

    Opts o = parse(argc, argv);
    signal(SIGINT, on_sigint);
    if ((o.cmd == "generate" || o.cmd == "range") && o.format == "solana") {
        if (o.cmd == "range") die("'-f solana' cannot be used with 'range': a solana key is a seed whose scalar is its hash - there is no key range");
        if (o.has_patterns_file) die("the argument '--patterns-file' cannot be used with '-f solana': pattern lists are not provided for this format");
        if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f solana': checkpoints are not provided for this format");
        if (o.has_base) die("the argument '--base-pubkey' cannot be used with '-f solana': a seed cannot be split");
    }
    if ((o.cmd == "generate" || o.cmd == "range") && o.format == "onion") {
        if (o.cmd == "range") die("'-f onion' cannot be used with 'range': an onion search walks from the base scalar of its seed - there is no key range");
        if (o.has_patterns_file) die("the argument '--patterns-file' cannot be used with '-f onion': pattern lists are not provided for this format");
        if (!o.checkpoint.empty()) die("the argument '--checkpoint' cannot be used with '-f onion': checkpoints are not provided for this format");
        if (o.has_base) die("the argument '--base-pubkey' cannot be used with '-f onion': split keys are not provided for this format");
    }
    if (o.cmd == "verify" && o.format == "onion") die("'-f onion' cannot be used with 'verify': the reference has no such format to verify against");
    if ((o.cmd == "generate" || o.cmd == "range") && o.has_patterns_file) {
        if (o.has_pattern) die("the argument '--patterns-file' cannot be used with '--pattern'");
        vgen_filter *list = load_pattern_list(o, format_id(o.format));
        uint8_t start[32] = {0}, end[32] = {0};
        if (o.cmd == "range") {
            if (o.puzzle) {
                if (o.puzzle < 1 || o.puzzle > 160) die("Puzzle number must be between 1 and 160");
                const int sb = o.puzzle - 1;
                start[31 - sb / 8] = (uint8_t)(1u << (sb % 8));
                for (int b = 0; b < o.puzzle; b++) end[31 - b / 8] |= (uint8_t)(1u << (b % 8));
            } else if (!o.range.empty()) {
                size_t c = o.range.find(':');
                if (c == std::string::npos || o.range.find(':', c + 1) != std::string::npos) die("Range must be in format START:END");
                if (!parse_hex_key(o.range.substr(0, c), start)) die("Invalid start hex");
                if (!parse_hex_key(o.range.substr(c + 1), end)) die("Invalid end hex");
            } else {
                die("Either --range or --puzzle must be specified");
            }
            bool start_zero = true;
            for (int i = 0; i < 32; i++) start_zero = start_zero && start[i] == 0;
            if (start_zero) start[31] = 1;
        }
        const int rc = run_search(o, std::string(), o.cmd == "range", start, end, list);
        vgen_filter_free(list);
        return rc;
    }
    if (o.cmd == "generate") {
        if (!o.has_pattern) die("the following required arguments were not provided: --pattern <PATTERN>");
        uint8_t z[32] = {0};
        const Resolved r = resolve_provider(o, false);
        return run_search(o, r.pattern, false, z, z);
    }
    if (o.cmd == "estimate") {
        if (!o.has_pattern) die("the following required arguments were not provided: --pattern <PATTERN>");
        return run_estimate(o);
    }
    if (o.cmd == "range") {
        uint8_t start[32], end[32];
        Resolved pr;
        if (o.has_pattern) {
            pr = resolve_provider(o, true);
            o.pattern = pr.pattern;
        }
        if (pr.from_provider && !o.puzzle && o.range.empty()) {   // the provider's own key range, lib.rs:623-631
            if (!pr.has_range) die("Provider '" + std::string(argv_pattern(argc, argv)) + "' has no key range. Use --range or --puzzle to specify range.");
            memcpy(start, pr.start, 32);
            memcpy(end, pr.end, 32);
        } else if (o.puzzle) {   // lib.rs:643-649
            if (o.puzzle < 1 || o.puzzle > 160) die("Puzzle number must be between 1 and 160");
            memset(start, 0, 32);
            memset(end, 0, 32);
            const int sb = o.puzzle - 1;   // start = 2^(p-1), end = 2^p - 1
            start[31 - sb / 8] = (uint8_t)(1u << (sb % 8));
            for (int b = 0; b < o.puzzle; b++) end[31 - b / 8] |= (uint8_t)(1u << (b % 8));
        } else if (!o.range.empty()) {   // lib.rs:650-657
            size_t c = o.range.find(':');
            if (c == std::string::npos || o.range.find(':', c + 1) != std::string::npos) die("Range must be in format START:END");
            if (!parse_hex_key(o.range.substr(0, c), start)) die("Invalid start hex");
            if (!parse_hex_key(o.range.substr(c + 1), end)) die("Invalid end hex");
        } else {
            die("Either --range, --puzzle, or a provider pattern with key range must be specified");
        }
        bool start_zero = true;
        for (int i = 0; i < 32; i++) start_zero = start_zero && start[i] == 0;
        if (start_zero) start[31] = 1;   // key 0 is not a key: the CPU path skips it (scanner.rs:294-295)
        return run_search(o, o.has_pattern ? o.pattern : ".", true, start, end);   // default pattern, lib.rs:519
    }
    if (o.cmd == "combine") {
        // The requester's side of a split-key search: final key = (secret + partial) mod n under the image that gives the address.
        // The secret comes from a file (32 raw bytes, or 64 hex digits with an optional 0x and trailing white space), never from
        // the command line, where every user of the machine could read it.
        if (o.secret_file.empty() || o.partial.empty() || o.address.empty())
            die("the following required arguments were not provided: --secret-file <PATH> --partial <HEX> --address <ADDRESS>");
        const int fmt = format_id(o.format);
        if (fmt == VGEN_FMT_ETHEREUM_CREATE2) die("'-f " + o.format + "' has no keys to combine");
        FILE *f = fopen(o.secret_file.c_str(), "rb");
        if (!f) die("cannot read secret file '" + o.secret_file + "'");
        char buf[256];
        const size_t n = fread(buf, 1, sizeof buf, f);
        fclose(f);
        uint8_t secret[32], partial[32], final_key[32];
        if (n == 32) {
            memcpy(secret, buf, 32);
        } else {
            std::string h(buf, n);
            while (!h.empty() && isspace((unsigned char)h.back())) h.pop_back();
            if (h.compare(0, 2, "0x") == 0 || h.compare(0, 2, "0X") == 0) h = h.substr(2);
            if (h.size() != 64 || !parse_hex_key(h, secret)) die("the secret file must hold 32 bytes, or 64 hex digits");
        }
        std::string ph = o.partial;
        if (ph.compare(0, 2, "0x") == 0 || ph.compare(0, 2, "0X") == 0) ph = ph.substr(2);
        if (!parse_hex_key(ph, partial)) die("--partial must be a partial key in hex (at most 64 digits)");
        uint32_t variant = 0;
        const int rc = vgen_split_combine((uint32_t)fmt, secret, partial, o.address.c_str(), final_key, &variant);
        memset(secret, 0, sizeof secret);
        memset(buf, 0, sizeof buf);
        if (rc == VGEN_E_RANGE) die("the secret is not a valid key, or secret + partial is not one");
        if (rc != VGEN_OK) die("no image of secret + partial has the address " + o.address + ": wrong secret file, partial key, address or format");
        char addr[128], wif[128];
        if (vgen_derive((uint32_t)fmt, final_key, addr, sizeof addr, wif, sizeof wif) != VGEN_OK) die("malformed or out-of-range secret key");
        std::string hex;
        for (int i = 0; i < 32; i++) {
            char b[3];
            snprintf(b, sizeof b, "%02x", final_key[i]);
            hex += b;
        }
        printf("Format  : %s\nAddress : %s\n%s: %s\nHex     : %s\nVariant : %u\n", format_display(fmt), addr, fmt == VGEN_FMT_NOSTR ? "Nsec    " : "WIF     ", wif,
               hex.c_str(), variant);
        return 0;
    }
    if (o.cmd == "list-gpus") {
        int n = 0;
        vgen_device_count(&n);
        if (o.json) printf("[");
        for (int i = 0; i < n; i++) {
            char name[256];
            vgen_device_name(i, name, sizeof name);
            if (o.json) printf("%s{\"index\":%d,\"name\":%s,\"backend\":\"hip\"}", i ? "," : "", i, json_str(name).c_str());
            else printf("[%d] %s (HIP)\n", i, name);
        }
        if (o.json) printf("]\n");
        if (!n && !o.json) printf("No GPU adapters found\n");
        return 0;
    }
    if (o.cmd == "verify") {
        // src/lib.rs:377-492: the key as WIF first, then as hex (an optional 0x in front); every address of the key; with
        // --address, MATCH when it is one of them (Bech32 in one case either way, Ethereum case-insensitively, raw 40 hex too)
        uint8_t k[32];
        bool is_wif = false;
        char addr[128], wif[128];
        if (parse_wif(o.key, k, nullptr)) {
            // the checksum: the key re-encoded in the form the string claims must be the string again
            bool compressed = false;
            (void)parse_wif(o.key, k, &compressed);
            if (vgen_derive(compressed ? VGEN_FMT_P2PKH : VGEN_FMT_P2PKH_UNCOMPRESSED, k, addr, sizeof addr, wif, sizeof wif) == VGEN_OK && o.key == wif)
                is_wif = true;
        }
        if (!is_wif) {
            std::string h = o.key;
            while (h.compare(0, 2, "0x") == 0) h = h.substr(2);   // trim_start_matches("0x")
            bool is_hex = !h.empty() && h.size() % 2 == 0;
            for (char c : h) is_hex = is_hex && isxdigit((unsigned char)c);
            if (!is_hex) die("Invalid key format (not WIF or hex)");
            if (h.size() != 64 || !parse_hex_key(h, k)) die("Hex key must be 32 bytes");
        }
        std::string a[6];
        const int fmts[6] = {VGEN_FMT_P2PKH, VGEN_FMT_P2PKH_UNCOMPRESSED, VGEN_FMT_P2WPKH, VGEN_FMT_P2SH_P2WPKH, VGEN_FMT_P2TR, VGEN_FMT_ETHEREUM};
        std::string wif_c, wif_u;
        for (int i = 0; i < 6; i++) {
            if (vgen_derive((uint32_t)fmts[i], k, addr, sizeof addr, wif, sizeof wif) != VGEN_OK) die("malformed or out-of-range secret key");
            a[i] = addr;
            if (fmts[i] == VGEN_FMT_P2PKH) wif_c = wif;
            if (fmts[i] == VGEN_FMT_P2PKH_UNCOMPRESSED) wif_u = wif;
        }
        std::string hex;
        for (int i = 0; i < 32; i++) {
            char b[3];
            snprintf(b, sizeof b, "%02x", k[i]);
            hex += b;
        }
        printf("Private key: %s\n", is_wif ? o.key.c_str() : wif_c.c_str());
        printf("WIF (uncompr.):     %s\n", wif_u.c_str());
        printf("Hex: %s\n\n", hex.c_str());
        printf("P2PKH address:      %s\n", a[0].c_str());
        printf("P2PKH (uncompr.):   %s\n", a[1].c_str());
        printf("P2WPKH address:     %s\n", a[2].c_str());
        printf("P2SH-P2WPKH addr:  %s\n", a[3].c_str());
        printf("P2TR address:       %s\n", a[4].c_str());
        printf("Ethereum address:   %s\n", a[5].c_str());
        if (!o.address.empty()) {
            auto lower = [](std::string t) {
                for (char &c : t) c = (char)tolower((unsigned char)c);
                return t;
            };
            const std::string &e = o.address;
            bool all_lower = true, all_upper = true, all_hex = true;
            for (char c : e) {
                if (isalpha((unsigned char)c)) {
                    all_lower = all_lower && islower((unsigned char)c);
                    all_upper = all_upper && isupper((unsigned char)c);
                }
                all_hex = all_hex && isxdigit((unsigned char)c);
            }
            const bool bech = e.size() >= 3 && lower(e.substr(0, 3)) == "bc1";
            const std::string norm = bech && (all_lower || all_upper) ? lower(e) : e;
            const std::string eth = norm.size() == 40 && all_hex ? "0x" + norm : norm;
            bool listed = false;
            for (const std::string &x : a) listed = listed || x == norm;
            if (listed) printf("\nMATCH!\n");
            else if (eth.size() >= 2 && lower(eth.substr(0, 2)) == "0x" && lower(a[5]) == lower(eth)) printf("\nMATCH! (Ethereum, case-insensitive)\n");
            else printf("\nMISMATCH! Expected: %s\n", e.c_str());
        }
        return 0;
    }
    usage();
    return 2;
}
