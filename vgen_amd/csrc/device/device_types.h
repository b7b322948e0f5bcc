// device_types.h — plain-data structures shared between the HIP kernels and the host runtime.
#pragma once
#include <stdint.h>

namespace vg {

// vgen_format values (include/vgen_hip.h), usable as template arguments in device code
enum : int {
    VGF_P2PKH = 0,
    VGF_P2WPKH = 1,
    VGF_P2SH_P2WPKH = 2,
    VGF_P2TR = 3,
    VGF_P2PKH_UNCOMPRESSED = 4,
    VGF_ETHEREUM = 5,
    VGF_ETHEREUM_CONTRACT = 6,  // address of the contract the account deploys with nonce 0 (not a format of the reference)
    VGF_ETHEREUM_CREATE2 = 7    // CREATE2 (EIP-1014) address searched by salt: no key, no curve point (not a format of the reference)
};
// Nostr public key (NIP-19 npub): the BIP-340 x-only key itself, 32 bytes, no hash (not a format of the reference).  Format 10: the
// numbers 8 and 9 stay unassigned - every entry point answers them as unknown formats, which callers and the suite rely on.
constexpr int VGF_NOSTR{10};
// Solana address: the Ed25519 public key of a 32-byte seed, 32 bytes, Base58 without checksum (not a format of the reference).  Format
// 12; 11 stays unassigned like 8 and 9.  The only format on another curve: its key is the SEED, its kernels are ed_keys_kernel.
constexpr int VGF_SOLANA{12};
// Tor v3 onion address: the Ed25519 public key of a SCALAR (Tor loads an expanded secret key, not a seed), 32 bytes, Base32 with a
// SHA3-256 checksum and a version byte (not a format of the reference).  Format 13.  The scalars a, a + 8, a + 16, ... are all keys, so
// this format walks: onion_fwd_kernel / onion_bwd_kernel.
constexpr int VGF_ONION{13};
// the formats on the Ed25519 curve: no secp256k1 scratch, offset table or generator table
constexpr bool vgf_is_ed(int fmt) { return fmt == VGF_SOLANA || fmt == VGF_ONION; }

// the two formats whose payload is (derived from) the Ethereum account address: hex strings, both coordinates hashed
constexpr bool vgf_is_eth(int fmt) { return fmt == VGF_ETHEREUM || fmt == VGF_ETHEREUM_CONTRACT; }
// the format whose address STRING a payload of `fmt` is written as: a contract's 20 bytes are spelled like an account's
constexpr int vgf_string_format(int fmt) { return (fmt == VGF_ETHEREUM_CONTRACT || fmt == VGF_ETHEREUM_CREATE2) ? (int)VGF_ETHEREUM : fmt; }
// the formats whose address string is "0x" + 40 hex digits with EIP-55 casing (vgf_is_eth says how the per-key kernels hash a
// point and stays what it is: a CREATE2 address has no point behind it)
constexpr bool vgf_is_hex(int fmt) { return vgf_string_format(fmt) == VGF_ETHEREUM; }
// payload words of a format: the 32-byte x-only keys (the taproot output key, the Nostr public key) take eight, everything else five
constexpr int vgf_payload_words(int fmt) { return (fmt == VGF_P2TR || fmt == VGF_NOSTR || fmt == VGF_SOLANA || fmt == VGF_ONION) ? 8 : 5; }
// keys tested per curve point on a VGEN_FLAG_ENDO context: the six endomorphism / negation images, or - x-only keys, where (x, y)
// and (x, -y) are one key - the three images x, beta x, beta^2 x
constexpr uint32_t vgf_endo_images(int fmt) { return fmt == VGF_NOSTR ? 3u : 6u; }


// Device-side prefilter program (built by host/filter.cpp from the pattern's DFA).
// The test runs on the 160-bit payload seen as five BIG-endian words H[0..4] (H[0] = bytes 0..3).
enum : uint32_t {
    DEVF_HOST_ALL = 0,   // no usable prefilter: every key is a candidate (dump + host filter)
    DEVF_RANGES = 1,     // any r:  lo_r <= H <= hi_r           (Base58 prefixes)
    DEVF_MASKED = 2,     // any t:  (H & mask_t) == value_t     (Bech32 / hex prefixes & suffixes)
    DEVF_ALL = 3,        // pattern accepts every address
    DEVF_DFA = 4,        // full match on the device: encode the address, walk the DFA (core/dfa_eval.h)
    DEVF_LIST = 5,       // pattern list: the payloads are dumped on the device and looked up in a table of intervals
                         // (core/ptab_eval.h, DevPtab); not evaluated through DevFilter
    DEVF_SCORE = 6       // score specification (hex formats): the payloads are scored by kernels of their own (core/score_eval.h,
                         // ScoreTerms by value in the kernel arguments); the rest of DevFilter is unused
};
// VGF_SOLANA only (filter_eval_sol, core/filter_eval.h).  There DEVF_RANGES compares all eight big-endian words, and one more kind
// tests the payload N, read as one big-endian number, modulo a power of 58 - the last characters of the address:
//     DEVF_SOL_RESIDUE   (n_ranges == 0 or any r < n_ranges: lo_r <= N <= hi_r)  and  any t >= n_ranges: N mod modulus == tests[t].a[0]
// with modulus = 58^k < 2^30 in `witver`, n_ranges in `chk_base` and `count` tests in all (fields no other kind of this format uses).
constexpr uint32_t DEVF_SOL_RESIDUE = 7;

constexpr uint32_t DEVF_MAX_TESTS = 64;
constexpr uint32_t DEVF_FLAG_BECH32_CHK = 1u;   // masked tests also constrain the bech32 checksum

constexpr int DEVF_WORDS = 8;   // payload words a test covers: 5 used for 20-byte payloads, 8 for P2TR and Nostr keys

struct DevFilterTest {
    uint32_t a[DEVF_WORDS];   // ranges: lo      masked: mask
    uint32_t b[DEVF_WORDS];   // ranges: hi      masked: value
    uint32_t chk_mask;   // bech32 checksum (30 bits, first symbol in bits 29..25)
    uint32_t chk_value;
};

struct DevFilter {
    uint32_t kind;
    uint32_t count;
    uint32_t flags;
    uint32_t witver;     // bech32: witness version symbol (0 for P2WPKH)
    // Bech32 checksum as an affine map of the payload bytes: chk = chk_base ^ XOR_i chk_lut[i*256 + byte_i]
    // (20 x 256 words; 32 x 256 for the 32-byte P2TR payload).  Device pointer in the device copy, host pointer in the host copy; nullptr = use
    // the step-by-step polymod.
    const uint32_t *chk_lut;
    uint32_t chk_base;
    uint32_t dfa_bytes;  // DEVF_DFA: size of the DFA blob (<= 48 KiB, staged in LDS by the kernel)
    // DEVF_DFA: the blob (layout in core/dfa_eval.h); device pointer in the device copy
    const uint32_t *dfa_blob;
    DevFilterTest tests[DEVF_MAX_TESTS];
};

// Pattern-list table (DEVF_LIST, core/ptab_eval.h): disjoint intervals [lo_j, hi_j] of the top 64 bits of the big-endian
// payload, sorted, with a first level over the top `bits` bits: bit b of `bitmap` is set when bucket b meets an interval,
// and offsets[b] is the first interval whose hi >= the bucket's first value (offsets[2^bits] = n).  Passed by value to the
// list kernels; not part of DevFilter, whose layout every other kernel reads.
struct DevPtab {
    const uint32_t *bitmap;      // 2^bits bits
    const uint32_t *offsets;     // 2^bits + 1 entries
    const uint64_t *lo;          // n interval bounds
    const uint64_t *hi;
    uint32_t bits;               // 16 .. 24
    uint32_t n;
};

// Match ring of one frame (device memory).  count may run past cap; records beyond cap are dropped.
struct DevMatch {
    uint32_t index;
    uint32_t reserved;
    uint32_t payload[8];
};

struct DevMatchHeader {
    uint32_t count;
    uint32_t cap;
    uint32_t clk_cycles;   // running sums (mod 2^32) over the frame's seq_bwd launches, first wave of each launch:
    uint32_t clk_ticks;    // shader-clock cycles and 100 MHz ticks it ran for (kernels.hip: "shader-clock sample")
};

// Arguments of the two list kernels of one dispatch: the payloads the per-key kernel dumped (images x stride slots, the
// first `count` of every image written), the hit mask (one bit per slot) and the frame's match ring.
struct PtabArgs {
    DevPtab tab;
    const uint32_t *payloads;    // slot s at payloads + s * payload_words
    unsigned long long *hits;    // images * stride / 64 words
    DevMatchHeader *mhdr;
    DevMatch *mrec;
    uint32_t stride;             // slots per image (the context's batch size; a multiple of 8192)
    uint32_t count;              // slots written per image (n of vgen_dispatch_keys, else stride)
    uint32_t images;             // 6 on an endomorphism dispatch (3 for the x-only Nostr keys), else 1
    uint32_t match_base;
    uint32_t match_cap;
    // (appended: the list kernels' view of the fields above is unchanged)  payload_filter_kernel, instead of a list's table: the
    // context's filter (device copy; nullptr = a list dispatch), the automaton of a DEVF_DFA filter and the address-string format
    const DevFilter *filter;
    const uint32_t *dfa_blob;
    uint32_t dfa_bytes;
    uint32_t fmt;
};

// Arguments of create2_kernel: the message of salt counter 0 (core/hash.h keccak256_create2_addr; uniform, scalar loads from the
// kernarg segment), the dispatch's first counter, and where the results go.  Lane i tests counter first + i.
struct Create2Args {
    uint32_t m[22];              // 0xff || deployer || salt_prefix || 0^8 || init_code_hash, bytes 85..87 zero
    unsigned long long first;
    uint32_t *payloads;          // slot i at payloads + 5 i: every slot (DUMP) or the slots of hit lanes only
    unsigned long long *hits;    // !DUMP: the hit mask, one bit per slot (batch / 64 words)
    const DevFilter *filter;     // !DUMP: the context's prefilter (kinds 1 - 3)
};

// Per-dispatch uniform points of the sequential kernel: Q_j = (k0 + N/2 - S/2 + j)*G and the
// canonical negations of their coordinates, nine 29-bit limbs each.
struct DevSeqQ {
    uint32_t qx[9], qy[9], nqx[9], nqy[9];
};

// Building the offset table on the device (rtab_build_kernel): lane u computes R_u = base + u * step from the
// doublings pw[b] = 2^b * step (affine, canonical limbs, passed by value), bits of u selecting the summands.
struct DevAffine {
    uint32_t x[9], y[9];
};
struct RtabArgs {
    uint32_t *rtab;            // [18][lanes], limb-major
    uint32_t lanes;
    uint32_t nbits;            // ceil(log2(lanes)) <= 24
    DevAffine base;
    DevAffine pw[24];
};

constexpr uint32_t SEQ_MAX_S = 16;   // keeps SeqArgs (passed by value as kernel arguments) under 4 KB
constexpr int SEQ_WG = 256;          // lanes per workgroup of the seq_* kernels

struct SeqArgs {
    const uint32_t *rtab;      // offset table, limb-major: [18][lanes]  (x limbs 0..8, y limbs 0..8)
    const DevFilter *filter;   // used when dump == nullptr
    uint32_t *dump;            // dump mode: N * 5 words
    DevMatchHeader *mhdr;      // filter mode: monotonic candidate counter ...
    DevMatch *mrec;            // ... and this frame's record ring
    uint32_t *pre;             // scratch: prefix products [S][9][lanes]
    uint32_t *tree;            // scratch: product-tree nodes [groups][9][SEQ_WG]
    uint32_t *root;            // scratch: tree roots / their inverses [9][groups]
    uint32_t *xs;              // scratch of the split form (compressed-key formats): [9][N] — eight words of x and the prefix byte 0x02 | parity(y) of
                               // every key, slot (2j + sgn) * lanes + u; nullptr = the fused seq_bwd_kernel does everything
    uint32_t lanes;            // N / (2*S)
    uint32_t groups;           // lanes / SEQ_WG
    uint32_t n;                // N
    uint32_t s;                // S
    uint32_t match_base;       // value of mhdr->count when this dispatch was enqueued
    uint32_t match_cap;
    const uint32_t *dfa_blob;  // DEVF_DFA: the automaton (device memory), staged into LDS by the kernel
    const uint32_t *gtab;      // P2TR: 8-bit fixed-window generator table (global memory) for the tweak multiplication
    const uint32_t *gtab16;    // ... and the wide-window one (built on the device at first use); nullptr = use gtab
    uint32_t gtab_bits;        // window width of gtab16 (16 | 20 | 22 | 24)
    uint32_t dfa_bytes;        // 0 = prefilter mode
    uint32_t fmt;              // VGF_* of the context (the DFA path needs the exact address format)
    uint32_t hash_kpl;         // split form: keys per lane of seq_hash_kernel (a divisor of 2S)
    uint32_t endo;             // seq_bwd: test the six endomorphism / negation images of every point (kernels.hip: ENDO)
    uint32_t lone;             // seq_bwd: at most one other frame of the context was in flight when this dispatch was issued: launch the variant without issue-slot yields
    // P2TR only: the tweaked points Q = P + t*G of a dispatch wait for a second shared inversion.
    uint32_t *tq;              // [2S key steps][27][lanes]: X(Q), Z(Q), running product of the lane's Z's
    uint32_t *tq_flag;         // [2S][lanes]: 1 = the key has an address (valid tweak, Q finite)
    uint32_t *tree2;           // product tree / roots of the lanes' final products, laid out like tree / root
    uint32_t *root2;
    DevSeqQ q[SEQ_MAX_S];      // per-dispatch uniform points, by value (scalar loads from the kernarg segment)
    // (appended behind q: the older kernels' view of the fields above is unchanged)
    unsigned long long *hits;  // xonly_bwd_kernel: non-null = the prefilter form - a.filter on the eight words in registers, hit bits into this
                               // slot-ordered mask (images x n / 64 words, every one written), hit lanes' payloads into a.dump
};

// Arbitrary-scalar path (keys_fwd_kernel -> seq_inv_kernel -> keys_bwd_kernel): one key per lane, full
// fixed-base multiplication over the 8-bit window table (32 windows x 255 points x 20 words = 652 800 B in
// global memory, core/ec.h); the Jacobian results go through global scratch and share their inversions exactly as
// the sequential path does (workgroup product tree, one root per lane in seq_inv_kernel).
constexpr int KEYS_WG = 256;

struct KeysArgs {
    const uint32_t *gtab;      // [32][255][20]: x limbs 0..8, y limbs 9..17 of d * 256^w * G (d = 1..255)
    const uint32_t *gtab16;    // wide windows: [windows][2^bits - 1][16 words] (core/ec.h: ec_mul_gen_wide); nullptr = use gtab
    uint32_t gtab_bits;        // window width of gtab16 (16 | 20 | 22)
    const uint8_t *keys_be;    // n * 32 bytes big-endian (uploaded, or drawn on the device by rnd_fill_kernel), or nullptr: key i = base + i
    const DevFilter *filter;
    uint32_t *dump;            // dump mode: n * 5 words (zeroed for invalid keys)
    DevMatchHeader *mhdr;
    DevMatch *mrec;
    uint32_t base[8];          // sequential variant: little-endian words of the first key
    uint32_t n;
    uint32_t match_base;
    uint32_t match_cap;
    uint32_t fmt;              // VGF_* of the context
    const uint32_t *dfa_blob;  // DEVF_DFA (see SeqArgs)
    uint32_t dfa_bytes;
    uint32_t groups;           // workgroups = ceil(n / KEYS_WG)
    uint32_t endo;             // keys_bwd: test the six endomorphism / negation images of every point (kernels.hip: ENDO) ...
    uint32_t vstride;          // ... image `variant` of key i is reported / dumped at variant * vstride + i (= the context's batch size)
    uint32_t *pts;             // P2TR: affine internal keys in key order, [n][16] words (written by keys_bwd_kernel<P2TR>,
                               // read by p2tr_tweak_kernel); y = 0 marks "no key"
    uint32_t *xyz;             // scratch: Jacobian results, limb-major [27][groups * KEYS_WG] (X, Y, Z limbs; the taproot stage: X, validity word, Z)
    uint32_t *tree;            // scratch: product-tree nodes [groups][9][KEYS_WG]
    uint32_t *root;            // scratch: tree roots / their inverses [9][groups]
    // (appended: the older kernels' view of the fields above is unchanged)
    unsigned long long *hits;  // keys_xonly_kernel: non-null = the prefilter form (as SeqArgs::hits; words beyond ceil(n / 256) * 4 of an image are the caller's to clear)
    // (appended behind hits, the same way)  split-key dispatches: has_base != 0 = keys_fwd_base_kernel runs in keys_fwd_kernel's place
    // and lane i's point is base_pt + k_i * G (canonical limbs); the infinity k_i * G = -base_pt is a "no key" slot
    uint32_t has_base;
    DevAffine base_pt;
};

// ---- score searches (DEVF_SCORE; appended: no structure above changes) ----------------------------------------------------------
// A score specification: 1 - 4 terms `metric >= min`, all of which must hold; the SCORE of a payload is the value of the first
// term's metric (core/score_eval.h).  Plain data: a host-side field of vgen_filter / vgen_ctx, by value in the kernel arguments.
enum : uint32_t {
    SCORE_ZERO_BYTES = 0,          // bytes equal to 0x00                      0 .. 20
    SCORE_LEADING_ZERO_BYTES = 1,  // length of the leading run of 0x00 bytes   0 .. 20
    SCORE_LEADING_DIGIT = 2,       // length of the leading run of hex digit d  0 .. 40
    SCORE_COUNT_DIGIT = 3          // hex digits equal to d                     0 .. 40
};
constexpr uint32_t SCORE_MAX_TERMS = 4;
constexpr uint32_t score_metric_max(uint32_t metric) { return metric <= SCORE_LEADING_ZERO_BYTES ? 20u : 40u; }

struct ScoreTerms {
    uint32_t n;
    struct {
        uint32_t metric, digit, min;
    } t[SCORE_MAX_TERMS];
};

// Arguments of payload_score_kernel: the geometry of payload_filter_kernel (images x stride slots, the first `count` of every image
// written).  One ballot per wave goes into `hits`; ptab_compact_kernel, with PtabArgs over the same two buffers, follows.
struct ScoreArgs {
    ScoreTerms terms;
    const uint32_t *payloads;    // slot s at payloads + 5 s
    unsigned long long *hits;    // one bit per slot
    uint32_t stride, count, images;
};

// Arguments of create2_score_kernel: the message and first counter of Create2Args (lane i tests counter first + i and owns slot i),
// the terms, the hit mask and where the hit lanes' payloads go; the compaction follows here too.
struct Create2ScoreArgs {
    ScoreTerms terms;
    uint32_t m[22];
    unsigned long long first;
    uint32_t *out;               // payloads of hit lanes only, slot i at out + 5 i
    unsigned long long *hits;    // one bit per slot (batch / 64 words)
};

// ---- CREATE3 jobs of a VGF_ETHEREUM_CREATE2 context (appended: no structure above changes) -------------------------------------
// Arguments of create3_kernel: lane i tests counter first + i.  Unguarded, m is the proxy stage's message of counter 0 as in
// Create2Args (the job's factory and proxy_init_code_hash) and w is unused.  Guarded, w is the guard stage's message of counter 0
// with its padding (core/hash.h create3_guard_message), the counter's bytes start at byte guard_off = guard_len + 24 of it, and m
// is the proxy stage's message with an all-zero salt, which the guard stage's digest fills.
struct Create3Args {
    uint32_t m[22];
    uint32_t w[26];
    uint32_t guard_off;
    unsigned long long first;
    uint32_t *payloads;          // the CONTRACT's address: slot i at payloads + 5 i, every slot (DUMP) or the slots of hit lanes only
    unsigned long long *hits;    // !DUMP: the hit mask, one bit per slot (batch / 64 words)
    const DevFilter *filter;     // !DUMP: the context's prefilter (kinds 1 - 3)
};

// Arguments of create3_score_kernel: Create3Args with the score terms in place of the prefilter.
struct Create3ScoreArgs {
    ScoreTerms terms;
    uint32_t m[22];
    uint32_t w[26];
    uint32_t guard_off;
    unsigned long long first;
    uint32_t *out;               // payloads of hit lanes only, slot i at out + 5 i
    unsigned long long *hits;    // one bit per slot (batch / 64 words)
};

// ---- Solana (VGF_SOLANA; appended: no structure above changes) ------------------------------------------------------------------
// Arguments of ed_keys_kernel: lane i tests seed i of the uploaded seeds (32 bytes each; lanes >= n have no key) or, seeds ==
// nullptr, the digest core/rnd.h draws for (seed, stream, first + i) - every draw is a key.  batch lanes are launched either way.
constexpr int ED_WG = 512;       // lanes per workgroup: its waves share one field inversion (kernels.hip)
struct EdArgs {
    const uint32_t *table;       // core/ed25519.h: ED_TABLE_WORDS words
    const uint8_t *seeds;
    uint32_t seed[6];            // RndSeed::w
    uint32_t stream;
    unsigned long long first;
    uint32_t n;
    uint32_t *payloads;          // slot i at payloads + 8 i: every slot (DUMP; zero where there is no key) or the slots of hit lanes only
    unsigned long long *hits;    // PRE: the hit mask, one bit per slot (batch / 64 words)
    const DevFilter *filter;     // PRE: the context's prefilter (kinds 1, 3, 7)
};

// ---- Tor v3 onion addresses (VGF_ONION; appended: no structure above changes) ----------------------------------------------------
// The walk: candidate i of a dispatch has the scalar base + 8 (first + i), its point is A(base + 8 first) + i (8B).  With L = batch /
// (2 ONION_S) lanes, lane u owns the affine table point R_u = (u S + S/2) (8B) and the dispatch shares the S points
// U_j = (base + 8 (first + L S - S/2 + j)) B; the 2 S keys of a lane are
//     U_j + R_u  at slot  L S + u S + j          U_j - R_u  at slot  L S - (u + 1) S + j,         j = 0 .. S - 1
// which together tile 0 .. batch - 1.  S = 32: a lane's S slots of either sign are one aligned 32-bit word of the hit mask.
constexpr int ONION_S = 32;
constexpr int ONION_WG = 512;                // lanes per workgroup: its waves share one field inversion, as ED_WG
constexpr int ONION_PT_WORDS = 27;           // x[9] y[9] t[9], canonical limbs
constexpr uint32_t ONION_NO_SLOT = 0xFFFFFFFFu;
// onion_points_kernel: point i = (start + i * step) B for i < n, with t = x y, or d x y when mul_d (the shared points).  Word w of
// point i goes to out[w * wstride + i * istride]: (L, 1) for the lane table - coalesced across lanes -, (1, ONION_PT_WORDS) for the
// shared points, which every lane reads at the same address.
struct OnionPointsArgs {
    const uint32_t *table;       // core/ed25519.h: ED_TABLE_WORDS words
    uint32_t start[8];           // little-endian words
    uint32_t step;
    uint32_t n;
    uint32_t mul_d;
    uint32_t wstride, istride;
    uint32_t *out;               // ONION_PT_WORDS x n words
};
// onion_fwd_kernel / onion_bwd_kernel.  Scratch of a frame: pre = 2 S x 9 x L words (prefix product before element e of lane g, word
// w, at [(e * 9 + w) * L + g]; element 2 j is 1 - k_j, element 2 j + 1 is 1 + k_j), then inv = 9 x L words (1 / the lane's product).
struct OnionArgs {
    const uint32_t *uni;         // the dispatch's S shared points: ONION_PT_WORDS x S words, [j * ONION_PT_WORDS + w]
    const uint32_t *lane;        // the context's lane points: ONION_PT_WORDS x L words, [w * L + u]
    uint32_t *pre;
    uint32_t *inv;
    uint32_t lanes;              // L
    uint32_t zero_slot;          // the slot whose scalar is 0 (no key: its payload is zero and it never hits), or ONION_NO_SLOT
    uint32_t *payloads;          // slot i at payloads + 8 i: every slot (dump) or the slots of hit lanes only
    uint32_t *hits;              // filter form: the hit mask as 32-bit words (bit s & 31 of word s >> 5), batch / 32 words
    const DevFilter *filter;     // filter form: the context's prefilter (kinds 2 and 3)
};

}  // namespace vg
