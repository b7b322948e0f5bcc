// encode.h — host-side hashing and address/WIF encoders of libvgen_hip.so.
//
// What the Rust host of the reference gets from rust-bitcoin / bitcoin_hashes / base58ck / bech32 /
// sha3 when it turns a device hash160 back into an address string and a WIF
// (src/gpu.rs:1034-1088, src/address.rs:92-151,168-198).  The block functions are the single-source
// ones in core/hash.h (the same code the kernels run).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../core/ec.h"
#include "scalar.h"

namespace vg {

void host_sha256(const uint8_t *msg, size_t len, uint8_t out[32]);
// the same with the choice of block function exposed (tests: the portable path against the SHA-extension path)
void host_sha256_with(const uint8_t *msg, size_t len, uint8_t out[32], bool allow_sha_ni);
void host_ripemd160(const uint8_t *msg, size_t len, uint8_t out[20]);
void host_keccak256(const uint8_t *msg, size_t len, uint8_t out[32]);
void host_hash160(const uint8_t *msg, size_t len, uint8_t out[20]);

std::string base58_encode(const uint8_t *data, size_t len);
std::string base58check(const uint8_t *payload, size_t len);
// hrp + '1' + data(5-bit regrouped, version first) + checksum; bech32 for v0, bech32m for v1+
std::string segwit_address(const char *hrp, int witver, const uint8_t *prog, size_t len);
// NIP-19 bare keys: Bech32 (BIP-173, constant 1 - not Bech32m) of 32 bytes under hrp "npub" (x-only public key) or "nsec" (secret
// key), no witness-version symbol: 52 data symbols (the last one carries one bit and four zero pad bits) + 6 checksum symbols.
std::string nip19_encode(const char *hrp, const uint8_t data[32]);
// The strict decoder: `hrp` + "1" + 58 symbols, all lower case or all upper case, zero pad bits, a valid checksum.
bool nip19_decode(const char *hrp, const std::string &text, uint8_t out[32]);
std::string eip55_address(const uint8_t addr20[20]);
std::string hex_lower(const uint8_t *data, size_t len);

// Address string from a device payload; empty string for an unsupported format.
std::string address_from_payload(uint32_t format, const uint8_t *payload);
// WIF (compressed unless P2PKH_UNCOMPRESSED); hex for Ethereum (src/address.rs:110); nsec1... for Nostr (the scalar as it is: BIP-340
// signers negate internally)
std::string key_to_wif(uint32_t format, const uint8_t key_be[32]);
// Host derivation of the device payload for one key (single-key / verify-style use, tests).
// Returns the payload length (20 / 32) or 0 for an invalid key.
int payload_from_key(uint32_t format, const uint8_t key_be[32], uint8_t out[32]);

// ---- split-key search: the host's side of P + k*G (vgen_set_base_point, vgen_split_derive / vgen_split_combine, make_match) ----
// The same derivation from a public key: an affine point with canonical coordinates.  Payload length, or 0 (unknown format, or a
// taproot tweak that is no scalar).
int payload_from_point(uint32_t format, const ge &p, uint8_t out[32]);
// SEC1 public key -> point: 33 bytes (02 / 03 + x) or 65 bytes (04 + x + y).  false for any other length or prefix (the hybrid 06 /
// 07 included), a coordinate >= p, an x whose x^3 + 7 has no square root, or a y off the curve.
bool point_from_sec1(const uint8_t *pub, size_t len, ge &out);
void point_to_sec1(const ge &p, uint8_t out65[65]);
// Image `variant` of a point, numbered as scalar_variant numbers a key's: (beta^(variant % 3) x, variant >= 3 ? -y : y).
void point_image(ge &r, const ge &p, uint32_t variant);
// out = base + k*G for any 256-bit k (taken mod n; k = 0 gives the base itself).  false when the sum is the point at infinity.
bool point_add_gen(const ge &base, const Scalar &k, ge &out);

}  // namespace vg
