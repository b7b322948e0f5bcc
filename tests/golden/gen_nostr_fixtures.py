#!/usr/bin/env python3
"""Generate tests/golden/nostr.json: NIP-19 strings of the keys of tests/golden/openssl_keys.json.

The x-only public keys are OpenSSL's (pub65[1:33] of that fixture: EC_POINT_mul on secp256k1, see gen_openssl_fixtures.py); the
strings come from the BIP-173 reference algorithm written out below.  Nothing here imports the oracle or the product library: it
pins them from outside.  Two anchors are checked before anything is written: the key NIP-19 itself publishes as its npub example,
and the public key of the secret key 1 (the generator's x).  The output is committed; the test-suite only reads the JSON.
"""
import json
import os

CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
GEN = (0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)


def polymod(values):
    chk = 1
    for v in values:
        b = chk >> 25
        chk = ((chk & 0x1FFFFFF) << 5) ^ v
        for i in range(5):
            if (b >> i) & 1:
                chk ^= GEN[i]
    return chk


def hrp_expand(hrp):
    return [ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp]


def bech32_encode(hrp, data32):
    """BIP-173 (checksum constant 1) of 32 bytes regrouped into 5-bit symbols, zero padded: 52 data + 6 checksum symbols."""
    acc, bits, syms = 0, 0, []
    for byte in data32:
        acc = (acc << 8) | byte
        bits += 8
        while bits >= 5:
            bits -= 5
            syms.append((acc >> bits) & 31)
    if bits:
        syms.append((acc << (5 - bits)) & 31)
    chk = polymod(hrp_expand(hrp) + syms + [0] * 6) ^ 1
    syms += [(chk >> (5 * (5 - i))) & 31 for i in range(6)]
    return hrp + "1" + "".join(CHARSET[s] for s in syms)


NIP19_X = "3bf0c63fcb93463407af97a5e5ee64fa883d107ef9e558472c4eb9aaaefa459d"
NIP19_NPUB = "npub180cvv07tjdrrgpa0j7j7tmnyl2yr6yr7l8j4s3evf6u64th6gkwsyjh6w6"
KEY1_NPUB = "npub10xlxvlhemja6c4dqv22uapctqupfhlxm9h8z3k2e72q4k9hcz7vqpkge6d"


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    keys = json.load(open(os.path.join(here, "openssl_keys.json")))["full"]
    assert bech32_encode("npub", bytes.fromhex(NIP19_X)) == NIP19_NPUB
    vectors = []
    for e in keys:
        x = bytes.fromhex(e["pub65"])[1:33]
        vectors.append({"key": e["key"], "x": x.hex(), "npub": bech32_encode("npub", x), "nsec": bech32_encode("nsec", bytes.fromhex(e["key"]))})
    assert vectors[0]["key"] == "%064x" % 1 and vectors[0]["npub"] == KEY1_NPUB
    assert all(len(v["npub"]) == 63 and len(v["nsec"]) == 63 and v["npub"][57 - 1] in "qs" for v in vectors)
    out = {"source": "x: OpenSSL libcrypto EC_POINT_mul(secp256k1) via openssl_keys.json; strings: BIP-173 reference algorithm, HRP npub / nsec (NIP-19)",
           "nip19_example": {"x": NIP19_X, "npub": NIP19_NPUB}, "vectors": vectors}
    path = os.path.join(here, "nostr.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes;", len(vectors), "keys")


if __name__ == "__main__":
    main()
