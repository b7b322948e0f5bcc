"""Writes tests/golden/solana.json: the fixtures of the Solana tests.  Run by hand (python tests/golden/gen_solana_fixtures.py); no
test calls it.

  openssl   64 (seed, public key) pairs made by the local `openssl genpkey -algorithm ed25519` - an implementation that shares
            nothing with this repository or with tests/solana_vectors.py (which must agree with it: asserted here)
  rfc8032   the seeds of RFC 8032 7.1 tests 1 - 3 with the public keys the Python reference gives (test 1 is d75a9801...f707511a)
  dump      the fixed (seed, stream, first index) of the GPU test's two dumps and the SHA-256 of the 8192 expected payloads each
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import solana_vectors as sv  # noqa: E402

DUMP_SEED, DUMP_STREAM, DUMP_BATCH = 20261020, 3, 8192
DUMP_FIRST = [0, 2**32 - 100]


def openssl_pair():
    der = subprocess.run(["openssl", "genpkey", "-algorithm", "ed25519", "-outform", "DER"], check=True, capture_output=True).stdout
    pub = subprocess.run(["openssl", "pkey", "-inform", "DER", "-pubout", "-outform", "DER"], input=der, check=True, capture_output=True).stdout
    # PKCS#8 ends with OCTET STRING(OCTET STRING(seed)), SubjectPublicKeyInfo with BIT STRING(public key)
    assert der[-34:-32] == b"\x04\x20" and pub[-33:-32] == b"\x00"
    return der[-32:], pub[-32:]


def main():
    pairs = []
    for _ in range(64):
        seed, pub = openssl_pair()
        assert sv.public_key(seed) == pub, "the Python reference disagrees with openssl"
        pairs.append({"seed": seed.hex(), "public_key": pub.hex(), "address": sv.address(pub)})
    rfc = []
    for seed in ("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
                 "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
                 "c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7"):
        pub = sv.public_key(bytes.fromhex(seed))
        rfc.append({"seed": seed, "public_key": pub.hex(), "address": sv.address(pub)})
    assert rfc[0]["public_key"] == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    assert rfc[1]["public_key"] == "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c"
    assert rfc[2]["public_key"] == "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025"
    dumps = []
    for first in DUMP_FIRST:
        blob = b"".join(sv.stream_payloads(DUMP_SEED, DUMP_STREAM, first, DUMP_BATCH))
        dumps.append({"seed": DUMP_SEED, "stream": DUMP_STREAM, "first_index": first, "batch": DUMP_BATCH,
                      "sha256": hashlib.sha256(blob).hexdigest()})
    with open(os.path.join(HERE, "solana.json"), "w") as f:
        json.dump({"openssl": pairs, "rfc8032": rfc, "dump": dumps}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
