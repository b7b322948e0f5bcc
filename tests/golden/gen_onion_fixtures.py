"""Writes tests/golden/onion.json: the SHA-256 of the reference's dumps (tests/onion_vectors.py: Python integers over
tests/solana_vectors.py, hashlib) for the three dispatches tests/test_gpu_onion.py runs, the base scalars they start from, and two
addresses of live onion services with their public keys as external known answers for decode, checksum and encode.

    python tests/golden/gen_onion_fixtures.py        (from the repository root; a few seconds)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import onion_vectors as ov   # noqa: E402

BATCH = 8192
SEED = 0x4F4E494F4E   # "ONION"
KNOWN = [
    ("duckduckgogg42xjoc72x3sjasowoarfbgcmvfimaftt6twagswzczad", "1d04a1d04a338c6e6ae970bfabee49049d6702250984ca950c01673f4ec034ad"),
    ("2gzyxa5ihm7nsggfxnu52rck2vv4rvmdlkiu3zzui5du4xyclen53wid", "d1b38b83a83b3ed918c5bb69dd444ad56bc8d5835a914de73447474e5f02591b"),
]


def main():
    base = ov.base_scalar(SEED, 0)
    rippling = (0x40000000 << 224) | (2**224 - 8)   # low seven words 0xFFFFFFF8 0xFFFFFFFF ...: 8 i carries through every word
    dumps = [("fixture base, first 0", base, 0), ("fixture base, first 2^32 - 100", base, 2**32 - 100), ("rippling base", rippling, 0)]
    out = {"batch": BATCH, "seed": SEED, "base": "%064x" % base, "dumps": [], "known": []}
    for name, b, first in dumps:
        out["dumps"].append({"name": name, "base": "%064x" % b, "first": first, "sha256": ov.digest(ov.walk_payloads(b, first, BATCH))})
    for addr, key in KNOWN:
        pub = bytes.fromhex(key)
        assert ov.decode(addr) == pub and ov.address(pub) == addr and ov.on_curve(ov.decode_point(pub))
        out["known"].append({"address": addr, "public_key": key})
    with open(os.path.join(ROOT, "tests", "golden", "onion.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
