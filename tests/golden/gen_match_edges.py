"""Writes tests/golden/match_edges.json: hash160 payloads whose Base58Check address ends in a given way, found by search
(a suffix lies in the checksum digits, so it cannot be planted; one hit costs 58^3 = 195 112 double SHA-256s).  Pure Python
and hashlib: nothing of the product or the oracle is used here, and the tests take the verdict on every payload from the
oracle, not from this file.  Per version byte (0: P2PKH and its uncompressed form, 5: P2SH-P2WPKH):

  abc      four payloads whose address ends in "abc"
  digits4  four payloads whose address ends in four digits
  own      a seeded random payload, then three more whose address ends in the same three characters

Run from the repository root: python tests/golden/gen_match_edges.py  (a few seconds)."""
import hashlib
import json
import os
import random

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def value_of(version, h160):
    body = bytes([version]) + h160
    return int.from_bytes(body + hashlib.sha256(hashlib.sha256(body).digest()).digest()[:4], "big")


def tail(v, k):
    out = ""
    for _ in range(k):
        v, d = divmod(v, 58)
        out = B58[d] + out
    return out


def search(rng, version, accept, count):
    found = []
    while len(found) < count:
        h = rng.randbytes(20)
        if accept(value_of(version, h)):
            found.append(h.hex())
    return found


def main():
    out = {}
    for version in (0, 5):
        rng = random.Random(7100 + version)
        own = rng.randbytes(20)
        t = value_of(version, own) % 58 ** 3
        abc = (B58.index("a") * 58 + B58.index("b")) * 58 + B58.index("c")
        out[str(version)] = {
            "abc": search(rng, version, lambda v: v % 58 ** 3 == abc, 4),
            "digits4": search(rng, version, lambda v: tail(v % 58 ** 4, 4).isdigit(), 4),
            "own": [own.hex()] + search(rng, version, lambda v: v % 58 ** 3 == t, 3),
        }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "match_edges.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
