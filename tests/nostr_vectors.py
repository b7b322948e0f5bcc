"""What the Nostr format (VGEN_FMT_NOSTR, format 10) must compute, without the code under test: a BIP-173 encoder and strict decoder written
out here, the fixture tests/golden/nostr.json (OpenSSL's public keys), and the x coordinates of a run of consecutive keys by affine
additions in Python integers, anchored at both ends on the oracle's scalar multiplication (oracle.pyoracle.pubkey).

Shared by tests/test_nostr.py (CPU) and tests/test_gpu_nostr.py; every expected value is computed once (lru_cache) and read-only."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle as vo  # noqa: E402

FMT = 10
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
# beta and lambda, the cube roots of unity mod p and mod n behind the endomorphism lambda (x, y) = (beta x, y) (libsecp256k1's constants)
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
assert pow(BETA, 3, P) == 1 and pow(LAMBDA, 3, N) == 1
CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
_GEN = (0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "nostr.json")))
VECTORS = FIXTURE["vectors"]


def _polymod(values):
    chk = 1
    for v in values:
        b = chk >> 25
        chk = ((chk & 0x1FFFFFF) << 5) ^ v
        for i in range(5):
            if (b >> i) & 1:
                chk ^= _GEN[i]
    return chk


def _hrp_expand(hrp):
    return [ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp]


def symbols(data32):
    """The 52 data symbols of 32 bytes (the last one: one bit and four zero pad bits)."""
    v = int.from_bytes(data32, "big") << 4
    return [(v >> (5 * (51 - i))) & 31 for i in range(52)]


def checksum(hrp, syms):
    chk = _polymod(_hrp_expand(hrp) + list(syms) + [0] * 6) ^ 1
    return [(chk >> (5 * (5 - i))) & 31 for i in range(6)]


def encode(hrp, data32):
    """BIP-173 (constant 1, not Bech32m), no witness-version symbol: hrp + '1' + 52 data symbols + 6 checksum symbols."""
    s = symbols(data32)
    return hrp + "1" + "".join(CHARSET[c] for c in s + checksum(hrp, s))


def decode(hrp, text):
    """Strict: None for another HRP, another length, mixed case, a foreign character, non-zero pad bits or a bad checksum."""
    if text != text.lower() and text != text.upper():
        return None
    t = text.lower()
    if len(t) != len(hrp) + 59 or not t.startswith(hrp + "1") or any(c not in CHARSET for c in t[len(hrp) + 1:]):
        return None
    s = [CHARSET.index(c) for c in t[len(hrp) + 1:]]
    if _polymod(_hrp_expand(hrp) + s) != 1 or s[51] & 15:
        return None
    v = 0
    for c in s[:52]:
        v = (v << 5) | c
    return (v >> 4).to_bytes(32, "big")


def npub_of_x(x):
    return encode("npub", x.to_bytes(32, "big"))


def xy_of(k):
    pub = vo.pubkey(k)
    return int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")


@functools.lru_cache(maxsize=None)
def walk_x(start, n):
    """x(k * G) for k = start .. start + n - 1 (None where k is no valid scalar), tuple of ints: one oracle multiplication at the first
    valid key, affine additions of G after it, the last valid key checked against the oracle again."""
    out, pt, last = [], None, None
    for i in range(n):
        k = start + i
        if not 0 < k < N:
            out.append(None)
            pt = None
            continue
        if pt is None:
            pt = xy_of(k)
        else:
            x1, y1 = pt
            lam = (GY - y1) * pow(GX - x1, -1, P) % P   # (k*G = +-G only for k = 1, n - 1: the walk starts there or ends there)
            x3 = (lam * lam - x1 - GX) % P
            pt = (x3, (lam * (x1 - x3) - y1) % P)
        out.append(pt[0])
        last = (k, pt)
    if last:
        assert xy_of(last[0]) == last[1]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dump_of(start, n, images=1):
    """uint8 [images * n, 32]: the dump of a sequential dispatch - image e of key i, x(lambda^e k) = beta^e x(k), at e * n + i; zeroed
    slots for keys that are no scalars."""
    xs = walk_x(start, n)
    rows = []
    for e in range(images):
        b = pow(BETA, e, P)
        rows += [bytes(32) if x is None else (b * x % P).to_bytes(32, "big") for x in xs]
    d = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32)
    d.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def strings_of(start, n, images=1):
    """The npub string of every slot of dump_of (None for a zeroed slot), tuple."""
    d = dump_of(start, n, images)
    return tuple(encode("npub", bytes(r)) if r.any() else None for r in d)


def key_of_slot(start, n, slot):
    """The secret key behind slot e * n + i of such a dispatch: lambda^e (start + i) mod n."""
    e, i = divmod(slot, n)
    return pow(LAMBDA, e, N) * (start + i) % N


def top_bits(row, nbits):
    """The first nbits bits of a 32-byte payload as an integer."""
    return int.from_bytes(bytes(row), "big") >> (256 - nbits)
