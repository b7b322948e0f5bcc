"""What a split-key search must compute, without the code under test.

A searcher given the requester's public key P = s * G that walks the partial keys k tests the points P + k * G: the address of partial
k is the address of the EFFECTIVE key (s + k) mod n, which only the requester knows.  Every expected value here is the oracle's for
that effective key: oracle.pyoracle payload / generate for the reference's formats, and for the two formats the oracle does not know
(6: the contract an account deploys with nonce 0; 10: Nostr's x-only key) the oracle's hashes and public keys over the published
definitions.  Images come from Python integers with the published lambda and beta, as in tests/nostr_vectors.py: image v of a key is
lambda^(v % 3) * key, negated for v >= 3, and its point (beta^(v % 3) x, +-y).

Shared by tests/test_splitkey.py, tests/test_splitkey_scan_host.py (CPU) and tests/test_gpu_splitkey.py; walks are computed once
(lru_cache) and read-only."""
import functools

import numpy as np

from oracle import pyoracle as vo
from tests import nostr_vectors as nv

N, P, BETA, LAMBDA = nv.N, nv.P, nv.BETA, nv.LAMBDA
FMT_CONTRACT, FMT_NOSTR = 6, 10
KEY_FORMATS = (0, 1, 2, 3, 4, 5, 6, 10)


def images_of(fmt):
    return 3 if fmt == FMT_NOSTR else 6


def payload_len(fmt):
    return 32 if fmt in (vo.FMT_P2TR, FMT_NOSTR) else 20


def image_key(key, v):
    """Image v of a key, as vgen_key_variant numbers them."""
    k = pow(LAMBDA, v % 3, N) * key % N
    return N - k if v >= 3 else k


def image_point(x, y, v):
    return pow(BETA, v % 3, P) * x % P, (P - y) if v >= 3 else y


def payload_of_point(fmt, x, y):
    """The payload of the public key (x, y): the published definition of each format over the oracle's hashes."""
    xb, yb = x.to_bytes(32, "big"), y.to_bytes(32, "big")
    pub33 = bytes([2 + (y & 1)]) + xb
    if fmt in (vo.FMT_P2PKH, vo.FMT_P2WPKH):
        return vo.hash160(pub33)
    if fmt == vo.FMT_P2SH_P2WPKH:
        return vo.hash160(b"\x00\x14" + vo.hash160(pub33))
    if fmt == vo.FMT_P2PKH_UNCOMPRESSED:
        return vo.hash160(b"\x04" + xb + yb)
    if fmt == vo.FMT_ETHEREUM:
        return vo.keccak256(xb + yb)[12:]
    if fmt == FMT_CONTRACT:                      # keccak256(rlp([account, 0]))[12:]
        return vo.keccak256(b"\xd6\x94" + vo.keccak256(xb + yb)[12:] + b"\x80")[12:]
    if fmt == FMT_NOSTR:
        return xb
    raise ValueError(fmt)


def payload_of_key(fmt, key):
    """The oracle's payload of a key (None when it is no key)."""
    if not 0 < key < N:
        return None
    if fmt <= vo.FMT_ETHEREUM:
        return vo.payload(fmt, key)
    return payload_of_point(fmt, *nv.xy_of(key))


def address_of_payload(fmt, pl):
    if fmt == FMT_NOSTR:
        return nv.encode("npub", pl)
    if fmt in (vo.FMT_ETHEREUM, FMT_CONTRACT):
        return vo.eip55(pl)
    if fmt == vo.FMT_P2TR:
        return vo.segwit_addr("bc", 1, pl)
    return vo.address_from_hash160(fmt, pl)


def address_of_key(fmt, key):
    if fmt <= vo.FMT_ETHEREUM:
        return vo.generate(fmt, key)["address"]
    return address_of_payload(fmt, payload_of_key(fmt, key))


def pub33(key):
    pub = vo.pubkey(key)
    return bytes([2 + (pub[64] & 1)]) + pub[1:33]


@functools.lru_cache(maxsize=None)
def walk_xy(first, n):
    """The points e * G for the effective keys e = (first + i) mod n, i < n, as (x, y) integers (None where e = 0): one oracle
    multiplication at the first key (and after a zero), affine additions of G in Python integers after it, the last point checked
    against the oracle again."""
    out, pt, last = [], None, None
    for i in range(n):
        e = (first + i) % N
        if e == 0:
            out.append(None)
            pt = None
            continue
        if pt is None:
            pt = nv.xy_of(e)
        else:
            x1, y1 = pt
            if x1 == nv.GX:                      # e - 1 = 1: a doubling (e - 1 = n - 1 is followed by the zero above)
                lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
            else:
                lam = (nv.GY - y1) * pow(nv.GX - x1, -1, P) % P
            x3 = (lam * lam - x1 - nv.GX) % P
            pt = (x3, (lam * (x1 - x3) - y1) % P)
        out.append(pt)
        last = (e, pt)
    if last:
        assert nv.xy_of(last[0]) == last[1]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dump_of(fmt, first, n, images=1):
    """uint8 [images * n, payload_len]: the dump of a dispatch whose slot i has the effective key (first + i) mod n - image v of key i at
    v * n + i, zeroed slots where there is no key.  Formats 0 - 5 without images: the oracle's own payload_seq where the walk does not
    wrap; everything else from walk_xy and the oracle's hashes (anchored on the oracle's payload at the first and the last key)."""
    plen = payload_len(fmt)
    first %= N
    if images == 1 and fmt <= vo.FMT_ETHEREUM and 0 < first and first + n <= N:
        d = np.frombuffer(vo.payload_seq(fmt, first, n), dtype=np.uint8).reshape(n, plen)
    else:
        assert fmt != vo.FMT_P2TR or images == 1
        pts = walk_xy(first, n)
        rows = []
        for v in range(images):
            for pt in pts:
                if pt is None:
                    rows.append(bytes(plen))
                elif fmt == vo.FMT_P2TR:
                    rows.append(vo.taproot_output_key(b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")))
                else:
                    rows.append(payload_of_point(fmt, *image_point(*pt, v)))
        d = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(images * n, plen)
        for i in (0, n - 1):                     # the definitions above against the oracle's own derivation
            e = (first + i) % N
            if e:
                assert bytes(d[i]) == payload_of_key(fmt, e)
    d = d.copy()
    d.flags.writeable = False
    return d
