"""A Tor v3 onion reference in Python integers, built on tests/solana_vectors.py (whose mul_base is pinned to OpenSSL and RFC 8032)
plus hashlib.sha3_256, hashlib.sha512 and base64: nothing on the expected side of the onion tests comes from the code under test.
The walk: candidate i of a dispatch has the scalar base + 8 (first + i), its point is A(base + 8 first) + i (8B)."""
import base64
import hashlib

from tests import solana_vectors as sv

P, D = sv.P, sv.D
FMT_ONION = 13
ALPHABET = "abcdefghijklmnopqrstuvwxyz234567"
NONCE_TAG = b"vgen-mi355x onion nonce key"
SQRT_M1 = pow(2, (P - 1) // 4, P)


def checksum(pub):
    return hashlib.sha3_256(b".onion checksum" + pub + b"\x03").digest()[:2]


def address(pub):
    """The 56 characters (without .onion) of a 32-byte public key."""
    return base64.b32encode(pub + checksum(pub) + b"\x03").decode().lower()


def decode(addr):
    """The public key, or None (strict: lower case, 56 characters, version 3, checksum)."""
    if addr.endswith(".onion"):
        addr = addr[:-6]
    if len(addr) != 56 or any(c not in ALPHABET for c in addr):
        return None
    raw = base64.b32decode(addr.upper())
    pub, chk, ver = raw[:32], raw[32:34], raw[34]
    return pub if ver == 3 and chk == checksum(pub) else None


def expand(a):
    """The 64 bytes behind the header of hs_ed25519_secret_key for the scalar a."""
    s = a.to_bytes(32, "little")
    return s + hashlib.sha512(NONCE_TAG + s).digest()[32:]


def base_scalar(seed, stream):
    """The base scalar of stream `stream`: the clamped scalar of the stream's candidate 0 read as an Ed25519 seed."""
    return sv.scalar_of_seed(sv.stream_seed(seed, stream, 0))


def decode_point(enc):
    v = int.from_bytes(enc, "little")
    y, sign = v & ((1 << 255) - 1), v >> 255
    return sv._recover_x(y, sign), y


def point_of(k):
    return decode_point(sv.mul_base(k))


def neg(p):
    return (-p[0]) % P, p[1]


def on_curve(p):
    x, y = p
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def pair(p, q):
    """(x(P+Q), y(P+Q), x(P-Q), y(P-Q)) by the affine law."""
    s, d = sv.add(p, q), sv.add(p, neg(q))
    return s[0], s[1], d[0], d[1]


def walk_payloads(base, first, n):
    """The n payloads of a dispatch: 32 zero bytes where the scalar is 0 (no key)."""
    start = base + 8 * first
    assert start + 8 * (n - 1) < 2**255
    g8 = point_of(8)
    ext8 = (g8[0], g8[1], 1, g8[0] * g8[1] % P)
    x, y = point_of(start)
    acc = (x, y, 1, x * y % P)
    out = []
    for i in range(n):
        zi = pow(acc[2], P - 2, P)
        enc = sv.encode_point(acc[0] * zi % P, acc[1] * zi % P)
        out.append(bytes(32) if start + 8 * i == 0 else enc)
        acc = sv._ext_add(acc, ext8)
    return out


def digest(payloads):
    return hashlib.sha256(b"".join(payloads)).hexdigest()


# ---- the points the pair formulas are tried on: neutral, P itself, -P, order 2, order 4 (both), order 8, random ----

def order8_point():
    """A point of order 8: the 8-torsion part L * Q of the first point Q (by y = 2, 3, ...) whose part has full order."""
    y = 2
    while True:
        x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
        if pow(x2, (P - 1) // 2, P) == 1:
            q = (sv._recover_x(y, 0), y)
            t = (0, 1)
            k, a = sv.L, q
            while k:
                if k & 1:
                    t = sv.add(t, a)
                a = sv.add(a, a)
                k >>= 1
            t2 = sv.add(t, t)
            t4 = sv.add(t2, t2)
            if t4 != (0, 1):
                assert sv.add(t4, t4) == (0, 1) and on_curve(t)
                return t
        y += 1


def edge_points(p):
    """Q's for a given P: neutral, P, -P, order 2, the two of order 4, one of order 8."""
    return [(0, 1), p, neg(p), (0, P - 1), (SQRT_M1, 0), (P - SQRT_M1, 0), order8_point()]


# ---- what a prefix means for the payload: characters 0 .. 48 are bits of y alone ----

def prefix_mask(prefix):
    """(mask, value) over the 256-bit big-endian reading of the 32 payload bytes for a literal prefix of <= 49 characters."""
    assert len(prefix) <= 49
    mask = value = 0
    for c, ch in enumerate(prefix):
        sh = 256 - 5 * (c + 1)
        mask |= 31 << sh
        value |= ALPHABET.index(ch) << sh
    return mask, value


def point_bytes(k):
    """The 32 encoded bytes of k * B."""
    return sv.mul_base(k)
