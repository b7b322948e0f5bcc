"""An Ed25519 / Solana reference in Python integers, written out here so that nothing on the expected side of the Solana
tests comes from the code under test: RFC 8032 arithmetic with hashlib.sha512, a 32 x 256 table of affine multiples of the base
point (8192 keys take a few seconds), Base58, the candidate stream of core/rnd.h with hashlib.sha256, and the range and
residue constructions the filter compiler is checked against."""
import hashlib
import struct

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
BY = (4 * pow(5, P - 2, P)) % P
ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
FMT_SOLANA = 12


def _recover_x(y, sign):
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    assert (x * x - x2) % P == 0
    return P - x if (x & 1) != sign else x


BX = _recover_x(BY, 0)


def add(p, q):
    """Affine addition on -x^2 + y^2 = 1 + d x^2 y^2 (complete)."""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P
    y3 = (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P
    return x3, y3


def _ext_add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        tab = []
        base = (BX, BY, 1, BX * BY % P)
        for _w in range(32):
            row = [(0, 1, 1, 0)]
            for _j in range(256):
                row.append(_ext_add(row[-1], base))
            base = row.pop()
            tab.append(row)
        _TABLE = tab
    return _TABLE


def encode_point(x, y):
    return (y | (x & 1) << 255).to_bytes(32, "little")


def mul_base(k):
    """k * B for 0 <= k < 2^256, as the 32 encoded bytes."""
    tab = _table()
    acc = (0, 1, 1, 0)
    for w in range(32):
        acc = _ext_add(acc, tab[w][(k >> (8 * w)) & 255])
    zi = pow(acc[2], P - 2, P)
    return encode_point(acc[0] * zi % P, acc[1] * zi % P)


def mul_base_slow(k):
    """The same by double-and-add over the affine law: a check of the table."""
    r, q = (0, 1), (BX, BY)
    while k:
        if k & 1:
            r = add(r, q)
        q = add(q, q)
        k >>= 1
    return encode_point(*r)


def scalar_of_seed(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a


def public_key(seed):
    return mul_base(scalar_of_seed(seed))


def b58encode(data):
    n = int.from_bytes(data, "big")
    s = ""
    while n:
        n, r = divmod(n, 58)
        s = ALPHABET[r] + s
    z = len(data) - len(data.lstrip(b"\0"))
    return "1" * z + s


def address(pub):
    return b58encode(pub)


def keypair_base58(seed):
    return b58encode(seed + public_key(seed))


def seed24(seed):
    """The 24 seed bytes the u64 seeds of the ABI stand for."""
    return struct.pack("<Q", seed) + bytes(16)


def stream_seed(seed, stream, index):
    """Candidate `index` of stream `stream`: the SHA-256 of the core/rnd.h message, every draw a key."""
    if isinstance(seed, int):
        seed = seed24(seed)
    return hashlib.sha256(b"vgen-mi355x-rand" + seed + struct.pack("<IQ", stream, index)).digest()


def stream_payloads(seed, stream, first, n):
    return [public_key(stream_seed(seed, stream, first + i)) for i in range(n)]


# ---- what a pattern means for the number N = the 32 bytes read big-endian ------------------------------------------

def val(s):
    v = 0
    for ch in s:
        v = v * 58 + ALPHABET.index(ch)
    return v


def prefix_ranges(s):
    """The inclusive ranges of N whose address starts with s."""
    z = len(s) - len(s.lstrip("1"))
    rest = s[z:]
    if not rest:   # only '1's: at least z leading zero bytes
        return [(0, 2 ** (8 * (32 - z)) - 1)]
    # exactly z leading zero bytes: 2^(8(31-z)) <= N < 2^(8(32-z)), and the digits of N start with rest
    lo_b, hi_b = 2 ** (8 * (31 - z)), 2 ** (8 * (32 - z)) - 1
    out = []
    for d in range(len(rest), 45):
        lo = val(rest) * 58 ** (d - len(rest))
        hi = (val(rest) + 1) * 58 ** (d - len(rest)) - 1
        lo, hi = max(lo, lo_b), min(hi, hi_b)
        if lo <= hi:
            out.append((lo, hi))
    return out


def suffix_residue(s):
    """(modulus, residue): an address of at least len(s) characters ends with s iff N mod 58^len(s) = val(s)."""
    return 58 ** len(s), val(s)
