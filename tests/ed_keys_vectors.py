"""Expected values of ed_keys_kernel (vgen_amd/csrc/device/kernels.hip) on tables the product never builds, in Python integers.

The kernel multiplies over EdArgs::table, a plain pointer: 32 windows of 256 entries, and lane i adds the entry its scalar's byte
selects in every window, low window first.  The scalar is clamp(SHA-512(seed)), so a test that chooses the seed knows the 32 digits and
with a CRAFTED table decides which curve points meet in the kernel's addition and which affine point reaches the shared inversion, the
encoder and the filter: points of order 1, 2, 4 and 8, a point added to itself, to its negative, to torsion; y = 0, x = 0, y a few
units from 0 and from p, both sign bits.  With the real table none of that can happen.

Built on tests/solana_vectors.py (P, D, scalar_of_seed, encode_point, stream_seed, prefix_ranges); nothing here comes from the code
under test.  tests/test_ed_keys_vectors.py holds it against the host build of the kernel's own functions and asserts that every
class a GPU test relies on is present; tests/test_gpu_ed_keys_kernel.py compares the shipped kernel with it, byte for byte."""
import functools
import random

from tests import solana_vectors as sv

P, D = sv.P, sv.D
WINDOWS, DIGITS, ENTRY_WORDS = 32, 256, 28
TABLE_WORDS = WINDOWS * DIGITS * ENTRY_WORDS
SQRT_M1 = pow(2, (P - 1) // 4, P)
NEUTRAL = (0, 1)
Q_NAMES = ("neutral", "order 2", "order 4, even x", "order 4, odd x", "order 8", "B", "B + order 8", "small y", "small y, -x", "y below p",
           "y below p, -x")

# the crafted dumps: two workgroups, the second with a ragged last keyed wave and a keyless one behind it
BATCH, N = 1024, 1000
# lanes that must hold a named class: first and last of a wave and of a workgroup, their neighbours, the last keyed pair (one leaf of
# the butterfly's first level)
NAMED = (0, 63, 64, 65, 511, 512, 513, N - 2, N - 1)


def on_curve(q):
    x, y = q
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def neg(q):
    return ((P - q[0]) % P, q[1])


def add(p, q):
    """The affine law of -x^2 + y^2 = 1 + d x^2 y^2, complete; one inversion for the two denominators (pow raises on a zero one)."""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    i = pow((1 + t) * (1 - t), -1, P)
    return (x1 * y2 + x2 * y1) * (1 - t) * i % P, (y1 * y2 + x1 * x2) * (1 + t) * i % P


def mul(k, q):
    r = NEUTRAL
    while k:
        if k & 1:
            r = add(r, q)
        q = add(q, q)
        k >>= 1
    return r


def xs_of_y(y):
    """The even-or-odd pair of x with (x, y) on the curve as (x, p - x), or None where there is none."""
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRT_M1 % P
    if (x * x - x2) % P:
        return None
    return x, (P - x) % P


@functools.lru_cache(maxsize=None)
def order8_point():
    """The first y = 2, 3, ... whose point, multiplied by the prime order of the base point's group, has order exactly 8."""
    y = 2
    while True:
        xs = xs_of_y(y)
        if xs:
            t = mul(sv.L, (xs[0], y))
            if mul(4, t) == (0, P - 1):
                return t
        y += 1


@functools.lru_cache(maxsize=None)
def small_y_point():
    """The curve point with the smallest y >= 2 (its smaller x)."""
    y = 2
    while xs_of_y(y) is None:
        y += 1
    return min(xs_of_y(y)), y


@functools.lru_cache(maxsize=None)
def fixed_points():
    """Q, with a name each."""
    b, t8 = (sv.BX, sv.BY), order8_point()
    x, y = small_y_point()
    q = [NEUTRAL, (0, P - 1), (SQRT_M1, 0), (P - SQRT_M1, 0), t8, b, add(b, t8), (x, y), (P - x, y), (x, P - y), (P - x, P - y)]
    assert SQRT_M1 % 2 == 0 and len(q) == len(Q_NAMES)
    return list(zip(Q_NAMES, q))


def Q():
    return [p for _, p in fixed_points()]


def small_order(q):
    """1, 2, 4 or 8 for a point of that order, None for any other."""
    for m in (1, 2, 4, 8):
        if q == NEUTRAL:
            return m
        q = add(q, q)
    return None


def limbs(v):
    """Nine canonical limbs of 29 bits (core/fe25519.h)."""
    assert 0 <= v < P
    return [(v >> (29 * k)) & 0x1FFFFFFF for k in range(9)]


@functools.lru_cache(maxsize=None)
def _entry(x, y):
    return tuple(limbs((y + x) % P) + limbs((y - x) % P) + limbs(2 * D * x * y % P) + [0])


def entry(x, y):
    """The 28 words of a table entry (core/ed25519.h): y + x, y - x, 2 d x y, one pad word."""
    return list(_entry(x, y))


NEUTRAL_ROW = tuple([NEUTRAL] * DIGITS)


@functools.lru_cache(maxsize=None)
def real_table():
    """table[w][j] = j 256^w B, affine, by repeated addition of the window's base."""
    tab, base = [], (sv.BX, sv.BY)
    for _ in range(WINDOWS):
        row = [NEUTRAL]
        for _ in range(DIGITS):
            row.append(add(row[-1], base))
        base = row.pop()
        tab.append(tuple(row))
    return tuple(tab)


def crafted_row():
    q = Q()
    return tuple(q[j % len(q)] for j in range(DIGITS))


TWO_W1, TWO_W2 = 5, 20


def two_window_rows():
    """C1[j] = Q[j % 8], C2[j] = +-Q[(j >> 3) % 8], negated where bit 6 of j is set."""
    q = Q()
    c1 = tuple(q[j % 8] for j in range(DIGITS))
    c2 = tuple(neg(q[(j >> 3) % 8]) if j & 64 else q[(j >> 3) % 8] for j in range(DIGITS))
    return c1, c2


REAL_BUT_W = 16
TABLES = ("one-window-1", "one-window-16", "one-window-31", "two-window", "real-but-one")


@functools.lru_cache(maxsize=None)
def table_points(name):
    if name == "real":
        return real_table()
    if name.startswith("one-window-"):
        w = int(name.rsplit("-", 1)[1])
        return tuple(crafted_row() if v == w else NEUTRAL_ROW for v in range(WINDOWS))
    if name == "two-window":
        c1, c2 = two_window_rows()
        return tuple(c1 if v == TWO_W1 else c2 if v == TWO_W2 else NEUTRAL_ROW for v in range(WINDOWS))
    if name == "real-but-one":
        return tuple(crafted_row() if v == REAL_BUT_W else row for v, row in enumerate(real_table()))
    raise KeyError(name)


def crafted_window(name):
    return {"one-window-1": 1, "one-window-16": 16, "one-window-31": 31, "real-but-one": REAL_BUT_W}[name]


def table_words(name):
    """The ED_TABLE_WORDS words of the table as a flat list: entry (w, j) at (256 w + j) * 28."""
    out = []
    for row in table_points(name):
        for x, y in row:
            out.extend(_entry(x, y))
    assert len(out) == TABLE_WORDS
    return out


def digits(seed):
    k = sv.scalar_of_seed(seed)
    return [(k >> (8 * w)) & 255 for w in range(WINDOWS)]


def point_of(points, seed):
    """The affine point a lane with this seed reaches: the sum over the 32 windows, low window first.  (Adding the neutral element
    by the law returns the other point exactly - x (1) + 0 over 1 + 0 - so a neutral entry is skipped, not divided for.)"""
    acc = NEUTRAL
    for w, j in enumerate(digits(seed)):
        q = points[w][j]
        if q != NEUTRAL:
            acc = add(acc, q)
    return acc


def payload(points, seed):
    return sv.encode_point(*point_of(points, seed))


# ---- what a lane of a crafted table is an example of ----------------------------------------------------------------------------------

def lane_classes(name, seed):
    """The names of the cases this seed stands for on table `name`."""
    q = Q()
    d = digits(seed)
    out = set()
    if name == "two-window":
        c1, c2 = two_window_rows()
        p1, p2 = c1[d[TWO_W1]], c2[d[TWO_W2]]
        s = add(p1, p2)
        small = set(q[:5]) | {neg(q[4])}
        if p1 == p2 and p1 != NEUTRAL:
            out.add("doubling")
            if p1 not in small:
                out.add("doubling of a point of large order")
        if s == NEUTRAL and p1 != NEUTRAL:
            out.add("cancelling")
            if p1 not in small:
                out.add("cancelling of a point of large order")
        if p1 in small and p1 != NEUTRAL and p2 not in small:
            out.add("torsion + large")
        if p2 in small and p2 != NEUTRAL and p1 not in small:
            out.add("large + torsion")
        if p1 in small and p2 in small and NEUTRAL not in (p1, p2):
            out.add("torsion + torsion")
        reached = s
    else:
        k = d[crafted_window(name)] % len(q)
        out.add("adds " + Q_NAMES[k])
        reached = q[k] if name.startswith("one-window") else None
    if reached is not None:
        x, y = reached
        if small_order(reached):
            out.add(f"reaches order {small_order(reached)}")
        if sv.encode_point(x, y) == bytes(32):
            out.add("zero payload")
        if sv.encode_point(x, y) == bytes(31) + b"\x80":
            out.add("payload 00..80")
        if x == 0:
            out.add("x = 0")
        if y == 0:
            out.add("y = 0")
        if 2 <= y < 64:
            out.add("y just above 0")
        if 2 <= P - y < 64:
            out.add("y just below p")
        out.add("sign bit %d" % (x & 1))
    return out


ONE_WINDOW_CLASSES = tuple(["adds " + n for n in Q_NAMES] +
                           ["reaches order 1", "reaches order 2", "reaches order 4", "reaches order 8", "zero payload", "payload 00..80",
                            "x = 0", "y = 0", "y just above 0", "y just below p", "sign bit 0", "sign bit 1"])
TWO_WINDOW_CLASSES = ("doubling", "doubling of a point of large order", "cancelling", "cancelling of a point of large order",
                      "torsion + large", "large + torsion", "torsion + torsion", "reaches order 1", "reaches order 2", "reaches order 4",
                      "reaches order 8", "zero payload", "payload 00..80", "sign bit 0", "sign bit 1")
REAL_BUT_CLASSES = tuple("adds " + n for n in Q_NAMES)


def required_classes(name):
    return TWO_WINDOW_CLASSES if name == "two-window" else REAL_BUT_CLASSES if name == "real-but-one" else ONE_WINDOW_CLASSES


# The class each named lane is re-drawn for.  Two-window: three rotations, so that doubling, cancelling and the zero payload each
# stand at EVERY named lane once - on both sides of the wave edge 63 | 64 and of the workgroup edge 511 | 512.
ROTATIONS = 3
TWO_NAMED = ("doubling", "cancelling", "zero payload")
# One window: the zero payload on both sides of both edges, other members of Q at the rest.
ONE_NAMED = {0: "payload 00..80", 63: "zero payload", 64: "zero payload", 65: "adds order 8", 511: "zero payload", 512: "zero payload",
             513: "adds y below p, -x", N - 2: "adds neutral", N - 1: "adds order 2"}


def named_class(name, rot, lane):
    if name == "two-window":
        return TWO_NAMED[(NAMED.index(lane) + rot) % 3]
    c = ONE_NAMED[lane]
    if name == "real-but-one" and not c.startswith("adds "):
        c = {"zero payload": "adds order 4, even x", "payload 00..80": "adds order 4, odd x"}[c]
    return c


@functools.lru_cache(maxsize=None)
def crafted_seeds(name, rot=0):
    """BATCH seeds for table `name` (those at and past N are uploaded and never read), drawn from a fixed generator, the named lanes
    re-drawn until they hold their class."""
    rng = random.Random(f"ed-keys {name} {rot}")
    seeds = [rng.randbytes(32) for _ in range(BATCH)]
    for lane in NAMED:
        want = named_class(name, rot, lane)
        tries = 0
        while want not in lane_classes(name, seeds[lane]):
            seeds[lane] = rng.randbytes(32)
            tries += 1
            assert tries < 5000, (name, rot, lane, want)
    return tuple(seeds)


def rotations(name):
    return range(ROTATIONS) if name == "two-window" else range(1)


@functools.lru_cache(maxsize=None)
def crafted_payloads(name, rot=0):
    """The BATCH expected payloads of the dump: the key where i < N, zero otherwise."""
    pts, seeds = table_points(name), crafted_seeds(name, rot)
    return tuple(payload(pts, seeds[i]) if i < N else bytes(32) for i in range(BATCH))


@functools.lru_cache(maxsize=None)
def crafted_class_lanes(name, rot=0):
    """class -> the keyed lanes that stand for it."""
    out = {}
    seeds = crafted_seeds(name, rot)
    for i in range(N):
        for c in lane_classes(name, seeds[i]):
            out.setdefault(c, []).append(i)
    return out


# ---- the real table: uploaded seeds and the stream ------------------------------------------------------------------------------------

REAL_LANES = 1025          # the largest n of a real-table test


@functools.lru_cache(maxsize=None)
def zero_seed_payload(name="real"):
    """What a keyless lane of an uploaded dispatch computes and must not report: the key of the all-zero seed."""
    return payload(table_points(name), bytes(32))


@functools.lru_cache(maxsize=None)
def real_seeds():
    """REAL_LANES seeds; lane 0 re-drawn until its address shares its first two characters with the all-zero seed's, so that a
    prefix taken from lane 0 is one the key of every keyless lane's seed would match; lane 1 re-drawn until its key starts with a zero
    byte, so that its address starts with '1' as the address of the all-zero PAYLOAD does - the payload a keyless lane hands the filter."""
    rng = random.Random("ed-keys real")
    seeds = [rng.randbytes(32) for _ in range(REAL_LANES)]
    two = sv.address(zero_seed_payload())[:2]
    for lane, ok in ((0, lambda k: sv.address(k)[:2] == two), (1, lambda k: k[0] == 0 and k[1] != 0)):
        tries = 0
        while not ok(sv.public_key(seeds[lane])):
            seeds[lane] = rng.randbytes(32)
            tries += 1
            assert tries < 200000
    return tuple(seeds)


@functools.lru_cache(maxsize=None)
def real_payloads():
    pts = real_table()
    return tuple(payload(pts, s) for s in real_seeds())


def dump_of(keys, batch, n):
    return [keys[i] if i < n else bytes(32) for i in range(batch)]


def prefix_hits(keys, prefix):
    """The indices whose 32 bytes, read big-endian, lie in a range of the prefix: exact for a literal prefix."""
    ranges = sv.prefix_ranges(prefix)
    return [i for i, p in enumerate(keys) if any(lo <= int.from_bytes(p, "big") <= hi for lo, hi in ranges)]


def uploaded_prefix(length):
    return sv.address(real_payloads()[0])[:length]


# the stream form: every lane of the batch draws a key, keyed or not
STREAM_SEED, STREAM = 0x5EED0123456789AB, 3
STREAM_FIRSTS = (0, 2**32 - 300, 2**40 + 7)
STREAM_SHAPES = ((512, 512), (1024, 700))


@functools.lru_cache(maxsize=None)
def stream_keys(first, batch):
    return tuple(sv.stream_payloads(STREAM_SEED, STREAM, first, batch))


def seed_words():
    """RndSeed::w of the u64 seed."""
    return [STREAM_SEED & 0xFFFFFFFF, STREAM_SEED >> 32, 0, 0, 0, 0]


STREAM_FILTER_SHAPE = (1024, 513)


@functools.lru_cache(maxsize=None)
def stream_prefix(length):
    """(first, prefix): the first stream position from STREAM_FIRSTS[1] on, in steps of the batch, at which some keyed lane's prefix of
    this length is also the prefix of a keyless lane's draw; the prefix is the first such keyed lane's."""
    batch, n = STREAM_FILTER_SHAPE
    first = STREAM_FIRSTS[1]
    for _ in range(64):
        strings = [sv.address(p) for p in stream_keys(first, batch)]
        keyless = {s[:length] for s in strings[n:]}
        for s in strings[:n]:
            if s[:length] in keyless:
                return first, s[:length]
        first += batch
    raise AssertionError("no stream position with a keyless lane that would match")
