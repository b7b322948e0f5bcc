"""Crafted offset tables for the sequential scan's kernels, and what they must compute - in Python integers only.

seq_bwd_kernel (vgen_amd/csrc/device/kernels.hip) adds the lane's table point R = (rx, ry) and its negation to S uniform points
Q_j = (qx, qy) with the affine formulas

    lam = (+-ry - qy) / (rx - qx),    x3 = lam^2 - rx - qx,    y3 = lam (qx - x3) - qy,

which never use the curve equation: for a fixed Q and ANY wanted result (T, T2) a table point exists,

    lam = (T2 + qy) / (qx - T),    rx = lam^2 - T - qx,    ry = +-(qy + lam (rx - qx)).

So a test can put x3 and y3 on the residues whose weak products (core/fe.h) leave [0, p) - below C = 2^32 + 977 the product comes out
in [p, 2^256), in [C, 8C) it comes out at or above 2^256 - where fe_canonicalize_product takes its slow path behind a wave ballot and
fe_parity_weak has to flip the raw bit 0.  With curve points that happens to one key in eight million.

This module shares no code with the product: integers for the additions, oracle.pyoracle for the hashes, the published value of
beta for the endomorphism images.  tests/test_seq_vectors.py checks the vectors themselves (targets reached, class counts, the
host build of fe.h replayed on every crafted key); tests/test_gpu_seq_kernels.py runs them through the shipped kernels.

Per lane at most ONE key (j*, sgn*) is crafted; the lane's other 2S - 1 keys follow from the same R and are compared as well.
Classes of a target, for T (x3) and for T2 (y3) alike:
    a   [0, C), with 0, 1, 2, C - 1            the weak product lies in [p, 2^256)
    b   [C, 8C), with C, C + 1, 8C - 1         the weak product reaches 2^256
    c   p - 1, p - 2, 2^255, 2^232 - 1, 2^232, and values with limbs 2..7 all ones below p - C: the superset test fires without need
    d   (six-image runs, T only) T' / beta and T' / beta^2 for T' of a and b: the IMAGE's product needs the fix, not x3
    e   controls in [2^45, p)
Waves (64 lanes) come in four kinds, in turn: no crafted lane; exactly one, at a random lane; every lane crafted at the same
(j*, sgn*); every lane crafted, positions mixed.  The uncrafted lanes of the first two kinds carry operand extremes
(rx, ry in {1, 2, p - 1, p - 2}), and so do some Q_j (qx or qy in {1, p - 1}: nqx = p - 1 gives dx, nsum and dy their largest limbs).
No coordinate handed to the kernels is 0 or >= p, and no denominator rx - qx_j is 0 (one zero poisons a whole workgroup's tree).
A six-image run gets no target y3 = 0: the kernels take the parity of p - y as the flipped parity of y, which holds for every y but 0,
and no point of a curve of odd order has y = 0 (kernels.hip says so where it negates).  Measured on an MI355X with y3 = 0 in the set
of 256 lanes, format 0: the three negated images of that one key carried prefix 0x03 where -0 = 0 asks for 0x02, every other slot
equal.  x3 = 0 stays in every set, and y3 = 0 in every run without the images."""
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle as vo  # noqa: E402

P = 2**256 - 2**32 - 977
C = 2**32 + 977
# beta, a primitive cube root of unity mod p: the secp256k1 endomorphism lambda (x, y) = (beta x, y)  (SEC 2 / Gallant-Lambert-Vanstone;
# the constant as libsecp256k1's field tests spell it)
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
assert pow(BETA, 3, P) == 1 and BETA != 1
M29 = (1 << 29) - 1

SPECIAL = {
    "a": [0, 1, 2, C - 1],
    "b": [C, C + 1, 8 * C - 1],
    "c": [P - 1, P - 2, 1 << 255, (1 << 232) - 1, 1 << 232],
}
# the turn of the classes among a set's crafted keys (coprime lengths: every pair of classes meets)
TURN_X = ["a", "b", "a", "b", "c", "a", "b", "e"]
TURN_X_ENDO = ["a", "b", "d", "a", "b", "d", "c", "a", "b", "d", "e"]
TURN_Y = ["a", "b", "a", "b", "c", "a", "b", "e", "b"]
KINDS = ("none", "one", "same", "mixed")
EXTREMES = [1, 2, P - 1, P - 2]

GEOMETRY = {"g256": (256, 8), "g512": (512, 16), "g65": (256 * 65, 2)}   # name -> (lanes, S)


def limbs_of(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def class_of(t):
    return "a" if t < C else "b" if t < 8 * C else None


class Crafted:
    __slots__ = ("u", "j", "sgn", "T", "T2", "cx", "cy", "index")


class Vectors:
    """One dispatch: the table, the Q_j, the crafted keys, and x3 / y3 of every key by dump index."""


def _draw(rng, cls, k, nonzero=False):
    """k-th target of a class: the listed values first, then random members (nonzero: without 0)."""
    listed = [t for t in SPECIAL.get(cls, []) if t or not nonzero]
    if k < len(listed):
        return listed[k]
    if cls == "a":
        return rng.randrange(1 if nonzero else 0, C)
    if cls == "b":
        return rng.randrange(C, 8 * C)
    if cls == "c":   # limbs 2..7 all ones and the top limb 2^24 - 1, below p - C: every other one hard against that bound
        low = rng.randrange((1 << 58) - (1 << 34), (1 << 58) - 2 * C) if k % 2 else rng.randrange(0, (1 << 58) - 2 * C)
        return (1 << 256) - (1 << 58) + low
    if cls == "d":   # beta^e T = T' with T' of class a (even k) or b, e = 1 or 2
        tp = _draw(rng, "ab"[k % 2], 10 + k)
        e = 1 + (k // 2) % 2
        return tp * pow(BETA, -e, P) % P
    return rng.randrange(1 << 45, P)


def _positions(S):
    """The (j*, sgn*) every set must cover: j = 0 (idx = inv), j = S - 1 (the first iteration), a middle j; both signs."""
    return sorted({(j, sgn) for j in (0, S - 1, S // 2) for sgn in (0, 1)})


@functools.lru_cache(maxsize=None)
def vectors(geometry, endo=False):
    lanes, S = GEOMETRY[geometry]
    rng = random.Random(f"seq vectors {geometry} {endo}")
    v = Vectors()
    v.geometry, v.lanes, v.S, v.endo, v.n, v.half = geometry, lanes, S, endo, 2 * S * lanes, S * lanes
    # Q_j: random residues, some coordinates at the extremes
    q = [[rng.randrange(3, P - 2), rng.randrange(3, P - 2)] for _ in range(S)]
    edges = [(2, 0, 1), (5, 1, P - 1), (6, 0, P - 1), (3, 1, 1)] if S > 2 else [(1, 0, P - 1), (0, 1, 1)]
    if not endo:   # (the six-image sets keep random Q_j: "some dispatches")
        for j, c, val in edges:
            q[j][c] = val
    assert len({x for x, _ in q}) == S
    v.q = [tuple(p) for p in q]
    qxs = {x for x, _ in q}

    turn_x = TURN_X_ENDO if endo else TURN_X
    seen = {}                     # class -> targets drawn so far, per coordinate
    rx, ry = [0] * lanes, [0] * lanes
    v.crafted, v.kinds = [], []
    covering = _positions(S)
    every = [(j, sgn) for j in range(S) for sgn in (0, 1)]

    def craft(u, j, sgn, cx, cy):
        for _ in range(8):
            kx, ky = seen.get(("x", cx), 0), seen.get(("y", cy), 0)
            T, T2 = _draw(rng, cx, kx), _draw(rng, cy, ky, nonzero=endo)
            qx, qy = v.q[j]
            seen[("x", cx)], seen[("y", cy)] = kx + 1, ky + 1
            if T == qx:
                continue
            lam = (T2 + qy) * pow(qx - T, -1, P) % P
            x = (lam * lam - T - qx) % P
            y = (qy + lam * (x - qx)) % P
            if sgn:
                y = -y % P
            if x == 0 or y == 0 or x in qxs:
                continue   # redraw: the next targets of the same classes
            rx[u], ry[u] = x, y
            c = Crafted()
            c.u, c.j, c.sgn, c.T, c.T2, c.cx, c.cy = u, j, sgn, T, T2, cx, cy
            c.index = v.half - (u + 1) * S + j if sgn else v.half + u * S + j
            v.crafted.append(c)
            return
        raise AssertionError("no table point for the target")

    def classes():
        k = len(v.crafted)
        return turn_x[k % len(turn_x)], TURN_Y[k % len(TURN_Y)]

    def plain(u, l):
        while True:
            x, y = rng.randrange(1, P), rng.randrange(1, P)
            if l % 16 in (3, 11):
                x = EXTREMES[(l // 16 + u // 64) % 4]
            if l % 16 in (7, 11):
                y = EXTREMES[(l // 16 + u // 64 + 1) % 4]
            if x not in qxs:
                rx[u], ry[u] = x, y
                return
            l += 16   # (an extreme that is some qx: the next one)

    for w in range(lanes // 64):
        kind = KINDS[w % 4]
        v.kinds.append(kind)
        base = w * 64
        if kind in ("none", "one"):
            for l in range(64):
                plain(base + l, l)
            if kind == "one":   # classes a and b in turn, on x3 and y3 in turn: one lane alone sends its wave through the slow path
                k = w // 4
                cls = "ab"[k % 2]
                j, sgn = covering[k % len(covering)]
                craft(base + rng.randrange(64), j, sgn, *((cls, "e") if (k // 2) % 2 == 0 else ("e", cls)))
        elif kind == "same":
            j, sgn = covering[(w // 4) % len(covering)]
            for l in range(64):
                craft(base + l, j, sgn, *classes())
        else:
            order = covering + [every[rng.randrange(len(every))] for _ in range(64 - len(covering))]
            rng.shuffle(order)
            for l in range(64):
                craft(base + l, *order[l], *classes())
    for u in range(lanes):
        assert 0 < rx[u] < P and 0 < ry[u] < P and all((rx[u] - qx) % P for qx in qxs), u
    v.rx, v.ry = rx, ry
    v.rtab = np.array([limbs_of(x) for x in rx], dtype=np.uint32).T.copy()
    v.rtab = np.ascontiguousarray(np.concatenate([v.rtab, np.array([limbs_of(y) for y in ry], dtype=np.uint32).T]))
    assert v.rtab.shape == (18, lanes)
    v.qlimbs = np.array([limbs_of(x) + limbs_of(y) for x, y in v.q], dtype=np.uint32)

    # every key of the dispatch: index half + u S + j for +R, half - (u + 1) S + j for -R
    v.x3, v.y3 = [None] * v.n, [None] * v.n
    for u in range(lanes):
        for j in range(S):
            qx, qy = v.q[j]
            inv = pow(rx[u] - qx, -1, P)
            for sgn in (0, 1):
                lam = ((-ry[u] if sgn else ry[u]) - qy) * inv % P
                x3 = (lam * lam - rx[u] - qx) % P
                index = v.half - (u + 1) * S + j if sgn else v.half + u * S + j
                assert v.x3[index] is None
                v.x3[index], v.y3[index] = x3, (lam * (qx - x3) - qy) % P
    assert None not in v.x3
    return v


def images(v):
    """(x, y) of every slot of the dump: the n keys, or - six-image runs - image sneg * 3 + e of key i at (sneg * 3 + e) n + i, with
    x-images beta^e x and y-images +-y."""
    if not v.endo:
        return list(zip(v.x3, v.y3))
    out = []
    for sneg in (0, 1):
        for e in range(3):
            b = pow(BETA, e, P)
            out += [(b * x % P, -y % P if sneg else y) for x, y in zip(v.x3, v.y3)]
    return out


def payload(fmt, x, y):
    """The 20 bytes the kernels hash out of an affine point, per format (the numbers of include/vgen_hip.h)."""
    X, Y = x.to_bytes(32, "big"), y.to_bytes(32, "big")
    if fmt in (0, 1):
        return vo.hash160(bytes([2 | (y & 1)]) + X)
    if fmt == 2:
        return vo.hash160(b"\x00\x14" + vo.hash160(bytes([2 | (y & 1)]) + X))
    if fmt == 4:
        return vo.hash160(b"\x04" + X + Y)
    account = vo.keccak256(X + Y)[12:]
    if fmt == 5:
        return account
    assert fmt == 6
    # RLP of [account, nonce 0]: a list of 22 payload bytes (0xc0 + 22), a 20-byte string (0x80 + 20), the empty string for 0
    return vo.keccak256(b"\xd6\x94" + account + b"\x80")[12:]


@functools.lru_cache(maxsize=None)
def dump_of(geometry, endo, fmt):
    """uint8 [slots, 20]: the whole dump of the dispatch (read-only: shared between tests)."""
    v = vectors(geometry, endo)
    d = np.frombuffer(b"".join(payload(fmt, x, y) for x, y in images(v)), dtype=np.uint8).reshape(-1, 20)
    assert d.shape[0] == v.n * (6 if endo else 1)
    d.flags.writeable = False
    return d


def census(v):
    """Crafted keys per class, read from the reference's x3 / y3 at the crafted positions, and waves per kind.  (Only crafted keys
    count: where an extreme ry meets qy = +-ry the slope is 0 and y3 = -qy is 1 without any product behind it - "slope 0" says how
    many such keys the set holds; they are compared like every other key.)"""
    out = {"x3 a": 0, "x3 b": 0, "y3 a": 0, "y3 b": 0, "d": 0}
    b1, b2 = BETA, BETA * BETA % P
    for c in v.crafted:
        x, y = v.x3[c.index], v.y3[c.index]
        if class_of(x):
            out["x3 " + class_of(x)] += 1
        if class_of(y):
            out["y3 " + class_of(y)] += 1
        if v.endo and (class_of(b1 * x % P) or class_of(b2 * x % P)):
            out["d"] += 1
    out["slope 0"] = sum(1 for u in range(v.lanes) for _, qy in v.q for y in (v.ry[u], P - v.ry[u]) if y == qy)
    for k in KINDS:
        out["waves " + k] = v.kinds.count(k)
    return out


def rare_keys(v):
    """Dump indices of the crafted keys of classes a and b, on either coordinate."""
    return [c.index for c in v.crafted if class_of(v.x3[c.index]) or class_of(v.y3[c.index])]


# ---- the launch configurations of tests/test_gpu_seq_kernels.py ----------------------------------------------------------------------

def _configs():
    out = []
    for g, (lanes, S) in GEOMETRY.items():
        out.append(dict(geometry=g, fmt=0))
        out.append(dict(geometry=g, fmt=0, lone=1))
        for fmt in (0, 2):
            for kpl in sorted({1, 2, 4, 2 * S} if S == 2 else {1, 4, 2 * S}):
                out.append(dict(geometry=g, fmt=fmt, split=1, kpl=kpl))
        for fmt in (2, 4, 5, 6):
            out.append(dict(geometry=g, fmt=fmt))
    for g in ("g256", "g512"):
        for fmt in (0, 2, 4, 5, 6):
            out.append(dict(geometry=g, fmt=fmt, endo=1))
    for c in out:
        for k in ("lone", "endo", "split", "kpl"):
            c.setdefault(k, 0)
        c["id"] = f"{c['geometry']}-fmt{c['fmt']}" + ("-lone" if c["lone"] else "") + ("-endo" if c["endo"] else "") + \
                  (f"-split{c['kpl']}" if c["split"] else "")
    return out


DUMP_CONFIGS = _configs()
FILTER_CONFIGS = [dict(geometry=g, fmt=0, lone=lone, endo=0, split=split, kpl=4 if split else 0,
                       id=f"{g}-" + ("lone" if lone else "split4" if split else "fused"))
                  for g in GEOMETRY for lone, split in ((0, 0), (1, 0), (0, 1))]
SETS = sorted({(c["geometry"], bool(c["endo"])) for c in DUMP_CONFIGS + FILTER_CONFIGS})


@functools.lru_cache(maxsize=None)
def filter_nibble(geometry):
    """The value of the top four bits of H[0] a filter-mode test asks for: the one most keys of classes a and b carry (format 0)."""
    v, d = vectors(geometry), dump_of(geometry, False, 0)
    top = d[rare_keys(v), 0] >> 4
    counts = np.bincount(top, minlength=16)
    return int(counts.argmax()), int(counts.max())
