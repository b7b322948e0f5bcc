"""The crafted vectors of tests/seq_vectors.py, checked without a GPU: that every crafted key reaches its target in the Python
reference, that every launch configuration of tests/test_gpu_seq_kernels.py holds the class counts and wave kinds it promises,
and - coverage evidence, and a check of the host build of core/fe.h - that the field routines the kernels chain
(fe_mul -> fe_sqr_add -> fe_canonicalize_product -> fe_mul_add -> fe_parity_weak / fe_canonicalize_product, with a canonical 1/dx)
leave [0, p) with their weak products on the keys of classes a and b, and still return the Python values.  The expected values of
the GPU test never come from here: they are seq_vectors' integers and oracle hashes.

Class counts asked of every configuration (each key counted from the reference's x3 / y3 alone): at least 64 keys of class a and
of class b on x3 and on y3 (32 at 256 lanes, which hold four waves), at least 32 of class d on six-image runs.  Four waves of each
kind are asked of the sets that have sixteen waves or more and of the configurations taken together: a set of 256 lanes has one
wave of each kind, one of 512 lanes two."""
import ctypes
import json
import os

import pytest

import seq_vectors as sv
from conftest import locked_make
from seq_vectors import BETA, C, P, limbs_of

HERE = os.path.dirname(os.path.abspath(__file__))
A9 = ctypes.c_uint32 * 9


@pytest.fixture(scope="module")
def core():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "libcoretest.so")
    return ctypes.CDLL(os.path.join(HERE, "native", "libcoretest.so"))


def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


SET_IDS = [f"{g}{'-endo' if e else ''}" for g, e in sv.SETS]


@pytest.mark.parametrize("geometry,endo", sv.SETS, ids=SET_IDS)
def test_crafted_keys_reach_their_targets(geometry, endo):
    v = sv.vectors(geometry, endo)
    assert len({c.u for c in v.crafted}) == len(v.crafted)   # at most one crafted key per lane
    for c in v.crafted:
        assert (v.x3[c.index], v.y3[c.index]) == (c.T, c.T2), (c.u, c.j, c.sgn)
        for cls, t in ((c.cx, c.T), (c.cy, c.T2)):
            if cls in "ab":
                assert sv.class_of(t) == cls
            elif cls == "c":
                assert t in sv.SPECIAL["c"] or (1 << 256) - (1 << 58) <= t < P - C
            elif cls == "e":
                assert 1 << 45 <= t < P
            else:
                assert sv.class_of(t) is None and (sv.class_of(BETA * t % P) or sv.class_of(BETA * BETA * t % P))
    assert all(y != 0 for y in v.y3) if endo else 0 in v.y3
    # the listed members of every class, on both coordinates
    for cls, members in sv.SPECIAL.items():
        assert set(members) <= {c.T for c in v.crafted if c.cx == cls}, cls
        assert set(members) - ({0} if endo else set()) <= {c.T2 for c in v.crafted if c.cy == cls}, cls   # (no y3 = 0 under six images: seq_vectors)
    # j = 0, j = S - 1 and a middle j, each with both signs; in waves crafted at one position and in mixed ones
    want = {(j, s) for j in (0, v.S - 1, v.S // 2) for s in (0, 1)}
    assert want <= {(c.j, c.sgn) for c in v.crafted}
    same = {(c.j, c.sgn) for c in v.crafted if v.kinds[c.u // 64] == "same"}
    assert same and (len(v.kinds) < 24 or want <= same)
    # operand extremes
    ext = set(sv.EXTREMES)
    assert ext - {x for x, _ in v.q} <= set(v.rx) and ext <= set(v.ry)   # (an rx that is some qx would be a zero denominator)
    if endo:
        assert ext <= set(v.rx)
    assert all(0 < x < P and 0 < y < P for x, y in v.q)
    if not endo:
        qxs, qys = {x for x, _ in v.q}, {y for _, y in v.q}
        assert ({1, P - 1} <= qxs and {1, P - 1} <= qys) if v.S > 2 else (P - 1 in qxs and 1 in qys)   # (S = 2 has two Q_j)
    # all indices of the dump are keys of exactly one (lane, j, sign): vectors() asserted it while filling


def test_every_configuration_holds_its_counts():
    total = dict.fromkeys(sv.KINDS, 0)
    for geometry, endo in sv.SETS:
        v = sv.vectors(geometry, endo)
        n = sv.census(v)
        configs = [c["id"] for c in sv.DUMP_CONFIGS + sv.FILTER_CONFIGS if (c["geometry"], bool(c["endo"])) == (geometry, endo)]
        print(f"{geometry}{' six images' if endo else ''}: {v.lanes} lanes x 2 x {v.S} = {v.n} keys, {len(v.crafted)} crafted; "
              f"{json.dumps(n)}; {len(configs)} configurations")
        least = 32 if v.lanes == 256 else 64
        for k in ("x3 a", "x3 b", "y3 a", "y3 b"):
            assert n[k] >= least, (geometry, endo, k, n[k])
        if endo:
            assert n["d"] >= 32, (geometry, n["d"])
        for k in sv.KINDS:
            assert n["waves " + k] >= (4 if v.lanes >= 1024 else 1), (geometry, k)
            total[k] += n["waves " + k] * len(configs)
    assert all(t >= 4 for t in total.values()), total
    # every instantiation the issue names is among the configurations
    ids = {c["id"] for c in sv.DUMP_CONFIGS}
    for g, (_, S) in sv.GEOMETRY.items():
        assert {f"{g}-fmt0", f"{g}-fmt0-lone", f"{g}-fmt2", f"{g}-fmt4", f"{g}-fmt5", f"{g}-fmt6"} <= ids
        for fmt in (0, 2):
            assert {f"{g}-fmt{fmt}-split{k}" for k in (1, 4, 2 * S)} <= ids
    for g in ("g256", "g512"):
        assert {f"{g}-fmt{f}-endo" for f in (0, 2, 4, 5, 6)} <= ids
    assert max(sv.GEOMETRY[c["geometry"]][0] for c in sv.DUMP_CONFIGS if c["endo"]) <= 512


def test_filter_value_takes_rare_keys():
    for g in sv.GEOMETRY:
        nibble, rare = sv.filter_nibble(g)
        print(f"{g}: top four bits {nibble:#x} take {rare} keys of classes a and b")
        assert rare >= 8, (g, nibble, rare)


def test_payloads_are_the_oracle_s():
    """payload() on the public key of a real scalar against the oracle's own payload of that scalar, and the published CREATE vector."""
    from oracle import pyoracle as vo
    for k in (1, 2, 0xDEADBEEF, 2**200 + 12345):
        pub = vo.pubkey(k)
        x, y = int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")
        for fmt in (0, 1, 2, 4, 5):
            assert sv.payload(fmt, x, y) == vo.payload(fmt, k), (k, fmt)
    with open(os.path.join(HERE, "golden", "eth_create.json")) as f:
        g = json.load(f)["key_1"]
    pub = vo.pubkey(1)
    x, y = int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")
    assert sv.payload(5, x, y).hex() == g["account"][2:].lower() and sv.payload(6, x, y).hex() == g["contract"][2:].lower()


# ---- the host build of fe.h on every crafted key ---------------------------------------------------------------------------

def where(weak):
    return "[p, 2^256)" if P <= weak < 1 << 256 else ">= 2^256" if weak >= 1 << 256 else "[0, p)"


EXPECT = {"a": "[p, 2^256)", "b": ">= 2^256"}


@pytest.mark.parametrize("geometry,endo", sv.SETS, ids=SET_IDS)
def test_host_replay_of_the_crafted_keys(core, geometry, endo):
    v = sv.vectors(geometry, endo)
    fired = {}

    def add(a, b):
        return A9(*[x + y for x, y in zip(a, b)])

    def neg1(a):
        r = A9()
        core.core_fe_neg(A9(*a), 1, r)
        return list(r)

    def canon(weak):
        r = A9()
        core.core_fe_canonicalize_product(A9(*weak), r)
        return list(r)

    for c in v.crafted:
        rx, ry, (qx, qy) = v.rx[c.u], v.ry[c.u], v.q[c.j]
        nqx, nqy = limbs_of(P - qx), limbs_of(P - qy)
        dy = add(neg1(limbs_of(ry)) if c.sgn else limbs_of(ry), nqy)
        idx = A9(*limbs_of(pow(rx - qx, -1, P)))
        lam, x3w, y3w = A9(), A9(), A9()
        core.core_fe_mul(dy, idx, lam)
        core.core_fe_mul_add(lam, lam, add(neg1(limbs_of(rx)), nqx), x3w, 1)
        x3 = canon(x3w)
        assert x3 == limbs_of(c.T), (c.u, "x3")
        core.core_fe_mul_add(lam, add(neg1(x3), limbs_of(qx)), A9(*nqy), y3w, 0)
        assert canon(y3w) == limbs_of(c.T2), (c.u, "y3")
        assert core.core_fe_parity_weak(y3w) == c.T2 & 1, (c.u, "parity")
        for name, cls, weak in (("x3", c.cx, val(x3w)), ("y3", c.cy, val(y3w))):
            assert weak % P == (c.T if name == "x3" else c.T2)
            if cls in EXPECT:
                assert where(weak) == EXPECT[cls], (c.u, name, cls, where(weak))
            fired[(name, cls, where(weak))] = fired.get((name, cls, where(weak)), 0) + 1
        if c.cx == "d":   # the images' products: beta x3, then beta (beta x3) from the canonical first image
            xe, beta = x3, A9(*limbs_of(BETA))
            hit = 0
            for e in (1, 2):
                w = A9()
                core.core_fe_mul(A9(*xe), beta, w)
                xe = canon(w)
                t = pow(BETA, e, P) * c.T % P
                assert xe == limbs_of(t), (c.u, "image", e)
                if sv.class_of(t):
                    assert where(val(w)) == EXPECT[sv.class_of(t)], (c.u, e, where(val(w)))
                    hit += 1
            assert hit == 1
            fired[("image", "d", "left [0, p)")] = fired.get(("image", "d", "left [0, p)"), 0) + 1
    print(f"{geometry}{' six images' if endo else ''}: weak products of the crafted keys: "
          + "; ".join(f"{n} {c} {w}: {k}" for (n, c, w), k in sorted(fired.items())))
    # classes c and e never leave [0, p): the superset test of class c fires without need
    assert all(w == "[0, p)" for (n, c, w) in fired if c in "ce")
