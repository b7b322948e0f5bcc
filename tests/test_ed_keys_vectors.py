"""tests/ed_keys_vectors.py - the expected side of tests/test_gpu_ed_keys_kernel.py - held against something other than itself, on
the CPU: the host build of the functions ed_keys_kernel inlines, run on the same crafted tables and seeds (tests/native/ed_keys_shim.cpp
-> libedkeystest.so: ed_mul_base on a caller's table, one fe25_inv, two fe25_mul, ed_encode).

  (a) with the real table the vectors' point_of is the RFC 8032 public key of tests/solana_vectors.py, and the vectors' table is the
      product's, word for word;
  (b) on every crafted table and every seed the GPU tests use, the host build's 32 bytes are the Python bytes;
  (c) for every crafted lane the host build's Z is not zero - core/ed25519.h's "the formula is COMPLETE ... Z is never 0", on which
      the kernel's shared product rests, asked of doublings, cancellations and torsion for the first time;
  (d) the classes and the edge placements the GPU tests promise are there, so the reference alone meets the presence conditions
      before a GPU is involved."""
import ctypes
import os

import numpy as np
import pytest

from conftest import locked_make
from tests import ed_keys_vectors as ev
from tests import solana_vectors as sv

HERE = os.path.dirname(os.path.abspath(__file__))
P = ev.P


@pytest.fixture(scope="module")
def shim():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "-f", "ed_keys.mk", "libedkeystest.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libedkeystest.so"))
    lib.edkshim_table_words.restype = ctypes.c_uint32
    lib.edkshim_keys.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
    lib.edkshim_real_table.argtypes = [ctypes.c_void_p]
    assert lib.edkshim_table_words() == ev.TABLE_WORDS
    return lib


def host_keys(shim, table, seeds):
    """(the 32 bytes of every seed, the Z-not-zero flags) of the host build over `table` (None: the product's)."""
    n = len(seeds)
    out, flags = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n)
    shim.edkshim_keys(None if table is None else table.ctypes.data_as(ctypes.c_void_p), b"".join(seeds), n, out, flags)
    return [out.raw[32 * i:32 * i + 32] for i in range(n)], list(flags.raw)


def test_fixed_points_are_what_their_names_say():
    q = dict(ev.fixed_points())
    assert len(set(q.values())) == len(ev.Q_NAMES) == 11 and all(ev.on_curve(p) for p in q.values())
    assert [ev.small_order(p) for p in ev.Q()] == [1, 2, 4, 4, 8] + [None] * 6
    assert sv.encode_point(*q["order 4, even x"]) == bytes(32) and sv.encode_point(*q["order 4, odd x"]) == bytes(31) + b"\x80"
    assert ev.add(q["order 8"], q["order 8"]) in (q["order 4, even x"], q["order 4, odd x"])
    x, y = q["small y"]
    assert y >= 2 and all(ev.xs_of_y(v) is None for v in range(2, y)) and y < 64
    assert {q["small y, -x"], q["y below p"], q["y below p, -x"]} == {(P - x, y), (x, P - y), (P - x, P - y)}
    assert {p[0] & 1 for p in (q["small y"], q["small y, -x"])} == {0, 1}
    assert ev.mul(sv.L, q["B"]) == ev.NEUTRAL and ev.small_order(ev.mul(sv.L, q["B + order 8"])) == 8
    # an entry is y + x, y - x, 2 d x y in nine 29-bit limbs and a pad word; the neutral element's is (1, 1, 0)
    assert ev.entry(0, 1) == [1] + [0] * 8 + [1] + [0] * 8 + [0] * 9 + [0]
    e = ev.entry(x, y)
    val = lambda l: sum(v << (29 * k) for k, v in enumerate(l))
    assert len(e) == 28 and max(e) < 2**29 and e[27] == 0
    assert (val(e[:9]), val(e[9:18]), val(e[18:27])) == ((y + x) % P, (y - x) % P, 2 * ev.D * x * y % P)


def test_real_table_is_the_products_and_point_of_is_the_public_key(shim):
    """(a)"""
    mine = np.array(ev.table_words("real"), dtype=np.uint32)
    theirs = np.zeros(ev.TABLE_WORDS, dtype=np.uint32)
    shim.edkshim_real_table(theirs.ctypes.data_as(ctypes.c_void_p))
    assert (mine == theirs).all(), np.flatnonzero(mine != theirs)[:8]
    seeds, keys = ev.real_seeds(), ev.real_payloads()
    assert len(seeds) == ev.REAL_LANES == 1025
    for i in list(range(0, ev.REAL_LANES, 16)) + [ev.REAL_LANES - 1]:
        assert keys[i] == sv.public_key(seeds[i]), i
    assert ev.zero_seed_payload() == sv.public_key(bytes(32))
    got, nonzero = host_keys(shim, None, list(seeds) + [bytes(32)])
    assert got == list(keys) + [ev.zero_seed_payload()] and all(nonzero)
    got, _ = host_keys(shim, mine, list(seeds[:64]))
    assert got == list(keys[:64])


@pytest.mark.parametrize("name", ev.TABLES)
def test_host_build_equals_the_vectors_on_crafted_tables(shim, name):
    """(b), (c), (d): every seed of every rotation, the never-read ones behind N and the all-zero seed of the keyless lanes included."""
    table = np.array(ev.table_words(name), dtype=np.uint32)
    pts = ev.table_points(name)
    assert all(ev.on_curve(q) for row in pts for q in set(row))
    uncrafted = [w for w in range(32) if pts[w] is ev.NEUTRAL_ROW]
    assert len(uncrafted) == {"two-window": 30, "real-but-one": 0}.get(name, 31)
    for w in uncrafted:
        assert (table[w * 256 * 28:(w + 1) * 256 * 28].reshape(256, 28) == np.array(ev.entry(0, 1), dtype=np.uint32)).all()
    for rot in ev.rotations(name):
        seeds = list(ev.crafted_seeds(name, rot)) + [bytes(32)]
        want = [ev.payload(pts, s) for s in seeds]
        assert tuple(want[i] if i < ev.N else bytes(32) for i in range(ev.BATCH)) == ev.crafted_payloads(name, rot)
        got, nonzero = host_keys(shim, table, seeds)
        bad = [i for i in range(len(seeds)) if got[i] != want[i]]
        assert not bad, (len(bad), bad[:8], sorted(ev.lane_classes(name, seeds[bad[0]])))
        assert all(nonzero), [i for i, f in enumerate(nonzero) if not f][:8]
        # (d) every class is present among the keyed lanes, and the named lanes hold theirs
        lanes = ev.crafted_class_lanes(name, rot)
        missing = [c for c in ev.required_classes(name) if not lanes.get(c)]
        assert not missing, missing
        for lane in ev.NAMED:
            assert lane < ev.N and lane in lanes[ev.named_class(name, rot, lane)], (lane, rot)
    # doubling, cancelling and the zero payload on each side of the wave edge 63 | 64 and of the workgroup edge 511 | 512
    if name == "two-window":
        for c in ev.TWO_NAMED:
            for lane in (63, 64, 511, 512):
                assert any(ev.named_class(name, rot, lane) == c for rot in ev.rotations(name)), (c, lane)
    elif name != "real-but-one":
        assert all(lane in ev.crafted_class_lanes(name)["zero payload"] for lane in (63, 64, 511, 512))
        w = ev.crafted_window(name)
        used = {ev.digits(s)[w] for s in ev.crafted_seeds(name)[:ev.N]}
        assert used <= set(range(64, 128)) if w == 31 else len(used) > 200     # clamping leaves window 31 the digits 64 .. 127


def test_two_window_classes_are_what_the_kernel_adds():
    """A doubling lane's two entries are one point, a cancelling lane's a point and its negative; the sum is what the law says."""
    c1, c2 = ev.two_window_rows()
    seeds, lanes = ev.crafted_seeds("two-window"), ev.crafted_class_lanes("two-window")
    for i in lanes["doubling"]:
        d = ev.digits(seeds[i])
        p = c1[d[ev.TWO_W1]]
        assert p == c2[d[ev.TWO_W2]] != ev.NEUTRAL and ev.point_of(ev.table_points("two-window"), seeds[i]) == ev.add(p, p)
    for i in lanes["cancelling"]:
        d = ev.digits(seeds[i])
        assert ev.add(c1[d[ev.TWO_W1]], c2[d[ev.TWO_W2]]) == ev.NEUTRAL != c1[d[ev.TWO_W1]]
        assert ev.crafted_payloads("two-window")[i] == sv.encode_point(0, 1)
    assert {ev.small_order(c1[ev.digits(seeds[i])[ev.TWO_W1]]) for i in lanes["doubling"]} >= {2, 4, 8, None}
    assert all(ev.crafted_payloads("two-window")[i] == bytes(32) for i in lanes["zero payload"])


def test_filter_cases_decide_something():
    """The presence conditions of the filter tests: keyed hits, keyed non-hits, and a keyless lane whose key would match."""
    keys = ev.real_payloads()
    zero = ev.zero_seed_payload()
    for length in (1, 2):
        prefix = ev.uploaded_prefix(length)
        assert sv.address(keys[0]).startswith(prefix) and sv.address(zero).startswith(prefix)
        assert ev.prefix_hits([zero], prefix) == [0]                               # what `has_key` alone keeps out
        for n in (65, 513, 1025):
            hits = ev.prefix_hits(keys[:n], prefix)
            assert hits == [i for i in range(n) if sv.address(keys[i]).startswith(prefix)]   # the ranges are exact for a literal
            assert 0 in hits and 0 < len(hits) < n
    assert all(any(k) for k in keys) and any(zero)
    # the kernel zeroes a keyless lane's payload BEFORE the filter, so what `has_key` keeps out of the ballot is the all-zero payload:
    # address '1' x 32.  Lane 1's address starts with one '1' and no keyed lane's with two.
    assert sv.address(bytes(32)) == "1" * 32 and ev.prefix_hits([bytes(32)], "1") == ev.prefix_hits([bytes(32)], "11") == [0]
    assert sv.address(keys[1]).startswith("1") and not sv.address(keys[1]).startswith("11")
    for n in (65, 513, 1025):
        assert 1 in ev.prefix_hits(keys[:n], "1") and len(ev.prefix_hits(keys[:n], "1")) < n and ev.prefix_hits(keys[:n], "11") == []
    batch, n = ev.STREAM_FILTER_SHAPE
    for length in (1, 2):
        first, prefix = ev.stream_prefix(length)
        draws = ev.stream_keys(first, batch)
        hits = ev.prefix_hits(draws, prefix)
        assert hits == [i for i in range(batch) if sv.address(draws[i]).startswith(prefix)]
        assert 0 < len([i for i in hits if i < n]) < n and [i for i in hits if i >= n]
    assert ev.stream_keys(0, 512)[:4] == tuple(sv.public_key(sv.stream_seed(ev.STREAM_SEED, ev.STREAM, i)) for i in range(4))
    assert ev.seed_words() == list(np.frombuffer(sv.seed24(ev.STREAM_SEED), dtype="<u4"))
