"""The onion walk's kernels - onion_points_kernel, onion_fwd_kernel, onion_bwd_kernel in its dump and filter forms, and the compaction
behind the latter (vgen_amd/csrc/device/kernels.hip) - at the edges of workgroups, waves and points.

Every other test reaches these kernels through a context, whose lane count is a multiple of 128 and whose points are consecutive
multiples of 8B.  Here a test-only driver (tests/native/onion_walk_dev.hip -> libonionwalkdev.so, linked against the product's own
build/lib/device/kernels.o) hands vg::launch_onion_points / vg::launch_onion the lane count, the lane table, the shared points and the
zero slot the test chooses:

  L = 1, 2, 63, 64, 65, 511, 512, 513, 577   one lane; a ragged first wave; a full wave; a wave with one live lane; a ragged workgroup; a
                                             workgroup with all eight waves live; a second workgroup with one live lane; a second workgroup
                                             with one full wave and one lane (blockIdx.x = 1, the per-workgroup inversion, scratch and
                                             hit-mask indices at g >= 512)
  lane points                                the walk's own (32 u + 16)(8B), and random points with the neutral element, U_0, -U_31,
                                             (0, p - 1) - U_5 and the points of order 2, 4 and 8 at the first and last lanes of waves and
                                             workgroups - through the prefix products in device scratch and the shared inversion, not one
                                             inversion per pair

Expected values are Python integers (tests/onion_batch_vectors.py: pairs, one pow per batch); every comparison is exact.  Every device
buffer starts poisoned with 1024 poisoned guard words behind it (128 records behind the ring) and comes back whole: the guards are
found intact, what must be written is found written, and what must be left alone is found poisoned."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

from tests import onion_batch_vectors as obv
from tests import onion_vectors as ov
from tests import solana_vectors as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, D, S = ov.P, ov.D, obv.S
LANE_COUNTS = [1, 2, 63, 64, 65, 511, 512, 513, 577]
HIP_ERROR_INVALID_VALUE = 1
HDR_REST = (0x11111111, 0x22222222, 0x33333333)   # cap, clk_cycles, clk_ticks of the header on entry
DEVF_MASKED, DEVF_ALL = 2, 3

u32, vp = ctypes.c_uint32, ctypes.c_void_p


class PointsJob(ctypes.Structure):   # onionwalk_points_job of tests/native/onion_walk_dev.hip, field by field
    _fields_ = [("start", u32 * 8), ("step", u32), ("n", u32), ("mul_d", u32), ("wstride", u32), ("istride", u32),
                ("launch_error", ctypes.c_int32), ("out", vp)]


class Job(ctypes.Structure):         # onionwalk_job
    _fields_ = [("alloc_lanes", u32), ("lanes", u32), ("batch", u32), ("zero_slot", u32), ("filter_form", u32), ("null_pre", u32),
                ("other_payloads", u32), ("match_base", u32), ("match_cap", u32), ("header_in", u32 * 4),
                ("lane", vp), ("uni", vp), ("filter", vp),
                ("launch_error", ctypes.c_int32), ("header_out", u32 * 4),
                ("pre_out", vp), ("inv_out", vp), ("payloads_out", vp), ("hits_out", vp), ("recs_out", vp)]


class FilterTest(ctypes.Structure):  # DevFilterTest (device/device_types.h)
    _fields_ = [("a", u32 * 8), ("b", u32 * 8), ("chk_mask", u32), ("chk_value", u32)]


class Filter(ctypes.Structure):      # DevFilter
    _fields_ = [("kind", u32), ("count", u32), ("flags", u32), ("witver", u32), ("chk_lut", vp), ("chk_base", u32),
                ("dfa_bytes", u32), ("dfa_blob", vp), ("tests", FilterTest * 64)]


@pytest.fixture(scope="module")
def dev():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libonionwalkdev.so"))
    assert lib.onionwalk_job_size() == ctypes.sizeof(Job) and lib.onionwalk_points_job_size() == ctypes.sizeof(PointsJob)
    assert lib.onionwalk_filter_size() == ctypes.sizeof(Filter)
    assert lib.onionwalk_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    for f in (lib.onionwalk_guard_words, lib.onionwalk_guard_records, lib.onionwalk_poison, lib.onionwalk_no_slot):
        f.restype = u32
    assert lib.onionwalk_no_slot() == obv.NO_SLOT and lib.onionwalk_guard_words() >= 1024 and lib.onionwalk_guard_records() * 10 >= 1024
    return lib


def ptr(a):
    return a.ctypes.data_as(vp)


def limbs(v):
    """The canonical limbs of 0 <= v < p: nine of 29 bits (core/fe25519.h)."""
    assert 0 <= v < P
    return [(v >> (29 * k)) & 0x1FFFFFFF for k in range(9)]


def lane_table(R):
    """[27][L]: x, y, t = x y."""
    return np.array([limbs(x) + limbs(y) + limbs(x * y % P) for x, y in R], dtype=np.uint32).T.copy()


def uni_table(U):
    """[32][27]: x, y, e = d x y."""
    return np.array([limbs(x) + limbs(y) + limbs(D * x * y % P) for x, y in U], dtype=np.uint32)


class Out:
    pass


def launch(dev, lane, uni, *, zero_slot=obv.NO_SLOT, filt=None, base=0, entry=0, cap=0, lanes=None, batch=None, null_pre=0, other=0):
    """One onionwalk_run.  Every array comes back split into what the launch owns and the guard words behind it."""
    L = lane.shape[1]
    guard, grecs, poison = dev.onionwalk_guard_words(), dev.onionwalk_guard_records(), dev.onionwalk_poison()
    assert lane.dtype == np.uint32 and lane.flags.c_contiguous and lane.shape == (27, L)
    assert uni.dtype == np.uint32 and uni.flags.c_contiguous and uni.shape == (S, 27)
    sizes = dict(pre=18 * S * L, inv=9 * L, payloads=8 * 2 * S * L, hits=2 * L)
    arrays = {k: np.zeros(n + guard, dtype=np.uint32) for k, n in sizes.items()}
    recs = np.zeros((cap + grecs, 10), dtype=np.uint32)
    j = Job(alloc_lanes=L, lanes=L if lanes is None else lanes, batch=2 * S * L if batch is None else batch, zero_slot=zero_slot,
            filter_form=int(filt is not None), null_pre=null_pre, other_payloads=other, match_base=base, match_cap=cap,
            header_in=(u32 * 4)(entry, *HDR_REST), lane=ptr(lane), uni=ptr(uni),
            pre_out=ptr(arrays["pre"]), inv_out=ptr(arrays["inv"]), payloads_out=ptr(arrays["payloads"]), hits_out=ptr(arrays["hits"]))
    if filt is not None:
        j.filter, j.recs_out = ctypes.addressof(filt), ptr(recs)
    rc = dev.onionwalk_run(ctypes.byref(j))
    assert rc == 0, f"onionwalk_run failed: {rc}"
    o = Out()
    o.err, o.header, o.poison, o.L = j.launch_error, list(j.header_out), poison, L
    guards = []
    for k, n in sizes.items():
        setattr(o, k, arrays[k][:n])
        guards.append(arrays[k][n:])
    o.recs, o.recs_guard = recs[:cap], recs[cap:]
    if filt is not None:
        guards.append(o.recs_guard.ravel())
    o.guards_intact = all(bool((g == poison).all()) for g in guards)
    return o


def dump_payloads(o):
    return [o.payloads[8 * i:8 * i + 8].tobytes() for i in range(2 * S * o.L)]


def assert_dump(o, want):
    assert o.err == 0, o.err
    got = dump_payloads(o)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8], [(i // S - o.L if i >= S * o.L else o.L - 1 - i // S, i % S) for i in bad[:8]])
    assert o.guards_intact, "guard words written"
    # the scratch: every word inside 18 * 32 * L and 9 * L was written (a limb never equals the poison); nothing else exists to write
    assert not (o.pre == o.poison).any() and not (o.inv == o.poison).any()
    assert (o.hits == o.poison).all(), "a dump wrote the hit mask"


# ---- the walk's own tables: lane u = (32 u + 16)(8B), shared points from a random start ---------------------------------------------

@functools.lru_cache(maxsize=None)
def walk_case(L):
    """(lane table, shared table, the 64 L payloads) of a dispatch from a random multiple of 8 of 253 bits."""
    start = random.Random(1000 + L).getrandbits(250) * 8
    U, R = obv.shared_points(start, L), obv.lane_points(L)
    want = obv.batch_payloads(U, R, L)
    # (the staging is the walk: slot i is (start + 8 i) B - three keys from the fixed-base table itself)
    for i in (0, S * L, 2 * S * L - 1):
        assert want[i] == ov.point_bytes(start + 8 * i)
    return lane_table(R), uni_table(U), want


@pytest.mark.parametrize("L", LANE_COUNTS)
def test_dump_of_the_walk_tables(dev, L):
    lane, uni, want = walk_case(L)
    assert_dump(launch(dev, lane, uni), want)


# ---- crafted lane points ----------------------------------------------------------------------------------------------------------------

def crafted_points(U):
    """(name, lane point): the points whose sums and differences with the shared points are the law's edge cases."""
    o2, o4a, o4b, o8 = (0, P - 1), (ov.SQRT_M1, 0), (P - ov.SQRT_M1, 0), ov.order8_point()
    return [("neutral", (0, 1)), ("U_0", U[0]), ("-U_31", ov.neg(U[31])), ("(0, p-1) - U_5", sv.add(o2, ov.neg(U[5]))), ("order 2", o2),
            ("order 4", o4a), ("order 4'", o4b), ("order 8", o8)]


@pytest.mark.parametrize("L", [65, 513])
def test_dump_of_crafted_lane_tables(dev, L):
    """Random curve points, and at the first and last lanes of waves and workgroups the eight crafted points, in eight rotations: every
    crafted point stands once at every such lane."""
    rng = random.Random(2000 + L)
    U = [ov.point_of(rng.getrandbits(255)) for _ in range(S)]
    R = [ov.point_of(rng.getrandbits(255)) for _ in range(L)]
    crafted = crafted_points(U)
    assert all(ov.on_curve(q) for _, q in crafted) and len({q for _, q in crafted}) == 8
    where = sorted({0, 63, 64, L - 1} | ({511, 512} if L == 513 else set()))
    assert max(where) < L
    uni = uni_table(U)
    base_rows = obv.pairs(U, R)
    crafted_rows = obv.pairs(U, [q for _, q in crafted])
    # what the crafted points are there for, on the reference: (xs, ys, xd, yd) of U_j +- R
    assert crafted_rows[0] == [(x, y, x, y) for x, y in U]                       # the neutral element: both are U_j
    assert crafted_rows[1][0][2:] == (0, 1) and crafted_rows[1][0][:2] == ov.pair(U[0], U[0])[:2]   # U_0 - U_0; U_0 doubled
    assert crafted_rows[2][31][:2] == (0, 1)                                     # U_31 + (-U_31)
    assert crafted_rows[3][5][:2] == (0, P - 1)                                  # y = p - 1
    assert crafted_rows[4] == [(P - x, P - y, P - x, P - y) for x, y in U]       # order 2: -x, -y
    assert all(ov.on_curve(r[:2]) and ov.on_curve(r[2:]) for row in crafted_rows for r in row)
    assert all(r[0] == (y * ov.SQRT_M1) % P and r[1] == (x * ov.SQRT_M1) % P for r, (x, y) in zip(crafted_rows[5], U))   # order 4: (x, y) -> (i y, i x)
    for rot in range(8):
        rows, table = list(base_rows), list(R)
        for i, u in enumerate(where):
            k = (i + rot) % 8
            rows[u], table[u] = crafted_rows[k], crafted[k][1]
        assert_dump(launch(dev, lane_table(table), uni), obv.place(rows, L))


def test_dump_with_a_sum_of_y_zero(dev):
    """Shared points that are themselves of small order (U_0 of order 8, U_1 and U_2 of order 4, U_3 of order 2, U_4 neutral) against the
    crafted lane points at L = 65: sums and differences with y = 0, y = p - 1, x = 0 - the whole 8-torsion group among the keys."""
    L = 65
    rng = random.Random(2100)
    o8 = ov.order8_point()
    U = [o8, (ov.SQRT_M1, 0), (P - ov.SQRT_M1, 0), (0, P - 1), (0, 1)] + [ov.point_of(rng.getrandbits(255)) for _ in range(S - 5)]
    R = [ov.point_of(rng.getrandbits(255)) for _ in range(L)]
    for u, (_, q) in zip((0, 1, 2, 3, 61, 62, 63, 64), crafted_points(U)):
        R[u] = q
    rows = obv.pairs(U, R)
    assert rows[1][0][1] == 0 and rows[1][0][2:] == (0, 1)                       # order 8 doubled: order 4, y = 0
    assert (0, P - 1) in {r[:2] for r in rows[62]} | {r[2:] for r in rows[62]}   # order 4 + order 4 = order 2
    assert_dump(launch(dev, lane_table(R), uni_table(U)), obv.place(rows, L))


# ---- zero_slot ----------------------------------------------------------------------------------------------------------------------------

def all_filter():
    return Filter(kind=DEVF_ALL, count=0)


def prefix_filter(prefix):
    mask, val = ov.prefix_mask(prefix)
    f = Filter(kind=DEVF_MASKED, count=1)
    for k in range(8):
        f.tests[0].a[k] = (mask >> (32 * (7 - k))) & 0xFFFFFFFF
        f.tests[0].b[k] = (val >> (32 * (7 - k))) & 0xFFFFFFFF
    return f


def records(o, n):
    assert (o.recs[:n, 1] == 0).all()
    return [(int(r[0]), r[2:].tobytes()) for r in o.recs[:n]]


def mask_of(hits, L):
    m = np.zeros(2 * L, dtype=np.uint32)
    for s in hits:
        m[s >> 5] |= np.uint32(1 << (s & 31))
    return m


@pytest.mark.parametrize("slot", [0, 31, 32, 32 * 65, 64 * 65 - 1, obv.NO_SLOT], ids=["0", "31", "32", "32L", "64L-1", "none"])
def test_zero_slot(dev, slot):
    L = 65
    lane, uni, want = walk_case(L)
    assert all(any(p) for p in want)
    n = 2 * S * L
    o = launch(dev, lane, uni, zero_slot=slot)
    expect = [bytes(32) if i == slot else p for i, p in enumerate(want)]
    assert_dump(o, expect)
    assert [i for i, p in enumerate(dump_payloads(o)) if not any(p)] == ([] if slot == obv.NO_SLOT else [slot])
    # match-all: exactly that slot is missing from the records, the mask and the count
    hits = [i for i in range(n) if i != slot]
    o = launch(dev, lane, uni, zero_slot=slot, filt=all_filter(), cap=n)
    assert o.err == 0 and o.guards_intact
    assert o.header == [len(hits), *HDR_REST]
    assert records(o, len(hits)) == [(i, want[i]) for i in hits]
    assert (o.recs[len(hits):] == o.poison).all()
    assert (o.hits == mask_of(hits, L)).all()


# ---- the filter form ----------------------------------------------------------------------------------------------------------------------

def reference_hits(want, prefix):
    mask, val = ov.prefix_mask(prefix)
    return [i for i, p in enumerate(want) if int.from_bytes(p, "big") & mask == val]


def check_filtered(o, want, hits, *, entry, base, cap):
    """The records of `hits` follow the ring's count on entry (record k at entry - base + k, dropped at or past cap), the header counts
    them all, the mask is the reference's, the guards are intact."""
    L = o.L
    assert o.err == 0, o.err
    assert o.guards_intact, "guard words written"
    assert o.header == [(entry + len(hits)) % 2**32, *HDR_REST]
    assert not (o.hits == o.poison).any(), "hit-mask words left unwritten"
    assert (o.hits == mask_of(hits, L)).all(), np.flatnonzero(o.hits != mask_of(hits, L))[:8]
    first = (entry - base) % 2**32
    written = max(0, min(cap - first, len(hits)))
    assert (o.recs[:first] == o.poison).all()
    got = o.recs[first:first + written]
    assert (got[:, 1] == 0).all()
    assert [(int(r[0]), r[2:].tobytes()) for r in got] == [(i, want[i]) for i in hits[:written]]
    assert (o.recs[first + written:] == o.poison).all(), "records beyond the hits or the cap written"
    assert not (o.pre == o.poison).any() and not (o.inv == o.poison).any()


@pytest.mark.parametrize("L", [1, 65, 512, 577])
def test_filter_form(dev, L):
    lane, uni, want = walk_case(L)
    n = 2 * S * L
    key = want[(2 * L - 1) * S + 7]                       # U_7 + R_(L-1): a key of the last lane
    assert want.index(key) // S == 2 * L - 1
    string = ov.address(key)
    # one character: about n / 32 hits; the count on entry wraps during the dispatch, match_base follows it
    one = reference_hits(want, string[:1])
    assert want.index(key) in one and len(one) == sum(1 for p in want if ov.address(p).startswith(string[:1]))
    if L >= 65:
        assert {want[i][31] >> 7 for i in one} == {0, 1}                                 # both signs among the hits' full payloads
        assert min(one) < S * L <= max(one)                                              # hits on the - and the + side
    entry = 2**32 - (len(one) + 1) // 2
    o = launch(dev, lane, uni, filt=prefix_filter(string[:1]), entry=entry, base=entry, cap=len(one) + 8)
    check_filtered(o, want, one, entry=entry, base=entry, cap=len(one) + 8)
    # three characters; three records of an earlier dispatch are in the ring
    three = reference_hits(want, string[:3])
    assert want.index(key) in three and len(three) <= len(one)
    o = launch(dev, lane, uni, filt=prefix_filter(string[:3]), entry=12348, base=12345, cap=len(three) + 8)
    check_filtered(o, want, three, entry=12348, base=12345, cap=len(three) + 8)
    # match-all, whole ...
    o = launch(dev, lane, uni, filt=all_filter(), cap=n)
    check_filtered(o, want, list(range(n)), entry=0, base=0, cap=n)
    # ... and with a ring smaller than the hits: exactly match_cap records, the count says the total
    for cap in (16, n - 1):
        o = launch(dev, lane, uni, filt=all_filter(), entry=5, base=5, cap=cap)
        check_filtered(o, want, list(range(n)), entry=5, base=5, cap=cap)
        assert (o.recs != o.poison).any(axis=1).sum() == cap


# ---- onion_points_kernel ------------------------------------------------------------------------------------------------------------------

RIPPLE_START = (0x5EEDBEEF << 224) | (2**224 - 1)          # the low seven words are 0xFFFFFFFF: adding i * step ripples to the top word


@functools.lru_cache(maxsize=None)
def point_of(k):
    return ov.point_of(k)


def points_starts(n):
    return [("runtime", 8 * 16, 8 * 32), ("start-0", 0, 8 * 32), ("ripple", RIPPLE_START, 8 * 32), ("range-end", 2**255 - 8 * 32 * n, 8 * 32)]


@pytest.mark.parametrize("n", [1, 32, 63, 64, 65, 130])
def test_onion_points(dev, n):
    guard, poison = dev.onionwalk_guard_words(), dev.onionwalk_poison()
    for name, start, step in points_starts(n):
        pts = [point_of(start + i * step) for i in range(n)]
        if name == "ripple" and n > 1:
            assert (start + step) >> 224 == (start >> 224) + 1
        for mul_d in (0, 1):
            want = np.array([limbs(x) + limbs(y) + limbs(x * y * (D if mul_d else 1) % P) for x, y in pts], dtype=np.uint32)   # [n][27]
            for wstride, istride in ((n, 1), (1, 27)):
                out = np.zeros(27 * n + guard, dtype=np.uint32)
                j = PointsJob(start=(u32 * 8)(*[(start >> (32 * k)) & 0xFFFFFFFF for k in range(8)]), step=step, n=n, mul_d=mul_d,
                              wstride=wstride, istride=istride, out=ptr(out))
                rc = dev.onionwalk_points(ctypes.byref(j))
                assert rc == 0 and j.launch_error == 0, (rc, j.launch_error)
                got = out[:27 * n].reshape(27, n).T if istride == 1 else out[:27 * n].reshape(n, 27)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, (name, mul_d, wstride, istride, bad[:8])
                assert (out[27 * n:] == poison).all(), "guard words written"


# ---- launches launch_onion refuses --------------------------------------------------------------------------------------------------------

def untouched(o):
    return o.err == HIP_ERROR_INVALID_VALUE and o.guards_intact and all(bool((a == o.poison).all()) for a in (o.pre, o.inv, o.payloads, o.hits)) \
        and bool((o.recs == o.poison).all())


def test_refused_launches_run_nothing(dev):
    L = 65
    lane, uni, want = walk_case(L)
    n = 2 * S * L
    for kw in (dict(lanes=0), dict(lanes=0, batch=0), dict(batch=n - 64), dict(batch=n + 64), dict(lanes=L - 1), dict(null_pre=1)):
        assert untouched(launch(dev, lane, uni, **kw)), kw
        o = launch(dev, lane, uni, filt=all_filter(), cap=64, **kw)
        assert untouched(o) and o.header == [0, *HDR_REST], kw
    o = launch(dev, lane, uni, filt=all_filter(), cap=64, other=1)       # the compaction would read another payload buffer
    assert untouched(o) and o.header == [0, *HDR_REST]
    # the same arguments with the fault taken out do run (the poison would otherwise prove nothing)
    assert_dump(launch(dev, lane, uni), want)
