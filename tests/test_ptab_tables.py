"""The synthetic interval tables of the list-kernel harness (tests/test_gpu_list_kernels.py), checked on the CPU.

A table builder and a lookup model, written here in numpy from the documented layout of DevPtab
(vgen_amd/csrc/device/device_types.h) and from nothing else of the product, against ptab_find (core/ptab_eval.h) as g++
compiles it (tests/native/core_shim.cpp: core_ptab_find).  The geometries are the awkward ones: a value exactly at lo, at hi
and at hi + 1, intervals that start inside the previous bucket, a bucket holding dozens of intervals, lo == hi, a first value
of 0, a last value of 2^64 - 1, empty first and last buckets.  tests/test_pattern_list.py only sees tables the product's own
compiler builds; the GPU module hands the same tables to ptab_lookup_kernel, so they have to be well-formed first."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = (1 << 64) - 1


class Table:
    """bits, n, bitmap (uint32, 2^bits bits), offsets (uint32, 2^bits + 1), lo, hi (uint64, n)."""

    def __init__(self, intervals, bits):
        iv = sorted(intervals)
        assert all(0 <= a <= b <= U64 for a, b in iv)
        assert all(iv[j][1] < iv[j + 1][0] for j in range(len(iv) - 1)), "intervals must be disjoint"
        self.bits, self.n, self.intervals = bits, len(iv), iv
        self.lo = np.array([a for a, _ in iv], dtype=np.uint64)
        self.hi = np.array([b for _, b in iv], dtype=np.uint64)
        nb, sh = 1 << bits, np.uint64(64 - bits)
        # offsets[b]: the number of intervals with hi below the first value of bucket b; offsets[2^bits] = n
        first = np.arange(nb, dtype=np.uint64) << sh
        self.offsets = np.empty(nb + 1, dtype=np.uint32)
        self.offsets[:nb] = np.searchsorted(self.hi, first, side="left")
        self.offsets[nb] = self.n
        # bitmap bit b: some interval meets bucket b, i.e. b lies in [lo_j >> sh, hi_j >> sh] for some j
        d = np.zeros(nb + 1, dtype=np.int64)
        np.add.at(d, (self.lo >> sh).astype(np.int64), 1)
        np.add.at(d, (self.hi >> sh).astype(np.int64) + 1, -1)
        self.met = np.cumsum(d[:nb]) > 0
        packed = np.packbits(self.met, bitorder="little")
        self.bitmap = np.concatenate([packed, np.zeros(-packed.size % 4, dtype=np.uint8)]).view("<u4").copy()
        assert self.bitmap.size == max(1, nb // 32)

    def find(self, x):
        """The lookup model: index of the interval that holds each x (uint64 array), or -1."""
        x = np.asarray(x, dtype=np.uint64)
        if self.n == 0:
            return np.full(x.shape, -1, dtype=np.int64)
        j = np.searchsorted(self.lo, x, side="right").astype(np.int64) - 1
        ok = (j >= 0) & (x <= self.hi[np.maximum(j, 0)])
        return np.where(ok, j, -1)


def mixed_intervals(bits, seed):
    """Single values, adjacent intervals, one spanning several buckets, a bucket where one ends and another begins, intervals
    that start in the bucket before, a bucket of 80 intervals, the first at 0, the last ending at 2^64 - 1."""
    W, nb = 1 << (64 - bits), 1 << bits
    iv = [(0, 5), (7, 7), (8, 8), (9, 20)]                        # from 0; lo == hi; hi + 1 == the next lo
    iv += [(3 * W + W // 2, 6 * W + 10)]                          # meets buckets 3 .. 6
    iv += [(6 * W + 12, 6 * W + 12), (7 * W - 1, 7 * W + 3)]      # bucket 6: one ends, two begin, the last on its last value
    iv += [(7 * W + 4, 7 * W + 4), (7 * W + 6, 7 * W + W // 3)]   # bucket 7: behind an interval that started in bucket 6
    base = 100 * W + 1000                                         # bucket 100: 80 intervals, every third touching the next
    for k in range(80):
        iv.append((base + 10 * k, base + 10 * k + (0, 3, 9)[k % 3]))
    iv += [(200 * W + 5, 201 * W - 1), (201 * W, 201 * W)]        # ends on a bucket's last value, the next on the next's first
    iv += [(210 * W - 2, 210 * W - 2), (210 * W - 1, 210 * W), (210 * W + 1, 210 * W + 1)]   # three in a row over a boundary
    rng = random.Random(seed)
    for b in rng.sample(range(300, nb - 300), 100):               # 1 .. 3 intervals inside each of 100 random buckets
        cuts = sorted(rng.sample(range(W // 8, W - W // 8), 6))
        for k in range(rng.randint(1, 3)):
            iv.append((b * W + cuts[2 * k], b * W + (cuts[2 * k] if rng.random() < 0.3 else cuts[2 * k + 1] - 1)))
    iv += [((nb - 2) * W + 9, (nb - 2) * W + 9), ((nb - 1) * W - 3, (nb - 1) * W + 2)]   # the last bucket's first starts before it
    iv += [(U64 - 1002, U64 - 1002), (U64 - 1000, U64)]           # up to 2^64 - 1
    return iv


def sparse_intervals(bits, seed):
    """Empty first and last buckets: the first interval starts on bucket 1's first value, the last ends on bucket 2^bits - 2's
    last value."""
    W, nb = 1 << (64 - bits), 1 << bits
    iv = [(W, W + 3), (W + 4, W + 4), ((nb - 1) * W - 10, (nb - 1) * W - 1)]
    rng = random.Random(seed)
    for b in rng.sample(range(2, nb - 2), 40):
        a = rng.randrange(0, W - 1)
        iv.append((b * W + a, b * W + rng.randrange(a, W)))
    return iv


def probes(t, n_random, seed):
    """Every lo, hi, lo - 1 and hi + 1 that exists, the first and last value of the buckets involved and of their neighbours,
    random values inside those buckets, random 64-bit values: uint64 array without duplicates."""
    W, nb = 1 << (64 - t.bits), 1 << t.bits
    rng = random.Random(seed)
    xs = set()
    buckets = set()
    for a, b in t.intervals:
        xs.update(v for v in (a, b, a - 1, b + 1) if 0 <= v <= U64)
        for e in (a // W, b // W):
            buckets.update(k for k in (e - 1, e, e + 1) if 0 <= k < nb)
    buckets.update((0, nb - 1))
    for k in buckets:
        xs.update((k * W, k * W + W - 1, k * W + rng.randrange(W)))
    xs.update((0, U64))
    while n_random > 0:
        v = rng.getrandbits(64)
        if v not in xs:
            xs.add(v)
            n_random -= 1
    return np.array(sorted(xs), dtype=np.uint64)


def brute_find(t, x):
    """The definition itself, in Python integers."""
    for j, (a, b) in enumerate(t.intervals):
        if a <= x <= b:
            return j
    return -1


GEOMETRIES = {"mixed": mixed_intervals, "sparse": sparse_intervals}


@pytest.fixture(scope="module")
def core():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "libcoretest.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libcoretest.so"))
    lib.core_ptab_find.restype = None
    return lib


def host_find(core, t, x):
    out = np.empty(x.size, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    core.core_ptab_find(ctypes.c_uint32(t.bits), ctypes.c_uint32(t.n), p(t.bitmap), p(t.offsets), p(t.lo), p(t.hi), p(x),
                        ctypes.c_int(x.size), p(out))
    return out.astype(np.int64)


def test_builder_follows_the_documented_layout():
    """The builder against the words of device_types.h, bucket by bucket in Python integers (a table small enough for that)."""
    bits = 6
    W, nb = 1 << (64 - bits), 1 << bits
    iv = [(0, 0), (W - 1, W), (W + 5, 3 * W + 1), (3 * W + 2, 3 * W + 2), (40 * W + 7, 40 * W + 9), (63 * W + 1, U64)]
    t = Table(iv, bits)
    for b in range(nb):
        first, last = b * W, b * W + W - 1
        met = any(a <= last and h >= first for a, h in iv)
        assert bool((int(t.bitmap[b >> 5]) >> (b & 31)) & 1) == met, b
        assert t.offsets[b] == sum(1 for _, h in iv if h < first), b
    assert t.offsets[nb] == len(iv) and t.offsets.size == nb + 1
    assert [b for b in range(nb) if t.met[b]] == [0, 1, 2, 3, 40, 63]


@pytest.mark.parametrize("bits", [16, 20])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_tables_are_well_formed_for_ptab_find(core, geometry, bits):
    t = Table(GEOMETRIES[geometry](bits, seed=bits), bits)
    x = probes(t, 3000, seed=7 * bits)
    want = t.find(x)
    n_hit, n_miss = int((want >= 0).sum()), int((want < 0).sum())
    print(f"{geometry} bits={bits}: {t.n} intervals, {x.size} probes, {n_hit} hits, {n_miss} misses")
    assert x.size >= 3500 and n_hit >= t.n and n_miss >= 3000
    assert set(want[want >= 0].tolist()) == set(range(t.n)), "every interval is probed"
    # the numpy model is the definition (checked in Python integers on every edge probe and a sample of the rest) ...
    edge = set()
    for a, b in t.intervals:
        edge.update((a, b, max(a - 1, 0), min(b + 1, U64)))
    rng = random.Random(1)
    for i in range(x.size):
        if int(x[i]) in edge or rng.random() < 0.05:
            assert want[i] == brute_find(t, int(x[i])), hex(int(x[i]))
    # ... and ptab_find over the built table agrees with it everywhere
    got = host_find(core, t, x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(x[i])), int(got[i]), int(want[i])) for i in bad[:5]]


def test_geometry_has_what_it_says():
    for bits in (16, 20, 24):
        W, nb = 1 << (64 - bits), 1 << bits
        t = Table(mixed_intervals(bits, seed=bits), bits)
        iv = t.intervals
        per_bucket = {}
        for a, b in iv:
            per_bucket[a // W] = per_bucket.get(a // W, 0) + 1
        assert max(per_bucket.values()) >= 64                                        # a crowded bucket
        assert iv[0][0] == 0 and iv[-1][1] == U64                                    # both ends of the value range
        assert sum(1 for a, b in iv if a == b) >= 30                                 # lo == hi
        assert sum(1 for j in range(t.n - 1) if iv[j][1] + 1 == iv[j + 1][0]) >= 25  # adjacent
        assert any(b // W - a // W >= 3 for a, b in iv)                              # spans buckets
        starts_before = [j for j, (a, b) in enumerate(iv) if a // W < b // W]        # starts inside the previous bucket ...
        assert len(starts_before) >= 4
        assert any(j + 1 < t.n and iv[j + 1][0] // W == iv[j][1] // W for j in starts_before)   # ... with more behind it there
        assert any(iv[j][1] // W == iv[j + 1][0] // W and iv[j][0] // W < iv[j][1] // W for j in range(t.n - 1))
        s = Table(sparse_intervals(bits, seed=bits), bits)
        assert not s.met[0] and not s.met[nb - 1] and s.met[1] and s.met[nb - 2]
        assert s.offsets[0] == s.offsets[1] == 0 and s.offsets[nb - 1] == s.offsets[nb] == s.n
