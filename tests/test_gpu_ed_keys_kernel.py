"""ed_keys_kernel (format 12, Solana) in its dump and filter forms and the compaction behind the latter
(vgen_amd/csrc/device/kernels.hip), on crafted tables and at the edges of the counts.

Every other test reaches this kernel through a context: sixteen full workgroups with n == batch, one dump with n = 65, the real table.
Here a test-only driver (tests/native/ed_keys_dev.hip -> libedkeysdev.so, linked against the product's own
build/lib/device/kernels.o) hands vg::launch_ed_keys what the test chooses:

  (batch, n)      512, 1024 and 1536 lanes with n = 1, 2, 63, 64, 65, 511, 512, 513, 577, 1023, 1025: one workgroup - the shared
                  inversion's second butterfly with seven keyless wave totals -, a keyless wave inside a keyed workgroup, a ragged
                  tail, a second and a third workgroup with one keyed lane
  the table       EdArgs::table is a plain pointer, and a lane's 32 digits are known from its seed.  Crafted tables
                  (tests/ed_keys_vectors.py) make the kernel's one addition, ed_madd, double a point, add a point to its negative
                  and add points of order 2, 4 and 8 - what core/ed25519.h's "the formula is COMPLETE ... Z is never 0" promises and
                  the real table can never ask - and put y = 0, x = 0, y next to 0 and to p and both signs through the shared
                  inversion into ed_encode
  the filter form n < batch: a keyless lane hashes a perfectly good all-zero seed (or draws a key), its payload is zeroed, and
                  `has_key` alone keeps it out of the ballot for every pattern a zero payload satisfies; the hit-mask words of
                  keyless waves are stored as 0; payload slots of lanes that did not hit stay untouched

Expected values are Python integers, held against the host build of the same functions in tests/test_ed_keys_vectors.py; every
comparison is exact bytes and no slot is left out.  Every device buffer starts poisoned with 1024 poisoned guard words behind it (128
records behind the ring) and comes back whole: the guards are found intact, what must be written is found written, and what must be
left alone is found poisoned."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import locked_make
from tests import ed_keys_vectors as ev
from tests import solana_vectors as sv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_ERROR_INVALID_VALUE = 1
HDR_REST = (0x11111111, 0x22222222, 0x33333333)   # cap, clk_cycles, clk_ticks of the header on entry
DEVF_RANGES, DEVF_ALL = 1, 3
SWITCHES = ("null_table", "null_payloads", "null_hits", "null_filter", "other_payloads", "other_hits", "other_stride", "other_images",
            "null_mhdr", "null_mrec")

u32, vp = ctypes.c_uint32, ctypes.c_void_p


class Job(ctypes.Structure):         # edkeys_job of tests/native/ed_keys_dev.hip, field by field
    _fields_ = [("alloc_batch", u32), ("batch", u32), ("n", u32), ("filter_form", u32), ("ci", u32)] + [(s, u32) for s in SWITCHES] + \
               [("match_base", u32), ("match_cap", u32), ("header_in", u32 * 4), ("seed", u32 * 6), ("stream", u32),
                ("first", ctypes.c_uint64), ("table", vp), ("seeds", vp), ("pattern", ctypes.c_char_p),
                ("launch_error", ctypes.c_int32), ("sync_error", ctypes.c_int32), ("filter_kind", u32), ("header_out", u32 * 4),
                ("payloads_out", vp), ("hits_out", vp), ("recs_out", vp), ("table_guard_out", vp), ("seeds_guard_out", vp)]


@pytest.fixture(scope="module")
def dev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "-f", "ed_keys.mk", "libedkeysdev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libedkeysdev.so"))
    assert lib.edkeys_job_size() == ctypes.sizeof(Job)
    assert lib.edkeys_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    for f in (lib.edkeys_guard_words, lib.edkeys_guard_records, lib.edkeys_poison, lib.edkeys_table_words, lib.edkeys_workgroup):
        f.restype = u32
    assert lib.edkeys_guard_words() >= 1024 and lib.edkeys_guard_records() * 10 >= 1024
    assert lib.edkeys_table_words() == ev.TABLE_WORDS and lib.edkeys_workgroup() == 512
    return lib


def ptr(a):
    return a.ctypes.data_as(vp)


@functools.lru_cache(maxsize=None)
def table_array(name):
    return np.array(ev.table_words(name), dtype=np.uint32)


class Out:
    pass


def launch(dev, *, batch, n, alloc=None, table=None, seeds=None, first=None, pattern=None, ci=0, base=0, entry=0, cap=0, **switches):
    """One edkeys_run: uploaded `seeds` (a sequence of 32-byte strings, padded with 0xEE bytes to the allocation - never read) or the
    stream form from `first`; the dump form or, with a pattern, the filter form.  Every array comes back split into what the launch
    owns and the guard words behind it."""
    alloc = batch if alloc is None else alloc
    assert (seeds is None) != (first is None) and not set(switches) - set(SWITCHES)
    guard, grecs, poison = dev.edkeys_guard_words(), dev.edkeys_guard_records(), dev.edkeys_poison()
    pay, hits = np.zeros(8 * alloc + guard, dtype=np.uint32), np.zeros(alloc // 32 + guard, dtype=np.uint32)
    recs = np.zeros((cap + grecs, 10), dtype=np.uint32)
    tguard, sguard = np.zeros(guard, dtype=np.uint32), np.zeros(guard, dtype=np.uint32)
    j = Job(alloc_batch=alloc, batch=batch, n=n, filter_form=int(pattern is not None), ci=ci, match_base=base, match_cap=cap,
            header_in=(u32 * 4)(entry, *HDR_REST), payloads_out=ptr(pay), hits_out=ptr(hits), recs_out=ptr(recs),
            table_guard_out=ptr(tguard), seeds_guard_out=ptr(sguard), **switches)
    if table is not None:
        tab = table_array(table)
        j.table = ptr(tab)
    if seeds is not None:
        blob = np.frombuffer(b"".join(seeds[:alloc]) + b"\xEE" * (32 * (alloc - min(alloc, len(seeds)))), dtype=np.uint8)
        assert blob.size == 32 * alloc
        j.seeds = ptr(blob)
    else:
        j.seed, j.stream, j.first = (u32 * 6)(*ev.seed_words()), ev.STREAM, first
    if pattern is not None:
        j.pattern = pattern.encode()
    rc = dev.edkeys_run(ctypes.byref(j))
    assert rc == 0, f"edkeys_run failed: {rc} (launch {j.launch_error}, sync {j.sync_error})"
    o = Out()
    o.err, o.sync, o.kind, o.header, o.poison, o.alloc = j.launch_error, j.sync_error, j.filter_kind, list(j.header_out), poison, alloc
    o.payloads, o.hits = pay[:8 * alloc].reshape(alloc, 8), hits[:alloc // 32]
    o.recs, o.recs_guard = recs[:cap], recs[cap:]
    guards = [pay[8 * alloc:], hits[alloc // 32:], tguard, sguard] + ([o.recs_guard.ravel()] if pattern is not None else [])
    o.guards_intact = all(bool((g == poison).all()) for g in guards)
    return o


def words_of(keys):
    """[len(keys)][8] words in memory order."""
    return np.frombuffer(b"".join(keys), dtype="<u4").reshape(len(keys), 8)


def assert_dump(o, want):
    """Every one of the alloc payload slots equals `want` (keys where keyed, zero where keyless), nothing else was written."""
    assert o.err == 0 and o.sync == 0, (o.err, o.sync)
    assert len(want) == o.alloc
    w = words_of(want)
    assert not (w == o.poison).any(), "an expected payload word equals the poison"
    bad = np.flatnonzero((o.payloads != w).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8])
    assert o.guards_intact, "guard words written"
    assert (o.hits == o.poison).all(), "a dump wrote the hit mask"


# ---- dump, real table, uploaded seeds ---------------------------------------------------------------------------------------------------

DUMP_SHAPES = [(512, 1), (512, 2), (512, 63), (512, 64), (512, 65), (512, 511), (512, 512), (1024, 513), (1024, 577), (1024, 1023), (1536, 1025)]


@pytest.mark.parametrize("batch,n", DUMP_SHAPES)
def test_dump_of_uploaded_seeds(dev, batch, n):
    o = launch(dev, batch=batch, n=n, seeds=ev.real_seeds())
    assert_dump(o, ev.dump_of(ev.real_payloads(), batch, n))


# ---- dump, the stream form --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch,n", ev.STREAM_SHAPES)
@pytest.mark.parametrize("first", ev.STREAM_FIRSTS, ids=["0", "2^32-300", "2^40+7"])
def test_dump_of_the_stream(dev, first, batch, n):
    """Lane i draws index first + i (the low word carries into the high one inside the batch from 2^32 - 300); lanes at and past n draw
    a key too and report none."""
    keys = ev.stream_keys(first, 1024)[:batch]
    assert keys[0] == sv.public_key(sv.stream_seed(ev.STREAM_SEED, ev.STREAM, first))
    o = launch(dev, batch=batch, n=n, first=first)
    assert_dump(o, ev.dump_of(keys, batch, n))


# ---- dump, crafted tables ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ev.TABLES)
def test_dump_of_crafted_tables(dev, name):
    """Batch 1024, n = 1000.  Every class the table is there for is present among the compared lanes (asserted here, shown to hold on
    the reference alone in tests/test_ed_keys_vectors.py): a vector change cannot empty a case silently."""
    for rot in ev.rotations(name):
        want = ev.crafted_payloads(name, rot)
        lanes = ev.crafted_class_lanes(name, rot)
        for c in ev.required_classes(name):
            assert lanes.get(c) and max(lanes[c]) < ev.N, c
        if name != "real-but-one":
            assert all(want[i] == bytes(32) for i in lanes["zero payload"]) and all(want[i] == bytes(31) + b"\x80" for i in lanes["payload 00..80"])
            assert {want[i][31] >> 7 for i in range(ev.N)} == {0, 1}
        o = launch(dev, batch=ev.BATCH, n=ev.N, table=name, seeds=ev.crafted_seeds(name, rot))
        assert_dump(o, want)


# ---- the filter form ---------------------------------------------------------------------------------------------------------------------

def mask_of(hits, alloc):
    m = np.zeros(alloc // 32, dtype=np.uint32)
    for s in hits:
        m[s >> 5] |= np.uint32(1 << (s & 31))
    return m


def check_filtered(o, keys, hits, *, kind, entry=0, base=0, cap):
    """`keys`: index -> the expected payload of every lane in `hits`.  The mask is exactly `hits` - every word of it written, those of
    keyless waves as 0 -, the records of `hits` follow the ring's count on entry in index order (record k at entry - base + k, dropped
    at or past cap), the header counts them all, the payload slots of `hits` hold their keys and every other slot is still poison."""
    assert o.err == 0 and o.sync == 0, (o.err, o.sync)
    assert o.kind == kind
    assert o.guards_intact, "guard words written"
    assert o.header == [(entry + len(hits)) % 2**32, *HDR_REST]
    assert not (o.hits == o.poison).any(), "hit-mask words left unwritten"
    want_mask = mask_of(hits, o.alloc)
    assert (o.hits == want_mask).all(), np.flatnonzero(o.hits != want_mask)[:8]
    first = (entry - base) % 2**32
    written = max(0, min(cap - first, len(hits)))
    assert (o.recs[:first] == o.poison).all()
    got = o.recs[first:first + written]
    assert (got[:, 1] == 0).all()
    assert [(int(r[0]), r[2:].tobytes()) for r in got] == [(i, keys[i]) for i in hits[:written]]
    assert (o.recs[first + written:] == o.poison).all(), "records beyond the hits or the cap written"
    want = np.full((o.alloc, 8), o.poison, dtype=np.uint32)
    if hits:
        w = words_of([keys[i] for i in hits])
        assert not (w == o.poison).any()
        want[hits] = w
    bad = np.flatnonzero((o.payloads != want).any(axis=1))
    assert bad.size == 0, ("payload slots", bad.size, bad[:8])


FILTER_SHAPES = [(512, 1), (512, 65), (1024, 513), (1536, 1025)]


@pytest.mark.parametrize("batch,n", FILTER_SHAPES)
def test_match_all_reports_the_keyed_lanes_only(dev, batch, n):
    """`.` (kind 3) accepts every payload, the key of a keyless lane's all-zero seed and of a keyless lane's draw included: the mask is
    bits 0 .. n - 1, the words of keyless waves are 0, the records are (i, key i) in index order, slots from n on are still poison."""
    keys = ev.real_payloads()
    o = launch(dev, batch=batch, n=n, seeds=ev.real_seeds(), pattern=".", cap=batch)
    check_filtered(o, keys, list(range(n)), kind=DEVF_ALL, cap=batch)
    first = ev.STREAM_FIRSTS[1]
    keys = ev.stream_keys(first, max(batch, 1024))
    o = launch(dev, batch=batch, n=n, first=first, pattern=".", entry=7, base=4, cap=batch + 3)
    check_filtered(o, keys, list(range(n)), kind=DEVF_ALL, entry=7, base=4, cap=batch + 3)


@pytest.mark.parametrize("length", [1, 2])
def test_literal_prefix_of_uploaded_seeds(dev, length):
    """The prefix is lane 0's own and that of the all-zero seed's key, which every keyless lane computes
    (tests/test_ed_keys_vectors.py asserts it, and that keyed hits and keyed non-hits both exist): a kernel that judged a keyless
    lane by the key it computed would report it.  (The shipped one zeroes the payload first: test_prefix_the_zero_payload_matches.)"""
    keys, prefix = ev.real_payloads(), ev.uploaded_prefix(length)
    assert ev.prefix_hits([ev.zero_seed_payload()], prefix) == [0]
    for batch, n in FILTER_SHAPES[1:]:
        hits = ev.prefix_hits(keys[:n], prefix)
        assert 0 in hits and len(hits) < n
        o = launch(dev, batch=batch, n=n, seeds=ev.real_seeds(), pattern="^" + prefix, entry=2**32 - 1, base=2**32 - 1, cap=len(hits) + 8)
        check_filtered(o, keys, hits, kind=DEVF_RANGES, entry=2**32 - 1, base=2**32 - 1, cap=len(hits) + 8)


@pytest.mark.parametrize("prefix", ["1", "11"])
def test_prefix_the_zero_payload_matches(dev, prefix):
    """The kernel zeroes a keyless lane's payload before it runs the filter, so the patterns for which `has_key` decides are those an
    all-zero payload satisfies: match-all above, and prefixes of '1's (leading zero bytes), kind 1.  '^1' has keyed hits (lane 1's key
    starts with a zero byte), '^11' has none: no bit, no record, the count as on entry - in both forms of the seeds."""
    keys = ev.real_payloads()
    assert ev.prefix_hits([bytes(32)], prefix) == [0]
    for batch, n in FILTER_SHAPES[1:]:
        hits = ev.prefix_hits(keys[:n], prefix)
        assert (1 in hits and len(hits) < n) if prefix == "1" else hits == []
        o = launch(dev, batch=batch, n=n, seeds=ev.real_seeds(), pattern="^" + prefix, entry=9, base=9, cap=16)
        check_filtered(o, keys, hits, kind=DEVF_RANGES, entry=9, base=9, cap=16)
    batch, n = ev.STREAM_FILTER_SHAPE
    first = ev.STREAM_FIRSTS[1]
    draws = ev.stream_keys(first, batch)
    hits = [i for i in ev.prefix_hits(draws, prefix) if i < n]
    o = launch(dev, batch=batch, n=n, first=first, pattern="^" + prefix, entry=9, base=9, cap=16)
    check_filtered(o, draws, hits, kind=DEVF_RANGES, entry=9, base=9, cap=16)


@pytest.mark.parametrize("length", [1, 2])
def test_literal_prefix_of_the_stream(dev, length):
    """Lanes at and past n draw real keys here, and at least one of them matches the prefix (asserted): it is not reported."""
    batch, n = ev.STREAM_FILTER_SHAPE
    first, prefix = ev.stream_prefix(length)
    keys = ev.stream_keys(first, batch)
    all_hits = ev.prefix_hits(keys, prefix)
    hits = [i for i in all_hits if i < n]
    assert hits and len(hits) < n and len(all_hits) > len(hits)
    o = launch(dev, batch=batch, n=n, first=first, pattern="^" + prefix, entry=12348, base=12345, cap=len(hits) + 8)
    check_filtered(o, keys, hits, kind=DEVF_RANGES, entry=12348, base=12345, cap=len(hits) + 8)


def test_a_zero_payload_is_a_hit_like_any_other(dev):
    """Match-all on the two-window crafted table: the lanes whose key is the point of order 4 with even x have an all-zero payload,
    which is also what a dump writes for "no key".  Nothing in ed_keys_kernel or in ptab_compact_kernel<8> treats a zero payload as
    "no key": such a lane is a hit, has its bit, its record and its (zero) payload slot like any other.  Pinned here; whether such a
    key has an address is the host's question (it has none)."""
    name = "two-window"
    keys, lanes = ev.crafted_payloads(name), ev.crafted_class_lanes(name)
    zero = lanes["zero payload"]
    assert zero and all(keys[i] == bytes(32) for i in zero) and {63, 64, 511, 512} & set(zero)
    o = launch(dev, batch=ev.BATCH, n=ev.N, table=name, seeds=ev.crafted_seeds(name), pattern=".", cap=ev.BATCH)
    check_filtered(o, keys, list(range(ev.N)), kind=DEVF_ALL, cap=ev.BATCH)
    assert all(not o.recs[i, 2:].any() and o.recs[i, 0] == i for i in zero)
    assert all(not o.payloads[i].any() for i in zero)


@pytest.mark.parametrize("cap", [0, 1, 100, 600])
def test_ring(dev, cap):
    """513 hits behind 40 003 - 40 000 = 3 records of an earlier dispatch: cap 0 and 1 (nothing fits), fewer slots than hits, more."""
    batch, n = 1024, 513
    keys = ev.real_payloads()
    o = launch(dev, batch=batch, n=n, seeds=ev.real_seeds(), pattern=".", entry=40003, base=40000, cap=cap)
    check_filtered(o, keys, list(range(n)), kind=DEVF_ALL, entry=40003, base=40000, cap=cap)
    assert (o.recs != o.poison).any(axis=1).sum() == max(0, min(cap - 3, n))


# ---- launches launch_ed_keys refuses -----------------------------------------------------------------------------------------------------

def untouched(o):
    return o.err == HIP_ERROR_INVALID_VALUE and o.sync == -1 and o.guards_intact and bool((o.payloads == o.poison).all()) \
        and bool((o.hits == o.poison).all()) and bool((o.recs == o.poison).all())


def test_refused_launches_run_nothing(dev):
    alloc, n = 1024, 513
    seeds, keys = ev.real_seeds(), ev.real_payloads()
    common = dict(alloc=alloc, seeds=seeds)
    geometry = [dict(batch=0, n=0), dict(batch=0, n=1), dict(batch=511, n=100), dict(batch=520, n=100), dict(batch=1024, n=0),
                dict(batch=1024, n=1025), dict(batch=512, n=513)]
    for kw in geometry + [dict(batch=1024, n=n, null_table=1), dict(batch=1024, n=n, null_payloads=1)]:
        assert untouched(launch(dev, **common, **kw)), kw
        o = launch(dev, **common, pattern=".", cap=64, **kw)
        assert untouched(o) and o.header == [0, *HDR_REST], kw
        assert untouched(launch(dev, alloc=alloc, first=5, **kw)), kw
    for s in SWITCHES[2:]:
        o = launch(dev, batch=1024, n=n, **common, pattern=".", cap=64, **{s: 1})
        assert untouched(o) and o.header == [0, *HDR_REST], s
    # the same arguments with the fault taken out do run (the poison would otherwise prove nothing)
    assert_dump(launch(dev, batch=1024, n=n, **common), ev.dump_of(keys, 1024, n))
    o = launch(dev, batch=1024, n=n, **common, pattern=".", cap=64)
    check_filtered(o, keys, list(range(n)), kind=DEVF_ALL, cap=64)
