"""The three kernels behind a list or contract dispatch - ptab_lookup_kernel<5|8>, payload_filter_kernel<FULL> and
ptab_compact_kernel<5|8> (vgen_amd/csrc/device/kernels.hip; only launch_ptab starts them) - on buffers filled word by word.

tests/test_gpu_pattern_list.py and tests/test_gpu_eth_contract.py reach these kernels through real keys, so hits land where
the hashes put them.  Here a test-only driver (tests/native/list_dev.hip -> liblistdev.so, linked against the product's own
build/lib/device/kernels.o) calls vg::launch_ptab on payloads, masks, rings and tables the test chooses, and everything that
comes back - the whole hit mask, the header, every record, and the guard words and records behind them - is compared, exactly,
with models written here in numpy from the documented layouts (device_types.h): interval lookup of the top 64 payload bits,
Python `re` on "0x" + hex for the deferred filter, and the compaction "hit h goes to record (count on entry - match_base) + h
if that is below match_cap; the count advances by every hit".  The tables come from tests/test_ptab_tables.py, which checks
them against the host build of ptab_find first.

What is pinned: the lookup at lo, hi, lo - 1, hi + 1, crowded buckets, 0 and 2^64 - 1 (a); placement at word, thread, wave
and image edges (b); more than one pass of the compaction loop, the second one ragged (c); a ring that fills at every edge
and a running count that wraps (d); ragged counts over stale payloads and a stale mask, and a second launch that continues
the first (e); both forms of the deferred filter (f); the launch check (g); and the product's own wiring at a six-image,
two-pass size, tail copy and sort included (h).  No case may be empty: each states the least number of hits and of non-hits
its model must produce."""
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

from conftest import locked_make
from test_ptab_tables import Table, mixed_intervals, probes, sparse_intervals

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 1 << 32
HIP_ERROR_INVALID_VALUE = 1
MASK_POISON = 0xA5A5A5A5A5A5A5A5
REC_POISON = 0xDEADBEEF
HDR_REST = (0x11111111, 0x22222222, 0x33333333)   # cap, clk_cycles, clk_ticks of the header: not the list kernels' to touch
PASS = 1 << 20                                    # slots per pass of the compaction: 1024 threads x 16 words x 64

u32, vp = ctypes.c_uint32, ctypes.c_void_p


class Job(ctypes.Structure):   # listdev_job of tests/native/list_dev.hip, field by field
    _fields_ = [("payload_words", u32), ("stride", u32), ("count", u32), ("images", u32), ("repeat", u32),
                ("match_base", u32), ("match_cap", u32), ("header_in", u32 * 4),
                ("payloads", vp), ("hits_in", vp), ("recs_in", vp),
                ("bits", u32), ("n", u32), ("bitmap_words", u32), ("offsets_count", u32),
                ("bitmap", vp), ("offsets", vp), ("lo", vp), ("hi", vp),
                ("filter", vp),
                ("launch_error", ctypes.c_int32), ("header_out", u32 * 4), ("hits_out", vp), ("recs_out", vp)]


@pytest.fixture(scope="module")
def dev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "liblistdev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "liblistdev.so"))
    assert lib.listdev_job_size() == ctypes.sizeof(Job)
    assert lib.listdev_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    return lib


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


def ptr(a):
    return a.ctypes.data_as(vp)


class Out:
    pass


def launch(dev, pay, *, stride, count, images, table=None, filt=None, entry=0, base=0, cap=0, repeat=1,
           mask_fill=MASK_POISON, pw=None):
    """One listdev_run.  pay: uint32 [images * stride, payload_words].  Returns the launch error, the mask and its guard words,
    the header and the cap + 64 records (10 words each), and the ring as it was uploaded (all poison)."""
    pw = pw or pay.shape[1]
    slots = images * stride
    assert pay.dtype == np.uint32 and pay.flags.c_contiguous and pay.shape == (slots, pw)
    words = slots // 64
    hits_in = np.full(words + 64, MASK_POISON, dtype=np.uint64)
    hits_in[:words] = mask_fill
    recs_in = np.full((cap + 64, 10), REC_POISON, dtype=np.uint32)
    o = Out()
    o.hits = np.zeros(words + 64, dtype=np.uint64)
    o.recs = np.zeros((cap + 64, 10), dtype=np.uint32)
    j = Job(payload_words=pw, stride=stride, count=count, images=images, repeat=repeat, match_base=base, match_cap=cap,
            header_in=(u32 * 4)(entry, *HDR_REST), payloads=ptr(pay), hits_in=ptr(hits_in), recs_in=ptr(recs_in),
            hits_out=ptr(o.hits), recs_out=ptr(o.recs))
    if filt is not None:
        j.filter = filt.value
    else:
        j.bits, j.n, j.bitmap_words, j.offsets_count = table.bits, table.n, table.bitmap.size, table.offsets.size
        j.bitmap, j.offsets, j.lo, j.hi = ptr(table.bitmap), ptr(table.offsets), ptr(table.lo), ptr(table.hi)
    rc = dev.listdev_run(ctypes.byref(j))
    assert rc == 0, f"listdev_run failed: {rc}"
    o.err, o.header, o.words, o.recs_in, o.hits_in = j.launch_error, list(j.header_out), words, recs_in, hits_in
    return o


# ---- models ------------------------------------------------------------------------------------------------------------

def top64(pay):
    """int.from_bytes(payload_bytes[:8], "big") of every slot."""
    b = pay.view(np.uint8).reshape(pay.shape[0], -1)
    return np.ascontiguousarray(b[:, :8]).view(">u8")[:, 0].astype(np.uint64)


def counted(stride, count, images):
    return np.tile(np.arange(stride) < count, images)


def lookup_model(pay, table, stride, count, images):
    return counted(stride, count, images) & (table.find(top64(pay)) >= 0) & pay.any(axis=1)


def compact_model(recs, hit, pay, entry, base, cap):
    """Applies one dispatch to the ring `recs` (in place); returns the header count on exit."""
    idx = np.flatnonzero(hit)
    pos = (entry - base) % U32 + np.arange(idx.size, dtype=np.int64)
    keep = pos < cap
    recs[pos[keep], 0] = idx[keep]
    recs[pos[keep], 1] = 0
    recs[pos[keep], 2:] = 0
    recs[pos[keep], 2:2 + pay.shape[1]] = pay[idx[keep]]
    return (entry + idx.size) % U32


def mask_words(hit):
    return np.packbits(hit, bitorder="little").view("<u8")


def check(o, hit, pay, *, entry, base, cap, repeat=1, tag="", min_hits, min_non):
    """Everything that came back against the models; `hit` is the model's mask (bool per slot)."""
    H, non = int(hit.sum()), int(hit.size - hit.sum())
    assert H >= min_hits and non >= min_non, (tag, H, non)
    assert o.err == 0, (tag, o.err)
    got = o.hits[:o.words]
    want = mask_words(hit)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, "mask word", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), bad.size)
    assert (o.hits[o.words:] == MASK_POISON).all(), (tag, "mask guard words written")
    recs = o.recs_in.copy()
    count = entry
    for _ in range(repeat):
        count = compact_model(recs, hit, pay, count, base, cap)
    assert o.header == [count, *HDR_REST], (tag, o.header, count)
    bad = np.flatnonzero((o.recs != recs).any(axis=1))
    assert bad.size == 0, (tag, "record", int(bad[0]), o.recs[bad[0]].tolist(), recs[bad[0]].tolist(), bad.size)
    stored = int((recs[:cap, 0] != REC_POISON).sum()) if cap else 0
    assert (recs[cap:] == REC_POISON).all()
    print(f"{tag}: {hit.size} slots, {H} hits, {stored} stored records (cap {cap}, count {entry} -> {count})")
    return H


def bswap(a):
    return np.asarray(a, dtype=np.uint32).byteswap()


def payloads_of(x, lower):
    """Payload words (memory order: little-endian words of the byte string) whose big-endian top 64 bits are x."""
    x = np.asarray(x, dtype=np.uint64)
    pay = np.empty((x.size, 2 + lower.shape[1]), dtype=np.uint32)
    pay[:, 0] = bswap((x >> np.uint64(32)).astype(np.uint32))
    pay[:, 1] = bswap((x & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    pay[:, 2:] = lower
    return pay


# ---- a. lookup geometry --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def table_of(geometry, bits):
    return Table({"mixed": mixed_intervals, "sparse": sparse_intervals}[geometry](bits, seed=bits), bits)


def lookup_case(dev, geometry, bits, pw):
    stride = 8192
    t = table_of(geometry, bits)
    rs = np.random.RandomState(1000 * bits + pw)
    edge = probes(t, 0, seed=bits)
    # payloads whose top 8 bytes are zero: all zero (the "no key" mark), one bit in the last word, one in word 2, lower words
    # random, and (8 words) only word 7 / only word 4 set; then values 1 .. 5 over zero lower words
    special = np.zeros((12, pw), dtype=np.uint32)
    special[1, pw - 1] = 1 << 31
    special[2, 2] = 1
    special[3, 2:] = rs.randint(1, U32, size=pw - 2, dtype=np.uint64)
    special[4, pw - 1] = 1
    special[5, min(4, pw - 1)] = 0x00010000
    special[6:11, 1] = bswap(np.arange(1, 6))
    n_rand = stride - edge.size - special.shape[0]
    assert n_rand >= 2000
    x = np.concatenate([edge, rs.randint(0, 1 << 63, size=n_rand, dtype=np.uint64) * np.uint64(2) + rs.randint(0, 2, size=n_rand).astype(np.uint64)])
    pay = np.concatenate([payloads_of(x, rs.randint(0, U32, size=(x.size, pw - 2), dtype=np.uint64).astype(np.uint32)), special])
    pay = np.ascontiguousarray(pay[rs.permutation(stride)])
    hit = lookup_model(pay, t, stride, stride, 1)
    zero_top = top64(pay) == 0
    assert zero_top.sum() >= 7 and (~pay.any(axis=1)).sum() >= 1
    if geometry == "mixed":   # the table holds 0: a zero top hits unless the whole payload is zero
        assert (hit[zero_top] == pay[zero_top].any(axis=1)).all() and hit[zero_top].sum() >= 6
    else:
        assert not hit[zero_top].any()
    o = launch(dev, pay, stride=stride, count=stride, images=1, table=t, cap=stride)
    check(o, hit, pay, entry=0, base=0, cap=stride, tag=f"a {geometry} bits={bits} words={pw}",
          min_hits=450 if geometry == "mixed" else 80, min_non=6000)


@pytest.mark.parametrize("pw", [5, 8])
@pytest.mark.parametrize("bits", [16, 20])
@pytest.mark.parametrize("geometry", ["mixed", "sparse"])
def test_lookup_geometry(dev, geometry, bits, pw):
    lookup_case(dev, geometry, bits, pw)


def test_lookup_geometry_24_bits(dev):
    lookup_case(dev, "mixed", 24, 5)


# ---- b / c. compaction placement ---------------------------------------------------------------------------------------------
# The table is one interval; a slot hits when the test plants the marker in its top bytes.  The other words depend on the slot,
# so that a record carrying another slot's payload is caught.

HIT_TOP, MISS_TOP = 0x40000000, 0x80000000


@functools.lru_cache(maxsize=None)
def marker_table():
    return Table([(HIT_TOP << 32, (HIT_TOP << 32) | 0xFFFFFFFF)], 16)


def marker_payloads(planted):
    slot = np.arange(planted.size, dtype=np.uint32)
    pay = np.empty((planted.size, 5), dtype=np.uint32)
    pay[:, 0] = bswap(np.where(planted, HIT_TOP, MISS_TOP).astype(np.uint32))
    pay[:, 1] = bswap(slot)
    pay[:, 2] = slot * np.uint32(2654435761) | np.uint32(1)
    pay[:, 3] = slot ^ np.uint32(0xA5A5A5A5)
    pay[:, 4] = ~slot
    return pay


def marker_case(dev, planted, stride, images, tag, min_hits, min_non, **ring):
    pay = marker_payloads(planted)
    hit = lookup_model(pay, marker_table(), stride, stride, images)
    assert (hit == planted).all()
    ring.setdefault("cap", planted.size)
    o = launch(dev, pay, stride=stride, count=stride, images=images, table=marker_table(), **ring)
    return check(o, hit, pay, entry=ring.get("entry", 0), base=ring.get("base", 0), cap=ring["cap"], tag=tag,
                 min_hits=min_hits, min_non=min_non)


def bits_at(n, *slots):
    m = np.zeros(n, dtype=bool)
    m[list(slots)] = True
    return m


def density(n, p, seed):
    return np.random.RandomState(seed).random_sample(n) < p


# name -> (mask of n slots, least hits, least non-hits)
PLACEMENT = {
    "empty": lambda n: (np.zeros(n, dtype=bool), 0, n),
    "every slot": lambda n: (np.ones(n, dtype=bool), n, 0),
    "slot 0": lambda n: (bits_at(n, 0), 1, n - 1),
    "last slot": lambda n: (bits_at(n, n - 1), 1, n - 1),
    "bits 0 and 63 of a word": lambda n: (bits_at(n, 64 * 37, 64 * 37 + 63), 2, n - 2),
    "a thread's edge": lambda n: (bits_at(n, 64 * 16 - 1, 64 * 16), 2, n - 2),                     # words 15 | 16
    "a run across an image boundary": lambda n: (bits_at(n, *range(8192 - 100, min(n, 8192 + 100))), 100, n - 200),
    "density 2^-10": lambda n: (density(n, 2.0 ** -10, 10), n // 2048, n - n // 512),
    "density 1/2": lambda n: (density(n, 0.5, 11), n // 2 - n // 32, n // 2 - n // 32),
    "density 63/64": lambda n: (density(n, 63 / 64, 12), n - n // 32, n // 128),
}


@pytest.mark.parametrize("images", [1, 6])
@pytest.mark.parametrize("name", sorted(PLACEMENT))
def test_compaction_placement(dev, name, images):
    n = images * 8192
    planted, min_hits, min_non = PLACEMENT[name](n)
    marker_case(dev, planted, 8192, images, f"b {name}, {images} image(s)", min_hits, min_non)


def two_pass_mask(stride, images, second_pass_only=False):
    """Hits on both sides of the pass boundary (slot 2^20), of the wave edge inside a pass (words 1023 | 1024), at the last
    slot, and at random positions with density 2^-8."""
    n = stride * images
    assert PASS < n < 2 * PASS
    m = density(n, 2.0 ** -8, n % 1000)
    m[[s for s in (PASS - 1, PASS, n - 1, 64 * 1024 - 1, 64 * 1024, PASS + 64 * 1024 - 1, PASS + 64 * 1024) if s < n]] = True
    if second_pass_only:
        m[:PASS] = False
    return m


TWO_PASS = {"one image": (PASS + 8192, 1), "six images": (3 << 16, 6)}   # 1 056 768 and 1 179 648 slots


@pytest.mark.parametrize("second_pass_only", [False, True])
@pytest.mark.parametrize("shape", sorted(TWO_PASS))
def test_two_passes(dev, shape, second_pass_only):
    stride, images = TWO_PASS[shape]
    n = stride * images
    planted = two_pass_mask(stride, images, second_pass_only)
    first = int(planted[:PASS].sum())
    if second_pass_only:
        assert first == 0 and planted[PASS] and planted[n - 1]
        least = (n - PASS) // 512
    else:
        assert first >= 3000 and planted[PASS - 1] and planted[PASS] and int(planted[PASS:].sum()) >= 20
        least = 3000
    if images == 6:   # the pass boundary lies inside image 5
        assert 5 * stride < PASS < 6 * stride
    marker_case(dev, planted, stride, images, f"c {shape}{', hits in the second pass only' if second_pass_only else ''}", least, n - n // 128)


# ---- d. ring edges -------------------------------------------------------------------------------------------------------------

def ring_cases(H, extra_caps=()):
    caps = [0, 1, H - 1, H, H + 1, *extra_caps]
    bases = [0, 12345, U32 - 5, U32 - H + 1]   # the last two wrap during the dispatch
    return [dict(cap=c, base=b, entry=b) for c in caps for b in bases] + \
           [dict(cap=c, base=777, entry=780) for c in (H + 4, H + 3, H + 2, 3, 2)]   # three records of an earlier dispatch in front


def test_ring_edges_one_pass(dev):
    stride, images = 8192, 6
    planted, min_hits, min_non = PLACEMENT["density 1/2"](stride * images)
    H = int(planted.sum())
    assert H > 20000
    for ring in ring_cases(H):
        o_H = marker_case(dev, planted, stride, images, f"d one pass {ring}", min_hits, min_non, **ring)
        assert o_H == H


def test_ring_edges_two_passes(dev):
    stride, images = TWO_PASS["one image"]
    planted = two_pass_mask(stride, images)
    H, first = int(planted.sum()), int(planted[:PASS].sum())
    assert 3000 <= first < H - 20
    pay = marker_payloads(planted)
    hit = lookup_model(pay, marker_table(), stride, stride, images)
    assert (hit == planted).all()
    # also a cap inside the first pass's hits, and one equal to the first pass's count exactly
    for ring in ring_cases(H, extra_caps=(first // 2, first)):
        o = launch(dev, pay, stride=stride, count=stride, images=images, table=marker_table(), **ring)
        check(o, hit, pay, tag=f"d two passes (first pass {first}) {ring}", min_hits=3000, min_non=PASS, **ring)


def test_records_follow_the_count_on_entry(dev):
    """Count on entry = match_base + 3: the dispatch's records start at record 3; records 0 .. 2 keep their poison."""
    planted, min_hits, min_non = PLACEMENT["density 2^-10"](8192)
    H = int(planted.sum())
    pay = marker_payloads(planted)
    o = launch(dev, pay, stride=8192, count=8192, images=1, table=marker_table(), entry=U32 - 2, base=U32 - 5, cap=H + 3)
    check(o, planted, pay, entry=U32 - 2, base=U32 - 5, cap=H + 3, tag="d count on entry = base + 3", min_hits=min_hits, min_non=min_non)
    assert (o.recs[:3] == REC_POISON).all() and o.recs[3, 0] == np.flatnonzero(planted)[0] and o.recs[H + 2, 0] == np.flatnonzero(planted)[-1]
    assert o.header[0] == (U32 - 2 + H) % U32


# ---- e. ragged counts and stale state ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("images", [1, 6])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 257, 8191])
def test_ragged_count_over_stale_state(dev, count, images):
    """Every slot at or past count holds a payload that would hit, and the mask starts as all ones: the lookup has to rewrite
    every word of the grid and to stop at count in every image.  Two launches back to back: the second reads the header the
    first wrote and continues the ring behind its records."""
    stride = 8192
    rs = np.random.RandomState(count * 7 + images)
    planted = np.ones((images, stride), dtype=bool)
    planted[:, :count] = rs.random_sample((images, count)) < 0.25
    planted[:, count - 1] = True
    planted = planted.reshape(-1)
    pay = marker_payloads(planted)
    hit = lookup_model(pay, marker_table(), stride, count, images)
    assert (hit == (planted & counted(stride, count, images))).all()
    H = int(hit.sum())
    stale = int((planted & ~hit).sum())
    assert H >= images and stale == images * (stride - count) >= images
    cap = H + (H + 1) // 2    # the second launch's records start at H and run past the cap
    for repeat in (1, 2):
        o = launch(dev, pay, stride=stride, count=count, images=images, table=marker_table(), entry=4242, base=4242, cap=cap,
                   repeat=repeat, mask_fill=0xFFFFFFFFFFFFFFFF)
        check(o, hit, pay, entry=4242, base=4242, cap=cap, repeat=repeat, tag=f"e count={count} images={images} repeat={repeat}",
              min_hits=images, min_non=images * (stride - count))
        assert o.header[0] == 4242 + repeat * H
        if repeat == 2:
            assert (o.recs[H:cap, 0] == np.flatnonzero(hit)[:cap - H]).all()


# ---- f. the deferred filter ------------------------------------------------------------------------------------------------------------

PATTERNS = [("^0xdead", True, 2), ("dead$", False, 2), ("^0x0000", False, 2), ("de[0-9]d", False, 4)]   # exact up to case on the device
PLANT = {"^0xdead": lambda r: "dEaD" + "%036x" % r.getrandbits(144), "dead$": lambda r: "%036x" % r.getrandbits(144) + "DeAd",
         "^0x0000": lambda r: "0000" + "%036x" % (r.getrandbits(144) | 1)}


def plant_de_d(r):
    h = list("%040x" % r.getrandbits(160))
    at = r.randrange(0, 37)   # (odd offsets too: the match is not byte aligned)
    h[at:at + 4] = "de%dd" % r.randrange(10)
    return "".join(h)


PLANT["de[0-9]d"] = plant_de_d


@functools.lru_cache(maxsize=None)
def filter_payloads(pattern, images):
    """Random payloads plus planted ones: in every image a hit in slot 0, in slots 256 and 8191 (the last counted slots of the two
    counts), in slot 257 (a would-be hit just past the smaller count) and in eight more slots below 256; slot 5 all zero.
    Returns the payload words and what Python's re says about "0x" + hex of every slot (case ignored)."""
    stride = 8192
    r = random.Random(f"{pattern}/{images}")
    b = np.frombuffer(r.randbytes(images * stride * 20), dtype=np.uint8).reshape(-1, 20).copy()
    for v in range(images):
        for s in [0, 256, 257, 8191] + r.sample(range(6, 256), 8):
            b[v * stride + s] = np.frombuffer(bytes.fromhex(PLANT[pattern](r)), dtype=np.uint8)
        b[v * stride + 5] = 0
    rx = re.compile(pattern, re.IGNORECASE)
    accepted = np.array([rx.search("0x" + row.tobytes().hex()) is not None for row in b])
    return np.ascontiguousarray(b).view("<u4").reshape(-1, 5).copy(), accepted


@pytest.mark.parametrize("fmt", [5, 6])
@pytest.mark.parametrize("pattern,ci,kind", PATTERNS)
def test_payload_filter(dev, vg, pattern, ci, kind, fmt):
    pat = vg.Pattern(pattern, ci, vg.AddressFormat(fmt))
    assert pat.device_kind == kind and (pat.dfa_bytes > 0) == (kind == 4)
    stride = 8192
    for images in (1, 6):
        pay, accepted = filter_payloads(pattern, images)
        for count in (8192, 257):
            hit = counted(stride, count, images) & accepted & pay.any(axis=1)
            for v in range(images):
                s = v * stride
                assert hit[s] and hit[s + count - 1] and not hit[s + 5] and accepted[s + 257] and hit[s + 257] == (count > 257)
                assert not pay[s + 5].any() and hit[s:s + 256].sum() >= 9
            cap = images * stride
            o = launch(dev, pay, stride=stride, count=count, images=images, filt=pat._h, entry=99, base=99, cap=cap)
            check(o, hit, pay, entry=99, base=99, cap=cap, tag=f"f {pattern!r} format {fmt} count={count} images={images}",
                  min_hits=10 * images, min_non=images * (count // 2))   # (an unanchored four-digit pattern takes < 1 % of random payloads)


# ---- g. rejected launches ------------------------------------------------------------------------------------------------------------

def untouched(o):
    return o.err == HIP_ERROR_INVALID_VALUE and (o.hits == o.hits_in).all() and (o.recs == o.recs_in).all() and o.header == [7, *HDR_REST]


def test_rejected_launches_run_nothing(dev, vg):
    t = marker_table()
    every = lambda n: marker_payloads(np.ones(n, dtype=bool))   # every payload would hit
    assert untouched(launch(dev, every(8192 + 64), stride=8192 + 64, count=8192, images=1, table=t, entry=7, cap=64)), "stride"
    assert untouched(launch(dev, every(8192), stride=8192, count=8193, images=1, table=t, entry=7, cap=64)), "count"
    assert untouched(launch(dev, every(0), stride=8192, count=8192, images=0, table=t, entry=7, cap=64)), "images"
    for bits in (0, 25):   # (arrays of the size the bits ask for, and a bitmap that names no bucket)
        bad = Out()
        bad.bits, bad.n, bad.lo, bad.hi = bits, 1, t.lo, t.hi
        bad.bitmap, bad.offsets = np.zeros(max(1, (1 << bits) // 32), dtype=np.uint32), np.zeros((1 << bits) + 1, dtype=np.uint32)
        assert untouched(launch(dev, every(8192), stride=8192, count=8192, images=1, table=bad, entry=7, cap=64)), bits
    pat = vg.Pattern("^0xdead", True, vg.AddressFormat(6))
    wide = np.zeros((8192, 8), dtype=np.uint32)
    wide[:, :5] = filter_payloads("^0xdead", 1)[0]
    assert untouched(launch(dev, wide, stride=8192, count=8192, images=1, filt=pat._h, entry=7, cap=64)), "filter with 8 words"
    # the same arguments with the fault taken out do run (the poison would otherwise prove nothing)
    o = launch(dev, every(8192), stride=8192, count=8192, images=1, table=t, entry=7, cap=64)
    assert o.err == 0 and o.header[0] == 7 + 8192 and (o.hits[:o.words] == 0xFFFFFFFFFFFFFFFF).all()


# ---- h. through the product's own wiring ---------------------------------------------------------------------------------------------

K0 = 2 ** 65 + 0x5EED0000
WIRED_BATCH = 3 << 16


def wired(vg, fmt, filt, accept, tag):
    """Dump of the six images of WIRED_BATCH keys, then the same dispatch through the filter: the records are exactly the slots
    `accept` (numpy over the dump) takes, in order, with the dump's payloads."""
    r = vg.GpuRunner(batch_size=WIRED_BATCH, fmt=vg.AddressFormat(fmt), frames=2, match_cap=1 << 17, endo=True)
    assert r.batch_size == WIRED_BATCH and r.match_cap == 1 << 17
    r.set_filter(None)
    r.dispatch(K0, 0)
    blob, _, tested = r.await_result(0)
    assert tested == 6 * WIRED_BATCH and len(blob) == 20 * 6 * WIRED_BATCH > 20 * PASS
    dump = np.frombuffer(blob, dtype=np.uint8).reshape(-1, 20)
    want = np.flatnonzero(accept(dump) & dump.any(axis=1))
    assert 256 < want.size < 1 << 17 and (want >= PASS).sum() > 256, want.size   # the tail copy runs; hits in the second pass
    r.set_filter(filt)
    r.dispatch(K0, 1)
    recs, n, tested = r.await_result(1)
    assert tested == 6 * WIRED_BATCH and n == len(recs) == want.size, (n, len(recs), want.size)
    assert np.array_equal(np.array([i for i, _ in recs]), want)
    assert b"".join(p for _, p in recs) == dump[want].tobytes()
    r.close()
    print(f"h {tag}: {dump.shape[0]} slots, {want.size} hits, {len(recs)} stored records")
    return want, dump


def test_through_the_runtime_at_a_two_pass_size(vg):
    rnd = random.Random(12)
    prefixes = sorted(rnd.sample(range(4096), 200))
    plist = vg.PatternList(["^0x%03x" % p for p in prefixes], case_insensitive=True, fmt=vg.AddressFormat(5))
    assert plist.device_kind == 5 and len(plist) == 200
    top12 = lambda d: (d[:, 0].astype(np.uint16) << 4) | (d[:, 1] >> 4)
    want, dump = wired(vg, 5, plist, lambda d: np.isin(top12(d), prefixes), "list of 200 prefixes, format 5")
    assert want.size > 6 * WIRED_BATCH // 25   # (about 5 % of 1.18 M slots)
    # a ring of 256 records: n is still every hit, the stored records are the first 256
    r = vg.GpuRunner(batch_size=WIRED_BATCH, fmt=vg.AddressFormat(5), frames=2, match_cap=256, endo=True)
    assert r.match_cap == 256
    r.set_filter(plist)
    r.dispatch(K0, 0)
    recs, n, tested = r.await_result(0)
    assert tested == 6 * WIRED_BATCH and n == want.size and len(recs) == 256
    assert [i for i, _ in recs] == want[:256].tolist() and b"".join(p for _, p in recs) == dump[want[:256]].tobytes()
    r.close()
    print(f"h list, ring of 256: {dump.shape[0]} slots, {n} hits, {len(recs)} stored records")


def test_deferred_filter_through_the_runtime_at_a_two_pass_size(vg):
    pat = vg.Pattern("^0xab", True, vg.AddressFormat(6))
    assert pat.device_kind == 2
    wired(vg, 6, pat, lambda d: d[:, 0] == 0xAB, "'^0xab' -i, format 6")
