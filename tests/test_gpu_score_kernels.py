"""payload_score_kernel and the compaction behind it (vgen_amd/csrc/device/kernels.hip; only launch_payload_score starts them) on
payloads crafted word by word.

tests/test_gpu_score.py reaches these kernels through real keys, so hits land where the hashes put them.  Here a test-only driver
(tests/native/score_dev.hip -> libscoredev.so by tests/native/score.mk, linked against the product's own build/lib/device/kernels.o) calls
vg::launch_payload_score on the crafted payloads of tests/score_vectors.py — every digit value in every one of the 40 positions, a
zero byte at each of the 20 positions, leading runs of 0 .. 40 digits that end on and across word boundaries, the near misses of a
borrowing zero-byte test (0x01 0x00, 0x00 0x01, 0x10, 0x0f, 0x80 0x00, within a word and across a word boundary), the all-zero and the
all-f payload — padded to 8192 slots, with 1 image and with 6, and with counts of 8192, 8191, 65, 64 and 1 over slots that hold stale
high-scoring payloads.  Everything that comes back — the whole hit mask, the header, every record, and the guard words and records
behind them — is compared, exactly, with a model that scores one hex digit at a time.  Refused launches must leave the poison in place."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import locked_make
import score_vectors as sv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_ERROR_INVALID_VALUE = 1
MASK_POISON = 0xA5A5A5A5A5A5A5A5
REC_POISON = 0xDEADBEEF
HDR_REST = (0x11111111, 0x22222222, 0x33333333)   # cap, clk_cycles, clk_ticks of the header: not these kernels' to touch
STRIDE = 8192
STALE = bytes(19) + b"\x01"                       # what an earlier dispatch left behind a ragged count: 19 zero bytes, 38 leading zeros

u32, vp = ctypes.c_uint32, ctypes.c_void_p


class Job(ctypes.Structure):   # scoredev_job of tests/native/score_dev.hip, field by field
    _fields_ = [("stride", u32), ("count", u32), ("images", u32), ("match_base", u32), ("match_cap", u32), ("n_terms", u32),
                ("terms", u32 * 12), ("header_in", u32 * 4), ("compact_stride", u32),
                ("payloads", vp), ("hits_in", vp), ("recs_in", vp),
                ("launch_error", ctypes.c_int32), ("header_out", u32 * 4), ("hits_out", vp), ("recs_out", vp)]


@pytest.fixture(scope="module")
def dev():
    so = os.path.join(HERE, "native", "libscoredev.so")
    if not os.path.exists(so):
        locked_make("-s", "-C", os.path.join(HERE, "native"), "-f", "score.mk")
    lib = ctypes.CDLL(so)
    assert lib.scoredev_job_size() == ctypes.sizeof(Job)
    assert lib.scoredev_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    return lib


SPECS = ["score:zero-bytes>=2", "score:leading-zero-bytes>=1&zero-bytes>=3", "score:leading:0>=3", "score:leading:f>=2&count:f>=5",
         "score:count:0>=6", "score:count:a>=3&count:5>=3&zero-bytes>=0&leading:a>=0"]


@functools.lru_cache(maxsize=None)
def slots(images):
    """images x 8192 payloads: the crafted ones first (image 0), rotated through the other images, random filler behind them."""
    crafted = sv.crafted_payloads()
    assert len(crafted) <= STRIDE
    out = []
    for im in range(images):
        filler = sv.random_payloads(STRIDE - len(crafted), seed=100 + im)
        rot = crafted[im * 37:] + crafted[:im * 37]
        out += (rot + filler) if im % 2 == 0 else (filler + rot)
    return out


@functools.lru_cache(maxsize=None)
def accepted(images, spec):
    """The model's verdict on every slot, computed once: every term holds and the payload is not the all-zero "no key" mark."""
    return [p != bytes(20) and sv.accepts(spec, p) for p in slots(images)]


def ptr(a):
    return a.ctypes.data_as(vp)


def run(dev, spec_terms, pay, *, stride=STRIDE, count, images, entry=0, base=0, cap=4096, compact_stride=None):
    n_slots = images * stride
    words = n_slots // 64 + 64
    hits_in = np.full(words, MASK_POISON, dtype=np.uint64)
    recs_in = np.full((cap + 64, 10), REC_POISON, dtype=np.uint32)
    hits_out, recs_out = np.zeros_like(hits_in), np.zeros_like(recs_in)
    j = Job()
    j.stride, j.count, j.images, j.match_base, j.match_cap = stride, count, images, base, cap
    j.n_terms = len(spec_terms)
    flat = [v for t in spec_terms for v in t] + [0] * 12
    j.terms = (u32 * 12)(*flat[:12])
    j.header_in = (u32 * 4)(entry, *HDR_REST)
    j.compact_stride = stride if compact_stride is None else compact_stride
    j.payloads, j.hits_in, j.recs_in, j.hits_out, j.recs_out = ptr(pay), ptr(hits_in), ptr(recs_in), ptr(hits_out), ptr(recs_out)
    rc = dev.scoredev_run(ctypes.byref(j))
    assert rc == 0, "scoredev_run: harness error %d" % rc
    return j.launch_error, hits_out, tuple(j.header_out), recs_out


def payload_array(payloads):
    return np.frombuffer(b"".join(payloads), dtype="<u4").reshape(len(payloads), 5).copy()


def model(payloads, verdict, *, stride, count, images, entry, base, cap):
    """-> mask words (+ 64 guard words), header, records (+ 64 guard records) as the kernels must leave them."""
    n_slots = images * stride
    bits = np.zeros(n_slots, dtype=bool)
    for im in range(images):
        for i in range(count):
            bits[im * stride + i] = verdict[im * stride + i]
    mask = np.full(n_slots // 64 + 64, MASK_POISON, dtype=np.uint64)
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    mask[:n_slots // 64] = (bits.reshape(-1, 64) * weights).sum(axis=1, dtype=np.uint64)
    recs = np.full((cap + 64, 10), REC_POISON, dtype=np.uint32)
    hit_slots = np.flatnonzero(bits)
    arr = payload_array(payloads)
    for h, s in enumerate(hit_slots):
        r = (entry - base + h) & 0xFFFFFFFF
        if r < cap:
            recs[r] = [s, 0, *arr[s], 0, 0, 0]
    return mask, ((entry + len(hit_slots)) & 0xFFFFFFFF, *HDR_REST), recs, len(hit_slots)


def check(dev, spec, *, count, images, entry=0, base=0, cap=4096, least_hits=1):
    payloads = list(slots(images))
    verdict = list(accepted(images, spec))
    if count < STRIDE:   # behind a ragged count: stale high scorers, which the model would accept and the kernel must not look at
        for im in range(images):
            for i in range(count, STRIDE):
                payloads[im * STRIDE + i] = STALE
                verdict[im * STRIDE + i] = True
    want_mask, want_hdr, want_recs, n_hits = model(payloads, verdict, stride=STRIDE, count=count, images=images, entry=entry, base=base, cap=cap)
    # the reference alone: at least one hit and at least one miss among the slots the kernel looks at
    assert n_hits >= least_hits and n_hits < images * count, (spec, n_hits)
    err, mask, hdr, recs = run(dev, sv.parse(spec), payload_array(payloads), count=count, images=images, entry=entry, base=base, cap=cap)
    assert err == 0
    assert np.array_equal(mask, want_mask), (spec, np.flatnonzero(mask != want_mask)[:8])
    assert hdr == want_hdr
    assert np.array_equal(recs, want_recs), (spec, np.flatnonzero((recs != want_recs).any(axis=1))[:8])


def test_the_model_has_hits_and_misses_for_every_specification_and_knows_the_near_misses():
    for spec in SPECS:
        v = accepted(1, spec)
        assert 0 < sum(v) < len(v), spec
    near = bytearray([0x33] * 20)
    near[3], near[4] = 0x01, 0x00                     # across a word boundary: one zero byte, not two
    assert bytes(near) in slots(1) and not sv.accepts("score:zero-bytes>=2", bytes(near))
    assert bytes(20) in slots(1) and sv.accepts("score:zero-bytes>=2", bytes(20)) and not accepted(1, "score:zero-bytes>=2")[slots(1).index(bytes(20))]


@pytest.mark.parametrize("images", [1, 6])
@pytest.mark.parametrize("spec", SPECS)
def test_crafted_payloads_full_count(dev, spec, images):
    check(dev, spec, count=STRIDE, images=images, cap=STRIDE * images)


@pytest.mark.parametrize("count,images", [(8191, 1), (65, 1), (64, 1), (8191, 6), (65, 6), (64, 6), (1, 6)])
def test_ragged_counts_over_stale_high_scoring_payloads(dev, count, images):
    """The first crafted payloads are twenty times 0x5a or 0xa5 with one digit replaced: 19, 20 or 21 digits 5 (and a), so that even the
    first 64 slots hold hits and misses of these two specifications.  (A count of 1 on one image — one slot cannot hold a hit and a miss — is
    test_a_count_of_one_on_one_image.)"""
    for spec in ("score:count:5>=20", "score:zero-bytes>=0&count:a>=20"):
        check(dev, spec, count=count, images=images)


def test_a_count_of_one_on_one_image(dev):
    """One slot looked at: a hit under one specification, a miss under the other (each against the model)."""
    payloads = list(slots(1))
    for i in range(1, STRIDE):
        payloads[i] = STALE
    first = payloads[0]
    hit_spec = "score:count:%s>=1" % first.hex()[0]
    miss_spec = "score:zero-bytes>=19"
    assert sv.accepts(hit_spec, first) and not sv.accepts(miss_spec, first) and sv.accepts(miss_spec, STALE)
    for spec, want in ((hit_spec, 1), (miss_spec, 0)):
        verdict = [sv.accepts(spec, first)] + [True] * (STRIDE - 1)
        want_mask, want_hdr, want_recs, n = model(payloads, verdict, stride=STRIDE, count=1, images=1, entry=5, base=5, cap=256)
        assert n == want
        err, mask, hdr, recs = run(dev, sv.parse(spec), payload_array(payloads), count=1, images=1, entry=5, base=5, cap=256)
        assert err == 0 and np.array_equal(mask, want_mask) and hdr == want_hdr and np.array_equal(recs, want_recs)


def test_a_ring_that_fills_and_a_running_count_that_carries_over(dev):
    spec = "score:count:0>=2"
    n = sum(accepted(1, spec))
    assert n > 300
    check(dev, spec, count=STRIDE, images=1, entry=1000, base=1000, cap=256)           # more hits than the ring holds: the count still advances
    check(dev, spec, count=STRIDE, images=1, entry=0xFFFFFF00, base=0xFFFFFF00 - 7, cap=4096)   # seven records of an earlier dispatch, a count that wraps


@pytest.mark.parametrize("what", ["count past stride", "stride no multiple of 256", "no terms", "five terms", "unknown metric", "digit 16",
                                  "threshold beyond the range", "compaction over another geometry"])
def test_refused_launches_leave_the_poison_in_place(dev, what):
    kw = dict(stride=STRIDE, count=STRIDE, images=1)
    terms = [(sv.ZERO_BYTES, 0, 1)]
    if what == "count past stride":
        kw["count"] = STRIDE + 1
    elif what == "stride no multiple of 256":
        kw["stride"] = kw["count"] = 8192 + 64
    elif what == "no terms":
        terms = []
    elif what == "five terms":
        terms = [(sv.ZERO_BYTES, 0, 1)] * 5
    elif what == "unknown metric":
        terms = [(4, 0, 1)]
    elif what == "digit 16":
        terms = [(sv.COUNT_DIGIT, 16, 1)]
    elif what == "threshold beyond the range":
        terms = [(sv.LEADING_ZERO_BYTES, 0, 21)]
    else:
        kw["compact_stride"] = STRIDE * 2
    pay = payload_array((list(slots(1)) + [STALE] * 64)[:kw["stride"]])
    err, mask, hdr, recs = run(dev, terms, pay, entry=3, base=3, cap=256, **kw)
    assert err == HIP_ERROR_INVALID_VALUE
    assert (mask == np.uint64(MASK_POISON)).all() and hdr == (3, *HDR_REST) and (recs == REC_POISON).all()


# ---- launch_create2_score: one batch against the host's function, and its argument checks -------------------------------------------

C2_ALLOC, C2_BATCH = 1024, 512
C2_DEPLOYER, C2_HASH, C2_PREFIX = bytes(range(0x01, 0x15)), bytes(range(0x20, 0x40)), bytes(range(0x80, 0x98))
PAY_POISON = 0xCAFEF00D


class C2Job(ctypes.Structure):   # scoredev_c2job of tests/native/score_dev.hip, field by field
    _fields_ = [("batch", u32), ("compact_stride", u32), ("compact_images", u32), ("match_base", u32), ("match_cap", u32), ("n_terms", u32),
                ("terms", u32 * 12), ("header_in", u32 * 4), ("deployer", ctypes.c_uint8 * 20), ("init_code_hash", ctypes.c_uint8 * 32),
                ("salt_prefix", ctypes.c_uint8 * 24), ("first", ctypes.c_uint64), ("alloc_slots", u32), ("null_out", u32),
                ("payloads_in", vp), ("hits_in", vp), ("recs_in", vp),
                ("launch_error", ctypes.c_int32), ("header_out", u32 * 4), ("payloads_out", vp), ("hits_out", vp), ("recs_out", vp)]


def run_create2(dev, terms, *, batch=C2_BATCH, first=0, compact_stride=None, compact_images=1, null_out=False, entry=9, base=9, cap=256):
    assert dev.scoredev_c2job_size() == ctypes.sizeof(C2Job)
    pay_in = np.full((C2_ALLOC, 5), PAY_POISON, dtype=np.uint32)
    hits_in = np.full(C2_ALLOC // 64 + 64, MASK_POISON, dtype=np.uint64)
    recs_in = np.full((cap + 64, 10), REC_POISON, dtype=np.uint32)
    pay_out, hits_out, recs_out = np.zeros_like(pay_in), np.zeros_like(hits_in), np.zeros_like(recs_in)
    j = C2Job()
    j.batch, j.compact_stride, j.compact_images, j.match_base, j.match_cap = batch, batch if compact_stride is None else compact_stride, compact_images, base, cap
    j.n_terms = len(terms)
    j.terms = (u32 * 12)(*([v for t in terms for v in t] + [0] * 12)[:12])
    j.header_in = (u32 * 4)(entry, *HDR_REST)
    j.deployer = (ctypes.c_uint8 * 20)(*C2_DEPLOYER)
    j.init_code_hash = (ctypes.c_uint8 * 32)(*C2_HASH)
    j.salt_prefix = (ctypes.c_uint8 * 24)(*C2_PREFIX)
    j.first, j.alloc_slots, j.null_out = first, C2_ALLOC, int(null_out)
    j.payloads_in, j.hits_in, j.recs_in = ptr(pay_in), ptr(hits_in), ptr(recs_in)
    j.payloads_out, j.hits_out, j.recs_out = ptr(pay_out), ptr(hits_out), ptr(recs_out)
    rc = dev.scoredev_run_create2(ctypes.byref(j))
    assert rc == 0, "scoredev_run_create2: harness error %d" % rc
    return j.launch_error, pay_out, hits_out, tuple(j.header_out), recs_out


@pytest.mark.parametrize("first", [0, 2**64 - C2_BATCH])
def test_create2_score_launch_against_the_hosts_addresses(dev, first):
    """Hash, score, ballot store, the hit lanes' payloads only: everything behind the batch keeps its poison."""
    import vgen_amd as vg
    spec = "score:count:0>=3&zero-bytes>=0"
    want = [vg.create2_address(C2_DEPLOYER, C2_PREFIX + (first + i).to_bytes(8, "big"), C2_HASH) for i in range(C2_BATCH)]
    verdict = [sv.accepts(spec, p) for p in want]
    hit_slots = [i for i, v in enumerate(verdict) if v]
    assert 0 < len(hit_slots) < C2_BATCH
    err, pay, mask, hdr, recs = run_create2(dev, sv.parse(spec), first=first)
    assert err == 0
    want_mask = np.full(C2_ALLOC // 64 + 64, MASK_POISON, dtype=np.uint64)
    bits = np.array(verdict, dtype=bool)
    want_mask[:C2_BATCH // 64] = (bits.reshape(-1, 64) * (np.uint64(1) << np.arange(64, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(mask, want_mask)
    want_pay = np.full((C2_ALLOC, 5), PAY_POISON, dtype=np.uint32)
    arr = payload_array(want)
    want_pay[hit_slots] = arr[hit_slots]
    assert np.array_equal(pay, want_pay)              # payloads of exactly the hit lanes
    want_recs = np.full((256 + 64, 10), REC_POISON, dtype=np.uint32)
    for h, s in enumerate(hit_slots[:256]):
        want_recs[h] = [s, 0, *arr[s], 0, 0, 0]
    assert hdr == (9 + len(hit_slots), *HDR_REST) and np.array_equal(recs, want_recs)


@pytest.mark.parametrize("what", ["zero batch", "batch no multiple of 256", "no payload buffer", "no terms", "five terms", "unknown metric",
                                  "threshold beyond the range", "compaction over another stride", "compaction over six images"])
def test_refused_create2_score_launches_leave_the_poison_in_place(dev, what):
    kw, terms = {}, [(sv.ZERO_BYTES, 0, 1)]
    if what == "zero batch":
        kw.update(batch=0, compact_stride=0)
    elif what == "batch no multiple of 256":
        kw.update(batch=320)
    elif what == "no payload buffer":
        kw.update(null_out=True)
    elif what == "no terms":
        terms = []
    elif what == "five terms":
        terms = [(sv.ZERO_BYTES, 0, 1)] * 5
    elif what == "unknown metric":
        terms = [(7, 0, 1)]
    elif what == "threshold beyond the range":
        terms = [(sv.COUNT_DIGIT, 3, 41)]
    elif what == "compaction over another stride":
        kw.update(compact_stride=C2_BATCH * 2)
    else:
        kw.update(compact_images=6)
    err, pay, mask, hdr, recs = run_create2(dev, terms, **kw)
    assert err == HIP_ERROR_INVALID_VALUE
    assert (pay == PAY_POISON).all() and (mask == np.uint64(MASK_POISON)).all() and hdr == (9, *HDR_REST) and (recs == REC_POISON).all()
