"""The sequential scan's kernels - seq_fwd_kernel, seq_inv_kernel, seq_bwd_kernel in its shipped instantiations and
seq_hash_kernel (vgen_amd/csrc/device/kernels.hip) - on crafted offset tables.

Every other test reaches these kernels with the real table R_u and real base points Q_j, where the slow path of
fe_canonicalize_product (a weak product at or above p: one key in eight million, core/fe.h) and the parity flip of fe_parity_weak
practically never run inside them.  Here a test-only driver (tests/native/seq_dev.hip -> libseqdev.so, linked against the product's
own build/lib/device/kernels.o) hands vg::launch_seq_fwd / vg::launch_seq_bwd the tables of tests/seq_vectors.py, whose affine
additions land on the residues that force those paths - in waves with no, one, sixty-four equal and sixty-four mixed crafted lanes,
at the first, a middle and the last iteration of the key loop, for both signs - and the whole dump is compared, byte for byte, with
Python integers and oracle hashes.  No key of a dump is left out or masked.  Behind the scratch, the dump and the ring lie poisoned
guard words, which every test finds intact.  (tests/test_seq_vectors.py checks the vectors and their class counts on the CPU.)

Instantiations, dump mode: format 0 fused, its one-frame twin (lone), formats 0 and 2 split with 1, 4 and 2S keys per hash lane,
formats 2, 4, 5 and 6 fused, and the six-image kernels of formats 0, 2, 4, 5 and 6 (beta x and p - y images included); at 256 lanes
(one workgroup: seq_inv_kernel inverts one root in a ragged wave), 512 lanes with S = 16 and 65 workgroups with S = 2 (a second,
ragged workgroup of seq_inv_kernel).  Filter mode: format 0 fused, lone and split behind a hand-built one-test masked filter.
Launches the launchers must refuse run nothing."""
import ctypes
import os

import numpy as np
import pytest

import seq_vectors as sv
from conftest import locked_make

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_ERROR_INVALID_VALUE = 1
HDR_REST = (0x11111111, 0x22222222, 0x33333333)   # cap, clk_cycles, clk_ticks of the header on entry
DEVF_MASKED = 2

u32, vp = ctypes.c_uint32, ctypes.c_void_p


class Job(ctypes.Structure):   # seqdev_job of tests/native/seq_dev.hip, field by field
    _fields_ = [("fmt", u32), ("lanes", u32), ("s", u32), ("lone", u32), ("endo", u32), ("split", u32), ("hash_kpl", u32),
                ("skip_fwd", u32), ("match_base", u32), ("match_cap", u32), ("header_in", u32 * 4),
                ("rtab", vp), ("q", vp), ("filter", vp),
                ("launch_error", ctypes.c_int32), ("failed_stage", u32), ("scratch_words", u32), ("dump_words", u32),
                ("header_out", u32 * 4), ("scratch_out", vp), ("dump_out", vp), ("recs_out", vp)]


class FilterTest(ctypes.Structure):   # DevFilterTest (device/device_types.h)
    _fields_ = [("a", u32 * 8), ("b", u32 * 8), ("chk_mask", u32), ("chk_value", u32)]


class Filter(ctypes.Structure):       # DevFilter
    _fields_ = [("kind", u32), ("count", u32), ("flags", u32), ("witver", u32), ("chk_lut", vp), ("chk_base", u32),
                ("dfa_bytes", u32), ("dfa_blob", vp), ("tests", FilterTest * 64)]


@pytest.fixture(scope="module")
def dev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "libseqdev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libseqdev.so"))
    assert lib.seqdev_job_size() == ctypes.sizeof(Job) and lib.seqdev_filter_size() == ctypes.sizeof(Filter)
    assert lib.seqdev_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    lib.seqdev_scratch_words.restype = lib.seqdev_dump_words.restype = ctypes.c_uint64
    lib.seqdev_guard_words.restype = lib.seqdev_poison.restype = u32
    return lib


def ptr(a):
    return a.ctypes.data_as(vp)


class Out:
    pass


def launch(dev, *, fmt, lanes, S, rtab, q, lone=0, endo=0, split=0, kpl=0, skip_fwd=0, filt=None, base=0, cap=0):
    """One seqdev_run.  Returns the launch error, the scratch, and the dump or the header and the cap + guard records - each array
    with its guard words, split off here - and what a poisoned word looks like."""
    guard, poison = dev.seqdev_guard_words(), dev.seqdev_poison()
    assert rtab.dtype == np.uint32 and rtab.flags.c_contiguous and rtab.shape == (18, lanes)
    assert q.dtype == np.uint32 and q.flags.c_contiguous and q.shape == (S, 18)
    sw, dw = dev.seqdev_scratch_words(lanes, S, split), dev.seqdev_dump_words(lanes, S, endo)
    o = Out()
    scratch = np.zeros(sw + guard, dtype=np.uint32)
    dump = np.zeros(dw + guard, dtype=np.uint32)
    recs = np.zeros((cap + guard // 8, 10), dtype=np.uint32)
    j = Job(fmt=fmt, lanes=lanes, s=S, lone=lone, endo=endo, split=split, hash_kpl=kpl, skip_fwd=skip_fwd, match_base=base,
            match_cap=cap, header_in=(u32 * 4)(base, *HDR_REST), rtab=ptr(rtab), q=ptr(q), scratch_out=ptr(scratch))
    if filt is not None:
        j.filter, j.recs_out = ctypes.addressof(filt), ptr(recs)
    else:
        j.dump_out = ptr(dump)
    rc = dev.seqdev_run(ctypes.byref(j))
    assert rc == 0, f"seqdev_run failed: {rc}"
    assert (j.scratch_words, j.dump_words) == (sw, dw)
    o.err, o.stage, o.header, o.poison = j.launch_error, j.failed_stage, list(j.header_out), poison
    o.scratch, o.scratch_guard = scratch[:sw], scratch[sw:]
    o.dump, o.dump_guard = dump[:dw], dump[dw:]
    o.recs, o.recs_guard = recs[:cap], recs[cap:]
    o.guards_intact = bool((o.scratch_guard == poison).all()) and \
        (bool((o.dump_guard == poison).all()) if filt is None else bool((o.recs_guard == poison).all()))
    return o


def run(dev, cfg, **kw):
    v = sv.vectors(cfg["geometry"], bool(cfg["endo"]))
    return v, launch(dev, fmt=cfg["fmt"], lanes=v.lanes, S=v.S, rtab=v.rtab, q=v.qlimbs, lone=cfg["lone"], endo=cfg["endo"],
                     split=cfg["split"], kpl=cfg["kpl"], **kw)


# ---- dump mode --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", sv.DUMP_CONFIGS, ids=[c["id"] for c in sv.DUMP_CONFIGS])
def test_dump_equals_the_reference(dev, cfg):
    v, o = run(dev, cfg)
    assert o.err == 0, (o.err, o.stage)
    want = sv.dump_of(cfg["geometry"], bool(cfg["endo"]), cfg["fmt"])
    got = o.dump.view(np.uint8).reshape(-1, 20)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    n = sv.census(v)
    print(f"{cfg['id']}: {want.shape[0]} payloads of {v.n} keys compared; keys of class a / b on x3: {n['x3 a']} / {n['x3 b']}, "
          f"on y3: {n['y3 a']} / {n['y3 b']}, of class d: {n['d']}; {bad.size} differ")
    if bad.size:
        rare = set(sv.rare_keys(v))
        i = int(bad[0])
        key = i % v.n
        hit = next((c for c in v.crafted if c.index == key), None)
        raise AssertionError((cfg["id"], "slot", i, "image", i // v.n, "key", key, got[i].tobytes().hex(), want[i].tobytes().hex(),
                              f"{bad.size} slots differ, {sum(1 for b in bad if int(b) % v.n in rare)} of them keys of classes a and b",
                              hit and (hit.u, hit.j, hit.sgn, hit.cx, hit.cy, hex(hit.T), hex(hit.T2))))
    assert o.guards_intact, "guard words written"
    if not cfg["split"]:   # (the scratch has exactly the regions the dispatch uses: the fused forms leave no xs)
        assert o.scratch.size == v.S * 9 * v.lanes + (v.lanes // 256) * 9 * 256 + 9 * (v.lanes // 256)


# ---- filter mode ------------------------------------------------------------------------------------------------------------

def nibble_filter(value):
    f = Filter(kind=DEVF_MASKED, count=1)
    f.tests[0].a[0], f.tests[0].b[0] = 0xF0000000, value << 28   # H[0] = the payload's first four bytes, big-endian
    return f


@pytest.mark.parametrize("cfg", sv.FILTER_CONFIGS, ids=[c["id"] for c in sv.FILTER_CONFIGS])
def test_filter_records_equal_the_reference(dev, cfg):
    v = sv.vectors(cfg["geometry"])
    want = sv.dump_of(cfg["geometry"], False, 0)
    nibble, rare_hits = sv.filter_nibble(cfg["geometry"])
    assert rare_hits >= 8
    hits = np.flatnonzero(want[:, 0] >> 4 == nibble)
    cap = hits.size + 64
    base = 0xFFFFFFF0 if cfg["split"] else 12345   # (a running count that wraps during the dispatch)
    v, o = run(dev, cfg, filt=nibble_filter(nibble), base=base, cap=cap)
    assert o.err == 0, (o.err, o.stage)
    assert (o.header[0] - base) % (1 << 32) == hits.size, (o.header, hits.size)
    assert o.header[1] == HDR_REST[0]   # (clk_cycles / clk_ticks: the first wave adds its clock sample)
    recs = o.recs[:hits.size]
    assert (recs[:, 1] == 0).all() and (recs[:, 7:] == 0).all()
    got = {(int(r[0]), r[2:7].tobytes()) for r in recs}
    ref = {(int(i), want[i].tobytes()) for i in hits}
    assert len(got) == hits.size and got == ref, (len(got), len(got - ref), len(ref - got))
    assert (o.recs[hits.size:] == o.poison).all(), "records beyond the hit count written"
    assert o.guards_intact, "guard words written"
    rare = set(sv.rare_keys(v))
    assert sum(1 for i in hits if int(i) in rare) == rare_hits
    print(f"{cfg['id']}: {v.n} keys, top four bits {nibble:#x}: {hits.size} records, {rare_hits} of them keys of classes a and b")


# ---- launches the launchers refuse --------------------------------------------------------------------------------------------

def untouched(o):
    return o.err == HIP_ERROR_INVALID_VALUE and bool((o.scratch == o.poison).all()) and bool((o.dump == o.poison).all()) and o.guards_intact


def random_job(lanes, S):
    rs = np.random.RandomState(lanes * 100 + S)
    return dict(lanes=lanes, S=S, rtab=rs.randint(1, 1 << 24, size=(18, lanes)).astype(np.uint32),
                q=rs.randint(1, 1 << 24, size=(S, 18)).astype(np.uint32))


def test_refused_launches_run_nothing(dev):
    for lanes, S in ((384, 8), (128, 8), (256, 1), (256, 17)):
        for split in (0, 1):
            o = launch(dev, fmt=0, split=split, kpl=2 if split else 0, **random_job(lanes, S))
            assert untouched(o) and o.stage == 1, (lanes, S, split, o.err, o.stage)
        o = launch(dev, fmt=0, skip_fwd=1, **random_job(lanes, S))   # the second launcher checks for itself
        assert untouched(o) and o.stage == 2, (lanes, S, o.err, o.stage)
    # split, with keys per hash lane that do not divide 2S = 16 (or are 0): the second launcher refuses before it starts anything ...
    for fmt in (0, 2):
        for kpl in (0, 3, 5, 32):
            o = launch(dev, fmt=fmt, split=1, kpl=kpl, skip_fwd=1, **random_job(256, 8))
            assert untouched(o) and o.stage == 2, (fmt, kpl, o.err, o.stage)
    # ... and behind a first half that ran (it wrote pre, tree and root: 8 * 9 * 256 + 9 * 256 + 9 words) xs and the dump stay as they were
    v = sv.vectors("g256")
    first_half = v.S * 9 * v.lanes + 9 * 256 + 9
    o = launch(dev, fmt=0, split=1, kpl=3, lanes=v.lanes, S=v.S, rtab=v.rtab, q=v.qlimbs)
    assert o.err == HIP_ERROR_INVALID_VALUE and o.stage == 2
    assert (o.scratch[first_half:] == o.poison).all() and (o.dump == o.poison).all() and o.guards_intact
    assert o.scratch.size == first_half + 9 * v.n
    # an unknown format
    o = launch(dev, fmt=9, skip_fwd=1, **random_job(256, 8))
    assert untouched(o) and o.stage == 2
    # the same arguments with the fault taken out do run (the poison would otherwise prove nothing)
    o = launch(dev, fmt=0, split=1, kpl=2, lanes=v.lanes, S=v.S, rtab=v.rtab, q=v.qlimbs)
    assert o.err == 0 and (o.dump.view(np.uint8).reshape(-1, 20) == sv.dump_of("g256", False, 0)).all() and o.guards_intact
    assert (o.scratch[first_half:] != o.poison).sum() >= 9 * v.n - 8   # xs was written (a word of x may equal the poison by chance)
