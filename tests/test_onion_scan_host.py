"""The host side of the onion format (format 13) without a device: cabi.cpp and the scan loop of scanner.cpp over the CPU stand-in of
the runtime with onion contexts added (tests/native/onion_rt.cpp beside fake_rt.cpp, built into libvgen_fake_onion.so by
tests/native/onion.mk), driven through the C ABI by a second instance of vgen_amd/api.py bound to that library.  The stand-in computes a
dispatch with the host build of the kernels' pair formulas (core/ed_walk.h), so the slot layout of the walk is checked here too.

Checked: dumps and records of the stand-in's dispatches, a seeded scan against the reference's walk in order (tests/onion_vectors.py:
hashlib and Python integers, nothing of the code under test), two shards walking from two bases, the VGEN_E_RANGE base, and every
refusal a context can give."""
import functools
import importlib.util
import os
import sys

import pytest

from tests import onion_vectors as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = ov.FMT_ONION
SO = os.path.join(ROOT, "tests", "native", "libvgen_fake_onion.so")
BATCH = 8192
SEED = 0x4F4E494F4E
E_INVALID, E_RANGE, E_STATE, E_UNSUPPORTED = -1, -7, -5, -8


@pytest.fixture(scope="module")
def vf():
    """vgen_amd/api.py over the stand-in's library (the mechanism of tests/conftest.py: hooks_api, with another library)."""
    assert os.path.exists(SO), f"{SO} not built (make -C tests/native -f onion.mk, or __graft_entry__.build())"
    spec = importlib.util.spec_from_file_location("vgen_amd_fake_onion_api", os.path.join(ROOT, "vgen_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    mod._SO_OVERRIDE = SO
    sys.modules["vgen_amd_fake_onion_api"] = mod
    spec.loader.exec_module(mod)
    assert mod.library_path() == SO
    return mod


def runner(vf, frames=2):
    return vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=frames, timing=False)


@functools.lru_cache(maxsize=None)
def batch_payloads(stream, batch_no):
    return ov.walk_payloads(ov.base_scalar(SEED, stream), batch_no * BATCH, BATCH)


@functools.lru_cache(maxsize=None)
def batch_strings(stream, batch_no):
    return [ov.address(p) for p in batch_payloads(stream, batch_no)]


def key_hex(stream, index):
    return (ov.base_scalar(SEED, stream) + 8 * index).to_bytes(32, "little").hex()


def test_status_codes_are_the_headers(vf):
    hdr = open(os.path.join(ROOT, "include", "vgen_hip.h")).read()
    for name, value in (("VGEN_E_INVALID", E_INVALID), ("VGEN_E_RANGE", E_RANGE), ("VGEN_E_STATE", E_STATE), ("VGEN_E_UNSUPPORTED", E_UNSUPPORTED)):
        assert "%s = %d" % (name, value) in hdr, name


def test_dispatches_of_the_stand_in(vf):
    r = runner(vf)
    base = ov.base_scalar(SEED, 0)
    assert vf.onion_base(SEED, 0) == base.to_bytes(32, "little")
    r.set_filter(None)
    r.dispatch_onion(base, 0, 0)
    blob, _, tested = r.await_result(0)
    want = batch_payloads(0, 0)
    assert tested == BATCH and blob[:32 * BATCH] == b"".join(want)
    prefix = batch_strings(0, 0)[5000][:2]
    r.set_filter(vf.Pattern("^" + prefix, False, FMT))
    r.dispatch_onion(base, 0, 1)
    recs, n, tested = r.await_result(1)
    assert recs == [(i, want[i]) for i, s in enumerate(batch_strings(0, 0)) if s.startswith(prefix)] and n == len(recs) >= 1
    # base 0: slot 0 has no key
    r.set_filter(None)
    r.dispatch_onion(0, 0, 0)
    blob, _, _ = r.await_result(0)
    assert blob[:32] == bytes(32) and blob[32:32 * BATCH] == b"".join(ov.walk_payloads(0, 0, BATCH)[1:])
    r.close()


def walk(stream, accept, count):
    out, b = [], 0
    while len(out) < count:
        out += [(b * BATCH + i, s) for i, s in enumerate(batch_strings(stream, b)) if accept(s)]
        b += 1
    return out[:count], b


def test_a_seeded_scan_is_the_references_walk_in_order(vf):
    r = runner(vf)
    prefix = batch_strings(0, 0)[777][:2]
    want, batches = walk(0, lambda s: s.startswith(prefix), 6)
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=6, seed=SEED), r)
    assert [(m.hex, m.address) for m in res.matches] == [(key_hex(0, i), s) for i, s in want]
    assert all(m.wif == m.hex and int(m.format) == FMT for m in res.matches)
    assert res.operations % BATCH == 0 and res.operations >= batches * BATCH
    # a suffix: filtered by the host from dumps (device kind 0)
    suffix = batch_strings(0, 0)[4242][-4:]
    want, _ = walk(0, lambda s: s.endswith(suffix), 1)
    res = vf.scan_gpu_with_runner(suffix + "$", vf.ScanConfig(format=FMT, count=1, seed=SEED), r)
    assert [(m.hex, m.address) for m in res.matches] == [(key_hex(0, i), s) for i, s in want]
    r.close()


def test_two_shards_walk_from_two_bases(vf):
    a, b = runner(vf), runner(vf)
    assert ov.base_scalar(SEED, 0) != ov.base_scalar(SEED, 1)
    prefix = batch_strings(0, 0)[777][:1]
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=None, seed=SEED, max_batches=1), [a, b])
    want = {(key_hex(st, i), s) for st in (0, 1) for i, s in enumerate(batch_strings(st, 0)) if s.startswith(prefix)}
    assert {(m.hex, m.address) for m in res.matches} == want and len(res.matches) == len(want) and res.operations == 2 * BATCH
    assert any(h == key_hex(1, i) for h, _ in want for i in range(BATCH) if batch_strings(1, 0)[i].startswith(prefix))
    a.close()
    b.close()


def test_the_range_end_and_a_base_off_the_grid(vf):
    r = runner(vf)
    r.set_filter(None)
    last = 2**255 - 8 * BATCH            # base + 8 (BATCH - 1) = 2^255 - 8: the last dispatch there is
    r.dispatch_onion(last, 0, 0)
    blob, _, _ = r.await_result(0)
    assert blob[32 * (BATCH - 1):32 * BATCH] == ov.point_bytes(2**255 - 8)
    for base, first in ((last + 8, 0), (last, 1), (2**255 - 8, 0), (2**254, 2**64 - 1), (2**255, 0)):
        with pytest.raises(vf.VgenError) as e:
            r.dispatch_onion(base, first, 0)
        assert e.value.status == E_RANGE
        with pytest.raises(vf.VgenError) as e:   # nothing was enqueued
            r.await_result(0)
        assert e.value.status == E_STATE
    for base in (1, 4, 2**254 + 7):
        with pytest.raises(vf.VgenError) as e:
            r.dispatch_onion(base, 0, 0)
        assert e.value.status == E_INVALID
    r.close()


def test_mixed_formats_are_refused(vf):
    a = runner(vf)
    b = vf.GpuRunner(batch_size=BATCH, fmt=vf.AddressFormat.P2pkh, device=0, frames=2, timing=False)
    with pytest.raises(vf.VgenError) as e:
        vf.scan_gpu_with_runner("^a", vf.ScanConfig(format=FMT, count=1), b)
    assert e.value.status == E_INVALID
    with pytest.raises(vf.VgenError) as e:
        vf.scan_gpu_with_runner("^1", vf.ScanConfig(format=vf.AddressFormat.P2pkh, count=1), a)
    assert e.value.status == E_INVALID
    with pytest.raises(vf.VgenError) as e:
        b.dispatch_onion(8, 0, 0)
    assert e.value.status == E_INVALID
    a.close()
    b.close()


def test_refusals(vf):
    r = runner(vf)
    with pytest.raises(vf.VgenError) as e:
        r.dispatch(1, 0)
    assert e.value.status == E_UNSUPPORTED and "vgen_dispatch_onion" in str(e.value)
    with pytest.raises(vf.VgenError) as e:
        r.dispatch_keys([1, 2], 0)
    assert e.value.status == E_UNSUPPORTED
    for seed in (5, bytes(24)):
        with pytest.raises(vf.VgenError) as e:
            r.dispatch_random(seed, 0, 0, 0)
        assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vf.VgenError) as e:
        vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=2, endo=True, timing=False)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vf.VgenError) as e:
        r.set_base(bytes.fromhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"))
    assert e.value.status == E_UNSUPPORTED
    for cfg in (vf.ScanConfig(format=FMT, count=1, start=5), vf.ScanConfig(format=FMT, count=1, start=5, end=9),
                vf.ScanConfig(format=FMT, count=1, checkpoint_path="/nonexistent/never-written")):
        with pytest.raises(vf.VgenError) as e:
            vf.scan_gpu_with_runner("^a", cfg, r)
        assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vf.VgenError) as e:
        vf.scan_gpu_with_runner("score:zero-bytes>=2", vf.ScanConfig(format=FMT, count=1), r)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vf.VgenError) as e:
        vf.PatternList(["^aa", "^bb"], False, FMT)
    assert e.value.status == E_UNSUPPORTED
    r.close()
