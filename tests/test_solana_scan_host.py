"""The host side of the Solana format (format 12) without a device: cabi.cpp and the scan loop of scanner.cpp over the CPU stand-in of
the runtime with Solana contexts added (tests/native/solana_rt.cpp beside fake_rt.cpp, built into libvgen_fake_solana.so by
tests/native/solana.mk), driven through the C ABI by a second instance of vgen_amd/api.py bound to that library.

Checked: dumps and records of the stand-in's dispatches, seeded scans against the reference's walk of the candidate stream in
order (tests/solana_vectors.py: hashlib and Python integers, nothing of the code under test), count / stop flag / max_batches,
disjoint streams of two contexts through vgen_scan_multi, and every refusal a context can give."""
import ctypes
import functools
import importlib.util
import os
import sys

import pytest

from tests import solana_vectors as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = sv.FMT_SOLANA
SO = os.path.join(ROOT, "tests", "native", "libvgen_fake_solana.so")
BATCH = 8192
SEED = 0x534F4C
E_INVALID, E_UNSUPPORTED = -1, -8


@pytest.fixture(scope="module")
def vf():
    """vgen_amd/api.py over the stand-in's library (the mechanism of tests/conftest.py: hooks_api, with another library)."""
    assert os.path.exists(SO), f"{SO} not built (make -C tests/native -f solana.mk, or __graft_entry__.build())"
    spec = importlib.util.spec_from_file_location("vgen_amd_fake_solana_api", os.path.join(ROOT, "vgen_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    mod._SO_OVERRIDE = SO
    sys.modules["vgen_amd_fake_solana_api"] = mod
    spec.loader.exec_module(mod)
    assert mod.library_path() == SO
    return mod


def runner(vf, frames=2):
    return vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=frames, timing=False)


@functools.lru_cache(maxsize=None)
def stream_strings(stream, batch_no):
    return [sv.address(p) for p in sv.stream_payloads(SEED, stream, batch_no * BATCH, BATCH)]


def test_dispatches_of_the_stand_in(vf):
    r = runner(vf)
    r.set_filter(None)
    r.dispatch_random(SEED, 0, 0, 0)
    blob, _, tested = r.await_result(0)
    want = sv.stream_payloads(SEED, 0, 0, BATCH)
    assert tested == BATCH and blob[:32 * BATCH] == b"".join(want)
    prefix = stream_strings(0, 0)[5000][:2]
    r.set_filter(vf.Pattern("^" + prefix, False, FMT))
    r.dispatch_random(SEED, 0, 0, 1)
    recs, n, tested = r.await_result(1)
    assert recs == [(i, want[i]) for i, s in enumerate(stream_strings(0, 0)) if s.startswith(prefix)] and n == len(recs) >= 1
    seeds = [bytes([i]) * 32 for i in range(65)]
    r.set_filter(None)
    r.dispatch_keys(seeds, 0)
    blob, _, tested = r.await_result(0)
    assert tested == 65 and blob[:32 * 65] == b"".join(sv.public_key(s) for s in seeds)
    r.close()


def walk(stream, accept, count):
    out, b = [], 0
    while len(out) < count:
        out += [(b * BATCH + i, s) for i, s in enumerate(stream_strings(stream, b)) if accept(s)]
        b += 1
    return out[:count], b


def test_a_seeded_scan_is_the_references_walk_in_order(vf):
    r = runner(vf)
    prefix = stream_strings(0, 0)[777][:2]
    want, batches = walk(0, lambda s: s.startswith(prefix), 6)
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=6, seed=SEED), r)
    assert [(m.hex, m.address) for m in res.matches] == [(sv.stream_seed(SEED, 0, i).hex(), s) for i, s in want]
    assert all(m.wif == m.hex and int(m.format) == FMT for m in res.matches)
    assert res.operations % BATCH == 0 and res.operations >= batches * BATCH
    # the flag is implied and accepted: the same results with it
    res2 = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=6, seed=SEED, random_keys=True), r)
    assert [m.hex for m in res2.matches] == [m.hex for m in res.matches]
    # a suffix, and a pattern the host filters from dumps (device kind 0)
    suffix = stream_strings(0, 0)[4242][-2:]
    want, _ = walk(0, lambda s: s.endswith(suffix), 3)
    res = vf.scan_gpu_with_runner(suffix + "$", vf.ScanConfig(format=FMT, count=3, seed=SEED), r)
    assert [m.address for m in res.matches] == [s for _, s in want]
    inner = stream_strings(0, 0)[99][10:13]
    want, _ = walk(0, lambda s: inner in s, 4)
    res = vf.scan_gpu_with_runner(inner, vf.ScanConfig(format=FMT, count=4, seed=SEED), r)
    assert [m.address for m in res.matches] == [s for _, s in want]
    r.close()


def test_max_batches_and_the_stop_flag(vf):
    r = runner(vf)
    prefix = stream_strings(0, 0)[777][:2]
    everything = [s for s in stream_strings(0, 0) if s.startswith(prefix)]
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=None, seed=SEED, max_batches=1), r)
    assert [m.address for m in res.matches] == everything and res.operations == BATCH
    stop = ctypes.c_int32(1)
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=None, seed=SEED), r, stop=stop)
    assert res.matches == [] and res.operations == 0
    r.close()


def test_two_contexts_draw_disjoint_streams(vf):
    a, b = runner(vf), runner(vf)
    prefix = stream_strings(0, 0)[777][:1]
    res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=None, seed=SEED, max_batches=1), [a, b])
    want = {s for st in (0, 1) for s in stream_strings(st, 0) if s.startswith(prefix)}
    assert {m.address for m in res.matches} == want and len(res.matches) == len(want) and res.operations == 2 * BATCH
    hexes = {m.hex for m in res.matches}
    assert sv.stream_seed(SEED, 1, next(i for i, s in enumerate(stream_strings(1, 0)) if s.startswith(prefix))).hex() in hexes
    a.close()
    b.close()


@pytest.mark.parametrize("every,ends_in_dumps", [(8, False), (2, True)], ids=["ring-grows", "switch-to-dumps"])
def test_a_ring_overflow_restarts_the_batch(vf, every, ends_in_dumps):
    """The compiler's estimates are exact for this format, so a scan sizes its ring up front; the stand-in is told to report every
    `every`-th slot besides the filter's candidates (a legitimate superset: the host confirms).  1024 candidates overflow the 256-record
    ring: the loop drains, grows the ring to 4096 and redoes the batch; 4096 candidates would need more than half a record per key:
    it switches to host-filtered dumps.  Either way the results are the reference's walk of the stream, in order, nothing twice."""
    import ctypes as ct
    r = vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=3, match_cap=256, timing=False)
    prefix = stream_strings(0, 0)[777][:2]
    count = sum(1 for s in stream_strings(0, 0) if s.startswith(prefix)) + 2    # past the first batch: the redone batch is followed by more
    want, batches = walk(0, lambda s: s.startswith(prefix), count)
    assert batches >= 2
    vf._L.vgen_fake_solana_loosen.argtypes = [ct.c_uint32]
    vf._L.vgen_fake_solana_loosen(every)
    try:
        res = vf.scan_gpu_with_runner("^" + prefix, vf.ScanConfig(format=FMT, count=count, seed=SEED), r)
    finally:
        vf._L.vgen_fake_solana_loosen(0)
    assert [(m.hex, m.address) for m in res.matches] == [(sv.stream_seed(SEED, 0, i).hex(), s) for i, s in want]
    cap = ct.c_uint32()
    vf._L.vgen_get_info(r._h, None, None, ct.byref(cap))
    assert cap.value == (256 if ends_in_dumps else 4096)                     # the ring grew, or was left for dumps
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
    a.close()
    b.close()


def test_refusals(vf):
    r = runner(vf)
    with pytest.raises(vf.VgenError) as e:
        r.dispatch(1, 0)
    assert e.value.status == E_UNSUPPORTED and "no walk" in str(e.value)
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
    for fmt in (8, 9, 11):
        with pytest.raises(vf.VgenError) as e:
            vf.GpuRunner(batch_size=BATCH, fmt=fmt, device=0, frames=2, timing=False)
        assert e.value.status == E_INVALID
    r.close()
