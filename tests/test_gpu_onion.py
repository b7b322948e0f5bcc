"""The onion format (VGEN_FMT_ONION, format 13) on the MI355X: the walk's kernels (onion_points_kernel, onion_fwd_kernel,
onion_bwd_kernel in its dump and filter forms) behind vgen_dispatch_onion, the compaction behind them, the device build of the format's
core functions (tests/native/onion_dev.hip), the scan loop over the kernels and the command line.

Smallest shapes that still have the structure: batch 8192 (128 lanes of 64 keys: two live waves of a workgroup of eight, whose other
six only take part in the inversion tree), two frames.  Expected values are those of tests/onion_vectors.py - Python integers over
tests/solana_vectors.py, whose multiplication is checked against OpenSSL - computed once and shared; the digest of each dump is the
golden one of tests/golden/onion.json.  Every test here fails on a library without the format (vgen_create: VGEN_E_INVALID)."""
import ctypes
import functools
import hashlib
import json
import os
import random
import re

import pytest

from tests import onion_vectors as ov
import vgen_amd as vg
from vgen_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = ov.FMT_ONION
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "onion.json")))
BATCH = 8192
KEY_INDEX = 5000
E_INVALID, E_STATE, E_RANGE, E_UNSUPPORTED = -1, -5, -7, -8
P = ov.P


@pytest.fixture(scope="module")
def runner():
    r = vg.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=2)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def expected(which):
    d = FIXTURE["dumps"][which]
    assert FIXTURE["batch"] == BATCH
    return ov.walk_payloads(int(d["base"], 16), d["first"], BATCH)


@functools.lru_cache(maxsize=None)
def expected_strings(which):
    return [ov.address(p) for p in expected(which)]


def dump(runner, base, first, frame=0):
    runner.set_filter(None)
    runner.dispatch_onion(base, first, frame)
    blob, _, tested = runner.await_result(frame)
    assert tested == BATCH and len(blob) == BATCH * 32
    return blob


@pytest.mark.parametrize("which", [0, 1, 2], ids=["first-0", "first-2^32-100", "rippling-base"])
def test_dump_equals_the_reference_and_the_golden_digest(runner, which):
    d = FIXTURE["dumps"][which]
    assert d["first"] == (0, 2**32 - 100, 0)[which]
    if which == 2:
        assert int(d["base"], 16) & (2**224 - 1) == 2**224 - 8
    blob = dump(runner, int(d["base"], 16), d["first"])
    want = expected(which)
    bad = [i for i in range(BATCH) if blob[32 * i:32 * i + 32] != want[i]]
    assert not bad, (len(bad), bad[:8])
    assert hashlib.sha256(blob).hexdigest() == d["sha256"] == hashlib.sha256(b"".join(want)).hexdigest()


def test_base_zero_has_no_key_in_slot_zero(runner):
    blob = dump(runner, 0, 0, frame=1)
    assert blob[:32] == bytes(32)
    want = ov.walk_payloads(0, 0, BATCH)
    assert want[1] == ov.point_bytes(8) and blob[32:] == b"".join(want[1:])
    # ... and in the filter form slot 0 never hits, not even under match-all
    runner.set_filter(vg.Pattern(".", False, FMT))
    runner.dispatch_onion(0, 0, 1)
    recs, n, _ = runner.await_result(1)
    assert n == BATCH - 1 and recs[0] == (1, want[1])


def test_the_range_end_enqueues_nothing(runner):
    runner.set_filter(None)
    for base, first in ((2**255 - 8 * BATCH + 8, 0), (2**255 - 8 * BATCH, 1), (2**255 - 8, 0)):
        with pytest.raises(vg.VgenError) as e:
            runner.dispatch_onion(base, first, 0)
        assert e.value.status == E_RANGE
        with pytest.raises(vg.VgenError) as e:
            runner.await_result(0)
        assert e.value.status == E_STATE
    with pytest.raises(vg.VgenError) as e:
        runner.dispatch_onion(2**254 + 4, 0, 0)
    assert e.value.status == E_INVALID
    blob = dump(runner, 2**255 - 8 * BATCH, 0)     # the last dispatch there is
    assert blob[-32:] == ov.point_bytes(2**255 - 8) and blob[:32] == ov.point_bytes(2**255 - 8 * BATCH)


def filtered(runner, pattern, ci=False, which=0):
    d = FIXTURE["dumps"][which]
    p = vg.Pattern(pattern, ci, FMT)
    runner.set_filter(p)
    runner.dispatch_onion(int(d["base"], 16), d["first"], 1)
    recs, n, tested = runner.await_result(1)
    assert tested == BATCH and n == len(recs)
    return p, recs


@pytest.mark.parametrize("length,ci", [(1, False), (2, False), (3, False), (3, True), (5, False), (7, False)])
def test_prefix_patterns(runner, length, ci):
    prefix = expected_strings(0)[KEY_INDEX][:length]
    p, recs = filtered(runner, "^" + prefix, ci)
    assert p.device_kind == 2
    want, strings = expected(0), expected_strings(0)
    hits = [i for i, s in enumerate(strings) if s.startswith(prefix)]
    idx = [i for i, _ in recs]
    assert KEY_INDEX in hits and idx == hits                            # a prefix's mask is exact (-i changes nothing: one case)
    assert idx == sorted(idx) and len(set(idx)) == len(idx)
    assert all(pl == want[i] for i, pl in recs)                         # the full 32 bytes, the sign bit included
    assert {pl[31] >> 7 for _, pl in recs} == {0, 1} or length > 1      # (both signs occur among a one-character prefix's ~256 hits)


def test_match_all_reports_every_key_and_the_first_records(runner):
    d = FIXTURE["dumps"][0]
    pat = vg.Pattern(".", False, FMT)
    assert pat.device_kind == 3
    api._check(api._L.vgen_set_match_cap(runner._h, 256), runner._h)
    runner.match_cap = 256
    try:
        runner.set_filter(pat)
        runner.dispatch_onion(int(d["base"], 16), d["first"], 1)
        recs, n, tested = runner.await_result(1)
        assert n == BATCH and tested == BATCH and len(recs) == 256
        assert recs == [(i, expected(0)[i]) for i in range(256)]
    finally:
        api._check(api._L.vgen_set_match_cap(runner._h, 4096), runner._h)
        runner.match_cap = 4096


SCAN_SEED = 77


@functools.lru_cache(maxsize=None)
def scan_strings():
    return [ov.address(p) for p in ov.walk_payloads(ov.base_scalar(SCAN_SEED, 0), 0, BATCH)]


def test_seeded_scan_equals_the_references_first_five(runner):
    strings = scan_strings()
    prefix = strings[123][:2]
    want = [i for i, s in enumerate(strings) if s.startswith(prefix)][:5]
    assert len(want) == 5                                               # (a two-character prefix: ~8 of 8192)
    res = vg.scan_gpu_with_runner("^" + prefix, vg.ScanConfig(format=FMT, count=5, seed=SCAN_SEED), runner)
    base = ov.base_scalar(SCAN_SEED, 0)
    assert [m.hex for m in res.matches] == [(base + 8 * i).to_bytes(32, "little").hex() for i in want]
    for m, i in zip(res.matches, want):
        assert m.address == strings[i] and m.wif == m.hex and int(m.format) == FMT


def test_command_line_search_and_its_writers(tmp_path):
    """`vgen-hip generate -f onion --seed`: the reference's first matches of stream 0, as jsonl (secret_key_hex of 128 digits,
    public_key_hex, no wif), as the three files of a hidden-service directory (modes 0700 / 0600) and as text."""
    import stat
    import subprocess
    cli = os.path.join(ROOT, "vgen_amd", "vgen-hip")
    strings = scan_strings()
    prefix = strings[123][:2]
    want = [i for i, s in enumerate(strings) if s.startswith(prefix)][:2]
    base = ov.base_scalar(SCAN_SEED, 0)
    common = ["generate", "-f", "onion", "-p", "^" + prefix, "--seed", str(SCAN_SEED), "-c", "2", "--gpu-batch-size", str(BATCH), "--frames", "2", "-q"]
    r = subprocess.run([cli, *common, "-o", "jsonl", "--key-dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(rows) == 2
    for row, i in zip(rows, want):
        a = base + 8 * i
        pub = ov.point_bytes(a)
        assert row["address"] == strings[i] and row["secret_key_hex"] == ov.expand(a).hex() and len(row["secret_key_hex"]) == 128
        assert row["public_key_hex"] == pub.hex() and "wif" not in row and row["format"] == "Tor v3 onion"
        d = tmp_path / (strings[i] + ".onion")
        assert stat.S_IMODE(d.stat().st_mode) == 0o700
        assert (d / "hs_ed25519_secret_key").read_bytes() == b"== ed25519v1-secret: type0 ==\0\0\0" + ov.expand(a)
        assert (d / "hs_ed25519_public_key").read_bytes() == b"== ed25519v1-public: type0 ==\0\0\0" + pub
        assert (d / "hostname").read_bytes() == (strings[i] + ".onion\n").encode()
        assert all(stat.S_IMODE((d / f).stat().st_mode) == 0o600 for f in ("hs_ed25519_secret_key", "hs_ed25519_public_key", "hostname"))
        assert len((d / "hs_ed25519_secret_key").read_bytes()) == 96 and len((d / "hs_ed25519_public_key").read_bytes()) == 64
    r = subprocess.run([cli, *common], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    a0 = base + 8 * want[0]
    assert f"Address : {strings[want[0]]}.onion\nSecret key : {ov.expand(a0).hex()}\n" in r.stdout and "WIF" not in r.stdout


def test_refusals_and_memory(runner):
    with pytest.raises(vg.VgenError) as e:
        runner.dispatch(1, 0)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vg.VgenError) as e:
        runner.dispatch_keys([1], 0)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vg.VgenError) as e:
        runner.dispatch_random(5, 0, 0, 0)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vg.VgenError) as e:
        vg.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=2, endo=True)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vg.VgenError) as e:
        runner.set_base(bytes.fromhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"))
    assert e.value.status == E_UNSUPPORTED
    m = runner.memory()
    lanes = BATCH // 64
    assert m["table_bytes"] == 32 * 256 * 28 * 4 + lanes * 27 * 4 and m["table_bits"] == 0     # the Ed25519 table and the lane points: no secp256k1 table
    assert m["frames_bytes"] >= 2 * 36 * BATCH                                                 # the walk scratch, 36 B per key and frame


# ---- the device build of the core functions ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libonniondev.so"))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.oniondev_pair.argtypes = [ctypes.c_int, u32p, u32p]
    lib.oniondev_filter.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, u32p]
    return lib


def pair_cases():
    """(P, Q) for the edge list of tests/test_onion.py: Q the neutral element, P, -P, the points of order 2, 4 and 8, random pairs."""
    rng = random.Random(13)
    cases = []
    for _ in range(3):
        p = ov.point_of(rng.getrandbits(253) * 8)
        cases += [(p, q) for q in ov.edge_points(p)]
        cases += [(q, p) for q in ov.edge_points(p)[3:]]
    cases += [(ov.point_of(rng.getrandbits(255)), ov.point_of(rng.getrandbits(255))) for _ in range(32)]
    cases += [((0, 1), (0, 1)), ((0, P - 1), (0, P - 1))]
    return cases


def test_pair_formulas_on_the_device(dev):
    cases = pair_cases()
    flat = [(v >> (32 * k)) & 0xFFFFFFFF for p, q in cases for v in (p[0], p[1], q[0], q[1]) for k in range(8)]
    out = (ctypes.c_uint32 * (32 * len(cases)))()
    assert dev.oniondev_pair(len(cases), (ctypes.c_uint32 * len(flat))(*flat), out) == 0
    for i, (p, q) in enumerate(cases):
        got = tuple(sum(out[32 * i + 8 * c + k] << (32 * k) for k in range(8)) for c in range(4))
        assert got == ov.pair(p, q), i


@pytest.mark.parametrize("length", [1, 6, 7, 13])
def test_filter_boundaries_on_the_device(dev, length):
    """One bit off on either side of the mask, and bit 7 of byte 31 flipped: prefixes of 7 and 13 characters cross word boundaries."""
    prefix = "catsandonions"[:length]
    mask, value = ov.prefix_mask(prefix)
    rng = random.Random(length)
    fill = rng.getrandbits(256) & ~mask
    lowest = 256 - 5 * length
    values = [(value | fill, True), (value | (fill ^ (1 << (lowest - 1))), True), ((value ^ (1 << lowest)) | fill, False),
              ((value ^ (1 << 255)) | fill, False), ((value ^ (1 << (lowest + 4))) | fill, False)]
    values += [(v ^ 0x80, w) for v, w in values]                        # big-endian reading: byte 31 is the lowest byte
    flags = ctypes.create_string_buffer(len(values))
    kind = ctypes.c_uint32()
    blob = b"".join(v.to_bytes(32, "big") for v, _ in values)
    assert dev.oniondev_filter(("^" + prefix).encode(), 0, len(values), blob, flags, ctypes.byref(kind)) == 0
    assert kind.value == 2
    assert [f for f in flags.raw] == [int(w) for _, w in values]
