"""The Solana format (VGEN_FMT_SOLANA, format 12) on the MI355X: ed_keys_kernel in its dump and prefilter forms behind
vgen_dispatch_random and vgen_dispatch_keys, the compaction behind it, the device build of the format's core functions
(tests/native/solana_dev.hip) and the scan loop over the kernel.

Smallest shapes that still have the structure: batch 8192 (sixteen workgroups of eight waves, each sharing one inversion), two frames.
Expected values are those of tests/solana_vectors.py - Python-integer RFC 8032 arithmetic checked against OpenSSL - computed once and
shared; the digest of each dump is the golden one of tests/golden/solana.json.  Every test here fails on a library without the
format (vgen_create: VGEN_E_INVALID)."""
import ctypes
import functools
import hashlib
import json
import os
import random
import re

import pytest

from tests import solana_vectors as sv
import vgen_amd as vg
from vgen_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = sv.FMT_SOLANA
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "solana.json")))
BATCH = 8192
KEY_INDEX = 5000
E_UNSUPPORTED = -8


@pytest.fixture(scope="module")
def runner():
    r = vg.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=2)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def expected(which):
    d = FIXTURE["dump"][which]
    assert d["batch"] == BATCH
    return sv.stream_payloads(d["seed"], d["stream"], d["first_index"], BATCH)


@functools.lru_cache(maxsize=None)
def expected_strings(which):
    return [sv.address(p) for p in expected(which)]


@pytest.mark.parametrize("which", [0, 1], ids=["first-0", "first-2^32-100"])
def test_random_dump_equals_the_reference_and_the_golden_digest(runner, which):
    d = FIXTURE["dump"][which]
    assert d["first_index"] == (0, 2**32 - 100)[which]
    runner.set_filter(None)
    runner.dispatch_random(d["seed"], d["stream"], d["first_index"], 0)
    blob, _, tested = runner.await_result(0)
    assert tested == BATCH and len(blob) == BATCH * 32
    want = expected(which)
    bad = [i for i in range(BATCH) if blob[32 * i:32 * i + 32] != want[i]]
    assert not bad, (len(bad), bad[:8])
    assert hashlib.sha256(blob).hexdigest() == d["sha256"] == hashlib.sha256(b"".join(want)).hexdigest()


def test_key_dispatch_of_one_wave_and_one_lane(runner):
    pairs = (FIXTURE["openssl"] + FIXTURE["rfc8032"])[:65]
    assert len(pairs) == 65
    runner.set_filter(None)
    runner.dispatch_keys([bytes.fromhex(v["seed"]) for v in pairs], 0)
    blob, _, tested = runner.await_result(0)
    assert tested == 65
    for i, v in enumerate(pairs):
        assert blob[32 * i:32 * i + 32].hex() == v["public_key"], i
    assert blob[32 * 65:] == bytes(32 * (BATCH - 65))


def filtered(runner, pattern, ci=False, which=0):
    d = FIXTURE["dump"][which]
    p = vg.Pattern(pattern, ci, FMT)
    runner.set_filter(p)
    runner.dispatch_random(d["seed"], d["stream"], d["first_index"], 1)
    recs, n, tested = runner.await_result(1)
    assert tested == BATCH and n == len(recs)
    return p, recs


def check_records(runner, pattern, kind, ci=False):
    p, recs = filtered(runner, pattern, ci)
    assert p.device_kind == kind
    want, strings = expected(0), expected_strings(0)
    rx = re.compile(pattern, re.I if ci else 0)
    hits = [i for i, s in enumerate(strings) if rx.search(s)]
    idx = [i for i, _ in recs]
    assert KEY_INDEX in hits and set(hits) <= set(idx)                   # every reference hit is among the records
    assert idx == sorted(idx) and len(set(idx)) == len(idx)             # ascending index order
    assert all(pl == want[i] for i, pl in recs)                         # each with the payload of its index
    return hits, idx


@pytest.mark.parametrize("length,ci", [(1, False), (2, False), (3, False), (3, True), (5, False)])
def test_prefix_patterns(runner, length, ci):
    prefix = expected_strings(0)[KEY_INDEX][:length]
    hits, idx = check_records(runner, "^" + prefix, 1, ci)
    if not ci:
        assert idx == hits                                              # a literal prefix's ranges are exact


@pytest.mark.parametrize("length", [1, 2, 5, 6])
def test_suffix_patterns(runner, length):
    s = expected_strings(0)[KEY_INDEX]
    hits, idx = check_records(runner, s[-length:] + "$", 7)
    if length <= 5:
        assert idx == hits


def test_a_pattern_anchored_at_both_ends(runner):
    s = expected_strings(0)[KEY_INDEX]
    hits, idx = check_records(runner, "^" + s[:1] + ".*" + s[-2:] + "$", 7)
    assert idx == hits


def test_match_all_reports_every_key_and_the_first_records(runner):
    d = FIXTURE["dump"][0]
    pat = vg.Pattern(".", False, FMT)
    assert pat.device_kind == 3
    api._check(api._L.vgen_set_match_cap(runner._h, 256), runner._h)
    runner.match_cap = 256
    try:
        runner.set_filter(pat)
        runner.dispatch_random(d["seed"], d["stream"], d["first_index"], 1)
        recs, n, tested = runner.await_result(1)
        assert n == BATCH and tested == BATCH and len(recs) == 256
        assert recs == [(i, expected(0)[i]) for i in range(256)]
    finally:
        api._check(api._L.vgen_set_match_cap(runner._h, 4096), runner._h)
        runner.match_cap = 4096


def test_seeded_scan_equals_the_references_first_five(runner):
    seed = 77
    strings = [sv.address(p) for p in sv.stream_payloads(seed, 0, 0, BATCH)]
    prefix = strings[123][:2]
    want = [i for i, s in enumerate(strings) if s.startswith(prefix)][:5]
    assert len(want) == 5                                               # (a two-character prefix: ~1 in 1000 of 8192)
    res = vg.scan_gpu_with_runner("^" + prefix, vg.ScanConfig(format=FMT, count=5, seed=seed), runner)
    assert [m.hex for m in res.matches] == [sv.stream_seed(seed, 0, i).hex() for i in want]
    for m, i in zip(res.matches, want):
        assert m.address == strings[i] and m.wif == m.hex and int(m.format) == FMT


def test_command_line_search_and_its_writers(tmp_path):
    """`vgen-hip generate -f solana --seed`: the reference's first matches of stream 0, as text (Address / Seed / Keypair), as jsonl
    (seed_hex, keypair_base58, public_key_hex, no wif) and as keypair files solana-keygen reads, mode 0600."""
    import stat
    import subprocess
    cli = os.path.join(ROOT, "vgen_amd", "vgen-hip")
    seed = 77
    strings = [sv.address(p) for p in sv.stream_payloads(seed, 0, 0, BATCH)]
    prefix = strings[123][:2]
    want = [i for i, s in enumerate(strings) if s.startswith(prefix)][:2]
    common = ["generate", "-f", "solana", "-p", "^" + prefix, "--seed", str(seed), "-c", "2", "--gpu-batch-size", str(BATCH), "--frames", "2", "-q"]
    r = subprocess.run([cli, *common, "-o", "jsonl", "--keypair-dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(rows) == 2
    for row, i in zip(rows, want):
        s = sv.stream_seed(seed, 0, i)
        assert row["address"] == strings[i] and row["seed_hex"] == s.hex() and row["public_key_hex"] == sv.public_key(s).hex()
        assert row["keypair_base58"] == sv.keypair_base58(s) and "wif" not in row and row["format"] == "Solana"
        path = tmp_path / (strings[i] + ".json")
        assert json.loads(path.read_text()) == list(s + sv.public_key(s)) and stat.S_IMODE(path.stat().st_mode) == 0o600
    r = subprocess.run([cli, *common], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    s0 = sv.stream_seed(seed, 0, want[0])
    assert f"Address : {strings[want[0]]}\nSeed    : {s0.hex()}\nKeypair : {sv.keypair_base58(s0)}\n" in r.stdout and "WIF" not in r.stdout


def test_refusals(runner):
    with pytest.raises(vg.VgenError) as e:
        runner.dispatch(1, 0)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(vg.VgenError) as e:
        vg.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=2, endo=True)
    assert e.value.status == E_UNSUPPORTED
    m = runner.memory()
    assert m["table_bytes"] == 32 * 256 * 28 * 4 and m["table_bits"] == 0


# ---- the device build of the core functions ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libsolanadev.so"))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.soldev_fe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p, u32p, u32p]
    lib.soldev_mul.argtypes = [ctypes.c_int, u32p, u32p]
    lib.soldev_filter.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, u32p]
    return lib


def words(values):
    return (ctypes.c_uint32 * (8 * len(values)))(*[(v >> (32 * k)) & 0xFFFFFFFF for v in values for k in range(8)])


def unwords(arr, n):
    return [sum(arr[8 * i + k] << (32 * k) for k in range(8)) for i in range(n)]


def test_field_edges_on_the_device(dev):
    P = sv.P
    rng = random.Random(1)
    edges = [0, 1, 19, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1]
    a = [x for x in edges for _ in edges] + [rng.getrandbits(256) for _ in range(64)]
    b = [y for _ in edges for y in edges] + [rng.getrandbits(256) for _ in range(64)]
    n = len(a)
    ops = {0: lambda x, y: x % P, 1: lambda x, y: x * y % P, 2: lambda x, y: x * x % P, 3: lambda x, y: pow(x, P - 2, P),
           4: lambda x, y: (x + y) % P, 5: lambda x, y: (x - y) % P}
    for op, f in ops.items():
        out = (ctypes.c_uint32 * (8 * n))()
        assert dev.soldev_fe(op, 0, n, words(a), words(b), out) == 0
        assert unwords(out, n) == [f(x, y) for x, y in zip(a, b)], op
    weak = (1 << 29) + (1 << 17)
    pats = [[(1 << 29) - 1] * 9, [weak] * 9, [2 * weak] * 9, [3 * weak] * 9]
    val = lambda l: sum(v << (29 * i) for i, v in enumerate(l))
    pa, pb = [pats[0], pats[1], pats[2], pats[1]], [pats[0], pats[1], pats[3], pats[3]]      # products up to m_a * m_b = 6
    flat = lambda ls: (ctypes.c_uint32 * (9 * len(ls)))(*[v for l in ls for v in l])
    out = (ctypes.c_uint32 * (8 * 4))()
    assert dev.soldev_fe(1, 1, 4, flat(pa), flat(pb), out) == 0
    assert unwords(out, 4) == [val(x) * val(y) % P for x, y in zip(pa, pb)]
    assert dev.soldev_fe(6, 1, 4, flat(pa), flat(pb), out) == 0
    assert unwords(out, 4) == [val(x) % P for x in pa]


def test_raw_scalars_on_the_device(dev):
    L = sv.L
    rng = random.Random(2)
    ks = [0, 2**256 - 1, 2**254, 2**255 - 8, L - 1, L, L + 1, 1, 255, 256] + [rng.getrandbits(256) for _ in range(60)]
    out = (ctypes.c_uint32 * (8 * len(ks)))()
    assert dev.soldev_mul(len(ks), words(ks), out) == 0
    got = bytes(out)
    for i, k in enumerate(ks):
        assert got[32 * i:32 * i + 32] == sv.mul_base(k), hex(k)


@pytest.mark.parametrize("pattern,ci", [("^So", False), ("^Ab", True), ("^11", False), ("pump$", False), ("^Ab.*xyz$", False)])
def test_filter_boundaries_on_the_device(dev, pattern, ci):
    values = []
    m = re.match(r"\^(\w+)", pattern)
    ranges = []
    if m:
        lits = {m.group(1)} if not ci else {"Ab", "AB", "ab", "aB"}
        for lit in lits:
            ranges += sv.prefix_ranges(lit)
        for lo, hi in ranges:
            values += [v for v in (lo - 1, lo, hi, hi + 1) if 0 <= v < 2**256]
    s = re.search(r"(\w+)\$", pattern)
    mod = res = None
    if s:
        mod, res = sv.suffix_residue(s.group(1))
        base = list(values) or [random.Random(4).getrandbits(256) for _ in range(8)]
        values = [v - v % mod + res + dd for v in base for dd in (-1, 0, 1) if 0 <= v - v % mod + res + dd < 2**256]
    flags = ctypes.create_string_buffer(len(values))
    kind = ctypes.c_uint32()
    assert dev.soldev_filter(pattern.encode(), int(ci), len(values), b"".join(v.to_bytes(32, "big") for v in values), flags, ctypes.byref(kind)) == 0
    assert kind.value == (7 if s else 1)
    for v, f in zip(values, flags.raw):
        want = (not ranges or any(lo <= v <= hi for lo, hi in ranges)) and (mod is None or v % mod == res)
        assert f == int(want), hex(v)
    assert 0 < sum(flags.raw) < len(values)
