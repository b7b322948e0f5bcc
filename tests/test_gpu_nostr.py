"""The Nostr format (VGEN_FMT_NOSTR, format 10) on the MI355X: xonly_bwd_kernel and keys_xonly_kernel in their dump and prefilter forms, the
eight-word deferred filter and the list kernels behind them, and the scan loop over them.

Smallest shapes that still have the structure: batch 8192 (two workgroups, eight waves, S = 8), two frames.  Expected values are
those of tests/nostr_vectors.py - Python-integer additions anchored on the oracle, beta for the images, a BIP-173 encoder written
out there - and of tests/seq_vectors.py for the crafted tables; each is computed once and shared.  Every test here fails on a
library without the format (vgen_create: VGEN_E_INVALID)."""
import ctypes
import os

import numpy as np
import pytest

from tests import nostr_vectors as nv
from tests import seq_vectors as sv
import vgen_amd as vg
from oracle import pyoracle as vo

pytestmark = pytest.mark.gpu

ROOT = nv.ROOT
FMT = nv.FMT
BATCH = 8192
KEY_INDEX = 5000                                  # the chosen key of the prefix / suffix patterns: in the second workgroup's half
BASES = {"random": int(nv.VECTORS[40]["key"], 16) % (nv.N - 2 * BATCH) + 1, "2^65": 2**65, "n-40": nv.N - 40}
PREFIX_SYMBOLS = [1, 6, 7, 12, 13, 51, 52]
SUFFIX_LENGTHS = [1, 6, 7, 8]
SEED = 0x6E6F737472


@pytest.fixture(scope="module")
def runners():
    made = {}

    def get(endo, fmt=FMT):
        if (endo, fmt) not in made:
            made[(endo, fmt)] = vg.GpuRunner(batch_size=BATCH, fmt=fmt, device=0, frames=2, endo=endo)
        return made[(endo, fmt)]
    yield get
    for r in made.values():
        r.close()


def dump(r, start, images):
    r.set_filter(None)
    r.dispatch(start, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * BATCH and len(blob) == images * BATCH * 32
    return np.frombuffer(blob, dtype=np.uint8).reshape(-1, 32)


def records(r, pattern, start, images, ci=False):
    """The records of one filtered dispatch: [(index, payload bytes)], in the order vgen_wait hands them over."""
    p = pattern if not isinstance(pattern, str) else vg.Pattern(pattern, ci, FMT)
    r.set_filter(p)
    r.dispatch(start, 1)
    recs, n, tested = r.await_result(1)
    assert tested == images * BATCH and n == len(recs) <= r.match_cap
    return recs


def cpu_hits(start, images, accept):
    """[(index, payload bytes)] of the slots whose npub string `accept`s, over the expected dump, in index order."""
    d, strings = nv.dump_of(start, BATCH, images), nv.strings_of(start, BATCH, images)
    return [(i, bytes(d[i])) for i, s in enumerate(strings) if s is not None and accept(s)]


# ---- dump parity --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("base", list(BASES))
def test_dump_parity(runners, base, endo):
    """All 8192 payloads (3 x 8192 with the images) are the expected x; keys past n leave zeroed slots (n - 40: the complete per-key path)."""
    images = 3 if endo else 1
    got = dump(runners(endo), BASES[base], images)
    want = nv.dump_of(BASES[base], BATCH, images)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (base, endo, bad[:8])
    if base == "n-40":
        assert not got[40:BATCH].any() and got[39].any()      # n - 1 is the last key


# ---- crafted tables: x3 on the residues that take the slow path of the canonicalisation ----------------------------------------

class XdevJob(ctypes.Structure):
    _fields_ = [("lanes", ctypes.c_uint32), ("s", ctypes.c_uint32), ("endo", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("rtab", ctypes.c_void_p), ("q", ctypes.c_void_p),
                ("launch_error", ctypes.c_int32), ("failed_stage", ctypes.c_uint32), ("dump_out", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def xdev():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libxonlydev.so"))
    lib.xdev_dump_words.restype = ctypes.c_uint64
    lib.xdev_dump_words.argtypes = [ctypes.c_uint32] * 3
    lib.xdev_poison.restype = lib.xdev_guard_words.restype = ctypes.c_uint32
    lib.xdev_run.argtypes = [ctypes.POINTER(XdevJob)]
    assert lib.xdev_job_size() == ctypes.sizeof(XdevJob)
    return lib


def crafted_expected(v, images):
    rows = []
    for e in range(images):
        b = pow(sv.BETA, e, sv.P)
        rows += [(b * x % sv.P).to_bytes(32, "big") for x in v.x3]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32)


def run_xdev(xdev, v, endo):
    rtab, q = np.ascontiguousarray(v.rtab), np.ascontiguousarray(v.qlimbs)
    guard, poison = xdev.xdev_guard_words(), xdev.xdev_poison()
    words = int(xdev.xdev_dump_words(v.lanes, v.S, int(endo)))
    out = np.zeros(words + guard, dtype=np.uint32)
    j = XdevJob(lanes=v.lanes, s=v.S, endo=int(endo), rtab=rtab.ctypes.data, q=q.ctypes.data, dump_out=out.ctypes.data)
    assert xdev.xdev_run(ctypes.byref(j)) == 0 and j.launch_error == 0, (j.launch_error, j.failed_stage)
    assert (out[words:] == poison).all(), "the kernel wrote behind its dump"
    return out[:words].view(np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("geometry,endo", [("g256", False), ("g512", False), ("g65", False), ("g256", True), ("g512", True)],
                         ids=["g256", "g512", "g65", "g256-endo", "g512-endo"])
def test_crafted_tables_dump(xdev, geometry, endo):
    v = sv.vectors(geometry, endo)
    images = 3 if endo else 1
    got, want = run_xdev(xdev, v, endo), crafted_expected(v, images)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (geometry, endo, bad[:8], len(sv.rare_keys(v)))
    assert len(sv.rare_keys(v)) >= 32      # the set holds keys whose products leave [0, p)


# ---- prefilter parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("base", ["random", "2^65"])
def test_prefilter_parity(runners, base, endo):
    images = 3 if endo else 1
    want = cpu_hits(BASES[base], images, lambda s: s.startswith("npub1q"))
    assert 150 * images < len(want) < 4096                    # 5 bits: about 256 per image, under the default match_cap
    assert records(runners(endo), "^npub1q", BASES[base], images) == want


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_prefix_and_suffix_patterns_of_one_key(runners, endo):
    """Every prefix and suffix length of the CPU list, taken from one key inside the batch: the device reports what the CPU does -
    that key alone for the long ones."""
    images = 3 if endo else 1
    start = BASES["random"]
    d = nv.dump_of(start, BATCH, images)
    slot = KEY_INDEX + (BATCH if endo else 0)                 # with the images: a key of image 1
    npub = nv.encode("npub", bytes(d[slot]))
    for n in PREFIX_SYMBOLS:
        want = cpu_hits(start, images, lambda s: s.startswith(npub[:5 + n]))
        assert (slot, bytes(d[slot])) in want and (n < 6 or len(want) == 1)
        assert records(runners(endo), "^" + npub[:5 + n], start, images) == want, n
    for n in SUFFIX_LENGTHS:
        want = cpu_hits(start, images, lambda s: s.endswith(npub[-n:]))
        assert (slot, bytes(d[slot])) in want and (n < 6 or len(want) == 1)
        assert records(runners(endo), npub[-n:] + "$", start, images) == want, n
    # a 52-symbol prefix that ends outside q / s matches nothing
    assert records(runners(endo), "^" + npub[:56] + "p", start, images) == []


# ---- patterns off the mask path -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_unanchored_pattern_runs_the_eight_word_automaton(runners, endo):
    images = 3 if endo else 1
    p = vg.Pattern("cat", False, FMT)
    assert p.device_kind == 4
    want = cpu_hits(BASES["2^65"], images, lambda s: "cat" in s)
    assert len(want) >= 4 * images
    assert records(runners(endo), p, BASES["2^65"], images) == want


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_ten_line_pattern_list(runners, endo):
    images = 3 if endo else 1
    heads = ["qq", "pz", "zr", "ry", "y9", "9x", "x8", "8g", "gf", "f2"]
    pl = vg.PatternList(["^npub1" + h for h in heads], False, FMT)
    want = cpu_hits(BASES["random"], images, lambda s: s[5:7] in heads)
    assert len(want) >= 40 * images
    assert records(runners(endo), pl, BASES["random"], images) == want


# ---- the other key paths ------------------------------------------------------------------------------------------------------

def scalars_300():
    keys = [int(v["key"], 16) for v in nv.VECTORS]
    rows = __import__("json").load(open(os.path.join(ROOT, "tests", "golden", "openssl_keys.json")))["short"]
    keys += [int(r[0], 16) for r in rows[:300 - len(keys) - 2]]
    keys[7:7] = [0]
    keys[150:150] = [nv.N]
    assert len(keys) == 300
    return keys


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_dispatch_keys(runners, endo):
    """300 fixture scalars, 0 and n among them: the dump has x(lambda^e k) at e * batch + i and zeroes for the two that are no keys;
    the prefilter reports the same slots."""
    images = 3 if endo else 1
    keys = scalars_300()
    r = runners(endo)
    r.set_filter(None)
    r.dispatch_keys(keys, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * 300
    got = np.frombuffer(blob, dtype=np.uint8).reshape(-1, 32)
    want = {}
    for i, k in enumerate(keys):
        x = nv.xy_of(k)[0] if 0 < k < nv.N else None
        for e in range(images):
            want[e * BATCH + i] = bytes(32) if x is None else (pow(nv.BETA, e, nv.P) * x % nv.P).to_bytes(32, "big")
    for slot, pl in want.items():
        assert bytes(got[slot]) == pl, slot
    assert not got[7].any() and not got[150].any()
    r.set_filter(vg.Pattern("^npub1[qpzr]", False, FMT))
    r.dispatch_keys(keys, 1)
    recs, n, tested = r.await_result(1)
    assert tested == images * 300
    assert recs == sorted((s, pl) for s, pl in want.items() if any(pl) and pl[0] >> 3 < 4)


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_dispatch_random(runners, endo):
    images = 3 if endo else 1
    r = runners(endo)
    r.set_filter(vg.Pattern("^npub1q", False, FMT))
    r.dispatch_random(SEED, 3, 1000, 0)
    recs, n, tested = r.await_result(0)
    assert tested == images * BATCH and 150 * images < n == len(recs)
    for slot, pl in recs[:40] + recs[-40:]:
        e, i = divmod(slot, BATCH)
        k = vg.random_key(SEED, 3, 1000 + i)
        assert k == vo.random_key(SEED, 3, 1000 + i)
        assert nv.xy_of(vg.key_variant(k, e))[0].to_bytes(32, "big") == pl and pl[0] >> 3 == 0
    # every hit of image 0, by the oracle's stream: the same set of indices
    want0 = [i for i in range(BATCH) if nv.xy_of(vo.random_key(SEED, 3, 1000 + i))[0] >> 251 == 0]
    assert [s for s, _ in recs if s < BATCH] == want0


# ---- scans --------------------------------------------------------------------------------------------------------------------

def check_results(res, want_keys, images):
    assert [int(m.hex, 16) for m in res.matches] == want_keys
    for m in res.matches:
        kind, key = vg.nostr_decode(m.wif)
        assert kind == "nsec" and key.hex() == m.hex
        assert nv.npub_of_x(nv.xy_of(int.from_bytes(key, "big"))[0]) == m.address and m.address.startswith("npub1qq")
    assert res.operations > 0 and res.operations % (images * BATCH) == 0


def test_scan_walk(runners):
    start = vo.seed_key(SEED, 0)
    want, batches = [], 0
    while len(want) < 3:
        xs = nv.walk_x(start + batches * BATCH, BATCH)
        want += [start + batches * BATCH + i for i, x in enumerate(xs) if x >> 246 == 0]
        batches += 1
    res = vg.scan_gpu_with_runner("^npub1qq", vg.ScanConfig(format=vg.FORMAT_NOSTR, count=3, seed=SEED), runners(False))
    check_results(res, want[:3], 1)


def test_scan_with_the_images(runners):
    """A seeded scan on an endomorphism context draws random keys (a walk from a seeded base is refused there): three keys per draw,
    image e of candidate i at e * batch + i, results in that order."""
    want, batch_no = [], 0
    while len(want) < 3:
        keys = [vo.random_key(SEED, 0, batch_no * BATCH + i) for i in range(BATCH)]
        xs = [nv.xy_of(k)[0] if 0 < k < nv.N else None for k in keys]
        for e in range(3):
            b = pow(nv.BETA, e, nv.P)
            want += [pow(nv.LAMBDA, e, nv.N) * k % nv.N for k, x in zip(keys, xs) if x is not None and (b * x % nv.P) >> 246 == 0]
        batch_no += 1
    cfg = vg.ScanConfig(format=vg.FORMAT_NOSTR, count=3, seed=SEED, random_keys=True)
    res = vg.scan_gpu_with_runner("^npub1qq", cfg, runners(True))
    check_results(res, want[:3], 3)


# ---- the other formats beside it ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [vo.FMT_P2PKH, vo.FMT_P2TR], ids=["p2pkh", "p2tr"])
def test_other_formats_in_the_same_process_still_dump_what_the_oracle_does(runners, fmt):
    runners(False)                       # (a Nostr context is alive beside it)
    r = runners(False, fmt)
    r.set_filter(None)
    r.dispatch(2**65, 0)
    blob, _, tested = r.await_result(0)
    assert tested == BATCH and blob == vo.payload_seq(fmt, 2**65, BATCH)


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_command_line_generate_prints_npub_nsec_and_public_key(tmp_path):
    """`vgen-hip generate -f nostr` end to end: jsonl and text writers, and the printed nsec derives the printed npub on the CPU."""
    import json
    import subprocess
    cli = os.path.join(ROOT, "vgen_amd", "vgen-hip")
    base = [cli, "generate", "-p", "^npub1q", "-f", "nostr", "--seed", "7", "--gpu-batch-size", str(BATCH), "--frames", "2", "-c", "2", "-q"]
    out = subprocess.run(base + ["-o", "jsonl"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2
    for m in rows:
        key = bytes.fromhex(m["private_key_hex"])
        x = nv.xy_of(int.from_bytes(key, "big"))[0].to_bytes(32, "big")
        assert m["address"] == nv.encode("npub", x) and m["address"].startswith("npub1q") and m["public_key_hex"] == x.hex()
        assert m["wif"] == nv.encode("nsec", key) and m["format"] == "Nostr (npub)"
    text = subprocess.run(base + ["-o", "text"], capture_output=True, text=True, timeout=120)
    assert text.returncode == 0 and "Nsec    : " + rows[0]["wif"] in text.stdout and "Pubkey  : " + rows[0]["public_key_hex"] in text.stdout
