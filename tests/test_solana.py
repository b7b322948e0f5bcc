"""The Solana format (VGEN_FMT_SOLANA, format 12) on the CPU: an address is Base58 of an Ed25519 public key, and the key is the 32-byte
SEED the wallet imports.

Expected values come from outside the code under test (tests/solana_vectors.py): Python-integer RFC 8032 arithmetic with hashlib's
SHA-512, checked against OpenSSL's key pairs (tests/golden/solana.json), a Base58 encoder written out there and the range and residue
constructions of the string.  Checked: the host build of the very functions the kernel runs (tests/native/solana_shim.cpp) - field
functions at the edges of the field and of the limb form, the SHA-512 block, the fixed-base multiplication on raw scalars - the
strings, the filter compiler with the device test evaluated on payloads at the bounds of every range and around every residue,
the 64-test fallback, the pattern front end, every refusal, and a stand-alone sanitizer build of the same code.  The reference
has no such format (src/address.rs:11-24)."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

from tests import solana_vectors as sv
import vgen_amd as vg
from vgen_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = sv.FMT_SOLANA
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "solana.json")))
PAIRS = FIXTURE["openssl"] + FIXTURE["rfc8032"]
E_INVALID, E_UNSUPPORTED, E_PATTERN = -1, -8, -6
P, L = sv.P, sv.L


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libsolanatest.so"))
    lib.sol_fe_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.sol_fe_op_limbs.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p]
    lib.sol_sha512_half.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.sol_mul_base.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.sol_filter_check.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                     ctypes.POINTER(ctypes.c_uint32)]
    return lib


# ---- the field ------------------------------------------------------------------------------------------------------------------

FIELD_EDGES = [0, 1, 19, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1, 2**255 - 20, 2 * P, 2 * P + 1]


def fe_op(shim, op, a, b=0):
    out = ctypes.create_string_buffer(32)
    shim.sol_fe_op(op, a.to_bytes(32, "little"), b.to_bytes(32, "little"), out)
    return int.from_bytes(out.raw, "little")


def test_field_functions_against_python_integers(shim):
    rng = random.Random(12)
    values = FIELD_EDGES + [rng.getrandbits(256) for _ in range(40)]
    for a in values:
        assert fe_op(shim, 0, a) == a % P
        assert fe_op(shim, 2, a) == a * a % P
        assert fe_op(shim, 3, a) == pow(a, P - 2, P)
        for b in FIELD_EDGES + [rng.getrandbits(256)]:
            assert fe_op(shim, 1, a, b) == a * b % P
            assert fe_op(shim, 4, a, b) == (a + b) % P
            assert fe_op(shim, 5, a, b) == (a - b) % P


def limbs_value(limbs):
    return sum(v << (29 * i) for i, v in enumerate(limbs))


def test_field_functions_on_limb_patterns_of_all_ones(shim):
    """Raw limbs at the magnitudes the functions state: every limb 2^29 - 1, 2^29 + 2^17 (weak), and products at m_a * m_b = 6."""
    weak = (1 << 29) + (1 << 17)
    pats = [[(1 << 29) - 1] * 9, [weak] * 9, [2 * weak] * 9, [3 * weak] * 9, [0x1FFFFFFF] * 8 + [0x7FFFFF], [0] * 8 + [weak]]
    arr = lambda l: (ctypes.c_uint32 * 9)(*l)
    out = ctypes.create_string_buffer(32)
    for a in pats:
        shim.sol_fe_op_limbs(0, arr(a), arr(a), out)
        assert int.from_bytes(out.raw, "little") == limbs_value(a) % P
        shim.sol_fe_op_limbs(6, arr(a), arr(a), out)
        assert int.from_bytes(out.raw, "little") == limbs_value(a) % P
        if max(a) <= 2 * weak:
            shim.sol_fe_op_limbs(2, arr(a), arr(a), out)
            assert int.from_bytes(out.raw, "little") == limbs_value(a) ** 2 % P
        for b in pats:
            if (max(a) // weak or 1) * (max(b) // weak or 1) <= 6 and max(a) * max(b) <= 6 * weak * weak:
                shim.sol_fe_op_limbs(1, arr(a), arr(b), out)
                assert int.from_bytes(out.raw, "little") == limbs_value(a) * limbs_value(b) % P
    seven = [7 * weak] * 9
    shim.sol_fe_op_limbs(0, arr(seven), arr(seven), out)
    assert int.from_bytes(out.raw, "little") == limbs_value(seven) % P
    shim.sol_fe_op_limbs(6, arr(seven), arr(seven), out)
    assert int.from_bytes(out.raw, "little") == limbs_value(seven) % P


def test_sha512_block_against_hashlib(shim):
    rng = random.Random(5)
    out = ctypes.create_string_buffer(32)
    for seed in [bytes(32), b"\xff" * 32, bytes(range(32))] + [rng.randbytes(32) for _ in range(50)]:
        shim.sol_sha512_half(seed, out)
        assert out.raw == hashlib.sha512(seed).digest()[:32]


RAW_SCALARS = [0, 2**256 - 1, 2**254, 2**255 - 8, L - 1, L, L + 1, 1, 2, 255, 256, 0xff << 248, 8 * L]


def test_multiplication_on_raw_scalars(shim):
    rng = random.Random(7)
    out = ctypes.create_string_buffer(32)
    for k in RAW_SCALARS + [rng.getrandbits(256) for _ in range(20)]:
        shim.sol_mul_base(k.to_bytes(32, "little"), out)
        assert out.raw == sv.mul_base(k), hex(k)
    for k in (0, L, 8 * L):
        assert sv.mul_base(k) == b"\x01" + bytes(31)                       # the neutral element
    assert sv.mul_base(2**256 - 1) == sv.mul_base_slow(2**256 - 1) and sv.mul_base(L + 1) == sv.mul_base_slow(1)


# ---- strings ----------------------------------------------------------------------------------------------------------------------

def test_the_reference_agrees_with_openssl_and_rfc8032():
    assert len(FIXTURE["openssl"]) >= 64
    assert FIXTURE["rfc8032"][0]["public_key"] == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    for v in PAIRS:
        assert sv.public_key(bytes.fromhex(v["seed"])).hex() == v["public_key"] and sv.address(bytes.fromhex(v["public_key"])) == v["address"]


def test_derive_encode_and_decode_over_the_fixture():
    for v in PAIRS:
        seed, pub = bytes.fromhex(v["seed"]), bytes.fromhex(v["public_key"])
        assert vg.solana_public_key(seed) == pub and vg.solana_address(seed) == v["address"]
        assert vg.address_from_payload(FMT, pub) == v["address"] and vg.solana_decode(v["address"]) == pub
        g = vg.derive(FMT, seed)
        assert g.address == v["address"] and g.wif == g.hex == v["seed"] and int(g.format) == FMT
        assert vg.key_to_wif(FMT, seed) == v["seed"]
        assert vg.solana_keypair_base58(seed) == sv.keypair_base58(seed) and len(vg.solana_keypair_base58(seed)) in (87, 88)
    # any 32 bytes are a key: 0 and 2^256 - 1 (no scalar of secp256k1) included
    for seed in (bytes(32), b"\xff" * 32):
        assert vg.derive(FMT, seed).address == sv.address(sv.public_key(seed))


def test_payloads_with_leading_zero_bytes():
    for z in (0, 1, 2, 3, 32):
        pl = bytes(z) + (b"" if z == 32 else b"\x01" + bytes(range(1, 32 - z)))
        s = vg.address_from_payload(FMT, pl)
        assert s == sv.b58encode(pl) and s.startswith("1" * z) and (z == 32 or s[z] != "1") and vg.solana_decode(s) == pl
    assert vg.address_from_payload(FMT, bytes(32)) == "1" * 32 and len(vg.address_from_payload(FMT, b"\xff" * 32)) == 44


def test_decode_refusals():
    good = PAIRS[0]["address"]
    assert vg.solana_decode(good) is not None
    for bad in ("", good[:-1] + "0", good[:-1] + "O", good[:-1] + "I", good[:-1] + "l", good + "1", "1" + good, "2" * 42, "1" * 31, "1" * 33,
                "z" * 44, good[:-1] + " ", sv.b58encode(bytes(1) + bytes.fromhex(PAIRS[0]["public_key"])), sv.b58encode(b"\x01" * 31)):
        assert vg.solana_decode(bad) is None, bad
    assert vg.solana_decode(sv.b58encode(b"\xff" * 32)) == b"\xff" * 32
    assert vg.solana_decode(sv.b58encode((2**256).to_bytes(33, "big"))) is None      # 44 characters, one more than 32 bytes hold


def test_the_candidate_stream():
    for seed, stream, index in ((0, 0, 0), (42, 3, 2**32 - 1), (2**64 - 1, 2**32 - 1, 2**64 - 1), (os.urandom(24), 5, 2**40)):
        assert vg.solana_seed(seed, stream, index) == sv.stream_seed(seed, stream, index)
    # the bytes vgen_random_key_seed returns, where that call accepts the draw
    k = vg.random_key(42, 1, 7)
    assert k is not None and vg.solana_seed(42, 1, 7) == k.to_bytes(32, "big")


# ---- the device test on the host build --------------------------------------------------------------------------------------------

def check(shim, pattern, payloads, ci=False):
    """-> (kind, count, n_ranges, modulus), tests [(a, b)] as integers, [(device, exact)] per payload."""
    out = ctypes.create_string_buffer(max(1, len(payloads)))
    info = (ctypes.c_uint32 * 4)()
    tests = (ctypes.c_uint32 * (16 * 64))()
    assert shim.sol_filter_check(pattern.encode(), int(ci), b"".join(payloads), len(payloads), out, info, tests) == 0, pattern
    tv = []
    for t in range(info[1] if info[0] in (1, 7) else 0):
        w = tests[16 * t:16 * t + 16]
        tv.append((int.from_bytes(b"".join(x.to_bytes(4, "big") for x in w[:8]), "big"), int.from_bytes(b"".join(x.to_bytes(4, "big") for x in w[8:]), "big")))
    return tuple(info), tv, [(b & 1, (b >> 1) & 1) for b in out.raw[:len(payloads)]]


def n_bytes(n):
    return n.to_bytes(32, "big")


PREFIXES = ["S", "So", "So1", "So1a", "So1an", "So1anA", "1", "11", "1A", "11B", "1So1", "2", "H", "J", "K", "z", "JE", "JEK", "zzz", "4vJ9"]


@pytest.mark.parametrize("prefix", PREFIXES)
def test_prefix_ranges_are_the_exact_ranges(shim, prefix):
    want = sorted(sv.prefix_ranges(prefix))
    edge = []
    for lo, hi in want:
        edge += [v for v in (lo - 1, lo, hi, hi + 1) if 0 <= v < 2**256]
    (kind, count, nr, mod), tests, flags = check(shim, "^" + prefix, [n_bytes(v) for v in edge])
    if not want:                       # e.g. "zzz": no 32-byte value starts so - an empty set of ranges, which accepts nothing
        rng = random.Random(9)
        probes = [0, 2**256 - 1, 2**248, 2**255] + [rng.getrandbits(256) for _ in range(20)]
        (kind, count, nr, mod), tests, flags = check(shim, "^" + prefix, [n_bytes(v) for v in probes])
        assert kind == 1 and count == 0 and all(dev == 0 and exact == 0 for dev, exact in flags)
        return
    assert kind == 1 and nr == count == len(want) and mod == 0 and len(want) <= 2
    assert sorted(tests) == want
    for v, (dev, exact) in zip(edge, flags):
        inside = any(lo <= v <= hi for lo, hi in want)
        assert dev == exact == int(inside) and sv.b58encode(n_bytes(v)).startswith(prefix) == inside, hex(v)
    lengths = {len(sv.b58encode(n_bytes(lo))) for lo, _ in want}
    if not prefix.startswith("1"):
        assert lengths <= {43, 44}


@pytest.mark.parametrize("pattern,ci", [("^So1", True), ("^[Ss]o", False), ("^(abc|Abd|1x)", False), ("^a[b-d]", False), ("^Ab", True), ("^1[12]", False)])
def test_prefix_classes_and_case_insensitivity(shim, pattern, ci):
    import itertools
    import re
    rx = re.compile(pattern, re.I if ci else 0)
    # the literal prefixes the pattern stands for, from the alphabet itself
    lits = [p for n in (2, 3) for p in map("".join, itertools.product(sv.ALPHABET, repeat=n)) if rx.match(p) and not any(rx.match(p[:m]) for m in range(1, n))]
    want = []
    for lit in lits:
        want += sv.prefix_ranges(lit)
    edge = []
    for lo, hi in want:
        edge += [v for v in (lo - 1, lo, hi, hi + 1) if 0 <= v < 2**256]
    (kind, count, nr, mod), tests, flags = check(shim, pattern, [n_bytes(v) for v in edge], ci)
    assert kind == 1 and 0 < count <= 64
    for v, (dev, exact) in zip(edge, flags):
        s = sv.b58encode(n_bytes(v))
        assert exact == int(bool(rx.match(s))) and dev >= exact, (hex(v), s)               # superset
        assert dev == int(any(lo <= v <= hi for lo, hi in tests))
    assert any(d for d, _ in flags) and not all(d for d, _ in flags)


@pytest.mark.parametrize("suffix", ["z", "1", "So1an", "11111", "So1anA", "zzzzzz", "pump", "Abcdefghij", "1111111111"])
def test_suffix_residues(shim, suffix):
    k = min(len(suffix), 5)
    mod, res = sv.suffix_residue(suffix[-k:])
    rng = random.Random(len(suffix))
    values = []
    for _ in range(6):
        base = rng.getrandbits(256)
        base -= base % mod
        for r in (res - 1, res, res + 1):
            if 0 <= base + r < 2**256:
                values.append(base + r)
    full_mod, full_res = sv.suffix_residue(suffix)
    exact_hit = rng.getrandbits(256) // full_mod * full_mod + full_res
    values += [exact_hit % 2**256, res, 2**256 - mod + res if 2**256 - mod + res < 2**256 else res, 2**248 - 1, 0]
    (kind, count, nr, m), tests, flags = check(shim, suffix + "$", [n_bytes(v) for v in values])
    assert kind == 7 and nr == 0 and count == 1 and m == mod and tests[0][0] >> 224 == res
    for v, (dev, exact) in zip(values, flags):
        s = sv.b58encode(n_bytes(v))
        assert exact == int(s.endswith(suffix)) and dev == int(v % mod == res) and dev >= exact, (hex(v), s)
        assert (v % full_mod == full_res) == s.endswith(suffix)                              # the string fact itself
    assert sum(d for d, _ in flags) >= 6


def test_a_pattern_anchored_at_both_ends_applies_both_tests(shim):
    ranges = sv.prefix_ranges("Ab")
    mod, res = sv.suffix_residue("xyz")
    values = []
    for lo, hi in ranges:
        for v in (lo - 1, lo, hi, hi + 1):
            values += [v - v % mod + res, v - v % mod + res + 1, v]
        mid = (lo + hi) // 2
        values += [mid - mid % mod + res, mid - mid % mod + res - 1]
    (kind, count, nr, m), tests, flags = check(shim, "^Ab.*xyz$", [n_bytes(v) for v in values])
    assert kind == 7 and nr == len(ranges) == 2 and count == 3 and m == mod
    for v, (dev, exact) in zip(values, flags):
        s = sv.b58encode(n_bytes(v))
        want = any(lo <= v <= hi for lo, hi in ranges) and v % mod == res
        assert dev == int(want) and exact == int(s.startswith("Ab") and s.endswith("xyz") and len(s) >= 5) and dev >= exact
    assert any(d for d, _ in flags) and any(e for _, e in flags)


def test_more_than_64_ranges_fall_back_to_a_shortened_prefix(shim):
    """`-i` on five letters: 2^5 spellings x two lengths pass 64 tests; the compiler keeps the longest shortened prefix that fits and
    never falls back to handing every key to the host."""
    rng = random.Random(3)
    hits = []
    for spelling in ("abcde", "ABCDE", "aBcDe", "AbCdE", "abcDE"):
        for lo, hi in sv.prefix_ranges(spelling):
            hits += [lo, hi, rng.randrange(lo, hi + 1)]
    misses = [rng.getrandbits(256) for _ in range(300)]
    (kind, count, nr, m), tests, flags = check(shim, "^abcde", [n_bytes(v) for v in hits + misses], ci=True)
    assert kind == 1 and 0 < count <= 64
    assert all(dev == 1 and exact == 1 for dev, exact in flags[:len(hits)])                     # no match is dropped
    rejected = sum(1 for dev, _ in flags[len(hits):] if not dev)
    assert rejected >= 290                                                                      # and it still filters
    for v, (dev, exact) in zip(misses, flags[len(hits):]):
        assert dev >= exact


def test_patterns_without_a_usable_end_are_host_filtered(shim):
    for pattern in ("So1", "a.c", "[0-9]{4}"):
        (kind, _, _, _), _, _ = check(shim, pattern, [])
        assert kind == 0, pattern
    for pattern in (".", "^", ".*"):
        (kind, _, _, _), _, _ = check(shim, pattern, [])
        assert kind == 3, pattern
    (kind, count, nr, m), _, _ = check(shim, "^1", [])
    assert kind == 1 and count == 1


# ---- front end and refusals -----------------------------------------------------------------------------------------------------------

def test_the_pattern_front_end():
    assert api._L.vgen_format_charset_name(FMT) == b"Base58"
    assert api._L.vgen_format_charset_name(11) is None and api._L.vgen_format_charset_name(8) is None and api._L.vgen_format_charset_name(9) is None
    assert vg.Pattern("^So1", False, FMT).estimate_difficulty() == 58**3 and vg.Pattern("^So1", True, FMT).estimate_difficulty() == 34**3
    assert vg.Pattern("^1a", False, FMT).estimate_difficulty() == 58**2                          # no constant prefix
    assert vg.Pattern("^S0l", False, FMT).validate_charset() == ["0", "l"] and vg.Pattern("^So1", False, FMT).validate_charset() == []
    p = vg.Pattern("^So1", False, FMT)
    assert p.device_kind == 1 and p.matches("So1anA") and not p.matches("so1anA")
    assert vg.Pattern("pump$", False, FMT).device_kind == 7 and vg.Pattern("^So.*pump$", False, FMT).device_kind == 7
    assert vg.Pattern(".", False, FMT).device_kind == 3 and vg.Pattern("So1", False, FMT).device_kind == 0


def compile_status(pattern, fmt, listed=False):
    h = ctypes.c_void_p()
    fn = api._L.vgen_filter_compile_list if listed else api._L.vgen_filter_compile
    rc = fn(pattern.encode(), 0, fmt, ctypes.byref(h))
    if rc == 0:
        api._L.vgen_filter_free(h)
    return rc, (api._L.vgen_last_error(None) or b"").decode()


def test_refusals_that_need_no_context():
    rc, msg = compile_status("^So\n^Ab\n", FMT, listed=True)
    assert rc == E_UNSUPPORTED and "solana" in msg
    rc, msg = compile_status("score:zero-bytes>=2", FMT)
    assert rc == E_UNSUPPORTED and msg
    out = ctypes.create_string_buffer(128)
    pub33 = bytes.fromhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798")
    assert api._L.vgen_split_derive(FMT, pub33, 33, (1).to_bytes(32, "big"), 0, out, 128) == E_UNSUPPORTED
    fin = ctypes.create_string_buffer(32)
    assert api._L.vgen_split_combine(FMT, (1).to_bytes(32, "big"), (1).to_bytes(32, "big"), b"x", fin, None) == E_UNSUPPORTED
    for fmt in (8, 9, 11, 13):
        assert compile_status("^a", fmt)[0] == 0          # (an unknown format compiles to "every key to the host"; contexts refuse it)
        assert api._L.vgen_address_from_payload(fmt, bytes(32), out, 128) == E_UNSUPPORTED
    assert api._L.vgen_abi_version() == 4


def test_the_sanitizer_build_of_the_same_code_runs_clean():
    """tests/native/solana_selftest.cpp, built with -fsanitize=address,undefined: field, multiplication, filter compile, derivation."""
    exe = os.path.join(ROOT, "tests", "native", "solana_selftest")
    assert os.path.exists(exe), f"{exe} not built (make -C tests/native -f solana.mk, or __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
