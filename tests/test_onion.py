"""The onion format (VGEN_FMT_ONION, format 13) on the CPU: a Tor v3 address is Base32 of an Ed25519 public key, a checksum and a
version byte, and the key is the SCALAR Tor loads, so keys walk in steps of 8.

Expected values come from outside the code under test (tests/onion_vectors.py): Python integers over tests/solana_vectors.py (pinned to
OpenSSL and RFC 8032), hashlib's SHA3-256 and SHA-512, base64, and two addresses of live services (tests/golden/onion.json).  Checked:
strings and the refusals of the strict decoder, the host's SHA3-256, the expanded key, the base scalar, the host build of the pair formulas
the kernels run (tests/native/onion_shim.cpp) on the edge points of the curve, the device test at the boundaries of its masks, and the
pattern front end.  The reference has no such format."""
import ctypes
import hashlib
import json
import os
import random

import pytest

from tests import onion_vectors as ov
from tests import solana_vectors as sv
import vgen_amd as vg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = ov.FMT_ONION
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "onion.json")))
P = ov.P


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libonniontest.so"))
    lib.onion_pair.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.onion_sha3_256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.onion_filter_check.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_uint32)]
    return lib


# ---- strings ----------------------------------------------------------------------------------------------------------------------

def test_the_format_is_public():
    assert vg.FORMAT_ONION == 13 == FMT
    hdr = open(os.path.join(ROOT, "include", "vgen_hip.h")).read()
    assert "#define VGEN_FMT_ONION 13u" in hdr


def test_known_addresses_of_live_services():
    assert len(FIXTURE["known"]) == 2
    for k in FIXTURE["known"]:
        pub = bytes.fromhex(k["public_key"])
        assert vg.onion_address(pub) == k["address"] == ov.address(pub)
        assert vg.onion_decode(k["address"]) == pub == vg.onion_decode(k["address"] + ".onion")
        assert vg.address_from_payload(FMT, pub) == k["address"]
        assert ov.on_curve(ov.decode_point(pub))


def test_the_no_key_mark_has_no_address():
    """An all-zero payload is what a dump holds where the scalar is 0; as a key it is y = 0, a point of order 4.  The plain encoder
    encodes any 32 bytes; the payload-to-address function refuses this one and no other."""
    assert vg.onion_address(bytes(32)) == ov.address(bytes(32))
    out = ctypes.create_string_buffer(128)
    assert vg.api._L.vgen_address_from_payload(FMT, bytes(32), out, 128) == -8
    for pub in (bytes(31) + b"\x80", b"\x01" + bytes(31), bytes(31) + b"\x01"):
        assert vg.address_from_payload(FMT, pub) == ov.address(pub)
    x, y = ov.decode_point(bytes(32))
    assert y == 0 and ov.on_curve((x, y)) and sv.add(sv.add((x, y), (x, y)), sv.add((x, y), (x, y))) == (0, 1)


def test_encode_and_the_shape_of_the_string():
    rng = random.Random(5)
    for pub in [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(40)]:
        s = vg.onion_address(pub)
        assert s == ov.address(pub) and len(s) == 56 and s[55] == "d" and s[54] in "aiqy" and s == s.lower()
        assert vg.onion_decode(s) == pub
        flipped = bytes(pub[:31]) + bytes([pub[31] ^ 0x80])            # the sign of x is stream bit 248, inside character 49
        t = vg.onion_address(flipped)
        assert t[:49] == s[:49] and t[49] != s[49]


def test_the_decoder_is_strict():
    good = FIXTURE["known"][0]["address"]
    assert vg.onion_decode(good) is not None
    bad = [good[:-1], good + "a", "", good.upper(), good[:5] + good[5].upper() + good[6:], good[:7] + "1" + good[8:], good[:7] + "8" + good[8:],
           good[:7] + "=" + good[8:], good + ".ONION", good + ".onion.onion", " " + good,
           good[:10] + ("b" if good[10] != "b" else "c") + good[11:],      # the checksum no longer matches
           good[:55] + "e"]                                                 # version 4
    pub = bytes.fromhex(FIXTURE["known"][0]["public_key"])
    import base64
    for ver in (0, 2, 4):                                                   # a valid checksum under the wrong version byte
        chk = hashlib.sha3_256(b".onion checksum" + pub + bytes([ver])).digest()[:2]
        bad.append(base64.b32encode(pub + chk + bytes([ver])).decode().lower())
    for s in bad:
        assert vg.onion_decode(s) is None and ov.decode(s) is None, s


def test_sha3_256_against_hashlib(shim):
    rng = random.Random(6)
    for n in [0, 1, 47, 48, 135, 136, 137, 271, 272, 273, 500]:            # around the rate of 136 bytes
        msg = rng.randbytes(n)
        out = ctypes.create_string_buffer(32)
        shim.onion_sha3_256(msg, n, out)
        assert out.raw == hashlib.sha3_256(msg).digest(), n


# ---- keys -------------------------------------------------------------------------------------------------------------------------

def test_the_expanded_key():
    rng = random.Random(7)
    for a in [8, 2**254, 2**255 - 8] + [rng.getrandbits(251) * 8 + 2**254 for _ in range(8)]:
        ex = vg.onion_expand(a)
        assert len(ex) == 64 and ex[:32] == a.to_bytes(32, "little") and ex == ov.expand(a)
        pub = ov.point_bytes(a)                                            # A == a * B
        g = vg.derive(FMT, a.to_bytes(32, "little"))
        assert g.address == ov.address(pub) and g.wif == g.hex == a.to_bytes(32, "little").hex() == vg.key_to_wif(FMT, a.to_bytes(32, "little"))
        assert vg.onion_expand(a + 8)[32:] != ex[32:]                      # neighbours on a walk do not share a nonce key
        assert vg.onion_expand(a.to_bytes(32, "little")) == ex


def test_the_base_scalar_is_the_streams_clamped_scalar():
    for seed, stream in ((0x4F4E494F4E, 0), (0x4F4E494F4E, 1), (1, 0), (2**64 - 1, 7), (bytes(range(24)), 3)):
        got = int.from_bytes(vg.onion_base(seed, stream), "little")
        assert got == ov.base_scalar(seed, stream) and got % 8 == 0 and 2**254 <= got < 2**255
    assert int(FIXTURE["base"], 16) == ov.base_scalar(FIXTURE["seed"], 0)


# ---- the pair formulas of the host build ------------------------------------------------------------------------------------------

def pair_host(shim, p, q):
    out = ctypes.create_string_buffer(128)
    le = lambda v: v.to_bytes(32, "little")
    shim.onion_pair(le(p[0]) + le(p[1]), le(q[0]) + le(q[1]), out)
    return tuple(int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(4))


def test_pair_formulas_on_the_edge_points(shim):
    rng = random.Random(13)
    o8 = ov.order8_point()
    assert ov.on_curve(o8) and ov.on_curve((ov.SQRT_M1, 0)) and ov.on_curve((0, P - 1))
    for _ in range(4):
        p = ov.point_of(rng.getrandbits(253) * 8)
        qs = ov.edge_points(p)
        assert len(qs) == 7
        for q in qs:
            assert pair_host(shim, p, q) == ov.pair(p, q), q
            assert pair_host(shim, q, p) == ov.pair(q, p), q
    for q in ov.edge_points((0, 1)):                                       # the edge points among themselves
        for p in ov.edge_points((0, 1)):
            assert pair_host(shim, p, q) == ov.pair(p, q)
    p = ov.point_of(8 * 12345)
    assert pair_host(shim, p, p)[2:] == (0, 1)                             # P - P is the neutral element
    assert pair_host(shim, p, ov.neg(p))[:2] == (0, 1)


def test_pair_formulas_on_random_pairs(shim):
    rng = random.Random(14)
    for _ in range(64):
        p, q = ov.point_of(rng.getrandbits(255)), ov.point_of(rng.getrandbits(255))
        assert pair_host(shim, p, q) == ov.pair(p, q)
    # a walk's own pair: (a + b) B and (a - b) B
    a, b = 8 * rng.getrandbits(250) + 2**254, 8 * 4321
    xs, ys, xd, yd = pair_host(shim, ov.point_of(a), ov.point_of(b))
    assert sv.encode_point(xs, ys) == ov.point_bytes(a + b) and sv.encode_point(xd, yd) == ov.point_bytes(a - b)


# ---- the device test --------------------------------------------------------------------------------------------------------------

def filter_check(shim, pattern, ci, payloads):
    flags = ctypes.create_string_buffer(len(payloads))
    info = (ctypes.c_uint32 * 2)()
    tests = (ctypes.c_uint32 * (16 * 64))()
    assert shim.onion_filter_check(pattern.encode(), int(ci), b"".join(payloads), len(payloads), flags, info, tests) == 0
    return info[0], info[1], list(flags.raw), tests


@pytest.mark.parametrize("length", [1, 6, 7, 13])
def test_the_mask_at_its_boundaries(shim, length):
    """Prefixes of 7 and 13 characters end at bits 35 and 65: they cross 32-bit word boundaries.  One bit off on either side of the
    mask, the first bit, and byte 31 bit 7 flipped (which must not change the verdict)."""
    prefix = "catsandonions"[:length]
    mask, value = ov.prefix_mask(prefix)
    assert bin(mask).count("1") == 5 * length
    rng = random.Random(length)
    fill = rng.getrandbits(256) & ~mask
    lowest = 256 - 5 * length                                              # the mask's last bit
    values = [(value | fill, True), (value | (fill ^ (1 << (lowest - 1))), True), ((value ^ (1 << lowest)) | fill, False),
              ((value ^ (1 << 255)) | fill, False), ((value ^ (1 << (lowest + 4))) | fill, False), (value, True), (value | ((1 << lowest) - 1), True)]
    values += [(v ^ 0x80, w) for v, w in values]                           # big-endian reading: byte 31 is the lowest byte
    kind, count, flags, tests = filter_check(shim, "^" + prefix, False, [v.to_bytes(32, "big") for v, _ in values])
    assert (kind, count) == (2, 1)
    got_mask = sum(tests[k] << (32 * (7 - k)) for k in range(8))
    got_value = sum(tests[8 + k] << (32 * (7 - k)) for k in range(8))
    assert (got_mask, got_value) == (mask, value)
    for (v, want), f in zip(values, flags):
        assert f & 1 == int(want), hex(v)
        assert (f >> 1) == int(ov.address(v.to_bytes(32, "big")).startswith(prefix))   # ... and the exact automaton agrees here


def test_the_device_test_is_a_superset_of_the_automaton(shim):
    rng = random.Random(21)
    payloads = [rng.randbytes(32) for _ in range(4096)]
    strings = [ov.address(p) for p in payloads]
    for pattern, ci in (("^a", False), ("^[ab]c", False), ("^A", True), ("^q.*d$", False), ("^(ab|cd)", False)):
        kind, count, flags, _ = filter_check(shim, pattern, ci, payloads)
        assert kind == 2 and 1 <= count <= 64
        assert all(f & 1 for f in flags if f & 2) and any(f & 2 for f in flags)
        if "$" not in pattern:
            assert all((f & 1) == (f >> 1) for f in flags), pattern         # a pure prefix: exact


# ---- the pattern front end --------------------------------------------------------------------------------------------------------

def test_the_pattern_front_end():
    assert vg.api._L.vgen_format_charset_name(FMT) == b"Base32"
    p = vg.Pattern("^cat", False, FMT)
    assert p.device_kind == 2 and p.estimate_difficulty() == 32**3 and p.validate_charset() == []
    assert vg.Pattern("^cat", True, FMT).estimate_difficulty() == 32**3
    assert vg.Pattern("^c0a1t89", False, FMT).validate_charset() == ["0", "1", "8", "9"]
    assert vg.Pattern("^Cat", False, FMT).validate_charset() == ["C"] and vg.Pattern("^Cat", True, FMT).validate_charset() == []
    assert vg.Pattern(".", False, FMT).device_kind == 3 and vg.Pattern("^.*", False, FMT).device_kind == 3
    for pattern in ("cat", "cat$", "yd$", "^.{49}a", "^[a-p]"):            # unanchored, suffixes, later characters, half the alphabet
        assert vg.Pattern(pattern, False, FMT).device_kind == 0, pattern
    assert vg.Pattern("^" + "a" * 49, False, FMT).device_kind == 2
    assert vg.Pattern("^" + "a" * 52, False, FMT).device_kind == 2         # (the first 49 characters on the device, the rest by the host)
    with pytest.raises(vg.VgenError):
        vg.PatternList(["^aa", "^bb"], False, FMT)
