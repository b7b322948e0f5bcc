"""The Nostr format (VGEN_FMT_NOSTR, format 10) on the CPU: the address is the key itself - Bech32 (BIP-173, HRP npub) of the BIP-340 x-only
public key - and the secret key is rendered as nsec1...

Expected values come from outside the code under test (tests/nostr_vectors.py): OpenSSL's public keys (tests/golden/nostr.json), a
BIP-173 encoder and strict decoder written out there, the oracle's scalar multiplication.  Checked: encode / decode round trips and
every rejection of the strict decoder, vgen_derive / vgen_key_to_wif, the pattern front end (invalid characters, difficulty), the
filter compiler with the host evaluation of the DEVICE test (tests/native/nostr_shim.cpp: the very functions the kernels run) on
payloads one bit away from a match, pattern lists, the refusal of score patterns, the three-image rule of vgen_key_variant, the ISA
of the new kernel symbols and the command line's help.  The reference has no such format (src/address.rs:11-24)."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import nostr_vectors as nv
import vgen_amd as vg
from vgen_amd import api

ROOT = nv.ROOT
FMT = nv.FMT
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
E_INVALID, E_UNSUPPORTED, E_PATTERN = -1, -8, -6
PREFIX_SYMBOLS = [1, 6, 7, 12, 13, 51, 52]     # 7 crosses the first 32-bit word, 13 the second; 52 reaches the pad bits
SUFFIX_LENGTHS = [1, 6, 7, 8]                  # 6: the checksum alone; 7: the last data symbol (pad rule) too


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libnostrtest.so"))
    lib.nostr_filter_check.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    return lib


def check(shim, pattern, payloads, ci=False):
    """-> (kind, count, flags, has_lut), [(device, exact, device without tables)] per payload."""
    out = ctypes.create_string_buffer(len(payloads))
    info = (ctypes.c_uint32 * 4)()
    assert shim.nostr_filter_check(pattern.encode(), int(ci), b"".join(payloads), len(payloads), out, info) == 0, pattern
    return tuple(info), [(b & 1, (b >> 1) & 1, (b >> 2) & 1) for b in out.raw]


def flip(payload, bit):
    """The payload with bit `bit` (0 = most significant) inverted."""
    v = int.from_bytes(payload, "big") ^ (1 << (255 - bit))
    return v.to_bytes(32, "big")


# ---- strings ------------------------------------------------------------------------------------------------------------------

def test_the_fixture_holds_the_two_published_strings():
    ex = nv.FIXTURE["nip19_example"]
    assert ex["npub"] == "npub180cvv07tjdrrgpa0j7j7tmnyl2yr6yr7l8j4s3evf6u64th6gkwsyjh6w6" and nv.encode("npub", bytes.fromhex(ex["x"])) == ex["npub"]
    assert nv.VECTORS[0]["key"] == "%064x" % 1 and nv.VECTORS[0]["npub"] == "npub10xlxvlhemja6c4dqv22uapctqupfhlxm9h8z3k2e72q4k9hcz7vqpkge6d"
    assert len(nv.VECTORS) >= 70
    for v in nv.VECTORS:
        assert nv.xy_of(int(v["key"], 16))[0] == int(v["x"], 16)   # OpenSSL and the oracle agree on every key


def test_encode_and_decode_round_trip_over_the_fixture():
    for v in nv.VECTORS:
        x, key = bytes.fromhex(v["x"]), bytes.fromhex(v["key"])
        assert vg.nostr_encode("npub", x) == v["npub"] and vg.nostr_encode("nsec", key) == v["nsec"]
        assert vg.nostr_decode(v["npub"]) == ("npub", x) and vg.nostr_decode(v["nsec"]) == ("nsec", key)
        assert vg.nostr_decode(v["npub"].upper()) == ("npub", x)        # all upper case is a Bech32 string too
        assert vg.address_from_payload(FMT, x) == v["npub"]
        assert len(v["npub"]) == 63 and v["npub"][56] in "qs"
    ex = nv.FIXTURE["nip19_example"]
    assert vg.nostr_encode("npub", bytes.fromhex(ex["x"])) == ex["npub"]


def test_the_strict_decoder_rejects_what_the_issue_lists():
    v = nv.VECTORS[5]
    good, x = v["npub"], bytes.fromhex(v["x"])
    assert vg.nostr_decode(good) == ("npub", x)
    syms = nv.symbols(x)
    bad = {
        "wrong hrp": nv.encode("note", x),
        "bech32m constant": "npub1" + "".join(nv.CHARSET[c] for c in syms + [(((nv._polymod(nv._hrp_expand("npub") + syms + [0] * 6) ^ 0x2bc830a3) >> (5 * (5 - i))) & 31) for i in range(6)]),
        "too short": good[:-1],
        "too long": good + "q",
        "mixed case": good[:20] + good[20:].upper(),
        "bad checksum": good[:-1] + ("q" if good[-1] != "q" else "p"),
        "foreign character": good[:10] + "b" + good[11:],
        "witness-version symbol": "npub1q" + good[5:-1],
    }
    # non-zero pad bits under a checksum that is otherwise right
    padded = syms[:51] + [syms[51] | 1]
    bad["pad bits"] = "npub1" + "".join(nv.CHARSET[c] for c in padded + nv.checksum("npub", padded))
    for why, text in bad.items():
        assert nv.decode("npub", text) is None and nv.decode("nsec", text) is None, why   # (the test's own decoder agrees)
        assert vg.nostr_decode(text) is None, why
    out = ctypes.create_string_buffer(32)
    kind = ctypes.c_uint32()
    assert api._L.vgen_nostr_decode(bad["pad bits"].encode(), ctypes.byref(kind), out) == E_INVALID
    assert api._L.vgen_nostr_encode(2, x, ctypes.create_string_buffer(128), 128) == E_INVALID
    assert api._L.vgen_nostr_encode(0, x, ctypes.create_string_buffer(63), 63) == E_INVALID   # no room for the terminator


def test_derive_and_key_to_wif():
    for v in nv.VECTORS:
        g = vg.derive(FMT, int(v["key"], 16))
        assert (g.address, g.wif, g.hex) == (v["npub"], v["nsec"], v["key"])
        assert vg.key_to_wif(FMT, int(v["key"], 16)) == v["nsec"]
        assert vg.npub_from_key(int(v["key"], 16)) == v["npub"] and vg.nsec_from_key(bytes.fromhex(v["key"])) == v["nsec"]
    assert vg.derive(FMT, 0) is None and vg.derive(FMT, nv.N) is None
    assert vg.FORMAT_NOSTR == 10 and vg.derive(vg.FORMAT_NOSTR, 1).format == 10 and vg.abi_version() == 4
    assert [int(x) for x in vg.AddressFormat] == list(range(8))      # outside the enumeration: 8 and 9 stay unknown formats
    for unknown in (8, 9, 11):
        assert api._L.vgen_address_from_payload(unknown, bytes(32), ctypes.create_string_buffer(128), 128) == E_UNSUPPORTED
    assert api._L.vgen_format_charset_name(FMT) == b"Bech32"


def test_three_images_per_point_not_six():
    """(x, y) and (x, -y) are one x-only key: vgen_key_variant 0 .. 2 are the images lambda^e k, with x(lambda^e k) = beta^e x(k)."""
    for v in nv.VECTORS[:12]:
        k, x = int(v["key"], 16), int(v["x"], 16)
        for e in range(3):
            ke = vg.key_variant(k, e)
            assert ke == pow(nv.LAMBDA, e, nv.N) * k % nv.N
            assert nv.xy_of(ke)[0] == pow(nv.BETA, e, nv.P) * x % nv.P
            assert vg.npub_from_key(ke) == nv.npub_of_x(pow(nv.BETA, e, nv.P) * x % nv.P)
        assert nv.xy_of(vg.key_variant(k, 3))[0] == x      # the negation: the same x-only key again


# ---- pattern front end --------------------------------------------------------------------------------------------------------

def invalid_chars(pattern, ci):
    out, n = ctypes.create_string_buffer(64), ctypes.c_size_t()
    assert api._L.vgen_pattern_invalid_chars(pattern.encode(), int(ci), FMT, out, 64, ctypes.byref(n)) == 0
    return out.value.decode()


def difficulty(pattern, ci):
    d = ctypes.c_uint64()
    assert api._L.vgen_pattern_difficulty(pattern.encode(), int(ci), FMT, ctypes.byref(d)) == 0
    return d.value


def test_invalid_chars_and_difficulty():
    assert invalid_chars("^npub1cat", False) == "" and difficulty("^npub1cat", False) == 32 ** 3
    assert invalid_chars("cat$", False) == "" and difficulty("cat$", False) == 32 ** 3
    # 'b' and '1' are no data symbols: valid inside the constant head only
    assert invalid_chars("^npub1b", False) == "b" and invalid_chars("^npub1cat1", False) == "1" and invalid_chars("b1", False) == "b1"
    assert invalid_chars("^NPUB1CAT", True) == "" and invalid_chars("^npub1CAT", True) == "" and invalid_chars("^npub1CAT", False) == "CAT"
    assert difficulty("^npub1CAT", True) == 32 ** 3 and difficulty("^NPUB1CAT", True) == 32 ** 3 and difficulty("^NPUB1CAT", False) == 32 ** 8 and difficulty("^npub1", False) == 1 and difficulty("^npub", False) == 1
    p = vg.Pattern("^npub1b", False, FMT)
    assert not any(p.matches(v["npub"]) for v in nv.VECTORS)


def test_score_patterns_are_unsupported():
    h = ctypes.c_void_p()
    assert api._L.vgen_filter_compile(b"score:zero-bytes>=2", 0, FMT, ctypes.byref(h)) == E_UNSUPPORTED


# ---- filter compiler ----------------------------------------------------------------------------------------------------------

KEY = nv.VECTORS[30]          # a random key of the fixture


@pytest.mark.parametrize("n", PREFIX_SYMBOLS)
def test_prefix_compiles_to_a_mask_over_all_its_bits(shim, n):
    x, npub = bytes.fromhex(KEY["x"]), KEY["npub"]
    pattern = "^" + npub[:5 + n]
    covered = min(5 * n, 256)
    others = [flip(x, covered - 1)] + ([flip(x, covered)] if covered < 256 else []) + [bytes.fromhex(v["x"]) for v in nv.VECTORS[:20]]
    info, res = check(shim, pattern, [x] + others)
    assert info[0] == 2 and info[1] == 1, info                     # DEVF_MASKED, one test
    assert res[0] == (1, 1, 1)                                     # the key itself: device test and exact automaton
    assert res[1] == (0, 0, 0), "last covered bit"                 # one bit inside the prefix
    if covered < 256:
        assert res[2] == (1, 1, 1), "first uncovered bit"          # one bit behind it: still a match, and the mask ends there
    p = vg.Pattern(pattern, False, FMT)
    for pl, r in zip([x] + others, res):
        assert r[0] == r[1] == r[2] == int(p.matches(nv.encode("npub", pl))) == int(nv.encode("npub", pl).startswith(pattern[1:]))


@pytest.mark.parametrize("n", SUFFIX_LENGTHS)
def test_suffix_compiles_to_checksum_and_trailing_symbol_masks(shim, n):
    x, npub = bytes.fromhex(KEY["x"]), KEY["npub"]
    pattern = npub[-n:] + "$"
    # payloads that keep / change the suffix: the key, its last bit flipped (the 52nd symbol), bit 250 flipped (symbol 51), others
    others = [flip(x, 255), flip(x, 250), flip(x, 0)] + [bytes.fromhex(v["x"]) for v in nv.VECTORS[:40]]
    info, res = check(shim, pattern, [x] + others)
    assert info[0] == 2 and info[1] >= 1 and info[2] & 1 and info[3] == 1, info      # masked, with the checksum and its byte tables
    assert res[0] == (1, 1, 1)
    p = vg.Pattern(pattern, False, FMT)
    for pl, r in zip([x] + others, res):
        s = nv.encode("npub", pl)
        assert r[1] == int(p.matches(s)) == int(s.endswith(npub[-n:]))
        assert r[0] == r[2] == r[1]       # suffixes of up to 8 symbols are exact on the device, with the tables and without
    if n >= 7:
        assert res[1][0] == 0             # the key bit of the last data symbol is covered


def test_a_52_symbol_prefix_ending_outside_q_and_s_matches_nothing(shim):
    x, npub = bytes.fromhex(KEY["x"]), KEY["npub"]
    for last in "pz":                     # p = 1, z = 2: pad bits set
        pattern = "^" + npub[:56] + last
        info, res = check(shim, pattern, [x, flip(x, 255)])
        assert info[0] == 2 and info[1] == 0 and res == [(0, 0, 0), (0, 0, 0)]
    other = "s" if npub[56] == "q" else "q"
    info, res = check(shim, "^" + npub[:56] + other, [x, flip(x, 255)])
    assert info[1] == 1 and res == [(0, 0, 0), (1, 1, 1)]


def test_classes_case_folding_and_unanchored_patterns(shim):
    xs = [bytes.fromhex(v["x"]) for v in nv.VECTORS]
    for pattern, ci, kind in (("^npub1[qp]", False, 2), ("^NPUB1[QP]", True, 2), ("^npub1.q", False, 2), ("cat", False, 4), ("^npub1", False, 3)):
        info, res = check(shim, pattern, xs, ci)
        assert info[0] == kind, (pattern, info)
        rx = re.compile(pattern, re.I if ci else 0)
        for v, r in zip(nv.VECTORS, res):
            assert r[1] == int(bool(rx.search(v["npub"]))), (pattern, v["npub"])
            assert r[0] >= r[1] and (kind != 4 or r[0] == r[1])        # a necessary condition; the automaton is exact
    # the on-device automaton over a string built to contain the literal
    syms = nv.symbols(xs[7])
    syms[20:23] = [nv.CHARSET.index(c) for c in "cat"]
    v = 0
    for c in syms:
        v = (v << 5) | c
    made = (v >> 4).to_bytes(32, "big")
    info, res = check(shim, "cat", [made, xs[7]])
    assert info[0] == 4 and res[0] == (1, 1, 1) and "cat" in nv.encode("npub", made)


def test_pattern_lists():
    npubs = [v["npub"] for v in nv.VECTORS[:10]]
    pl = vg.PatternList(["^" + s[:5 + 4 + i] for i, s in enumerate(npubs)], False, FMT)
    for i, v in enumerate(nv.VECTORS[:10]):
        assert i in pl.which(v["npub"])
    h = ctypes.c_void_p()
    text = ("^" + npubs[0][:9] + "\n" + npubs[1][-4:] + "$\n").encode()
    assert api._L.vgen_filter_compile_list(text, 0, FMT, ctypes.byref(h)) == E_PATTERN
    assert api._L.vgen_last_error(None).decode().startswith("line 2:")


# ---- kernels and front ends ---------------------------------------------------------------------------------------------------

def test_new_kernel_symbols_have_no_scratch_no_atomic_and_are_in_the_committed_table():
    isa = open(os.path.join(ROOT, "build", "lib", "device", "kernels.s")).read()
    table = open(os.path.join(ROOT, "profiles", "r05_kernel_resources.txt")).read()
    found = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S*(?:xonly|payload_filter8)\S*)\n(.*?)\.end_amdhsa_kernel", isa, re.M | re.S):
        sym, meta = m.group(1), m.group(2)
        found += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, sym
        assert sym.replace("_ZN2vg", "", 1) + "\t" in table, sym
        if "xonly" in sym:    # no LDS beyond the product tree
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", meta).group(1)) == 9 * 256 * 4, sym
        body = isa.split("\n" + sym + ":", 1)[1].split(".end_amdhsa_kernel", 1)[0]
        assert "_atomic" not in body and "v_mfma" not in body, sym      # payloads and plain hit-mask stores: the compaction makes the records
    assert found == 4 + 4 + 2


def test_the_command_line_knows_the_format():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "nostr" in r.stderr + r.stdout and "npub1" in r.stderr + r.stdout
    r = subprocess.run([CLI, "generate", "-f", "nosuch", "-p", "x"], capture_output=True, text=True)
    assert r.returncode != 0 and "nostr" in r.stderr
