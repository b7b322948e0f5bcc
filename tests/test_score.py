"""Score specifications on the CPU: parsing and refusals, the word-wise evaluation of core/score_eval.h (its g++ build, the source
the two score kernels compile) against a plain Python model that looks at one hex digit at a time, the host filter
(vgen_filter_matches / vgen_filter_which / vgen_score), and the exact difficulty and selectivity of single terms."""
import ctypes
import os
import random
import subprocess
import sys
from fractions import Fraction
from math import comb

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_vectors as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE, E_PATTERN, E_UNSUPPORTED = -1, -5, -6, -8
HEX_FORMATS = (5, 6, 7)


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    return vgen_amd


@pytest.fixture(scope="module")
def L(vg):
    from vgen_amd import api
    return api._L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_shim") / "libscoreshim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "native", "score_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.score_shim_metric.restype = ctypes.c_uint32
    lib.score_shim_metric.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    lib.score_shim_eval.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.score_shim_metric_many.restype = None
    lib.score_shim_metric_many.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    return lib


def compile_rc(L, spec, fmt, ci=0):
    h = ctypes.c_void_p()
    rc = L.vgen_filter_compile(spec.encode(), ci, fmt, ctypes.byref(h))
    if rc == 0:
        L.vgen_filter_free(h)
    return rc


def addr(vg, payload, fmt=5):
    return vg.address_from_payload(fmt, payload)


# ---- the specification ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", HEX_FORMATS)
def test_a_specification_compiles_to_device_kind_6(vg, fmt):
    p = vg.Pattern("score:zero-bytes>=2&leading-zero-bytes>=1&leading:A>=0&count:f>=40", fmt=vg.AddressFormat(fmt))
    assert p.device_kind == 6 and p.dfa_bytes == 0
    from vgen_amd import api
    n = ctypes.c_uint32()
    assert api._L.vgen_filter_pattern_count(p._h, ctypes.byref(n)) == 0 and n.value == 1
    assert p.validate_charset() == []


@pytest.mark.parametrize("spec", [
    "score:", "score:zero-bytes", "score:zero-bytes>=", "score:zero-bytes>=x", "score:zero-bytes>=21", "score:leading-zero-bytes>=21",
    "score:leading:0>=41", "score:count:f>=41", "score:leading:g>=1", "score:leading:>=1", "score:leading:00>=1", "score:count>=1",
    "score:zeros>=1", "score:>=1", "score:zero-bytes>=1&", "score:&zero-bytes>=1", "score:zero-bytes>=1&&count:0>=1",
    "score:zero-bytes>=1&zero-bytes>=1&zero-bytes>=1&zero-bytes>=1&zero-bytes>=1", "score:zero-bytes>1", "score:zero-bytes=1",
    "score:zero-bytes>=-1", "score:zero-bytes>= 1", "score:zero-bytes>=1000", "score: zero-bytes>=1"])
def test_malformed_specifications_are_pattern_errors_with_a_message(vg, L, spec):
    for fmt in HEX_FORMATS:
        assert compile_rc(L, spec, fmt) == E_PATTERN, spec
        assert L.vgen_last_error(None), spec


@pytest.mark.parametrize("spec,full,score,nearly_holds", [
    ("score:zero-bytes>=0", bytes(20), 20, True), ("score:zero-bytes>=20", bytes(20), 20, False), ("score:leading:0>=40", bytes(20), 40, False),
    ("score:count:F>=40", b"\xff" * 20, 40, False), ("score:zero-bytes>=1&zero-bytes>=1&zero-bytes>=1&zero-bytes>=1", bytes(20), 20, True)])
def test_the_limits_are_accepted_and_hold_at_the_end_of_the_range(vg, spec, full, score, nearly_holds):
    p = vg.Pattern(spec, fmt=vg.AddressFormat.EthereumCreate2)
    assert p.device_kind == 6                        # (as a regular expression the string would compile too, and match nothing)
    assert p.matches(addr(vg, full, 7)) and p.score(addr(vg, full, 7)) == score
    nearly = b"\x12" + full[1:]                       # one byte (two digits) short of the range's end
    assert p.matches(addr(vg, nearly, 7)) == nearly_holds


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4])
def test_other_formats_are_unsupported(L, fmt):
    assert compile_rc(L, "score:zero-bytes>=1", fmt) == E_UNSUPPORTED
    assert compile_rc(L, "score:bogus", fmt) == E_UNSUPPORTED   # (the format decides first)


def test_case_insensitive_plays_no_part(vg):
    a = addr(vg, bytes.fromhex("00aa00" + "bc" * 17))
    for ci in (False, True):
        p = vg.Pattern("score:count:A>=2", case_insensitive=ci, fmt=vg.AddressFormat.Ethereum)
        assert p.matches(a) and p.matches(a.lower()) and p.matches("0x" + a[2:].upper()) and p.score(a) == 2


def test_pattern_lists_keep_refusing_such_lines(vg):
    for text in ("score:zero-bytes>=1", "^0x00\nscore:leading:0>=2"):
        with pytest.raises(vg.VgenError) as e:
            vg.PatternList(text, fmt=vg.AddressFormat.Ethereum)
        assert e.value.status == E_PATTERN and "line" in str(e.value)


# ---- the score function ------------------------------------------------------------------------------------------------------

def test_the_crafted_payloads_hold_what_they_claim():
    c = sv.crafted_payloads()
    assert bytes(20) in c and b"\xff" * 20 in c
    assert {sv.metric(sv.LEADING_DIGIT, 0, p) for p in c} == set(range(41))
    assert {sv.metric(sv.LEADING_DIGIT, 0xf, p) for p in c} == set(range(41))
    assert {sv.metric(sv.LEADING_ZERO_BYTES, 0, p) for p in c} == set(range(21))
    # the near misses: a 0x01 above a zero byte, inside a word and across a word boundary, in a payload with no other zero byte
    for at in (1, 3):
        p = bytearray([0x33] * 20)
        p[at], p[at + 1] = 0x01, 0x00
        assert bytes(p) in c and sv.metric(sv.ZERO_BYTES, 0, bytes(p)) == 1


def all_metrics():
    return [(sv.ZERO_BYTES, 0), (sv.LEADING_ZERO_BYTES, 0)] + [(m, d) for m in (sv.LEADING_DIGIT, sv.COUNT_DIGIT) for d in range(16)]


def test_every_metric_on_crafted_and_random_payloads_equals_the_digit_by_digit_model(shim):
    payloads = sv.crafted_payloads() + sv.random_payloads(4000)
    blob = b"".join(payloads)
    out = (ctypes.c_uint32 * len(payloads))()
    for m, d in all_metrics():
        shim.score_shim_metric_many(m, d, blob, len(payloads), out)
        want = [sv.metric(m, d, p) for p in payloads]
        got = list(out)
        bad = [(p.hex(), g, w) for p, g, w in zip(payloads, got, want) if g != w]
        assert not bad, (m, d, bad[:5])


def test_a_one_above_a_zero_byte_is_not_a_zero_byte(shim):
    """What the borrowing form (x - 0x01010101) & ~x & 0x80808080 gets wrong."""
    for at in range(19):
        p = bytearray([0x33] * 20)
        p[at], p[at + 1] = 0x01, 0x00
        assert shim.score_shim_metric(sv.ZERO_BYTES, 0, bytes(p)) == 1, at
        p[at], p[at + 1] = 0x10, 0x00
        assert shim.score_shim_metric(sv.COUNT_DIGIT, 0, bytes(p)) == 3, at
        p[at], p[at + 1] = 0x11, 0x00   # digit 1 above digit 0, four times over
        assert shim.score_shim_metric(sv.COUNT_DIGIT, 0, bytes(p)) == 2, at


def test_conjunctions_and_the_score_are_the_models(shim):
    payloads = sv.crafted_payloads()[::7] + sv.random_payloads(600, seed=11)
    specs = ["score:zero-bytes>=2", "score:leading-zero-bytes>=1&zero-bytes>=2", "score:count:0>=5&leading:0>=1&zero-bytes>=1&count:f>=1",
             "score:leading:f>=1&count:f>=3", "score:count:a>=0", "score:zero-bytes>=20", "score:leading:5>=1&count:a>=1"]
    for spec in specs:
        terms = sv.parse(spec)
        flat = (ctypes.c_uint32 * (3 * len(terms)))(*[v for t in terms for v in t])
        hits = 0
        for p in payloads:
            sc = ctypes.c_uint32(99)
            ok = shim.score_shim_eval(len(terms), flat, p, ctypes.byref(sc))
            assert ok == int(sv.accepts(spec, p)) and sc.value == sv.score(spec, p), (spec, p.hex())
            hits += ok
        assert 0 < hits, spec


# ---- the host filter ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", HEX_FORMATS)
def test_filter_matches_which_and_score_agree_with_the_model(vg, L, fmt):
    payloads = sv.crafted_payloads()[::5] + sv.random_payloads(500, seed=fmt)
    for spec in ["score:zero-bytes>=2", "score:leading:0>=3&count:0>=6", "score:count:f>=4", "score:leading-zero-bytes>=1&zero-bytes>=3"]:
        p = vg.Pattern(spec, fmt=vg.AddressFormat(fmt))
        n_hit = 0
        for pl in payloads:
            a = addr(vg, pl, fmt)
            want = sv.accepts(spec, pl)
            assert p.matches(a) == want, (spec, a)
            idx, n = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
            assert L.vgen_filter_which(p._h, a.encode(), idx, 4, ctypes.byref(n)) == 0
            assert (n.value, idx[0]) == ((1, 0) if want else (0, 0))
            assert p.score(a) == sv.score(spec, pl)
            n_hit += want
        assert 0 < n_hit < len(payloads)


def test_a_string_that_is_no_address_matches_nothing_and_has_no_score(vg, L):
    p = vg.Pattern("score:zero-bytes>=0", fmt=vg.AddressFormat.Ethereum)
    good = addr(vg, bytes(20))
    assert p.matches(good) and p.score(good) == 20
    v = ctypes.c_uint32()
    for s in ["", "0x", good[:-1], good + "0", "1x" + good[2:], good[:10] + "g" + good[11:], "1BoatSLRHtKNngkdXEeobR76b53LETtpyT"]:
        assert not p.matches(s), s
        assert L.vgen_score(p._h, s.encode(), ctypes.byref(v)) == E_INVALID, s
    plain = vg.Pattern("^0x00", fmt=vg.AddressFormat.Ethereum)
    assert L.vgen_score(plain._h, good.encode(), ctypes.byref(v)) == E_INVALID
    assert vg.score("score:count:0>=1", good) == 40
    assert vg.score(p, good) == 20


def test_leading_zero_digits_accept_exactly_what_the_prefix_filter_accepts(vg):
    s4, r4 = vg.Pattern("score:leading:0>=4", fmt=vg.AddressFormat.Ethereum), vg.Pattern("^0x0000", fmt=vg.AddressFormat.Ethereum)
    rng = random.Random(4)
    n = 0
    for i in range(4000):
        pl = bytearray(rng.getrandbits(8) for _ in range(20))
        z = i % 8                                    # 0 .. 7 leading zero digits forced
        for k in range(z):
            pl[k // 2] &= 0x0f if k % 2 == 0 else 0xf0
        a = addr(vg, bytes(pl))
        assert s4.matches(a) == r4.matches(a), a
        n += r4.matches(a)
    assert 1000 < n < 3000


def tail(N, q, n):
    """payloads of (q + 1)^N with at least n of the N fields equal to one given value"""
    return sum(comb(N, k) * q ** (N - k) for k in range(n, N + 1))


def single_term_odds():
    out = []
    for n in range(21):
        out.append(("score:zero-bytes>=%d" % n, Fraction(tail(20, 255, n), 256 ** 20)))
        out.append(("score:leading-zero-bytes>=%d" % n, Fraction(1, 256 ** n)))
    for n in range(41):
        for h in "07f":
            out.append(("score:count:%s>=%d" % (h, n), Fraction(tail(40, 15, n), 16 ** 40)))
            out.append(("score:leading:%s>=%d" % (h, n), Fraction(1, 16 ** n)))
    return out


def test_difficulty_of_every_single_term_is_the_exact_reciprocal_rounded_down(vg):
    for spec, p in single_term_odds():
        want = min((1 / p).__floor__(), 2 ** 64 - 1)
        assert vg.Pattern(spec, fmt=vg.AddressFormat.Ethereum).estimate_difficulty() == want, spec


def test_difficulty_of_a_conjunction_is_its_hardest_term_a_lower_bound(vg):
    d = lambda s: vg.Pattern(s, fmt=vg.AddressFormat.EthereumCreate2).estimate_difficulty()
    assert d("score:zero-bytes>=3&leading:0>=2&count:0>=9") == max(d("score:zero-bytes>=3"), d("score:leading:0>=2"), d("score:count:0>=9"))
    assert d("score:leading:0>=2&zero-bytes>=0") == 256


@pytest.fixture(scope="module")
def coretest():
    from conftest import locked_make
    locked_make("-s", "-C", os.path.join(ROOT, "tests", "native"), "libcoretest.so")
    return ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libcoretest.so"))


def selectivity(coretest, spec, fmt=5):
    kind, sel = ctypes.c_int(), ctypes.c_double()
    assert coretest.core_filter_check(spec.encode(), 0, fmt, b"", 0, None, ctypes.byref(kind), ctypes.byref(sel)) == 0 and kind.value == 6
    return sel.value


def test_selectivity_of_every_single_term_is_the_exact_fraction(coretest):
    """The filter turns an exact 160-bit count of payloads into a double: four limbs, one rounding each, and the division by 2^160 is
    exact — a few units in the last place of a double (2^-53) at the most, far inside 1e-13."""
    for spec, p in single_term_odds():
        got = selectivity(coretest, spec)
        assert abs(got - float(p)) <= 1e-13 * float(p), (spec, got, float(p))


def test_selectivity_of_a_conjunction_is_its_rarest_term_an_upper_bound(coretest):
    parts = ["score:zero-bytes>=3", "score:leading:0>=2", "score:count:0>=9"]
    assert selectivity(coretest, "score:zero-bytes>=3&leading:0>=2&count:0>=9", 7) == min(selectivity(coretest, s, 7) for s in parts)
