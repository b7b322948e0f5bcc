"""Crafted payloads for the two headers that decide whether a key is reported - core/filter_eval.h (hash160 ranges, Bech32 /
hex masks) and core/dfa_eval.h (the full matcher) - and references that share no code with them.  No tests here: the CPU
module (tests/test_match_edges.py, the headers as g++ compiles them) and the GPU module (tests/test_gpu_match_device.py, as
hipcc compiles them, behind tests/native/match_dev.hip) both run these cases and make the same assertions.

References.  The address of a payload is the oracle's (oracle/pyoracle.py); the exact verdict is the oracle's regex on it.
Ranges and masks are re-evaluated here on Python integers from the compiled tests as the host build exports them
(core_filter_tests): any(lo <= H <= hi), any((H & mask) == value and (chk & chk_mask) == chk_value), the Bech32 checksum
read back from the last six characters of the oracle's address.  Ethereum's device automaton is the case-folded language:
Python `re` with re.I on "0x" + hex.

What the vectors pin (a .. f below): a payload at, next to and one word away from every range bound, and payloads that share
their leading word with a bound; the same from the Base58 value of prefix + '1' * k and prefix + 'z' * k; waves with no, one
and only `near` lanes; masks on every single-bit neighbour of a payload, checksum bits included; zero runs of every length;
values at 58^(5c); divmod_d5 at its quotient edges.  No case may pass vacuously: the reference alone accepts at least 3 and
rejects at least 3 payloads of every pattern that can match at all, and a range case has an accepted and a rejected vector
within 2 of a bound."""
import ctypes
import functools
import json
import os
import random
import re

from conftest import locked_make

from oracle import pyoracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BECH32 = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
HEXL = "0123456789abcdef"
M32, M160 = (1 << 32) - 1, (1 << 160) - 1
D5 = 58 ** 5
HEAD = {1: 4, 3: 4, 5: 2}                       # characters every address of the format shares ("bc1q", "bc1p", "0x")
VERSION = {0: 0, 4: 0, 2: 5}
MIN_ACCEPT = MIN_REJECT = 3
GOLDEN = json.load(open(os.path.join(HERE, "golden", "match_edges.json")))


def payload_len(fmt):
    return 32 if fmt == 3 else 20


@functools.lru_cache(maxsize=None)
def address(fmt, payload):
    return vo.segwit_addr("bc", 1, payload) if fmt == 3 else vo.address_from_hash160(fmt, payload)


def value(payload):
    return int.from_bytes(payload, "big")


def b58_value(s):
    v = 0
    for c in s:
        v = v * 58 + B58.index(c)
    return v


# ---- the host build of the headers and of the filter compiler ------------------------------------------------------------

_core = None


def core():
    global _core
    if _core is None:
        locked_make("-s", "-C", os.path.join(HERE, "native"), "libcoretest.so")
        lib = ctypes.CDLL(os.path.join(HERE, "native", "libcoretest.so"))
        lib.core_filter_check.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_char_p, ctypes.c_int,
                                          ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
        lib.core_dfa_check.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
        lib.core_filter_tests.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
        _core = lib
    return _core


class Compiled:
    """The device tests of one compiled pattern, as integers over the payload's big-endian words."""


@functools.lru_cache(maxsize=None)
def compiled(pattern, ci, fmt):
    hdr, raw = (ctypes.c_uint32 * 6)(), (ctypes.c_uint32 * (64 * 18))()
    assert core().core_filter_tests(pattern.encode(), int(ci), fmt, hdr, raw) == 0, pattern
    c = Compiled()
    c.kind, c.flags, c.count, c.witver, c.has_lut, c.dfa_bytes = list(hdr)
    nw = payload_len(fmt) // 4
    join = lambda ws: functools.reduce(lambda v, w: (v << 32) | w, ws, 0)
    c.tests = []
    for t in range(c.count if c.kind in (1, 2) else 0):
        o = raw[18 * t:18 * t + 18]
        assert not any(o[nw:8]) and not any(o[8 + nw:16])      # nothing beyond the payload's words
        c.tests.append((join(o[:nw]), join(o[8:8 + nw]), o[16], o[17]))
    c.header = list(hdr)
    return c


def host_run(case):
    """The case through the host build: the device test's verdict per payload (the prefilter, or the full matcher for kind
    4), and the product's own exact automaton on the product's own encoding of the address."""
    n = len(case.payloads)
    flags = ctypes.create_string_buffer(n)
    blob = b"".join(case.payloads)
    if compiled(case.pattern, case.ci, case.fmt).kind == 4:
        assert core().core_dfa_check(case.pattern.encode(), int(case.ci), case.fmt, blob, n, flags) == 4
    else:
        kind, sel = ctypes.c_int(), ctypes.c_double()
        assert core().core_filter_check(case.pattern.encode(), int(case.ci), case.fmt, blob, n, flags, ctypes.byref(kind), ctypes.byref(sel)) == 0
    return [b & 1 for b in flags.raw], [(b >> 1) & 1 for b in flags.raw]


# ---- references ----------------------------------------------------------------------------------------------------------

def chk_of(addr):
    """The 30 checksum bits of a Bech32(m) address, first checksum symbol in bits 29..25."""
    return functools.reduce(lambda v, ch: (v << 5) | BECH32.index(ch), addr[-6:], 0)


def model(c, fmt, payloads, addrs):
    if c.kind == 1:
        return [int(any(lo <= value(p) <= hi for lo, hi, _, _ in c.tests)) for p in payloads]
    assert c.kind == 2
    chks = [chk_of(a) if fmt in (1, 3) else 0 for a in addrs]
    return [int(any((value(p) & m) == v and (chk & cm) == cv for m, v, cm, cv in c.tests)) for p, chk in zip(payloads, chks)]


class Case:
    def __init__(self, group, fmt, pattern, ci, payloads, kind=None, impossible=False):
        self.group, self.fmt, self.pattern, self.ci, self.kind, self.impossible = group, fmt, pattern, ci, kind, impossible
        self.payloads = list(dict.fromkeys(payloads)) if group != "b" else list(payloads)   # (a wave layout keeps its lanes)
        assert all(len(p) == payload_len(fmt) for p in self.payloads)

    @property
    def tag(self):
        return f"{self.group} format {self.fmt} {self.pattern!r}{' -i' if self.ci else ''}"


class Ref:
    pass


_refs = {}


def reference(case):
    """Computed once per case and shared.  want: what the device test must answer, payload by payload; exact: the oracle's
    verdict on the oracle's address.  The conditions that keep the case from passing vacuously are asserted here, on the
    reference alone."""
    if case.tag in _refs:
        return _refs[case.tag]
    c = compiled(case.pattern, case.ci, case.fmt)
    r = Ref()
    r.kind = c.kind
    assert case.kind is None or c.kind == case.kind, (case.tag, c.kind)
    assert c.kind in (1, 2, 4), (case.tag, c.kind)
    addrs = [address(case.fmt, p) for p in case.payloads]
    rx = vo.Regex(case.pattern, case.ci)
    r.exact = [int(rx.matches(a)) for a in addrs]
    if c.kind == 4:
        if case.fmt == 5:
            folded = re.compile(case.pattern, re.I)
            r.want = [int(folded.search("0x" + p.hex()) is not None) for p in case.payloads]
        else:
            r.want = r.exact
    else:
        r.want = model(c, case.fmt, case.payloads, addrs)
        if c.flags & 1:
            assert c.has_lut, case.tag        # a filter that tests the checksum carries its byte tables
    lost = [a for a, w, e in zip(addrs, r.want, r.exact) if e and not w]
    assert not lost, (case.tag, "the reference itself loses a match", lost[:3])
    r.accepted, r.rejected, r.matched = sum(r.want), len(r.want) - sum(r.want), sum(r.exact)
    r.at_bound = None
    if case.impossible:
        assert r.accepted == 0 and r.matched == 0, case.tag
    else:
        assert r.accepted >= MIN_ACCEPT and r.rejected >= MIN_REJECT, (case.tag, r.accepted, r.rejected)
    if c.kind == 1:
        bounds = [b for lo, hi, _, _ in c.tests for b in (lo, hi)]
        close = [w for p, w in zip(case.payloads, r.want) if min(abs(value(p) - b) for b in bounds) <= 2]
        r.at_bound = (sum(close), len(close) - sum(close))
        assert r.at_bound[0] >= 1 and r.at_bound[1] >= 1, (case.tag, r.at_bound)
    _refs[case.tag] = r
    return r


def check(case, got, who):
    """The assertions both builds must meet, `got` being one verdict per payload."""
    r = reference(case)
    assert len(got) == len(r.want)
    bad = [i for i, (g, w) in enumerate(zip(got, r.want)) if g != w]
    assert not bad, (case.tag, who, len(bad), [(case.payloads[i].hex(), got[i], r.want[i]) for i in bad[:4]])
    assert all(g or not e for g, e in zip(got, r.exact)), (case.tag, who, "rejected a real match")
    return r


def line(case, r):
    at = f", {r.at_bound[0]} accepted and {r.at_bound[1]} rejected within 2 of a bound" if r.at_bound else ""
    return f"{case.tag}: kind {r.kind}, {len(r.want)} payloads, {r.accepted} accepted ({r.matched} exact matches), {r.rejected} rejected{at}"


# ---- a. range bounds -----------------------------------------------------------------------------------------------------
# pattern -> the literal prefixes it accepts (for the string-derived vectors)

RANGE_PATTERNS = {
    0: [("^1Cat", ["1Cat"]), ("^11", ["11"]), ("^111", ["111"]), ("^1z", ["1z"]), ("^1QLb", ["1QLb"]), ("^12", ["12"]),
        ("^1zzzz", ["1zzzz"]), ("^1[1-3]", ["11", "12", "13"]), ("^1Cat|^1Dog", ["1Cat", "1Dog"])],
    2: [("^3Cat", ["3Cat"]), ("^31", ["31"]), ("^3R", ["3R"]), ("^3Q", ["3Q"]), ("^32", ["32"])],
    4: [("^1Dog", ["1Dog"])],
}


def h160(v):
    return v.to_bytes(20, "big")


def string_vectors(fmt, prefixes):
    """The Base58 value of prefix + '1' * k and prefix + 'z' * k for every total length 26 .. 35, without its four checksum
    bytes, and the values 1 and 2 away; kept where the version byte is the format's."""
    out = []
    for p in prefixes:
        for total in range(26, 36):
            for fill in "1z":
                v = b58_value(p + fill * (total - len(p))) >> 32
                out += [x & M160 for x in (v - 2, v - 1, v, v + 1, v + 2) if x >= 0 and x >> 160 == VERSION[fmt]]
    return out


def bound_vectors(c, rng):
    """From the exported ranges: every bound, the values next to it, the bound with one of its five words one up or down,
    and 32 payloads that share the leading word of a bound (so that words 1 - 4 of the comparison decide)."""
    out = []
    bounds = [b for lo, hi, _, _ in c.tests for b in (lo, hi)]
    for b in bounds:
        out += [x for x in (b - 1, b, b + 1) if 0 <= x <= M160]
        for i in range(5):
            sh = 32 * (4 - i)
            w = (b >> sh) & M32
            out += [b & ~(M32 << sh) | (((w + d) & M32) << sh) for d in (1, -1)]
    for k in range(32):
        out.append(bounds[k % len(bounds)] >> 128 << 128 | rng.getrandbits(128))
    return out


def is_near(c, v):
    return any(lo >> 128 <= v >> 128 <= hi >> 128 for lo, hi, _, _ in c.tests)


def far_values(c, rng, n):
    """Random values whose leading word lies in no range's [lo_0, hi_0]."""
    out = []
    for _ in range(100 * n):
        v = rng.getrandbits(160)
        if not is_near(c, v):
            out.append(v)
            if len(out) == n:
                return out
    raise AssertionError("the ranges leave no room for far payloads")


@functools.lru_cache(maxsize=None)
def range_values(fmt, pattern):
    prefixes = dict(RANGE_PATTERNS[fmt])[pattern]
    c = compiled(pattern, False, fmt)
    assert c.kind == 1 and 1 <= c.count <= 64, (pattern, c.kind, c.count)
    rng = random.Random(f"a/{fmt}/{pattern}")
    return list(dict.fromkeys(bound_vectors(c, rng) + string_vectors(fmt, prefixes) + far_values(c, rng, 8)))


def range_cases():
    return [Case("a", fmt, pat, False, [h160(v) for v in range_values(fmt, pat)], kind=1) for fmt in RANGE_PATTERNS for pat, _ in RANGE_PATTERNS[fmt]]


# ---- b. wave layouts -----------------------------------------------------------------------------------------------------

LONE_LANES = (0, 31, 32, 63)


def wave_case(fmt, pattern):
    """The vectors of (a) as waves of 64 consecutive payloads: waves without a `near` lane (the wave skips the five-word
    comparison), waves with exactly one near lane at lane 0, 31, 32 or 63 (63 lanes run a comparison they did not need),
    waves of near lanes only, a wave without one again, and a ragged last wave of 10 with its near lane first."""
    c = compiled(pattern, False, fmt)
    rng = random.Random(f"b/{fmt}/{pattern}")
    vectors = range_values(fmt, pattern)
    near = [v for v in vectors if is_near(c, v)]
    far_pool = [v for v in vectors if not is_near(c, v)] + far_values(c, rng, 256)
    far = lambda: rng.choice(far_pool)
    assert len(near) >= 8
    lanes = []
    for _ in range(2):
        lanes += [far() for _ in range(64)]
    for j, v in enumerate(near[:64]):
        wave = [far() for _ in range(64)]
        wave[LONE_LANES[j % 4]] = v
        lanes += wave
    full = near + [rng.choice(near) for _ in range(-len(near) % 64)]
    lanes += full
    lanes += [far() for _ in range(64)]
    lanes += [near[0]] + [far() for _ in range(9)]
    case = Case("b", fmt, pattern, False, [h160(v) for v in lanes], kind=1)
    per_wave = [[is_near(c, v) for v in lanes[w:w + 64]] for w in range(0, len(lanes), 64)]
    case.shape = {"none": sum(1 for w in per_wave if len(w) == 64 and not any(w)),
                  "lone": sorted({w.index(True) for w in per_wave if len(w) == 64 and sum(w) == 1}),
                  "all": sum(1 for w in per_wave if len(w) == 64 and all(w)),
                  "ragged": (len(per_wave[-1]), sum(per_wave[-1]))}
    assert case.shape["none"] >= 3 and case.shape["lone"] == sorted(LONE_LANES) and case.shape["all"] >= 1 and case.shape["ragged"] == (10, 1), case.shape
    return case


def wave_cases():
    return [wave_case(fmt, pat) for fmt in RANGE_PATTERNS for pat, _ in RANGE_PATTERNS[fmt]]


# ---- c / e. fixed-length symbol strings: Bech32, Bech32m, hex ---------------------------------------------------------------

def symbols(fmt):
    return (HEXL, 4) if fmt == 5 else (BECH32, 5)


@functools.lru_cache(maxsize=None)
def symbol_payloads(fmt):
    """One random payload, every single-bit neighbour of it (160 or 256), 256 random payloads, and 64 payloads that differ
    from the first in several bits behind bit 40 and before the last 16 bits and keep its whole checksum: found by Gaussian
    elimination over the checksum differences of the single-bit neighbours, the checksums being read from the oracle's
    addresses (the checksum is affine in the payload bits).  Without them a pattern on checksum symbols would accept the
    first payload alone."""
    rng = random.Random(4000 + fmt)
    nbits = 8 * payload_len(fmt)
    base = rng.getrandbits(nbits)
    raw = lambda v: v.to_bytes(nbits // 8, "big")
    flips = [base ^ (1 << (nbits - 1 - i)) for i in range(nbits)]
    chk = (lambda v: chk_of(address(fmt, raw(v)))) if fmt != 5 else (lambda v: 0)
    c0 = chk(base)
    pivots, kernel = {}, []          # leading bit of a checksum difference -> (difference, payload mask)
    for i in range(40, nbits - 16):
        d, m = chk(flips[i]) ^ c0, 1 << (nbits - 1 - i)
        while d:
            top = d.bit_length()
            if top not in pivots:
                pivots[top] = (d, m)
                break
            d, m = d ^ pivots[top][0], m ^ pivots[top][1]
        if not d:
            kernel.append(m)
    assert len(kernel) >= 64
    same = [base ^ functools.reduce(lambda a, b: a ^ b, rng.sample(kernel, rng.randrange(1, 4))) for _ in range(64)]
    assert all(chk(v) == c0 for v in same)
    rand = [rng.getrandbits(nbits) for _ in range(256)]
    return raw(base), [raw(v) for v in [base] + flips + rand + same]


def plant(fmt, rng, pieces):
    """A random payload with the pieces' symbols written over it: pieces = [(first data symbol, text), ...]."""
    alphabet, bits = symbols(fmt)
    nbits = 8 * payload_len(fmt)
    v = rng.getrandbits(nbits)
    for pos, text in pieces:
        for k, ch in enumerate(text.lower()):
            sh = nbits - bits * (pos + k + 1)
            assert sh >= 0
            v = v & ~(((1 << bits) - 1) << sh) | (alphabet.index(ch) << sh)
    return v.to_bytes(nbits // 8, "big")


def mask_cases(fmt):
    """(c) Patterns grown from the first payload's own address: a prefix of 1 - 4 characters behind the head, a suffix of 1 - 4
    (checksum symbols for Bech32; matched in either case for Ethereum), prefix-and-suffix pairs; P2TR: a suffix of seven, which
    reaches the 52nd data symbol with its four pad bits, and the two patterns on that symbol alone."""
    base, payloads = symbol_payloads(fmt)
    a, head, ci = address(fmt, base), HEAD[fmt], fmt == 5
    cases = []
    for k in range(1, 5):
        cases.append(Case("c", fmt, "^" + a[:head + k], False, payloads, kind=2))
        cases.append(Case("c", fmt, a[-k:] + "$", ci, payloads, kind=2))
    cases.append(Case("c", fmt, "^" + a[:head + 1] + ".*" + a[-3:] + "$", ci, payloads, kind=2))
    cases.append(Case("c", fmt, "^" + a[:head + 2] + ".*" + a[-1:] + "$", ci, payloads, kind=2))
    if fmt == 3:
        cases.append(Case("c", fmt, a[-7:] + "$", False, payloads, kind=2))
        # the 52nd data symbol holds one payload bit and four pad bits: only 'q' and 's' can appear there
        cases.append(Case("c", fmt, "^bc1p.{51}q", False, payloads))
        cases.append(Case("c", fmt, "^bc1p.{51}[as]", False, payloads))                     # 'a' cannot appear: 's' alone is left
        cases.append(Case("c", fmt, "^bc1p.{51}[ac]", False, payloads, impossible=True))    # neither can: nothing matches
    return cases


SYMBOL_PATTERNS = {
    # pattern -> plants (pieces per planted payload); a near miss of every plant (its last symbol changed) is added too
    1: {"dead": [[(0, "dead")], [(7, "dead")], [(28, "dead")]], "q{3}": [[(1, "qqq")], [(14, "qqq")], [(29, "qqq")]], "[0-9]{5}": [],
        "xyz.*acd": [[(0, "xyz"), (3, "acd")], [(5, "xyz"), (20, "acd")], [(11, "xyz"), (29, "acd")]]},
    3: {"dead": [[(0, "dead")], [(7, "dead")], [(47, "dead")]], "q{3}": [[(1, "qqq")], [(14, "qqq")], [(48, "qqq")]], "[0-9]{5}": [],
        "xyz.*acd": [[(0, "xyz"), (3, "acd")], [(5, "xyz"), (20, "acd")], [(11, "xyz"), (48, "acd")]], "bc1p.*p$": []},
    # Ethereum: 'q', 'x', 'y', 'z' are no hex digits, so the two patterns that use them can match nothing there (kept, as cases
    # that must reject everything); "a{3}" and "abc.*def" take their place
    5: {"dead": [[(0, "dead")], [(7, "dead")], [(36, "dead")]], "a{3}": [[(1, "aaa")], [(14, "aaa")], [(37, "aaa")]], "[0-9]{5}": [],
        "abc.*def": [[(0, "abc"), (3, "def")], [(5, "abc"), (20, "def")], [(11, "abc"), (37, "def")]]},
}
SYMBOL_IMPOSSIBLE = {5: ["q{3}", "xyz.*acd"]}


def full_symbol_cases(fmt):
    """(e) The full matcher over Bech32 / Bech32m / hex: unanchored patterns, each with payloads that carry it at the first, an
    odd and the last possible symbol, and a piece of the first payload's own address that straddles the end of the data part
    (Ethereum has no checksum: a piece that straddles a word boundary of the payload)."""
    base, payloads = symbol_payloads(fmt)
    a = address(fmt, base)
    alphabet, _ = symbols(fmt)
    cases = []
    for pat, plants in SYMBOL_PATTERNS[fmt].items():
        rng = random.Random(f"e/{fmt}/{pat}")
        extra = []
        for pieces in plants:
            extra.append(plant(fmt, rng, pieces))
            pos, text = pieces[-1]
            miss = text[:-1] + next(ch for ch in alphabet if ch not in "qdeacfzyx0123456789" and ch != text[-1])
            extra.append(plant(fmt, rng, pieces[:-1] + [(pos, miss)]))
        cases.append(Case("e", fmt, pat, False, payloads + extra, kind=2 if pat == "bc1p.*p$" else 4))   # (a suffix: masks on the checksum)
    for pat in SYMBOL_IMPOSSIBLE.get(fmt, []):
        cases.append(Case("e", fmt, pat, False, payloads, impossible=True))
    if fmt == 5:
        cases.append(Case("e", fmt, a[2 + 6:2 + 10], True, payloads, kind=4))
    else:
        end = len(a) - 6
        cases.append(Case("e", fmt, a[end - 2:end + 2], False, payloads, kind=4))
    return cases


# ---- d. the full matcher, Base58Check -----------------------------------------------------------------------------------------

def planted_base58(fmt, rng, at, text):
    """A hash160 whose address carries `text` from character `at` on: the value of a string with it, without the four checksum
    bytes (the real checksum moves the last six or seven characters only)."""
    while True:
        lead = "1" + rng.choice("23456789ABCDEFGH") if VERSION[fmt] == 0 else "3" + rng.choice("23456789ABCDEFGHJKLMNP")
        s = lead + "".join(rng.choice(B58[1:]) for _ in range(32))
        s = s[:at] + text + s[at + len(text):]
        v = b58_value(s) >> 32
        if v >> 160 == VERSION[fmt]:
            return h160(v & M160)


@functools.lru_cache(maxsize=None)
def base58_payloads(fmt):
    """Zero runs of every length (0 .. 19 bytes, then 19 and a one, all zero), all ones, the values 58^(5c) >> 32 and their
    neighbours at 1 and at 1 + 2^j (the first non-zero digit sits at a chunk edge; below it the top chunk is empty), the first payload of the
    golden suffix search with its eight low single-bit neighbours (they share every character but the last few), and 1024
    random payloads."""
    rng = random.Random(5000 + fmt)
    out = [bytes(k) + rng.randbytes(20 - k) for k in range(20)]                     # (out[3]: full_base58_cases grows a pattern from it)
    out += [bytes(19) + b"\x01", b"\xff" * 20, bytes(20)]
    for c in range(1, 7):
        edge = D5 ** c >> 32
        out += [h160(x) for x in (edge - 1, edge, edge + 1) if x >= 0]
        out += [h160(x) for j in range(4) for x in (edge - 1 - (1 << j), edge + 1 + (1 << j)) if x >= 0]   # (5c and 5c + 1 digits)
    own = bytes.fromhex(GOLDEN[str(VERSION[fmt])]["own"][0])
    out += [h160(value(own) ^ (1 << j)) for j in range(8)]
    out += [h160(value(out[3]) ^ (1 << j)) for j in range(8)]        # (the same around the payload with three zero bytes)
    out += [rng.randbytes(20) for _ in range(1024)]
    out += [bytes(k) + rng.randbytes(20 - k) for k in range(1, 20) for _ in range(3)]   # three more of every run: the length patterns
    return out


LDS_PATTERN = "a.{9}b.c|d{12}"     # (tests/test_gpu_parity.py: an automaton of 46.7 KB, the LDS limit being 48 KiB)


# Patterns that count the digits behind the leading '1's, modulo 5: a digit lost or doubled where the `started` logic crosses
# from one five-digit chunk to the next changes the verdict on the values around 58^(5c), whatever the digits are.  (A P2SH
# payload always has 34 digits: these are for version 0.)
DIGITS_5C, DIGITS_5C_1 = "^1*[^1].{4}(.{5})*$", "^1*[^1](.{5})*$"
# Patterns on the whole length, leading '1's included: the two above throw the run away, and "11" and "1111" stop counting at
# four, so only these notice a run that comes out one too long or too short once it is longer than that (a zero digit of a
# lower chunk let through as a '1', a count that stops before the last zero byte).  26 and 27 are the lengths of the longest
# runs (19 zero bytes and more), 30 of a run of about ten.
LENGTHS = ["^.{30}$", "^.{26}$", "^.{27}$", "^(.{5})*$"]
# cases per format (the tests take them one by one: compiling an unanchored Base58 pattern takes 0.4 s)
BASE58_CASES = {0: 18, 2: 12, 4: 18}


@functools.lru_cache(maxsize=None)
def full_base58_cases(fmt):
    payloads = base58_payloads(fmt)
    gold = {k: [bytes.fromhex(h) for h in v] for k, v in GOLDEN[str(VERSION[fmt])].items()}
    first = "1" if VERSION[fmt] == 0 else "3"
    plants = {"11": ["11"], "1111": ["1111"], "Cat": ["Cat"], "1[Oo]ri": ["1ori", "1ori", "1oro"], "(?i)dead": ["dEaD", "DEAd", "dEaF"],
              LDS_PATTERN: ["a" + "x" * 9 + "bxc", "d" * 12, "aBCDEFGHJKbLc", "d" * 11 + "e"]}
    cases = []
    counted = [DIGITS_5C, DIGITS_5C_1] + LENGTHS if VERSION[fmt] == 0 else []
    for pat in ["11", "1111", "Cat", "1[Oo]ri", "abc$", "[0-9]{4}$", "^" + first + ".*7$", "(?i)dead", LDS_PATTERN] + counted:
        rng = random.Random(f"d/{fmt}/{pat}")
        extra = []
        for text in plants.get(pat, []):
            extra += [planted_base58(fmt, rng, at, text) for at in (2, 9, 20)]
        extra += gold["abc"] if pat == "abc$" else gold["digits4"] if pat == "[0-9]{4}$" else []
        cases.append(Case("d", fmt, pat, False, payloads + extra, kind=4))
    # grown from the vectors' own addresses: a middle piece of two of them, and the last three characters of one
    own = address(fmt, gold["own"][0])
    zeros = address(fmt, payloads[3])
    cases.append(Case("d", fmt, own[8:11], False, payloads, kind=4))
    cases.append(Case("d", fmt, zeros[10:13], False, payloads, kind=4))
    cases.append(Case("d", fmt, own[-3:] + "$", False, payloads + gold["own"], kind=4))
    assert compiled(LDS_PATTERN, False, fmt).dfa_bytes > 45000 and len(cases) == BASE58_CASES[fmt]
    return cases


# ---- f. divmod_d5 ------------------------------------------------------------------------------------------------------------------

def divmod_inputs():
    """(hi, lo) with hi < 58^5: q * 58^5 + r at the quotient's and the remainder's edges, the largest input, 2000 random."""
    rng = random.Random(6000)
    vals = [q * D5 + r for q in (0, 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1) for r in (0, 1, D5 - 1)]
    vals = [v for v in vals if v >> 32 < D5]
    assert len(vals) == 15
    vals.append((D5 - 1) << 32 | M32)
    vals += [rng.randrange(D5) << 32 | rng.getrandbits(32) for _ in range(2000)]
    return vals
