"""Split-key search on the host, without a device: vgen_split_derive / vgen_split_combine, the parsing of a base point
(vgen_set_base_point's refusals, reached through vgen_split_derive, which parses with the same function) and the per-dispatch
uniform points of the sequential walk with a base (vg::host_seq_points, tests/native/splitkey_shim.cpp built by
tests/native/splitkey.mk).

Expected values are the oracle's for the effective key (s + k) mod n (tests/splitkey_vectors.py); images from Python integers with
the published lambda.  Nothing comes from the code under test."""
import ctypes
import os
import random

import pytest

import vgen_amd as vg
from oracle import pyoracle as vo
from tests import splitkey_vectors as sv

N, P = sv.N, sv.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "libsplitkeytest.so")
E_INVALID, E_RANGE, E_UNSUPPORTED = -1, -7, -8


def pairs(fmt, n):
    rnd = random.Random(0x5EED0 + fmt)
    out = [(rnd.randrange(1, N), rnd.randrange(0, N)) for _ in range(n)]
    s = rnd.randrange(2, N)
    return out + [(s, 0), (s, N - 1), (N - 1, N - 1), (1, 1), (s, N - s + 1)]       # no partial, wraps s + k > n, e = 2 and e = 1


@pytest.mark.parametrize("fmt", sv.KEY_FORMATS)
def test_split_derive_is_the_oracles_address_of_the_effective_key(fmt):
    # a few hundred (s, k) over the formats, every image of each: 60 pairs per format of the oracle's own, 30 for formats 6 and 10
    for s, k in pairs(fmt, 55 if fmt <= 5 else 25):
        e = (s + k) % N
        pub = vo.pubkey(s)
        for v in range(sv.images_of(fmt)):
            want = sv.address_of_key(fmt, sv.image_key(e, v))
            assert vg.split_derive(fmt, pub, k, v) == want, (fmt, hex(s), hex(k), v)
        assert vg.split_derive(fmt, sv.pub33(s), k, 0) == vg.split_derive(fmt, pub, k, 0)     # 33 and 65 bytes of one P
        assert vg.split_derive(fmt, pub.hex(), k) == sv.address_of_key(fmt, e)


def test_split_derive_wrap_zero_sum_and_bad_arguments():
    s = 0x1234567890ABCDEF << 100
    pub = vo.pubkey(s)
    assert vg.split_derive(0, pub, N - s, 0) is None                                           # s + k = 0 (mod n): VGEN_E_RANGE
    assert vg.split_derive(0, pub, N, 0) is None and vg.split_derive(0, pub, 2**256 - 1, 0) is None   # a partial key is below n
    assert vg.split_derive(0, pub, N - s + 5, 0) == vo.generate(0, 5)["address"]               # the wrap s + k > n is exact
    assert vg.split_derive(0, pub, s, 0) == vo.generate(0, 2 * s % N)["address"]               # k * G = P: a doubling
    for fmt, v in ((0, 6), (10, 3), (3, 7)):
        with pytest.raises(vg.VgenError) as e:
            vg.split_derive(fmt, pub, 1, v)
        assert e.value.status == E_INVALID
    for fmt in (7, 8, 9, 11):                                                                   # CREATE2 has no key; unknown formats
        with pytest.raises(vg.VgenError) as e:
            vg.split_derive(fmt, pub, 1, 0)
        assert e.value.status == E_UNSUPPORTED


def no_root_x():
    """An x below p whose x^3 + 7 is no square."""
    x = 5
    while pow((x**3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    return x


PUB = vo.pubkey(0xC0FFEE)
X, Y = PUB[1:33], PUB[33:]
BAD_POINTS = {
    "empty": b"",
    "32 bytes": PUB[:32],
    "34 bytes": sv.pub33(0xC0FFEE) + b"\x00",
    "64 bytes": PUB[1:],
    "66 bytes": PUB + b"\x00",
    "prefix 00": b"\x00" + X,
    "prefix 05 (33)": b"\x05" + X,
    "prefix 02 on 65 bytes": b"\x02" + X + Y,
    "prefix 04 on 33 bytes": b"\x04" + X,
    "hybrid 06": bytes([6 + (Y[-1] & 1)]) + X + Y,
    "hybrid 07": bytes([7 - (Y[-1] & 1)]) + X + Y,
    "x = p": b"\x02" + P.to_bytes(32, "big"),
    "x = p + 1 (65)": b"\x04" + (P + 1).to_bytes(32, "big") + Y,
    "y >= p": b"\x04" + X + (2**256 - 1).to_bytes(32, "big"),
    "x without a root": b"\x03" + no_root_x().to_bytes(32, "big"),
    "off the curve": b"\x04" + X + (int.from_bytes(Y, "big") ^ 1).to_bytes(32, "big"),
    "negated x": b"\x04" + (P - int.from_bytes(X, "big")).to_bytes(32, "big") + Y,
}


@pytest.mark.parametrize("name", sorted(BAD_POINTS))
def test_a_bad_base_point_is_refused(name):
    pub = BAD_POINTS[name]
    out = ctypes.create_string_buffer(128)
    from vgen_amd import api
    assert api._L.vgen_split_derive(0, pub, len(pub), (1).to_bytes(32, "big"), 0, out, 128) == E_INVALID
    # ... and the well-formed keys are accepted, both parities
    for k in (0xC0FFEE, 0xC0FFEF, 0xC0FFF0):
        assert vg.split_derive(0, sv.pub33(k), 1, 0) == vg.split_derive(0, vo.pubkey(k), 1, 0) == vo.generate(0, k + 1)["address"]


@pytest.mark.parametrize("fmt", sv.KEY_FORMATS)
def test_split_combine_round_trip_and_refusals(fmt):
    rnd = random.Random(0xC0B1 + fmt)
    for s, k in [(rnd.randrange(1, N), rnd.randrange(0, N)) for _ in range(6)] + [(N - 5, 2**65 + 12345)]:
        e = (s + k) % N
        images = sv.images_of(fmt) if fmt != vo.FMT_P2TR else 3            # x-only output keys: (x, y) and (x, -y) share an address
        for v in range(images):
            key = sv.image_key(e, v)
            addr = sv.address_of_key(fmt, key)
            assert vg.split_combine(fmt, s, k, addr) == (key, v)
            assert sv.address_of_key(fmt, vg.split_combine(fmt, s, k, vg.split_derive(fmt, vo.pubkey(s), k, v))[0]) == addr
        addr = sv.address_of_key(fmt, e)
        for args in ((s, k, sv.address_of_key(fmt, (e + 1) % N or 1)), (s % (N - 1) + 1, k, addr), (s, (k + 1) % N, addr)):
            with pytest.raises(vg.VgenError) as err:                          # a wrong address, a wrong secret, a wrong partial key
                vg.split_combine(fmt, *args)
            assert err.value.status == E_INVALID
    for s, k in ((0, 5), (N, 5), (5, N), (5, N - 5)):                        # no secret, no partial key, a zero sum
        with pytest.raises(vg.VgenError) as err:
            vg.split_combine(fmt, s, k, "x")
        assert err.value.status == E_RANGE


# ---- the walk's uniform points with a base --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shim():
    assert os.path.exists(SHIM), f"{SHIM} not built (make -C tests/native -f splitkey.mk, or __graft_entry__.build())"
    L = ctypes.CDLL(SHIM)
    L.seqpts_new.restype = ctypes.c_void_p
    L.seqpts_free.argtypes = [ctypes.c_void_p]
    L.seqpts_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint)]
    return L


def points(L, cache, kb, S, base):
    out, st = ctypes.create_string_buffer(64 * S), ctypes.c_uint()
    rc = L.seqpts_get(cache, kb.to_bytes(32, "big"), S, base, len(base) if base else 0, out, ctypes.byref(st))
    return rc, [out.raw[64 * j:64 * j + 64] for j in range(S)], (st.value >> 8, st.value & 255)


def want_points(e, S):
    return [vo.pubkey((e + j) % N)[1:] for j in range(S)]


def test_host_seq_points_with_a_base_through_the_look_ahead(shim):
    S, stride = 8, 12 * 16384
    s = 0x7A3B << 200 | 0x1357
    base, kb = vo.pubkey(s), 2**65 + 12345 + 8192 - 4
    cache = shim.seqpts_new()
    ahead_used = 0
    for d in range(40):                                   # 40 consecutive dispatches at a constant stride
        rc, got, (pos, fill) = points(shim, cache, kb + d * stride, S, base)
        assert rc == 1 and got == want_points(s + kb + d * stride, S), d
        ahead_used += pos > 0
    assert ahead_used >= 24                               # ... most of them handed out by the look-ahead (eight per refill)
    kb2 = kb + 40 * stride
    for d in range(12):                                   # a stride change
        rc, got, _ = points(shim, cache, kb2 + d * 16384, S, base)
        assert rc == 1 and got == want_points(s + kb2 + d * 16384, S), d
    s2 = N - 77
    for b, e0 in ((sv.pub33(s2), s2), (None, 0), (base, s)):      # a base change in mid-walk (33-byte form), to no base, and back
        for d in range(12, 24):
            rc, got, _ = points(shim, cache, kb2 + d * 16384, S, b)
            assert rc == 1 and got == want_points(e0 + kb2 + d * 16384, S), (e0, d)
    shim.seqpts_free(cache)


def test_host_seq_points_at_the_bases_own_exceptions(shim):
    S, kb = 8, 2**65 + 12345 + 8192 - 4
    cache = shim.seqpts_new()
    rc, got, _ = points(shim, cache, kb, S, vo.pubkey(kb))                      # kb * G = P: the seed addition is a doubling
    assert rc == 1 and got == want_points(2 * kb, S)
    rc, got, _ = points(shim, cache, kb, S, vo.pubkey(N - kb - 3))              # effective keys -3 .. 4: the point at infinity inside
    assert rc == 0
    rc, got, _ = points(shim, cache, kb, S, vo.pubkey(N - kb - 5000))           # the zero crossing S keys ahead: exact on both sides
    assert rc == 1 and got == want_points(N - 5000, S)
    rc, got, _ = points(shim, cache, kb + 16384, S, vo.pubkey(N - kb - 5000))
    assert rc == 1 and got == want_points(N - 5000 + 16384, S)
    assert points(shim, cache, kb, S, b"\x02" + P.to_bytes(32, "big"))[0] == -1
    shim.seqpts_free(cache)
