"""The host side of a split-key scan without a device: cabi.cpp and the scan loop of scanner.cpp over the CPU stand-in of the runtime
with split-key dispatches added (tests/native/splitkey_rt.cpp beside fake_rt.cpp, built into libvgen_fake_split.so by
tests/native/splitkey.mk), driven through the C ABI by a second instance of vgen_amd/api.py bound to that library.

What is checked: results carry the PARTIAL key as walked (hex = wif = "0x..."), an endomorphism index v * batch + i becomes the
partial key of slot i with the address of image v of the point, candidates whose payload the stand-in corrupts are dropped by the
host's re-derivation and counted, the refusals, and that clearing the base gives the plain scan back.  Expected keys and addresses
are the oracle's for the effective key (s + k) mod n (tests/splitkey_vectors.py): nothing of the code under test."""
import ctypes
import functools
import importlib.util
import os
import sys

import pytest

from oracle import pyoracle as vo
from tests import nostr_vectors as nv
from tests import splitkey_vectors as sv

ROOT = nv.ROOT
N = sv.N
SO = os.path.join(ROOT, "tests", "native", "libvgen_fake_split.so")
FMT = vo.FMT_P2PKH
BATCH = 8192
START = 2**65 + 12345
SECRET = 0x51C2E7 << 216 | 0xA11CE
SEED = 0x73706C6974
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -5, -8


@pytest.fixture(scope="module")
def vf():
    """vgen_amd/api.py over the stand-in's library (the mechanism of tests/conftest.py: hooks_api, with another library)."""
    assert os.path.exists(SO), f"{SO} not built (make -C tests/native -f splitkey.mk, or __graft_entry__.build())"
    spec = importlib.util.spec_from_file_location("vgen_amd_fake_split_api", os.path.join(ROOT, "vgen_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    mod._SO_OVERRIDE = SO
    sys.modules["vgen_amd_fake_split_api"] = mod     # (dataclasses look their module up there)
    spec.loader.exec_module(mod)
    assert mod.library_path() == SO
    mod._L.splitkey_rt_corrupt.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    mod._L.splitkey_rt_corrupt.restype = None
    return mod


def runner(vf, endo=False, base=SECRET, frames=2):
    r = vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=frames, endo=endo, timing=False)
    if base is not None:
        r.set_base(vo.pubkey(base))
    return r


@functools.lru_cache(maxsize=None)
def walk_addresses(first, b):
    """The oracle's addresses of the effective keys first + b * BATCH + i, i < BATCH."""
    return tuple(vo.address_from_hash160(FMT, bytes(pl)) for pl in sv.dump_of(FMT, first + b * BATCH, BATCH))


def walk_matches(secret, accept, count, skip=lambda k: False):
    """(partial key, address) of the first `count` partial keys from START whose effective key's address `accept`s."""
    out, b = [], 0
    while len(out) < count:
        out += [(START + b * BATCH + i, a) for i, a in enumerate(walk_addresses(secret + START, b))
                if accept(a) and not skip(START + b * BATCH + i)]
        b += 1
    return out[:count]


def check_partial(res, want):
    assert [(int(m.hex, 16), m.address) for m in res.matches] == want
    for m in res.matches:
        assert m.hex == m.wif == "0x%064x" % int(m.hex, 16) and int(m.format) == FMT


ACCEPT = lambda a: a.startswith("1A")   # noqa: E731


def test_results_carry_the_partial_key(vf):
    r = runner(vf)
    assert r.base == vo.pubkey(SECRET)
    want = walk_matches(SECRET, ACCEPT, 40)
    res = vf.scan_gpu_with_runner("^1A", vf.ScanConfig(format=FMT, count=40, start=START), r)
    check_partial(res, want)
    assert res.operations % BATCH == 0 and r.split_dropped == 0
    for m in res.matches[:5] + res.matches[-5:]:          # the requester's side: the final key is the oracle's key of that address
        key, v = vf.split_combine(FMT, SECRET, int(m.hex, 16), m.address)
        assert v == 0 and key == (SECRET + int(m.hex, 16)) % N and vo.generate(FMT, key)["address"] == m.address
        assert vf.split_derive(FMT, r.base, int(m.hex, 16), 0) == m.address
    r.close()


def test_a_wrap_of_the_effective_key_is_exact(vf):
    r = runner(vf, base=N - 5)                             # effective keys START - 5 ..
    want = walk_matches(N - 5, ACCEPT, 10)
    assert want[0][1] == vo.generate(FMT, want[0][0] - 5)["address"]
    check_partial(vf.scan_gpu_with_runner("^1A", vf.ScanConfig(format=FMT, count=10, start=START), r), want)
    r.close()


@functools.lru_cache(maxsize=None)
def random_batch(secret, seed, stream, b):
    """(partial key, address) of every slot of batch b of a six-image random-key scan under the base, image-major as the dispatch
    orders them: the partial key of slot v * BATCH + i is draw i itself, its address that of image v of the effective key."""
    draws = [vo.random_key(seed, stream, b * BATCH + i) for i in range(BATCH)]
    pts = [nv.xy_of((secret + k) % N) if 0 < k < N and (secret + k) % N else None for k in draws]
    out = []
    for v in range(6):
        out += [(k, vo.address_from_hash160(FMT, sv.payload_of_point(FMT, *sv.image_point(*pt, v)))) for k, pt in zip(draws, pts) if pt]
    return tuple(out)


def test_an_image_index_becomes_the_partial_key_of_its_slot(vf):
    r = runner(vf, endo=True)
    accept = lambda a: a.startswith("1Ab")   # noqa: E731
    want, b = [], 0
    while len(want) < 20:
        want += [(k, a) for k, a in random_batch(SECRET, SEED, 0, b) if accept(a)]
        b += 1
    res = vf.scan_gpu_with_runner("^1Ab", vf.ScanConfig(format=FMT, count=20, seed=SEED, random_keys=True), r)
    check_partial(res, want[:20])
    assert res.operations % (6 * BATCH) == 0
    variants = set()
    for m in res.matches:                                  # no image is applied to the key: the requester finds it
        k = int(m.hex, 16)
        key, v = vf.split_combine(FMT, SECRET, k, m.address)
        assert key == sv.image_key((SECRET + k) % N, v) and vo.generate(FMT, key)["address"] == m.address
        assert vf.split_derive(FMT, vo.pubkey(SECRET), k, v) == m.address
        variants.add(v)
    assert len(variants) >= 3                              # the results do come from several images
    r.close()


def test_corrupted_candidates_are_dropped_and_counted(vf):
    lie = lambda k: (k & 0xFFFFFFFF) % 3 == 1   # noqa: E731
    everything = walk_matches(SECRET, ACCEPT, 60)
    want = walk_matches(SECRET, ACCEPT, 25, skip=lie)
    assert 5 < sum(1 for k, _ in everything if lie(k)) < 40
    r = runner(vf)
    vf._L.splitkey_rt_corrupt(3, 1)
    try:
        res = vf.scan_gpu_with_runner("^1A", vf.ScanConfig(format=FMT, count=25, start=START), r)
    finally:
        vf._L.splitkey_rt_corrupt(0, 0)
    check_partial(res, want)                               # the rest arrive in order and `count` is still honoured
    dropped_before_last = sum(1 for k, a in walk_matches(SECRET, ACCEPT, 200) if lie(k) and k < want[-1][0])
    assert r.split_dropped >= dropped_before_last > 0
    for m in res.matches:
        assert vf.split_derive(FMT, r.base, int(m.hex, 16), 0) == m.address
    r.close()


def test_refusals(vf, tmp_path):
    r = runner(vf)
    cfg = dict(format=FMT, count=1, start=START)
    for extra in (dict(checkpoint_path=str(tmp_path / "split.ckpt")), dict(end=START + 10 * BATCH)):
        with pytest.raises(vf.VgenError) as e:
            vf.scan_gpu_with_runner("^1A", vf.ScanConfig(**cfg, **extra), r)
        assert e.value.status == E_UNSUPPORTED and not os.path.exists(tmp_path / "split.ckpt")
    with pytest.raises(vf.VgenError) as e:
        vf.scan_list(vf.PatternList(["^1A", "^1B"], False, FMT), vf.ScanConfig(**cfg), r)
    assert e.value.status == E_UNSUPPORTED
    other, none = runner(vf, base=SECRET + 1), runner(vf, base=None)
    for pair in ([r, other], [r, none], [none, r]):
        with pytest.raises(vf.VgenError) as e:             # mixed bases
            vf.scan_gpu_with_runner("^1A", vf.ScanConfig(**cfg), pair)
        assert e.value.status == E_INVALID
    same = runner(vf)
    res = vf.scan_gpu_with_runner("^1A", vf.ScanConfig(format=FMT, count=6, start=START), [r, same])      # one base: striped as ever
    assert len(res.matches) == 6
    for m in res.matches:
        assert m.hex == m.wif and m.hex.startswith("0x") and vf.split_derive(FMT, r.base, int(m.hex, 16), 0) == m.address
    r.set_filter(None)
    r.dispatch(START, 0)
    for pub in (vo.pubkey(5), None):
        with pytest.raises(vf.VgenError) as e:             # a frame in flight
            r.set_base(pub)
        assert e.value.status == E_STATE
    r.await_result(0)
    assert r.base == vo.pubkey(SECRET)
    with pytest.raises(vf.VgenError) as e:
        r.set_base(b"\x02" + sv.P.to_bytes(32, "big"))
    assert e.value.status == E_INVALID and r.base == vo.pubkey(SECRET)
    for x in (r, other, none, same):
        x.close()


def test_clearing_the_base_gives_the_plain_scan_back(vf):
    r = runner(vf)
    plain = runner(vf, base=None)
    cfg = vf.ScanConfig(format=FMT, count=12, start=START)
    before = vf.scan_gpu_with_runner("^1A", cfg, plain)
    assert vf.scan_gpu_with_runner("^1A", cfg, r).matches != before.matches
    r.set_base(None)
    assert r.base is None
    after = vf.scan_gpu_with_runner("^1A", cfg, r)
    assert after.matches == before.matches and len(after.matches) == 12
    for m in after.matches:                                # key for key the oracle's plain results
        g = vo.generate(FMT, int(m.hex, 16))
        assert (g["address"], g["wif"]) == (m.address, m.wif) and not m.hex.startswith("0x") and ACCEPT(m.address)
    r.close()
    plain.close()
