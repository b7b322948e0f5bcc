"""The host side of the Nostr format (format 10) without a device: cabi.cpp and the scan loop of scanner.cpp over the CPU stand-in of
the runtime with Nostr contexts added (tests/native/nostr_rt.cpp beside fake_rt.cpp, built into libvgen_fake_nostr.so by
tests/native/nostr.mk), driven through the C ABI by a second instance of vgen_amd/api.py bound to that library.

What is checked is the factor 3: a VGEN_FLAG_ENDO dispatch tests 3 x batch keys, image e of key i sits at e * batch + i in dumps
and match records, the match ring holds at most 3 x batch records, and vgen_scan, vgen_scan_multi and vgen_scan_list turn such an
index into the key lambda^e (k0 + i) and count 3 x batch operations per batch.  Expected keys and strings are those of
tests/nostr_vectors.py (Python integers over the oracle's multiplication, beta and lambda as published, a BIP-173 encoder written out
there): nothing of the code under test."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import nostr_vectors as nv
from oracle import pyoracle as vo

ROOT = nv.ROOT
FMT = nv.FMT
SO = os.path.join(ROOT, "tests", "native", "libvgen_fake_nostr.so")
BATCH = 8192
SEED = 0x6E6F737472
START = 2**65 + 12345


@pytest.fixture(scope="module")
def vf():
    """vgen_amd/api.py over the stand-in's library (the mechanism of tests/conftest.py: hooks_api, with another library)."""
    assert os.path.exists(SO), f"{SO} not built (make -C tests/native -f nostr.mk, or __graft_entry__.build())"
    spec = importlib.util.spec_from_file_location("vgen_amd_fake_nostr_api", os.path.join(ROOT, "vgen_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    mod._SO_OVERRIDE = SO
    sys.modules["vgen_amd_fake_nostr_api"] = mod     # (dataclasses look their module up there)
    spec.loader.exec_module(mod)
    assert mod.library_path() == SO
    return mod


def runner(vf, endo, frames=2):
    return vf.GpuRunner(batch_size=BATCH, fmt=FMT, device=0, frames=frames, endo=endo, timing=False)


def hits(start, images, accept):
    d, strings = nv.dump_of(start, BATCH, images), nv.strings_of(start, BATCH, images)
    return [(i, bytes(d[i])) for i, s in enumerate(strings) if accept(s)]


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_dispatch_counts_and_places_three_images(vf, endo):
    images = 3 if endo else 1
    r = runner(vf, endo)
    r.set_filter(None)
    r.dispatch(START, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * BATCH
    got = np.frombuffer(blob, dtype=np.uint8).reshape(-1, 32)[:images * BATCH]
    assert (got == nv.dump_of(START, BATCH, images)).all()               # image e of key i at e * batch + i
    r.set_filter(vf.Pattern("^npub1q", False, FMT))
    r.dispatch(START, 1)
    recs, n, tested = r.await_result(1)
    want = hits(START, images, lambda s: s.startswith("npub1q"))
    assert tested == images * BATCH and n == len(recs) and recs == want and 150 * images < n < 4096
    if endo:
        assert max(i for i, _ in recs) >= 2 * BATCH                       # records of the third image carry its indices
    for slot, pl in recs[:5] + recs[-5:]:
        e, i = divmod(slot, BATCH)
        k = vf.key_variant(START + i, e)
        assert k == nv.key_of_slot(START, BATCH, slot) and nv.xy_of(k)[0].to_bytes(32, "big") == pl
    # the ring cannot be asked to hold more than the dispatch tests keys: 3 x batch, not 6 x batch
    vf._check(vf._L.vgen_set_match_cap(r._h, 0xFFFFFFFF), r._h)
    import ctypes
    cap = ctypes.c_uint32()
    vf._L.vgen_get_info(r._h, None, None, ctypes.byref(cap))
    assert cap.value == images * BATCH
    # explicit keys: n x images keys, the same index convention over the context's batch size
    keys = [int(v["key"], 16) for v in nv.VECTORS[:50]] + [0, nv.N]
    r.set_filter(None)
    r.dispatch_keys(keys, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * len(keys)
    got = np.frombuffer(blob, dtype=np.uint8).reshape(-1, 32)
    for i, k in enumerate(keys):
        for e in range(images):
            want_pl = bytes(32) if not 0 < k < nv.N else (pow(nv.BETA, e, nv.P) * nv.xy_of(k)[0] % nv.P).to_bytes(32, "big")
            assert bytes(got[e * BATCH + i]) == want_pl
    r.close()


def check(res, want_keys, images):
    assert [int(m.hex, 16) for m in res.matches] == want_keys
    for m in res.matches:
        key = int(m.hex, 16)
        assert m.address == nv.npub_of_x(nv.xy_of(key)[0]) and m.wif == nv.encode("nsec", key.to_bytes(32, "big")) and int(m.format) == FMT
    assert res.operations > 0 and res.operations % (images * BATCH) == 0


def walk_matches(start, accept, count, stride=1):
    """The first `count` keys of the walk from `start` whose npub `accept`s, batch after batch."""
    out, b = [], 0
    while len(out) < count:
        s = nv.strings_of(start + b * BATCH, BATCH, 1)
        out += [start + b * BATCH + i for i, t in enumerate(s) if accept(t)]
        b += 1
    return out[:count], b


@functools.lru_cache(maxsize=None)
def random_batch(seed, stream, b):
    """(key, npub) of every slot of batch b of a three-image random-key scan, image-major as the dispatch orders them."""
    keys = [vo.random_key(seed, stream, b * BATCH + i) for i in range(BATCH)]
    xs = [nv.xy_of(k)[0] if 0 < k < nv.N else None for k in keys]
    out = []
    for e in range(3):
        beta, lam = pow(nv.BETA, e, nv.P), pow(nv.LAMBDA, e, nv.N)
        out += [(lam * k % nv.N, nv.npub_of_x(beta * x % nv.P)) for k, x in zip(keys, xs) if x is not None]
    return tuple(out)


def random_matches(seed, stream, accept, count):
    """The first `count` keys of a three-image random-key scan, in dispatch order: batch by batch, image-major within a batch."""
    out, b = [], 0
    while len(out) < count:
        out += [k for k, s in random_batch(seed, stream, b) if accept(s)]
        b += 1
    return out[:count], b


ACCEPT = lambda s: s.startswith("npub1qq")   # noqa: E731


def test_scan_walk(vf):
    r = runner(vf, False)
    want, _ = walk_matches(vo.seed_key(SEED, 0), ACCEPT, 3)
    check(vf.scan_gpu_with_runner("^npub1qq", vf.ScanConfig(format=FMT, count=3, seed=SEED), r), want, 1)
    r.close()


def test_scan_with_three_images(vf):
    r = runner(vf, True)
    want, batches = random_matches(SEED, 0, ACCEPT, 3)
    res = vf.scan_gpu_with_runner("^npub1qq", vf.ScanConfig(format=FMT, count=3, seed=SEED, random_keys=True), r)
    check(res, want, 3)
    assert res.operations >= batches * 3 * BATCH
    # a seeded walk on such a context is refused (its keys are no contiguous range), with the format's count in the message
    with pytest.raises(vf.VgenError) as e:
        vf.scan_gpu_with_runner("^npub1qq", vf.ScanConfig(format=FMT, count=1, seed=SEED), r)
    assert "three for x-only keys" in str(e.value)
    r.close()


def rendered(m):
    key = int(m.hex, 16)
    return m.address == nv.npub_of_x(nv.xy_of(key)[0]) and m.wif == nv.encode("nsec", key.to_bytes(32, "big")) and int(m.format) == FMT


def test_scan_multi_stripes_the_walk(vf):
    rs = [runner(vf, False), runner(vf, False)]
    res = vf.scan_gpu_with_runner("^npub1qq", vf.ScanConfig(format=FMT, count=4, seed=SEED), rs)
    base = vo.seed_key(SEED, 0)
    assert len(res.matches) == 4 and res.operations > 0 and res.operations % BATCH == 0
    for m in res.matches:      # the two contexts stripe ONE walk by batches: every match is a key of its first batches
        assert 0 <= int(m.hex, 16) - base < 8 * BATCH and rendered(m) and ACCEPT(m.address)
    for r in rs:
        r.close()


def test_scan_multi_draws_three_images_per_candidate(vf):
    rs = [runner(vf, True), runner(vf, True)]
    res = vf.scan_gpu_with_runner("^npub1qq", vf.ScanConfig(format=FMT, count=4, seed=SEED, random_keys=True), rs)
    assert len(res.matches) == 4 and res.operations > 0 and res.operations % (3 * BATCH) == 0
    drawn = {vo.random_key(SEED, stream, i) for stream in (0, 1) for i in range(4 * BATCH)}     # the candidates of the two streams
    images = set()
    for m in res.matches:      # every match is lambda^e times a candidate of one of the streams, rendered for that key
        key = int(m.hex, 16)
        e = [e for e in range(3) if pow(nv.LAMBDA, -e, nv.N) * key % nv.N in drawn]
        assert len(e) == 1 and rendered(m) and ACCEPT(m.address)
        images.add(e[0])
    for r in rs:
        r.close()


def test_scan_list_with_three_images(vf):
    heads = ["q", "p", "z", "r"]
    pl = vf.PatternList(["^npub1" + h for h in heads], False, FMT)
    r = runner(vf, True)
    res = vf.scan_list(pl, vf.ScanConfig(format=FMT, count=None, seed=SEED, random_keys=True), r)
    assert res.operations > 0 and res.operations % (3 * BATCH) == 0
    assert sorted(m.pattern_index for m in res.matches) == [0, 1, 2, 3]            # one address per line
    drawn = {vo.random_key(SEED, 0, i) for i in range(4 * BATCH)}
    for m in res.matches:
        key = int(m.hex, 16)
        assert any(pow(nv.LAMBDA, -e, nv.N) * key % nv.N in drawn for e in range(3)) and rendered(m) and m.address[5] == heads[m.pattern_index]
    r.close()
