"""Split-key search on the MI355X: a runner with the requester's public key P = s * G as its base point tests P + k * G and reports
partial keys.  The sequential walk (the host folds P into the uniform points; the kernels are the plain ones), the arbitrary-scalar
path (keys_fwd_base_kernel: the complete addition, infinity parked as Z = 1), the fallback at the top of the range, random keys,
a zero crossing of the effective key inside a walked batch, no residue after the base is cleared, and the command-line tool.

Smallest shapes that still have the structure: batch 8192 (16384 where the zero crossing needs S = 8 and more than one workgroup of
lanes), two frames.  Expected values are the oracle's for the effective key (s + k) mod n (tests/splitkey_vectors.py), images from
Python integers with the published lambda and beta; each is computed once and shared.  Every test here fails on a library without
vgen_set_base_point."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import nostr_vectors as nv
from tests import splitkey_vectors as sv
import vgen_amd as vg
from oracle import pyoracle as vo

pytestmark = pytest.mark.gpu

ROOT = nv.ROOT
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
N = sv.N
BATCH = 8192
K0 = 2**65 + 12345
SECRET = 0x51C2E7 << 216 | 0xA11CE
SEED = 0x73706C6974
FORMATS = {"p2pkh": 0, "uncompressed": 4, "ethereum": 5, "contract": 6, "p2tr": 3, "nostr": 10}


@pytest.fixture(scope="module")
def runners():
    made = {}

    def get(fmt, endo=False, batch=BATCH):
        key = (fmt, endo, batch)
        if key not in made:
            made[key] = vg.GpuRunner(batch_size=batch, fmt=fmt, device=0, frames=2, endo=endo)
        return made[key]
    yield get
    for r in made.values():
        r.close()


def rows(blob, fmt):
    return np.frombuffer(blob, dtype=np.uint8).reshape(-1, sv.payload_len(fmt))


def dump(r, fmt, start, images, batch=BATCH):
    r.set_filter(None)
    r.dispatch(start, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * batch
    return rows(blob, fmt)[:images * batch]


def images_for(fmt, endo):
    return sv.images_of(fmt) if endo else 1


def bad_rows(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero((got != want).any(axis=1))


def address_of(fmt, row):
    return sv.address_of_payload(fmt, bytes(row))


# ---- 1. the walk: dump parity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,endo", [(n, e) for n in FORMATS for e in (False, True) if not (e and n == "p2tr")],      # (taproot has no images)
                         ids=lambda v: v if isinstance(v, str) else ("images" if v else "plain"))
def test_walk_dump_parity(runners, name, endo):
    fmt = FORMATS[name]
    images = images_for(fmt, endo)
    r = runners(fmt, endo)
    r.set_base(vo.pubkey(SECRET))
    got = dump(r, fmt, K0, images)
    bad = bad_rows(got, sv.dump_of(fmt, SECRET + K0, BATCH, images))
    assert bad.size == 0, (name, endo, bad[:8])


# ---- 2. the effective key wraps past n --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("endo", [False, True], ids=["plain", "images"])
def test_modular_wrap(runners, endo):
    images = 6 if endo else 1
    r = runners(0, endo)
    r.set_base(sv.pub33(N - 5))                            # effective keys 2^65 + 12340 ..
    got = dump(r, 0, K0, images)
    want = sv.dump_of(0, K0 - 5, BATCH, images)
    assert bad_rows(got, want).size == 0
    if endo:
        res = vg.scan_gpu_with_runner("^1A", vg.ScanConfig(format=0, count=8, seed=SEED, random_keys=True), r)
    else:
        res = vg.scan_gpu_with_runner("^1A", vg.ScanConfig(format=0, count=8, start=K0), r)
        ok = [i for i in range(BATCH) if address_of(0, want[i]).startswith("1A")][:8]
        assert [int(m.hex, 16) for m in res.matches] == [K0 + i for i in ok]
    assert len(res.matches) == 8
    for m in res.matches:                                  # results combine to keys the oracle maps to the reported addresses
        assert m.hex == m.wif and m.hex.startswith("0x") and m.address.startswith("1A")
        key, v = vg.split_combine(0, N - 5, int(m.hex, 16), m.address)
        assert vo.generate(0, key)["address"] == m.address and key == sv.image_key((int(m.hex, 16) - 5) % N, v) and (endo or v == 0)


# ---- 3. records -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("endo", [False, True], ids=["plain", "images"])
@pytest.mark.parametrize("name,pattern,head", [("p2pkh", "^1A", "1A"), ("nostr", "^npub1q", "npub1q")])
def test_records_are_the_oracles_matches(runners, name, pattern, head, endo):
    fmt = FORMATS[name]
    images = images_for(fmt, endo)
    r = runners(fmt, endo)
    r.set_base(vo.pubkey(SECRET))
    r.set_filter(vg.Pattern(pattern, False, fmt))
    r.dispatch(K0, 1)
    recs, n, tested = r.await_result(1)
    want = sv.dump_of(fmt, SECRET + K0, BATCH, images)
    hits = [(i, bytes(want[i])) for i in range(len(want)) if address_of(fmt, want[i]).startswith(head)]
    assert tested == images * BATCH and n == len(recs) and sorted(recs) == hits
    assert 0.01 * len(want) < len(hits) < 0.08 * len(want)            # a few percent


# ---- 4. the arbitrary-scalar kernel on crafted keys ----------------------------------------------------------------------------------

CRAFT_N = 300                                              # one full workgroup and a partial one


def crafted_keys(s):
    """300 scalars: random ones, and at an even lane, an odd lane, lane 0, lane 255 and lane 256 the doubling k = s', the infinity
    k = n - s', 0, n and 2^256 - 1 - each beside at least one valid pair-lane neighbour."""
    import random
    rnd = random.Random(0xC4AF7)
    keys = [rnd.randrange(1, N) for _ in range(CRAFT_N)]
    special = {0: N - s, 255: s, 256: N - s, 100: s, 37: N - s, 140: 0, 141: 7, 143: N, 200: 2**256 - 1, 299: s}
    keys[1], keys[254], keys[257], keys[101], keys[36], keys[142], keys[201], keys[298] = (rnd.randrange(1, N) for _ in range(8))
    for lane, k in special.items():
        keys[lane] = k
    return keys, special


@pytest.mark.parametrize("name,endo", [("p2pkh", False), ("p2tr", False), ("nostr", False), ("p2pkh", True), ("nostr", True)],
                         ids=["p2pkh", "p2tr", "nostr", "p2pkh-images", "nostr-images"])
def test_crafted_keys_doubling_infinity_and_no_keys(runners, name, endo):
    fmt = FORMATS[name]
    images = images_for(fmt, endo)
    s = SECRET ^ 0x77
    keys, special = crafted_keys(s)
    r = runners(fmt, endo)
    r.set_base(vo.pubkey(s))
    r.set_filter(None)
    r.dispatch_keys(keys, 0)
    blob, _, tested = r.await_result(0)
    assert tested == images * CRAFT_N
    got = rows(blob, fmt)
    plen = sv.payload_len(fmt)
    dead = []
    for i, k in enumerate(keys):
        e = (s + k) % N
        no_key = not 0 < k < N or e == 0
        if no_key:
            dead.append(i)
        for v in range(images):
            want = bytes(plen) if no_key else sv.payload_of_key(fmt, sv.image_key(e, v))
            assert bytes(got[v * BATCH + i]) == want, (name, i, v, hex(k))      # the infinity's pair lane and workgroup included
    assert sorted(dead) == sorted(l for l, k in special.items() if k in (N - s, 0, N, 2**256 - 1))
    assert bytes(got[255]) == sv.payload_of_key(fmt, 2 * s % N)               # the doubling
    if name == "p2pkh":
        r.set_filter(vg.Pattern("^1", False, fmt))                            # every address: the "no key" slots are absent from records
        r.dispatch_keys(keys, 1)
        recs, n, _ = r.await_result(1)
        assert n == len(recs) == images * (CRAFT_N - len(dead))
        assert sorted(i % BATCH for i, _ in recs) == sorted(i for i in range(CRAFT_N) if i not in dead for _ in range(images))


# ---- 5. the top of the range: the fallback path ----------------------------------------------------------------------------------

def test_walk_at_the_top_of_the_range(runners):
    r = runners(0)
    r.set_base(vo.pubkey(SECRET))
    got = dump(r, 0, N - 100, 1)
    want = sv.dump_of(0, SECRET + N - 100, 100)            # slots i < 100: the effective keys (s + n - 100 + i) mod n
    assert bad_rows(got[:100], want).size == 0
    assert not got[100:].any()                             # partial keys at or beyond n yield nothing


# ---- 6. random keys -------------------------------------------------------------------------------------------------------------

def test_random_keys_with_a_base(runners):
    n_draws = 4096
    r = runners(0)
    r.set_base(vo.pubkey(SECRET))
    r.set_filter(None)
    r.dispatch_random(SEED, 3, 1000, 0)
    blob, _, tested = r.await_result(0)
    got = rows(blob, 0)
    assert tested == BATCH
    for i in range(n_draws):
        k = vo.random_key(SEED, 3, 1000 + i)
        want = vo.payload(0, (SECRET + k) % N) if 0 < k < N else bytes(20)
        assert bytes(got[i]) == want, i


# ---- 7. the effective key passes zero inside a walked batch ---------------------------------------------------------------------------

def test_zero_crossing_inside_a_walked_batch(monkeypatch):
    """Base -(K0 + 5000) * G: slot 5000 is the point at infinity and the lanes whose offsets meet Q_j = +-R_u garble their
    workgroup's shared inversion - at most one workgroup's share of the dump, 2 * S * 256 = 4096 slots, arithmetic only.  Everything
    else is exact (keys below the crossing are n - |e|), and a scan over the range returns only addresses the host re-derived."""
    batch, S = 16384, 8
    monkeypatch.setenv("VGEN_SEQ_S", str(S))
    r = vg.GpuRunner(batch_size=batch, fmt=0, device=0, frames=2)
    monkeypatch.delenv("VGEN_SEQ_S")
    secret = N - (K0 + 5000)
    r.set_base(vo.pubkey(secret))
    got = dump(r, 0, K0, 1, batch)                          # the run completes
    want = sv.dump_of(0, N - 5000, batch)
    bad = bad_rows(got, want)
    assert bad.size <= 2 * S * 256, bad.size
    assert not want[5000].any()
    res = vg.scan_gpu_with_runner("^1A", vg.ScanConfig(format=0, count=None, start=K0, max_batches=1), r)
    ok = {K0 + i for i in range(batch) if want[i].any() and address_of(0, want[i]).startswith("1A")}
    found = {int(m.hex, 16) for m in res.matches}
    assert found <= ok and len(ok - found) <= bad.size and len(found) > 0.01 * batch
    for m in res.matches:
        assert vg.split_derive(0, r.base, int(m.hex, 16), 0) == m.address
    r.close()


# ---- 8. no residue --------------------------------------------------------------------------------------------------------------

def test_no_residue_after_clearing_the_base(runners):
    r = runners(0)
    r.set_base(vo.pubkey(SECRET))
    assert bad_rows(dump(r, 0, K0, 1), sv.dump_of(0, SECRET + K0, BATCH)).size == 0
    r.set_base(None)
    assert r.base is None
    assert bad_rows(dump(r, 0, K0, 1), sv.dump_of(0, K0, BATCH)).size == 0               # the same runner, plain again
    keys = [K0 + 3 * i for i in range(CRAFT_N)]
    r.dispatch_keys(keys, 0)
    blob, _, _ = r.await_result(0)
    assert all(bytes(rows(blob, 0)[i]) == vo.payload(0, k) for i, k in enumerate(keys))
    for fmt in (0, 3):                                     # a second runner of the process that never had a base
        fresh = vg.GpuRunner(batch_size=BATCH, fmt=fmt, device=0, frames=2)
        assert fresh.base is None
        assert bad_rows(dump(fresh, fmt, K0, 1), sv.dump_of(fmt, K0, BATCH)).size == 0
        fresh.close()


def test_a_salt_search_context_takes_no_base():
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.EthereumCreate2, device=0, frames=2)
    with pytest.raises(vg.VgenError) as e:                 # CREATE2 / CREATE3 have no key
        r.set_base(vo.pubkey(SECRET))
    assert e.value.status == -8 and r.base is None
    r.close()


# ---- 9. the command-line tool -----------------------------------------------------------------------------------------------------

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def wif_key(wif):
    v = 0
    for c in wif:
        v = v * 58 + B58.index(c)
    raw = v.to_bytes(38, "big")
    assert raw[0] == 0x80 and raw[33] == 0x01 and vo.sha256(vo.sha256(raw[:34]))[:4] == raw[34:]
    return int.from_bytes(raw[1:33], "big")


@pytest.mark.parametrize("name,pattern", [("p2pkh", "^1Ca"), ("nostr", "^npub1ca")])
def test_cli_generate_and_combine(tmp_path, name, pattern):
    secret_file = tmp_path / "secret.hex"
    secret_file.write_text("%064x\n" % SECRET)
    pub = sv.pub33(SECRET).hex()
    g = subprocess.run([CLI, "generate", "-f", name, "-p", pattern, "--base-pubkey", pub, "--seed", "1", "-c", "2", "-o", "jsonl", "-q"],
                       capture_output=True, text=True, timeout=300)
    assert g.returncode == 0, g.stderr
    lines = [json.loads(ln) for ln in g.stdout.splitlines() if ln.strip()]
    assert len(lines) == 2
    for j in lines:
        assert "wif" not in j and j["base_public_key"].lower() in (pub, vo.pubkey(SECRET).hex()) and j["address"].startswith(pattern[1:])
        partial = int(j["partial_key_hex"], 16)
        assert vg.split_derive(FORMATS[name], pub, partial, j["variant"]) == j["address"]
        c = subprocess.run([CLI, "combine", "-f", name, "--secret-file", str(secret_file), "--partial", j["partial_key_hex"],
                            "--address", j["address"]], capture_output=True, text=True, timeout=60)
        assert c.returncode == 0, c.stderr
        words = c.stdout.split()
        if name == "nostr":
            nsec = next(w for w in words if w.startswith("nsec1"))
            key = int.from_bytes(nv.decode("nsec", nsec), "big")
            assert nv.npub_of_x(nv.xy_of(key)[0]) == j["address"]
        else:
            key = wif_key(next(w for w in words if w[0] in "KL" and len(w) == 52))
            assert vo.generate(0, key)["address"] == j["address"]
        assert key == sv.image_key((SECRET + partial) % N, j["variant"])
        fields = dict((ln.split(":", 1)[0].strip(), ln.split(":", 1)[1].strip()) for ln in c.stdout.splitlines() if ":" in ln)
        assert int(fields["Variant"]) == j["variant"] and fields["Address"] == j["address"]
    bad = subprocess.run([CLI, "combine", "-f", name, "--secret-file", str(secret_file), "--partial", "%064x" % 12345, "--address", lines[0]["address"]],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and bad.stderr.strip()
