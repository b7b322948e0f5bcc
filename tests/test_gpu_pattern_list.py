"""Pattern lists on the MI355X: every dispatch path of a list filter (device kind 5: the per-key kernels in dump mode into a
device-only buffer, then ptab_lookup_kernel + ptab_compact_kernel) reports a superset of the oracle's matches whose confirmed
part is exactly the oracle's, and vgen_scan_list returns the first keys of the walk per pattern, across contexts and
checkpoints.  Hits land here where the hashes put them; the kernel-level edges (interval bounds, word / thread / wave / pass
boundaries of the compaction, a full ring, a wrapping count, ragged counts over stale buffers) are in
tests/test_gpu_list_kernels.py."""
import os
import random

import pytest

pytestmark = pytest.mark.gpu

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BECH32 = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
HEX = "0123456789abcdefABCDEF"
HEAD = {0: "^1", 4: "^1", 2: "^3", 1: "^bc1q", 3: "^bc1p", 5: "^0x"}
SYMS = {0: B58, 4: B58, 2: "23456789ABCDEFGHJKLMNPQ", 1: BECH32, 3: BECH32, 5: HEX}


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


def short_list(fmt, seed, n=200, long_from=()):
    """~n prefixes of three symbols after the format's head (two for Base58: '1' is part of the head), plus long
    prefixes of the given addresses."""
    rnd = random.Random(seed)
    sym = SYMS[fmt]
    k = 2 if fmt in (0, 2, 4) else 3
    if fmt == 2:   # P2SH: only the second character is bounded (SYMS[2]); the third is any Base58 digit
        pats = {"^3" + rnd.choice(sym) + rnd.choice(B58) for _ in range(n)}
    else:
        pats = {HEAD[fmt] + "".join(rnd.choice(sym) for _ in range(k)) for _ in range(n)}
    for a in long_from:
        pats.add("^" + a[:len(HEAD[fmt]) + 7])
    return sorted(pats)


def payloads(blob, width, n):
    return [blob[width * i:width * i + width] for i in range(n)]


def check(vg, fmt, plist, recs, n_found, want_payloads, idx_of=lambda i: i):
    """recs: the device's candidates; want_payloads: {index: oracle payload}."""
    assert n_found == len(recs)
    got = {}
    for idx, p in recs:
        assert idx in want_payloads and want_payloads[idx] == p, idx
        got[idx] = p
    expected = {i for i, p in want_payloads.items() if any(p) and plist.matches(vg.address_from_payload(fmt, p))}
    confirmed = {i for i, p in got.items() if plist.matches(vg.address_from_payload(fmt, p))}
    assert confirmed == expected
    assert expected <= set(got)
    assert list(sorted(got)) == [i for i, _ in recs]   # ascending index order
    return len(expected)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4, 5])
def test_dispatch_parity(vg, vo, fmt):
    batch = 1 << 16
    start = vo.seed_key(21, fmt)
    width = 32 if fmt == 3 else 20
    blob = vo.payload_seq(fmt, start, batch)
    want = dict(enumerate(payloads(blob, width, batch)))
    longs = [vg.address_from_payload(fmt, want[i]) for i in (5, 40000)]
    plist = vg.PatternList(short_list(fmt, fmt, long_from=longs), fmt=vg.AddressFormat(fmt))
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(fmt), match_cap=batch, frames=2)
    r.set_filter(plist)
    for rep in range(2):   # the ring's running count carries over between dispatches
        r.dispatch(start, rep)
        recs, n, tested = r.await_result(rep)
        assert tested == batch
        assert check(vg, fmt, plist, recs, n, want) > 10
        assert {5, 40000} <= {i for i, _ in recs}
    assert r.memory()["mode_bytes"] >= 2 * batch * width
    r.close()


def test_dispatch_parity_endo(vg, vo):
    batch = 8192
    start = vo.seed_key(22, 0)
    plist = vg.PatternList(short_list(0, 7), fmt=vg.AddressFormat.P2pkh)
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat.P2pkh, endo=True, match_cap=6 * batch)
    r.set_filter(plist)
    r.dispatch(start, 0)
    recs, n, tested = r.await_result(0)
    assert tested == 6 * batch
    want = {}
    for v in range(6):
        for i in range(batch):
            want[v * batch + i] = vo.payload(0, vg.key_variant(start + i, v))
    assert check(vg, 0, plist, recs, n, want) > 50
    r.close()


@pytest.mark.parametrize("fmt", [0, 3])
def test_dispatch_keys_parity(vg, vo, fmt):
    batch = 8192
    rnd = random.Random(fmt)
    keys = [rnd.getrandbits(256) % (2**256 - 2**32) + 1 for _ in range(3000)] + [0]   # 0: an invalid scalar, no record
    # a pattern whose interval holds the top-64 value 0, so the all-zero payload of the invalid scalar reaches the lookup's
    # exclusion (the dump's "no key" mark is never a candidate)
    zero = {0: "^1111111", 3: "^bc1pqqqqqq"}[fmt]
    plist = vg.PatternList(short_list(fmt, 30 + fmt) + [zero], fmt=vg.AddressFormat(fmt))
    assert len(plist) - 1 in plist.which(vg.address_from_payload(fmt, bytes(32 if fmt == 3 else 20)))
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(fmt), match_cap=batch)
    r.set_filter(plist)
    r.dispatch_keys(keys, 0)
    recs, n, tested = r.await_result(0)
    width = 32 if fmt == 3 else 20
    want = {i: (vo.payload(fmt, k) if vo.key_valid(k) else bytes(width)) for i, k in enumerate(keys)}
    assert check(vg, fmt, plist, recs, n, want) > 5
    assert len(keys) - 1 not in {i for i, _ in recs}
    r.close()


def test_dispatch_random_parity(vg, vo):
    batch = 8192
    plist = vg.PatternList(short_list(1, 40), fmt=vg.AddressFormat.P2wpkh)
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat.P2wpkh, match_cap=batch)
    r.set_filter(plist)
    r.dispatch_random(99, 3, 5 * batch, 0)
    recs, n, tested = r.await_result(0)
    want = {}
    for i in range(batch):
        k = vo.random_key(99, 3, 5 * batch + i)
        want[i] = vo.payload(1, k) if k else bytes(20)
    assert check(vg, 1, plist, recs, n, want) > 5
    r.close()


def first_keys(vg, vo, plist, fmt, start, n_keys, per):
    """The oracle's walk: per pattern, the first `per` keys (in walk order) that satisfy it, applying vgen_scan_list's rule."""
    blob = vo.payload_seq(fmt, start, n_keys)
    got = [0] * len(plist)
    out = []
    for i in range(n_keys):
        a = vg.address_from_payload(fmt, blob[20 * i:20 * i + 20])
        w = plist.which(a)
        if w and any(got[j] < per for j in w):
            for j in w:
                got[j] += 1
            out.append((start + i, a))
    return out


def test_scan_list_first_key_per_pattern(vg, vo):
    fmt = 0
    plist = vg.PatternList(short_list(fmt, 50, n=50), fmt=vg.AddressFormat(fmt))
    r = vg.GpuRunner(batch_size=1 << 16, fmt=vg.AddressFormat(fmt), frames=4)
    cfg = vg.ScanConfig(format=vg.AddressFormat(fmt), count=None, seed=77)
    res = vg.scan_list(plist, cfg, r, per_pattern=1)
    assert len(res.matches) == len(plist)
    assert sorted(m.pattern_index for m in res.matches) != [] and all(plist.which(m.address) for m in res.matches)
    covered = set()
    for m in res.matches:
        covered.update(plist.which(m.address))
        g = vo.generate(fmt, int(m.hex, 16))
        assert (g["address"], g["wif"]) == (m.address, m.wif)
    assert covered == set(range(len(plist)))
    start = vo.seed_key(77, 0)
    last = max(int(m.hex, 16) for m in res.matches)
    want = first_keys(vg, vo, plist, fmt, start, last - start + 1, 1)
    assert [(int(m.hex, 16), m.address) for m in res.matches] == want

    # per_pattern = 3 with a total cap
    res3 = vg.scan_list(plist, vg.ScanConfig(format=vg.AddressFormat(fmt), count=60, seed=77), r, per_pattern=3)
    assert len(res3.matches) == 60
    want3 = first_keys(vg, vo, plist, fmt, start, int(res3.matches[-1].hex, 16) - start + 1, 3)
    assert [(int(m.hex, 16), m.address) for m in res3.matches] == want3[:60]

    # two contexts on one device: the same results
    r2 = vg.GpuRunner(batch_size=1 << 16, fmt=vg.AddressFormat(fmt), frames=4)
    res2 = vg.scan_list(plist, cfg, [r, r2], per_pattern=1)
    assert [m.address for m in res2.matches] == [m.address for m in res.matches]
    r2.close()
    r.close()


def test_scan_list_checkpoint_resume(vg, vo, tmp_path):
    fmt = 1
    plist = vg.PatternList(short_list(fmt, 60, n=40), fmt=vg.AddressFormat(fmt))
    r = vg.GpuRunner(batch_size=1 << 16, fmt=vg.AddressFormat(fmt), frames=4)
    full = vg.scan_list(plist, vg.ScanConfig(format=vg.AddressFormat(fmt), count=None, seed=5), r, per_pattern=1)
    ck = str(tmp_path / "list.ck")
    part = vg.scan_list(plist, vg.ScanConfig(format=vg.AddressFormat(fmt), count=None, seed=5, max_batches=1, checkpoint_path=ck), r, per_pattern=1)
    assert len(part.matches) < len(full.matches)
    rest = vg.scan_list(plist, vg.ScanConfig(format=vg.AddressFormat(fmt), count=None, seed=5, checkpoint_path=ck), r, per_pattern=1)
    assert [m.address for m in rest.matches] == [m.address for m in full.matches]
    other = vg.PatternList(short_list(fmt, 61, n=40), fmt=vg.AddressFormat(fmt))
    with pytest.raises(vg.VgenError):
        vg.scan_list(other, vg.ScanConfig(format=vg.AddressFormat(fmt), count=None, seed=5, checkpoint_path=ck), r, per_pattern=1)
    r.close()


def test_full_size_dispatch_with_a_hundred_thousand_prefixes(vg, vo):
    rnd = random.Random(100)
    pats = set()
    while len(pats) < 100000:
        pats.add("1" + "".join(rnd.choice(B58) for _ in range(4)))
    plist = vg.PatternList(["^" + p for p in sorted(pats)])
    batch = 1 << 20
    start = vo.seed_key(9, 0)
    blob = vo.payload_seq(0, start, batch)
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat.P2pkh, match_cap=1 << 16, frames=2)
    r.set_filter(plist)
    r.dispatch(start, 0)
    recs, n, tested = r.await_result(0)
    assert n <= len(recs) and tested == batch
    want_idx = set()
    for i in range(batch):
        a = vg.address_from_payload(0, blob[20 * i:20 * i + 20])
        if a[:5] in pats:
            want_idx.add(i)
    got = {i for i, p in recs if vg.address_from_payload(0, p)[:5] in pats}
    assert got == want_idx and len(want_idx) > 100
    for i, p in recs:
        assert blob[20 * i:20 * i + 20] == p
    r.close()


def test_cli_generate_patterns_file_end_to_end(vg, vo, tmp_path):
    """vgen-hip generate --patterns-file F -f p2wpkh --seed 7 -o jsonl: one line per pattern (distinct prefixes of one
    length, so no key satisfies two), each with its pattern, every address re-derived from its key by the oracle."""
    import json
    import subprocess
    rnd = random.Random(77)
    pats = sorted({"^bc1q" + "".join(rnd.choice(BECH32) for _ in range(2)) for _ in range(12)})
    f = tmp_path / "names.txt"
    f.write_text("# twelve prefixes\n" + "\n".join(pats) + "\n")
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vgen_amd", "vgen-hip")
    r = subprocess.run([cli, "generate", "--patterns-file", str(f), "-f", "p2wpkh", "--seed", "7", "-o", "jsonl", "-q"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert sorted(row["pattern"] for row in rows) == pats
    for row in rows:
        assert row["address"].startswith(row["pattern"][1:])
        g = vo.generate(vo.FMT_P2WPKH, int(row["private_key_hex"], 16))
        assert (g["address"], g["wif"]) == (row["address"], row["wif"])
