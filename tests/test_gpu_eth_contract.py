"""The Ethereum-contract format (VGEN_FMT_ETHEREUM_CONTRACT = 6) on the MI355X, through the C ABI: every dispatch path
(sequential walk, six-image contexts, uploaded and random scalars, prefilter, on-device DFA, pattern lists, vgen_scan) against
the oracle formula  C = keccak256(0xd6 0x94 || oracle payload(5, key) || 0x80)[12:],  address = oracle eip55(C).
Nothing on the expected side comes from the code under test.  The reference has no such format (src/address.rs:11-24).

No comparison may be empty: for the scan range below the oracle alone finds 9 keys with ^0x0000, 12 with ^0xdead (any case),
7 with dead$ and every three-digit prefix more than 200 times, so a test that finds fewer fails rather than shrinks."""
import json
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
FMT = 6
K0 = 2**65 + 0x5EED0000
BIG = 1 << 20


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


def create0(vo, account):
    return vo.keccak256(b"\xd6\x94" + account + b"\x80")[12:]


def oracle_seq(vo, start, n):
    """Contract payloads of the keys start .. start + n - 1 (20 zero bytes for a key >= the group order)."""
    acc = vo.payload_seq(vo.FMT_ETHEREUM, start, n)
    zero = bytes(20)
    return b"".join(create0(vo, acc[20 * i:20 * i + 20]) if 0 < start + i < N else zero for i in range(n))


def oracle_key(vo, k):
    return create0(vo, vo.payload(vo.FMT_ETHEREUM, k)) if vo.key_valid(k) else bytes(20)


@pytest.fixture(scope="module")
def big(vo):
    """The oracle's contract payloads of the 2^20 keys from K0 (the scan range of the issue)."""
    return oracle_seq(vo, K0, BIG)


def first_diff(a, b):
    assert len(a) == len(b), (len(a), len(b))
    if a == b:
        return None
    i = next(i for i in range(0, len(a), 20) if a[i:i + 20] != b[i:i + 20])
    return i // 20, a[i:i + 20].hex(), b[i:i + 20].hex()


def test_full_size_dump_is_the_oracle(vg, vo, big):
    r = vg.GpuRunner(batch_size=BIG, fmt=vg.AddressFormat(FMT), frames=2)
    r.set_filter(None)
    r.dispatch(K0, 0)
    blob, _, tested = r.await_result(0)
    assert tested == BIG
    assert first_diff(blob, big) is None
    r.close()
    # a dispatch that straddles the group order: keys >= n yield nothing
    batch = 8192
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(FMT))
    r.set_filter(None)
    for start in (N - 5000, N - batch - 3, 1):
        r.dispatch(start, 0)
        blob, _, tested = r.await_result(0)
        want = oracle_seq(vo, start, batch)
        assert first_diff(blob, want) is None, hex(start)
        if start == N - 5000:
            assert blob[20 * 5000:] == bytes(20 * (batch - 5000)) and any(blob[20 * 4999:20 * 5000])
    r.close()


ENDO_BATCH = 1 << 16
LAMBDA = 0x5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72


def variant_key(k, v):
    kv = pow(LAMBDA, v % 3, N) * k % N
    return N - kv if v >= 3 else kv


@pytest.fixture(scope="module")
def six(vo):
    """(start, the oracle's contract payloads of the six images of ENDO_BATCH keys from it: image v of key i at v * batch + i)."""
    start = vo.seed_key(6, 0)
    return start, oracle_seq(vo, start, ENDO_BATCH) + b"".join(oracle_key(vo, variant_key(start + i, v)) for v in range(1, 6) for i in range(ENDO_BATCH))


def test_endomorphism_dump_is_the_oracle_on_all_six_images(vg, vo, six):
    batch = ENDO_BATCH
    start, want = six
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(FMT), endo=True)
    r.set_filter(None)
    r.dispatch(start, 0)
    blob, _, tested = r.await_result(0)
    assert tested == 6 * batch and len(blob) == 6 * batch * 20
    for v in range(6):
        assert vg.key_variant(start + 77, v) == variant_key(start + 77, v)
        assert first_diff(blob[20 * v * batch:20 * (v + 1) * batch], want[20 * v * batch:20 * (v + 1) * batch]) is None, v
    r.close()


PATTERNS = [("^0xdead", True, 2), ("dead$", False, 2), ("^0x0000", False, 2), ("de[0-9]d", False, 4)]


def check_filter(vg, vo, r, start, want_payloads, n_keys):
    """Every pattern: the records are exactly the keys whose oracle address the oracle's regex accepts once case is folded
    (the device sees the payload, not the EIP-55 casing), and those the exact regex confirms are exactly the oracle's matches."""
    addrs = [vo.eip55(want_payloads[20 * i:20 * i + 20]) for i in range(n_keys)]
    for pattern, ci, kind in PATTERNS:
        pat = vg.Pattern(pattern, ci, vg.AddressFormat(FMT))
        assert pat.device_kind == kind, pattern
        r.set_filter(pat)
        r.dispatch(start, 1)
        recs, n, tested = r.await_result(1)
        assert tested == n_keys and n == len(recs), (pattern, n, len(recs))
        exact, folded = vo.Regex(pattern, ci), vo.Regex(pattern, True)
        want = [i for i in range(n_keys) if exact.matches(addrs[i])]
        want_folded = [i for i in range(n_keys) if folded.matches(addrs[i])]
        print(f"{pattern!r} ci={ci}: {len(recs)} records, oracle {len(want)} exact / {len(want_folded)} case-folded")
        # (dead$ is written in lower case: EIP-55 spells few addresses that way, so its exact set may be empty - the device's is not)
        assert len(want_folded) > 0 and (len(want) > 0 or pattern == "dead$"), pattern
        for idx, pl in recs:
            assert pl == want_payloads[20 * idx:20 * idx + 20], (pattern, idx)
        assert sorted(idx for idx, _ in recs) == want_folded, pattern
        assert sorted(idx for idx, pl in recs if exact.matches(vo.eip55(pl))) == want, pattern
        assert sorted(idx for idx, pl in recs if pat.matches(vg.address_from_payload(FMT, pl))) == want, pattern


def test_filter_mode_equals_the_oracle_regex_over_the_dump(vg, vo, big):
    r = vg.GpuRunner(batch_size=BIG, fmt=vg.AddressFormat(FMT), frames=2, match_cap=1 << 16)
    check_filter(vg, vo, r, K0, big, BIG)
    r.close()


def test_filter_mode_on_a_six_image_context(vg, vo, six):
    batch = ENDO_BATCH
    start, want = six
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(FMT), endo=True, match_cap=1 << 16)
    check_filter(vg, vo, r, start, want, 6 * batch)
    r.close()


def test_uploaded_and_random_scalars(vg, vo):
    batch = 8192
    rng = random.Random(66)
    keys = [0, N - 1, N, 1, 2, N + 1, 2**256 - 1] + [rng.randrange(1, N) for _ in range(4096 - 7)]
    r = vg.GpuRunner(batch_size=batch, fmt=vg.AddressFormat(FMT))
    r.set_filter(None)
    r.dispatch_keys(keys, 0)
    blob, _, tested = r.await_result(0)
    assert tested == len(keys) == 4096
    want = b"".join(oracle_key(vo, k) for k in keys)
    assert first_diff(blob[:20 * len(keys)], want) is None
    assert blob[:20] == bytes(20) and any(blob[20:40]) and blob[40:60] == bytes(20)
    assert blob[20 * len(keys):] == bytes(20 * (batch - len(keys)))
    # filter mode on the same scalars
    pat = vg.Pattern("^0x[0-3]", False, vg.AddressFormat(FMT))
    ore = vo.Regex("^0x[0-3]", False)
    r.set_filter(pat)
    r.dispatch_keys(keys, 1)
    recs, n, _ = r.await_result(1)
    want_idx = [i for i, k in enumerate(keys) if vo.key_valid(k) and ore.matches(vo.eip55(oracle_key(vo, k)))]
    assert [i for i, _ in recs] == want_idx and len(want_idx) > 800
    # one batch of keys drawn on the device
    r.set_filter(None)
    r.dispatch_random(99, 3, 5 * batch, 0)
    blob, _, tested = r.await_result(0)
    assert tested == batch
    want = b"".join(oracle_key(vo, vo.random_key(99, 3, 5 * batch + i)) for i in range(batch))
    assert first_diff(blob, want) is None
    r.close()


def test_scan_returns_the_first_matches_of_the_walk(vg, vo, big):
    ore = vo.Regex("^0x0000", False)
    oracle = [(K0 + i, vo.eip55(big[20 * i:20 * i + 20])) for i in range(BIG) if big[20 * i:20 * i + 2] == b"\0\0"]
    assert all(ore.matches(a) for _, a in oracle) and len(oracle) >= 3
    print("oracle ^0x0000 offsets:", [k - K0 for k, _ in oracle])
    r = vg.GpuRunner(batch_size=1 << 18, fmt=vg.AddressFormat(FMT), frames=4)
    cfg = vg.ScanConfig(format=vg.AddressFormat(FMT), count=3, start=K0, end=K0 + BIG - 1)
    res = vg.scan_gpu_with_runner("^0x0000", cfg, r)
    got = [(int(m.hex, 16), m.address, m.wif) for m in res.matches]
    assert got == [(k, a, "%064x" % k) for k, a in oracle[:3]]
    assert all(m.format == vg.AddressFormat.EthereumContract for m in res.matches)
    # the whole range: every match, in order
    res = vg.scan_gpu_with_runner("^0x0000", vg.ScanConfig(format=vg.AddressFormat(FMT), count=None, start=K0, end=K0 + BIG - 1), r)
    assert [(int(m.hex, 16), m.address) for m in res.matches] == oracle and res.complete
    r.close()


def test_scan_list_first_key_per_prefix(vg, vo, big):
    prefixes = ["000", "dea", "c0f", "1e7", "abc", "f00", "5ee", "999"]
    plist = vg.PatternList(["^0x" + p for p in prefixes], case_insensitive=True, fmt=vg.AddressFormat(FMT))
    assert plist.device_kind == 5
    first = {}
    for i in range(BIG):
        h = big[20 * i:20 * i + 2].hex()[:3]
        if h in prefixes and h not in first:
            first[h] = i
    assert sorted(first) == sorted(prefixes)
    want = sorted((K0 + i, vo.eip55(big[20 * i:20 * i + 20])) for i in first.values())
    r = vg.GpuRunner(batch_size=1 << 18, fmt=vg.AddressFormat(FMT), frames=4)
    cfg = vg.ScanConfig(format=vg.AddressFormat(FMT), count=None, start=K0, end=K0 + BIG - 1)
    res = vg.scan_list(plist, cfg, r, per_pattern=1)
    assert [(int(m.hex, 16), m.address) for m in res.matches] == want
    assert sorted(prefixes[m.pattern_index] for m in res.matches) == sorted(prefixes)
    r.close()


def test_cli_generate_reports_the_deployer(vg, vo):
    r = subprocess.run([CLI, "generate", "-f", "ethereum-contract", "-p", "^0xdead", "-i", "--seed", "42", "-c", "1", "-o", "json", "-q"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    row = json.loads(r.stdout)
    key = int(row["private_key_hex"], 16)
    account = vo.payload(vo.FMT_ETHEREUM, key)
    assert row["deployer"] == vo.eip55(account) == vg.derive(5, key).address
    assert row["address"] == vo.eip55(create0(vo, account)) == vo.eip55(vg.contract_address(row["deployer"], 0))
    assert row["address"].lower().startswith("0xdead") and row["wif"] == row["private_key_hex"] == "%064x" % key
    assert list(row)[:2] == ["address", "deployer"] and row["format"].startswith("Ethereum contract")
    # text and jsonl carry the field too; csv and minimal keep their columns; plain Ethereum has no such field
    common = ["-p", "^0xdea", "-i", "--seed", "42", "-c", "1", "-q"]
    t = subprocess.run([CLI, "generate", "-f", "ethereum-contract", *common], capture_output=True, text=True, timeout=300)
    assert t.returncode == 0 and "\nDeployer: 0x" in t.stdout, t.stderr
    j = subprocess.run([CLI, "generate", "-f", "ethereum-contract", *common, "-o", "jsonl"], capture_output=True, text=True, timeout=300)
    assert json.loads(j.stdout)["deployer"] == vg.derive(5, int(json.loads(j.stdout)["private_key_hex"], 16)).address
    c = subprocess.run([CLI, "generate", "-f", "ethereum-contract", *common, "-o", "csv"], capture_output=True, text=True, timeout=300)
    assert c.stdout.splitlines()[0] == "address,wif,private_key_hex,format,pattern,operations,elapsed_secs,rate" and len(c.stdout.splitlines()[1].split(",")) == 8
    m = subprocess.run([CLI, "generate", "-f", "ethereum-contract", *common, "-o", "minimal"], capture_output=True, text=True, timeout=300)
    assert len(m.stdout.split()) == 1 and len(m.stdout.strip()) == 64
    e = subprocess.run([CLI, "generate", "-f", "ethereum", *common, "-o", "json"], capture_output=True, text=True, timeout=300)
    assert "deployer" not in json.loads(e.stdout)


def test_cli_range_patterns_file_and_estimate(vg, vo, big, tmp_path):
    f = tmp_path / "names.txt"
    f.write_text("^0x000\n^0xdea\n")
    rng = "%x:%x" % (K0, K0 + BIG - 1)
    r = subprocess.run([CLI, "range", "--range", rng, "-f", "ethereum-contract", "-i", "--patterns-file", str(f), "-o", "jsonl", "-q"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.strip()]
    want = []
    for p in ("000", "dea"):
        i = next(i for i in range(BIG) if big[20 * i:20 * i + 2].hex()[:3] == p)
        want.append((K0 + i, vo.eip55(big[20 * i:20 * i + 20]), "^0x" + p))
    assert sorted((int(x["private_key_hex"], 16), x["address"], x["pattern"]) for x in rows) == sorted(want)
    for x in rows:
        assert x["deployer"] == vo.eip55(vo.payload(vo.FMT_ETHEREUM, int(x["private_key_hex"], 16)))
    # estimate: format 5's difficulty for the same pattern
    out = {}
    for name in ("ethereum", "ethereum-contract"):
        e = subprocess.run([CLI, "estimate", "-f", name, "-p", "^0xdead"], capture_output=True, text=True, timeout=300)
        assert e.returncode == 0, e.stderr
        out[name] = [l for l in e.stdout.splitlines() if l.startswith("Estimated difficulty:")]
    assert out["ethereum-contract"] == out["ethereum"] == ["Estimated difficulty: 1 in %d" % 16 ** 4]
