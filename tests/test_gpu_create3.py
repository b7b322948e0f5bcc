"""CREATE3 jobs on a VGEN_FMT_ETHEREUM_CREATE2 context, on the MI355X through the C ABI: the chained Keccak kernels (two blocks per
salt, three with a guard) in their dump, prefilter and score forms, the deferred paths behind the dump form, the change of job on
one context, vgen_scan_create3 and the command line.

Expected values are the host's vgen_create3_address - held against the oracle's keccak256 and the pinned fixture in
tests/test_create3.py - for all 8192 salts of a dispatch, the oracle's keccak256 over bytes written out here on a sample of them,
and plain byte tests of those payloads for what a filter should report.  Batch 8192 (the smallest the ABI allows), 2 frames."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_vectors as sv  # noqa: E402

CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
FMT = 7
BATCH = 8192
# 20 + 32 + 24 pairwise distinct bytes, and a guard of 64 more: a byte-order slip in any message word shows
FACTORY, PHASH, PREFIX = bytes(range(0x01, 0x15)), bytes(range(0x20, 0x40)), bytes(range(0x80, 0x98))
GUARD64 = bytes(range(0xA0, 0xE0))
GUARD_LENS = [0, 1, 2, 3, 20, 32, 52, 63, 64]      # every byte alignment of the counter, the padding byte in word 24
CROSS = 2**32 - 100                                # carries the counter across its two words


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


def job_of(vg, guard_len):
    """guard_len None: no guard."""
    return vg.Create3Job(FACTORY, PHASH, PREFIX, None if guard_len is None else GUARD64[:guard_len])


_want = {}


def want(vg, guard_len, first):
    """The 8192 contract addresses of the counters from `first` on, by the host's function (computed once per job and counter)."""
    if (guard_len, first) not in _want:
        j = job_of(vg, guard_len)
        _want[guard_len, first] = [j.address(first + i) for i in range(BATCH)]
    return _want[guard_len, first]


def oracle_address(vo, guard_len, counter):
    salt = PREFIX + counter.to_bytes(8, "big")
    s2 = salt if guard_len is None else vo.keccak256(GUARD64[:guard_len] + salt)
    proxy = vo.keccak256(b"\xff" + FACTORY + s2 + PHASH)[12:]
    return vo.keccak256(b"\xd6\x94" + proxy + b"\x01")[12:]


def runner(vg, guard_len, **kw):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2, **kw)
    r.set_create3(job_of(vg, guard_len))
    return r


def hits(vg, guard_len, first, pred):
    return [(i, p) for i, p in enumerate(want(vg, guard_len, first)) if pred(p)]


def dump(r, first, frame=0):
    r.dispatch_create2(first, frame)
    blob, _, tested = r.await_result(frame)
    assert tested == BATCH and len(blob) == 20 * BATCH
    return blob


def check_dump(vg, vo, guard_len, first):
    r = runner(vg, guard_len)
    r.set_filter(None)
    blob = dump(r, first)
    r.close()
    exp = want(vg, guard_len, first)
    bad = [i for i in range(BATCH) if blob[20 * i:20 * i + 20] != exp[i]]
    assert not bad, (guard_len, hex(first), bad[:5], blob[20 * bad[0]:20 * bad[0] + 20].hex(), exp[bad[0]].hex())
    for i in list(range(0, BATCH, 509)) + [99, 100, 101, 255, 256, BATCH - 1]:
        assert blob[20 * i:20 * i + 20] == oracle_address(vo, guard_len, first + i), (guard_len, hex(first), i)


# ---- dump parity --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, CROSS, 2**64 - BATCH])
def test_dump_without_a_guard_is_the_hosts_function_and_the_oracle(vg, vo, first):
    check_dump(vg, vo, None, first)


@pytest.mark.parametrize("guard_len", GUARD_LENS)
def test_dump_with_a_guard_is_the_hosts_function_and_the_oracle(vg, vo, guard_len):
    check_dump(vg, vo, guard_len, CROSS)


def test_a_guard_of_length_zero_is_not_no_guard(vg):
    assert want(vg, 0, CROSS)[:4] != want(vg, None, CROSS)[:4]


def test_a_batch_past_the_counter_space_is_refused_and_nothing_is_enqueued(vg):
    for guard_len in (None, 20):
        r = runner(vg, guard_len)
        r.set_filter(None)
        with pytest.raises(vg.VgenError) as e:
            r.dispatch_create2(2**64 - BATCH + 1, 0)
        assert e.value.status == -7
        with pytest.raises(vg.VgenError) as e:       # nothing in flight on the frame
            r.await_result(0)
        assert e.value.status == -5
        r.close()


def test_set_create3_needs_a_create2_context_and_a_valid_guard(vg):
    e5 = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.Ethereum, frames=2)
    with pytest.raises(vg.VgenError) as e:
        e5.set_create3(job_of(vg, None))
    assert e.value.status == -1
    e5.close()
    from vgen_amd import api
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    for guard, n in ((GUARD64, 65), (GUARD64, -2), (None, 1)):
        assert api._L.vgen_set_create3(r._h, FACTORY, PHASH, PREFIX, guard, n) == -1
    with pytest.raises(vg.VgenError) as e:           # ... and none of them installed a job
        r.dispatch_create2(0, 0)
    assert e.value.status == -5
    r.close()


# ---- inline prefilter ------------------------------------------------------------------------------------------------------------

INLINE = [("^0x00", 2, lambda p: p[0] == 0), ("00$", 2, lambda p: p[19] == 0), ("^0x", 3, lambda p: True)]


@pytest.mark.parametrize("pat,kind,pred", INLINE)
@pytest.mark.parametrize("guard_len", [None, 20])
def test_inline_prefilter_reports_exactly_the_cpu_filter_of_the_dump(vg, guard_len, pat, kind, pred):
    p = vg.Pattern(pat, False, FMT)
    assert p.device_kind == kind
    r = runner(vg, guard_len, match_cap=BATCH)
    r.set_filter(p)
    r.dispatch_create2(CROSS, 1)
    recs, n, tested = r.await_result(1)
    r.close()
    exp = hits(vg, guard_len, CROSS, pred)
    assert len(exp) > 10                                       # ~32 expected for the byte tests, 8192 for match-all: never empty
    assert tested == BATCH and n == len(exp)
    assert recs == exp                                         # indices ascending, payloads of exactly the hit lanes


def test_two_frames_in_flight(vg):
    p = vg.Pattern("^0x0", False, FMT)
    pred = lambda p: p[0] >> 4 == 0                            # noqa: E731
    for guard_len in (None, 64):
        r = runner(vg, guard_len)
        r.set_filter(p)
        r.dispatch_create2(CROSS, 0)
        r.dispatch_create2(0 if guard_len is None else CROSS, 1)
        for frame, first in ((0, CROSS), (1, 0 if guard_len is None else CROSS)):
            recs, n, _ = r.await_result(frame)
            exp = hits(vg, guard_len, first, pred)
            assert n == len(exp) > 300 and recs == exp, (guard_len, frame)
        r.close()


# ---- deferred paths: automaton and list behind the dump form ---------------------------------------------------------------------

@pytest.mark.parametrize("guard_len", [None, 3])
def test_on_device_automaton(vg, guard_len):
    p = vg.Pattern("ab", False, FMT)
    assert p.device_kind == 4
    r = runner(vg, guard_len)
    r.set_filter(p)
    r.dispatch_create2(CROSS, 0)
    recs, n, tested = r.await_result(0)
    r.close()
    exp = hits(vg, guard_len, CROSS, lambda p: "ab" in p.hex())
    assert tested == BATCH and n == len(exp) > 100 and recs == exp


@pytest.mark.parametrize("guard_len", [None, 32])
def test_pattern_list_of_two_lines(vg, guard_len):
    pl = vg.PatternList(["^0x00", "^0xab"], fmt=vg.AddressFormat(FMT))
    r = runner(vg, guard_len)
    r.set_filter(pl)
    r.dispatch_create2(CROSS, 1)
    recs, n, tested = r.await_result(1)
    r.close()
    exp = hits(vg, guard_len, CROSS, lambda p: p[0] in (0x00, 0xAB))
    assert tested == BATCH and n == len(exp) > 30 and recs == exp


# ---- score: the fused kernel -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guard_len", [None, 20])
def test_score_filter_and_set_score_min_between_dispatches(vg, guard_len):
    spec = "score:count:0>=6&zero-bytes>=0"
    p = vg.Pattern(spec, fmt=vg.AddressFormat(FMT))
    assert p.device_kind == 6
    pay = want(vg, guard_len, CROSS)
    low = [(i, q) for i, q in enumerate(pay) if sv.accepts(spec, q)]
    high = [(i, q) for i, q in enumerate(pay) if sv.accepts("score:count:0>=8", q)]
    assert 0 < len(high) < len(low) < BATCH
    r = runner(vg, guard_len)
    r.set_filter(p)
    r.dispatch_create2(CROSS, 0)
    r.set_score_min(8)                        # while frame 0 is in flight: it keeps the threshold it was enqueued with
    r.dispatch_create2(CROSS, 1)
    recs0, n0, _ = r.await_result(0)
    recs1, n1, _ = r.await_result(1)
    r.close()
    assert (n0, recs0) == (len(low), low) and (n1, recs1) == (len(high), high)


# ---- the two kinds of job on one context ---------------------------------------------------------------------------------------------

def test_create2_then_create3_then_create2_on_one_context(vg):
    j2 = vg.Create2Job(FACTORY, init_code_hash=PHASH, salt_prefix=PREFIX)
    c2 = b"".join(j2.address(CROSS + i) for i in range(BATCH))
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    r.set_filter(None)
    r.set_create2(j2)
    first = dump(r, CROSS)
    assert first == c2
    for guard_len in (None, 20):
        r.set_create3(job_of(vg, guard_len))
        assert dump(r, CROSS) == b"".join(want(vg, guard_len, CROSS)), guard_len
    r.set_create2(j2)
    assert dump(r, CROSS, 1) == first
    r.close()
    assert c2[:20] != want(vg, None, CROSS)[0]


# ---- scan ------------------------------------------------------------------------------------------------------------------------------

def first_five(vg, guard_len):
    """The first five counters from 0 on whose contract address starts 0x00, by the host's function (~ 1300 salts)."""
    j, out, c = job_of(vg, guard_len), [], 0
    while len(out) < 5:
        a = j.address(c)
        if a[0] == 0:
            out.append((c, a))
        c += 1
        assert c < 20 * BATCH
    return out


@pytest.mark.parametrize("guard_len", [None, 20])
def test_scan_over_one_and_two_contexts_gives_the_same_first_five(vg, vo, guard_len):
    five = first_five(vg, guard_len)
    j = job_of(vg, guard_len)
    for n_ctx in (1, 2):
        rs = [vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2) for _ in range(n_ctx)]
        res = vg.scan_create3("^0x00", j, vg.ScanConfig(format=vg.AddressFormat(FMT), count=5), rs)
        for r in rs:
            r.close()
        assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in five], n_ctx
        assert [m.address for m in res.matches] == [vo.eip55(oracle_address(vo, guard_len, c)) for c, _ in five]
        assert all(m.wif == m.hex and int(m.format) == FMT for m in res.matches)
        assert res.operations % BATCH == 0 and res.operations >= BATCH and not res.complete


def test_scan_best_yields_strictly_rising_scores(vg):
    j = job_of(vg, 20)
    pay = want(vg, 20, 0)
    best, exp = -1, []
    for c, q in enumerate(pay):
        s = sv.metric(sv.COUNT_DIGIT, 0, q)
        if s >= 1 and s > best:
            best = s
            exp.append((c, s))
    assert len(exp) >= 3
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    res = vg.scan_create3("score:count:0>=1", j, vg.ScanConfig(format=vg.AddressFormat(FMT), count=None, max_batches=1, best=True), r)
    r.close()
    got = [(int(m.hex[-16:], 16), vg.score("score:count:0>=1", m.address)) for m in res.matches]
    assert got == exp and all(a[1] < b[1] for a, b in zip(got, got[1:]))
    assert [bytes.fromhex(m.address[2:]) for m in res.matches] == [pay[c] for c, _ in exp]


def test_scan_refusals_are_those_of_the_create2_scan(vg):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    j = job_of(vg, None)
    for bad in (dict(seed=5), dict(start=1), dict(n_shards=2), dict(checkpoint_path="/tmp/vgen-create3-never-written.ckpt")):
        with pytest.raises(vg.VgenError) as e:
            vg.scan_create3("^0x00", j, vg.ScanConfig(format=vg.AddressFormat(FMT), count=1, **bad), r)
        assert e.value.status == -8 and "vgen_scan_create3" in str(e.value), bad
    with pytest.raises(vg.VgenError) as e:
        vg.scan_create3("^0x00", j, vg.ScanConfig(format=vg.AddressFormat.Ethereum, count=1), r)
    assert e.value.status == -1
    r.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------

def test_cli_generate_json(vg, vo):
    guard = GUARD64[:20]
    args = [CLI, "generate", "-f", "ethereum-create3", "-p", "^0x00", "--deployer", "0x" + FACTORY.hex(), "--proxy-init-code-hash", "0x" + PHASH.hex(),
            "--salt-prefix", "0x" + PREFIX.hex(), "--salt-guard", "0x" + guard.hex(), "-c", "2", "-o", "json", "-q", "--gpu-batch-size", str(BATCH), "--frames", "2"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows, dec, pos = [], json.JSONDecoder(), 0
    text = r.stdout.strip()
    while pos < len(text):
        row, pos = dec.raw_decode(text, pos)
        rows.append(row)
        while pos < len(text) and text[pos].isspace():
            pos += 1
    assert len(rows) == 2
    five = first_five(vg, 20)
    for row, (c, a) in zip(rows, five):
        salt = bytes.fromhex(row["private_key_hex"][2:])
        assert salt == PREFIX + c.to_bytes(8, "big") and row["wif"] == row["private_key_hex"]
        gs = vo.keccak256(guard + salt)
        proxy = vo.keccak256(b"\xff" + FACTORY + gs + PHASH)[12:]
        assert row["guarded_salt"] == "0x" + gs.hex() and row["proxy"] == "0x" + proxy.hex()
        assert row["deployer"] == "0x" + FACTORY.hex() and row["proxy_init_code_hash"] == "0x" + PHASH.hex()
        assert row["address"] == vo.eip55(vo.keccak256(b"\xd6\x94" + proxy + b"\x01")[12:]) == vo.eip55(a)
        assert "init_code_hash" not in row
