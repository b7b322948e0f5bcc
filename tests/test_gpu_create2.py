"""The CREATE2 format (VGEN_FMT_ETHEREUM_CREATE2 = 7) on the MI355X, through the C ABI: the Keccak-only salt kernel in its two
forms (dump; inline prefilter with the ordered compaction), the deferred paths behind the dump form (on-device automaton, pattern
list), the refusals, the memory a context holds, vgen_scan_create2 and the command line.

Expected values are the host's vgen_create2_address - itself held against the oracle and EIP-1014 in tests/test_create2.py - for
all 8192 salts of a dispatch, the oracle's keccak256 over bytes written out here on a sample of them, and plain byte tests of
those payloads for what a filter should report.  Batch 8192 (the smallest the ABI allows), 2 frames."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
FMT = 7
BATCH = 8192
# 20 + 32 + 24 pairwise distinct bytes: a byte-order slip in any message word shows
DEPLOYER, HASH, PREFIX = bytes(range(0x01, 0x15)), bytes(range(0x20, 0x40)), bytes(range(0x80, 0x98))
FIRSTS = [0, 0xFFFFFFFF - 100, 0x00FFFFFFFFFFFF00, 2**64 - BATCH]


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def job(vg):
    assert len(set(DEPLOYER + HASH + PREFIX)) == 76
    return vg.Create2Job(DEPLOYER, init_code_hash=HASH, salt_prefix=PREFIX)


_want = {}


def want(vg, first):
    """The 8192 payloads of the counters from `first` on, by the host's function (computed once per first counter)."""
    if first not in _want:
        _want[first] = [vg.create2_address(DEPLOYER, PREFIX + (first + i).to_bytes(8, "big"), HASH) for i in range(BATCH)]
    return _want[first]


def runner(vg, job, **kw):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2, **kw)
    r.set_create2(job)
    return r


def hits(vg, first, pred):
    return [(i, p) for i, p in enumerate(want(vg, first)) if pred(p)]


# ---- dump parity --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", FIRSTS)
def test_dump_is_the_hosts_function_and_the_oracle(vg, vo, job, first):
    r = runner(vg, job)
    r.set_filter(None)
    r.dispatch_create2(first, 0)
    blob, _, tested = r.await_result(0)
    r.close()
    assert tested == BATCH and len(blob) == 20 * BATCH
    exp = want(vg, first)
    bad = [i for i in range(BATCH) if blob[20 * i:20 * i + 20] != exp[i]]
    assert not bad, (hex(first), bad[:5], blob[20 * bad[0]:20 * bad[0] + 20].hex(), exp[bad[0]].hex())
    for i in list(range(0, BATCH, 97)) + [99, 100, 101, 102, 255, 256, BATCH - 1]:
        salt = PREFIX + (first + i).to_bytes(8, "big")
        assert blob[20 * i:20 * i + 20] == vo.keccak256(b"\xff" + DEPLOYER + salt + HASH)[12:], (hex(first), i)


def test_a_batch_past_the_counter_space_is_refused_and_nothing_is_enqueued(vg, job):
    r = runner(vg, job)
    r.set_filter(None)
    with pytest.raises(vg.VgenError) as e:
        r.dispatch_create2(2**64 - BATCH + 1, 0)
    assert e.value.status == -7
    with pytest.raises(vg.VgenError) as e:       # nothing in flight on the frame
        r.await_result(0)
    assert e.value.status == -5
    r.close()


def test_dispatch_without_a_job_is_a_state_error(vg):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    with pytest.raises(vg.VgenError) as e:
        r.dispatch_create2(0, 0)
    assert e.value.status == -5
    r.close()


# ---- inline prefilter ------------------------------------------------------------------------------------------------------------

INLINE = [("^0x00", lambda p: p[0] == 0), ("^0x0", lambda p: p[0] >> 4 == 0), ("ff$", lambda p: p[19] == 0xFF)]


@pytest.mark.parametrize("pat,pred", INLINE)
@pytest.mark.parametrize("first", [0, 0xFFFFFFFF - 100])
def test_inline_prefilter_reports_exactly_the_cpu_filter_of_the_dump(vg, job, pat, pred, first):
    p = vg.Pattern(pat, False, FMT)
    assert p.device_kind == 2
    r = runner(vg, job)
    r.set_filter(p)
    r.dispatch_create2(first, 1)
    recs, n, tested = r.await_result(1)
    r.close()
    exp = hits(vg, first, pred)
    assert len(exp) > (300 if pat == "^0x0" else 10)          # ~512 / ~32 expected: no comparison is empty
    assert tested == BATCH and n == len(exp)
    assert recs == exp                                         # indices ascending, payloads of exactly the hit lanes


def test_match_all_pattern_fills_the_ring_in_index_order(vg, job):
    p = vg.Pattern("^0x", False, FMT)
    assert p.device_kind == 3
    r = runner(vg, job, match_cap=256)
    assert r.match_cap == 256
    r.set_filter(p)
    r.dispatch_create2(5, 0)
    recs, n, tested = r.await_result(0)
    r.close()
    assert n == BATCH and len(recs) == 256
    assert recs == list(enumerate(want(vg, 5)[:256]))


def test_two_frames_in_flight_and_the_ring_base_carries_over(vg, job):
    p = vg.Pattern("^0x0", False, FMT)
    r = runner(vg, job)
    r.set_filter(p)
    pred = INLINE[1][1]
    for a, b in ((0, 0xFFFFFFFF - 100), (0x00FFFFFFFFFFFF00, 0), (2**64 - BATCH, 0xFFFFFFFF - 100)):
        r.dispatch_create2(a, 0)
        r.dispatch_create2(b, 1)
        for frame, first in ((0, a), (1, b)):
            recs, n, _ = r.await_result(frame)
            exp = hits(vg, first, pred)
            assert n == len(exp) > 300 and recs == exp, (hex(a), hex(b), frame)
    r.close()


# ---- deferred paths: automaton and list behind the dump form ---------------------------------------------------------------------------

@pytest.mark.parametrize("pat,pred", [("ab", lambda p: "ab" in p.hex()), ("de[0-9]d", lambda p: re.search("de[0-9]d", p.hex()) is not None)])
def test_on_device_automaton(vg, job, pat, pred):
    p = vg.Pattern(pat, False, FMT)
    assert p.device_kind == 4
    r = runner(vg, job)
    r.set_filter(p)
    for frame, first in ((0, 0), (1, 0xFFFFFFFF - 100), (0, 0)):
        r.dispatch_create2(first, frame)
        recs, n, tested = r.await_result(frame)
        exp = hits(vg, first, pred)
        assert tested == BATCH and n == len(exp) > 5 and recs == exp, (pat, hex(first))
    r.close()


def test_pattern_list(vg, job):
    pl = vg.PatternList(["^0x00", "^0xab"], fmt=vg.AddressFormat(FMT))
    r = runner(vg, job)
    r.set_filter(pl)
    for frame, first in ((0, 0), (1, 0x00FFFFFFFFFFFF00), (0, 0xFFFFFFFF - 100)):
        r.dispatch_create2(first, frame)
        recs, n, tested = r.await_result(frame)
        exp = hits(vg, first, lambda p: p[0] in (0x00, 0xAB))
        assert tested == BATCH and n == len(exp) > 30 and recs == exp, hex(first)
    r.close()


def test_filters_can_be_changed_between_dispatches(vg, job):
    """dump -> inline -> automaton -> dump on one context: the buffers of each mode are made at its first use."""
    r = runner(vg, job)
    r.set_filter(None)
    r.dispatch_create2(0, 0)
    assert r.await_result(0)[0] == b"".join(want(vg, 0))
    r.set_filter(vg.Pattern("^0x00", False, FMT))
    r.dispatch_create2(0, 0)
    assert r.await_result(0)[0] == hits(vg, 0, INLINE[0][1])
    r.set_filter(vg.Pattern("ab", False, FMT))
    r.dispatch_create2(0, 1)
    assert r.await_result(1)[0] == hits(vg, 0, lambda p: "ab" in p.hex())
    r.set_filter(None)
    r.dispatch_create2(0, 1)
    assert r.await_result(1)[0] == b"".join(want(vg, 0))
    r.close()


def test_kernel_timer(vg, job):
    r = runner(vg, job, timing=True)
    r.set_filter(vg.Pattern("^0x00", False, FMT))
    r.dispatch_create2(0, 0)
    r.await_result(0)
    assert 0.0 < r.kernel_ms(0) < 1000.0 and r.kernel_ms(0) <= r.dispatch_ms(0) + 1e-3
    r.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_key_dispatches_and_scans_refuse_the_format(vg, job):
    r = runner(vg, job)
    r.set_filter(None)
    for call in (lambda: r.dispatch(1, 0), lambda: r.dispatch_keys([1, 2, 3], 0), lambda: r.dispatch_random(7, 0, 0, 0),
                 lambda: vg.scan_gpu_with_runner("^0x00", vg.ScanConfig(format=vg.AddressFormat(FMT), count=1, seed=1), r),
                 lambda: vg.scan_gpu_with_runner("^0x00", vg.ScanConfig(format=vg.AddressFormat(FMT), count=1, seed=1), [r], force_multi=True),
                 lambda: vg.scan_list(vg.PatternList(["^0x00"], fmt=vg.AddressFormat(FMT)), vg.ScanConfig(format=vg.AddressFormat(FMT), seed=1), r)):
        with pytest.raises(vg.VgenError) as e:
            call()
        assert e.value.status == -8 and "create2" in str(e.value), str(e.value)
    r.dispatch_create2(0, 0)                     # and nothing was left in flight or broken by them
    assert r.await_result(0)[0] == b"".join(want(vg, 0))
    r.close()


def test_set_create2_needs_a_create2_context_and_endo_is_refused(vg, job):
    e5 = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.Ethereum, frames=2)
    with pytest.raises(vg.VgenError) as e:
        e5.set_create2(job)
    assert e.value.status == -1
    with pytest.raises(vg.VgenError) as e:
        e5.dispatch_create2(0, 0)
    assert e.value.status == -1
    with pytest.raises(vg.VgenError) as e:
        vg.scan_create2("^0x00", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=1), e5)
    assert e.value.status == -1
    e5.close()
    with pytest.raises(vg.VgenError) as e:
        vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2, endo=True)
    assert e.value.status == -8


# ---- memory ------------------------------------------------------------------------------------------------------------------------

def test_a_create2_context_holds_no_point_arithmetic_scratch(vg, job):
    e5 = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.Ethereum, frames=2)
    c2 = runner(vg, job)
    m5, m7 = e5.memory(), c2.memory()
    e5.close()
    assert 0 < m7["frames_bytes"] < m5["frames_bytes"] / 2, (m7, m5)
    assert m7["table_bytes"] == 0 and m7["mode_bytes"] == 0
    # what it does hold: two rings of 4096 records of 40 bytes (+ header), the filter program
    assert 2 * 4096 * 40 <= m7["frames_bytes"] < 2 * 4096 * 40 + 16384
    c2.set_filter(vg.Pattern("^0x00", False, FMT))
    assert c2.memory()["mode_bytes"] >= 2 * BATCH * 20      # the frames' payload buffers and hit masks, at the filter's first use
    c2.close()


# ---- scan ----------------------------------------------------------------------------------------------------------------------------

def cpu_walk(vo, pattern_pred, count, limit):
    out = []
    for c in range(limit):
        a = vo.keccak256(b"\xff" + DEPLOYER + PREFIX + c.to_bytes(8, "big") + HASH)[12:]
        if pattern_pred(a):
            out.append((c, a))
            if len(out) == count:
                break
    return out


@pytest.fixture(scope="module")
def first_five(vo):
    """The first five counters whose address starts 0x000, by the oracle alone (~ 20 000 salts, three batches)."""
    w = cpu_walk(vo, lambda a: a[0] == 0 and a[1] >> 4 == 0, 5, 200000)
    assert len(w) == 5
    return w


def check_scan(vg, vo, res, first_five):
    assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in first_five]
    assert [m.address for m in res.matches] == [vo.eip55(a) for _, a in first_five]
    assert all(m.wif == m.hex and int(m.format) == FMT for m in res.matches)
    last = first_five[-1][0]
    assert res.operations % BATCH == 0 and res.operations >= (last // BATCH + 1) * BATCH and not res.complete


def test_scan_finds_the_first_five_salts_in_order(vg, vo, job, first_five):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    seen = []
    res = vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=5), r, first_counter=0, progress_cb=seen.append)
    check_scan(vg, vo, res, first_five)
    assert seen and seen == sorted(seen) and seen[-1] == res.operations
    # from a later counter: the results that lie behind it
    start = first_five[1][0] + 1
    res = vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=3), r, first_counter=start)
    assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in first_five[2:]]
    r.close()


def test_scan_over_two_contexts_gives_the_same_results(vg, vo, job, first_five):
    rs = [vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2) for _ in range(2)]
    res = vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=5), rs)
    check_scan(vg, vo, res, first_five)
    for r in rs:
        r.close()


def test_scan_limits_and_refusals(vg, vo, job, first_five):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)
    cfg = vg.ScanConfig(format=vg.AddressFormat(FMT), count=None, max_batches=1)
    res = vg.scan_create2("^0x000", job, cfg, r)
    assert res.operations == BATCH and not res.complete
    assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in first_five if c < BATCH]
    rs = [r, vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2)]
    res = vg.scan_create2("^0x000", job, cfg, rs)
    assert res.operations == 2 * BATCH                         # one batch per context
    assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in first_five if c < 2 * BATCH]
    rs[1].close()
    # the end of the counter space: the last whole batch, then complete
    res = vg.scan_create2("^0x", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=None), r, first_counter=2**64 - 2 * BATCH - 5)
    assert res.complete and res.operations == 2 * BATCH and len(res.matches) == 2 * BATCH
    assert res.matches[-1].hex == "0x" + (PREFIX + (2**64 - 6).to_bytes(8, "big")).hex()
    # a pattern without a device filter is filtered on the host from dumps
    p = vg.Pattern("^0x000", True, FMT)
    res = vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=2, case_insensitive=True), r)
    assert [m.hex for m in res.matches] == ["0x" + (PREFIX + c.to_bytes(8, "big")).hex() for c, _ in first_five[:2]] and p.matches(res.matches[0].address)
    for bad in (dict(checkpoint_path="/tmp/vgen-create2-never-written.ckpt"), dict(seed=5), dict(start=1), dict(end=2**200), dict(n_shards=2), dict(random_keys=True)):
        with pytest.raises(vg.VgenError) as e:
            vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=1, **bad), r)
        assert e.value.status == -8, bad
    assert not os.path.exists("/tmp/vgen-create2-never-written.ckpt")
    with pytest.raises(vg.VgenError) as e:
        vg.scan_create2("^0x000", job, vg.ScanConfig(format=vg.AddressFormat.Ethereum, count=1), r)
    assert e.value.status == -1
    r.close()


def test_scan_grows_the_rings_for_a_permissive_pattern(vg, job):
    """^0x0 brings ~512 candidates per batch: rings of 256 records overflow, the scan enlarges them and repeats the batch."""
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(FMT), frames=2, match_cap=256)
    res = vg.scan_create2("^0x0", job, vg.ScanConfig(format=vg.AddressFormat(FMT), count=None, max_batches=2), r)
    exp = [i for i, p in enumerate(want(vg, 0)) if p[0] >> 4 == 0] + [BATCH + i for i, p in enumerate(want(vg, BATCH)) if p[0] >> 4 == 0]
    assert [int(m.hex[-16:], 16) for m in res.matches] == exp and res.operations == 2 * BATCH
    r.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------

def test_cli_generate(vg, vo):
    args = [CLI, "generate", "-f", "ethereum-create2", "-p", "^0x00", "--deployer", "0x" + DEPLOYER.hex(), "--init-code-hash", "0x" + HASH.hex(),
            "--salt-prefix", "0x" + PREFIX[:20].hex(), "--salt-start", "1000", "-c", "2", "-o", "jsonl", "-q", "--gpu-batch-size", str(BATCH), "--frames", "2"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 2
    prefix = PREFIX[:20] + bytes(4)
    counters = []
    for row in rows:
        salt = bytes.fromhex(row["private_key_hex"][2:])
        assert salt[:24] == prefix and row["deployer"] == "0x" + DEPLOYER.hex() and row["init_code_hash"] == "0x" + HASH.hex()
        addr = vg.create2_address(DEPLOYER, salt, HASH)
        assert addr == vo.keccak256(b"\xff" + DEPLOYER + salt + HASH)[12:] and addr[0] == 0
        assert row["address"] == vo.eip55(addr) and row["wif"] == row["private_key_hex"]
        counters.append(int.from_bytes(salt[24:], "big"))
    assert 1000 <= counters[0] < counters[1]
    # and they are the first two from --salt-start on
    assert [c for c in range(1000, counters[1] + 1) if vg.create2_address(DEPLOYER, prefix + c.to_bytes(8, "big"), HASH)[0] == 0] == counters
    # text output names the salt and the deployer
    r = subprocess.run(args[:args.index("-o")] + ["-o", "text", "-q", "--gpu-batch-size", str(BATCH), "--frames", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Salt    : 0x" + prefix.hex() in r.stdout and "Deployer: 0x" + DEPLOYER.hex() in r.stdout and "InitHash: 0x" + HASH.hex() in r.stdout, r.stdout
