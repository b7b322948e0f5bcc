"""Score searches on the MI355X, through the C ABI: create2_score_kernel (format 7) against vgen_create2_address on the host, and
payload_score_kernel behind the per-key kernels (formats 5 and 6, plain and with VGEN_FLAG_ENDO, walked, uploaded and random
scalars) against the oracle's payloads, scored by the digit-by-digit model of tests/score_vectors.py.  Nothing on the expected side
comes from the code under test.

Every case first asserts on the reference alone that it has at least one hit and at least one miss; the counts in the tables below
were computed on the CPU for exactly these inputs.  Records are exact (every term holds), so record sets are compared, not supersets."""
import json
import os
import subprocess

import pytest

import score_vectors as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BATCH = 8192
DEPLOYER = bytes.fromhex("4e59b44847b379578588920ca78fbf26c0b4956c")   # the deterministic-deployment proxy
BASE_KEY = (1 << 252) + 1                                               # 0x1000...0001


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


def model_hits(spec, payloads):
    """[(index, payload)] the model accepts; asserts that the reference alone has a hit and a miss."""
    want = [(i, p) for i, p in enumerate(payloads) if p != bytes(20) and sv.accepts(spec, p)]
    assert 0 < len(want) < len(payloads), (spec, len(want))
    return want


# ---- CREATE2 (format 7): hash and score in one kernel ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def job(vg):
    return vg.Create2Job(DEPLOYER, init_code=b"\x00", salt_prefix=b"")


@pytest.fixture(scope="module")
def c2(job):
    """The host's addresses of the counters 0 .. 4 x 8192 - 1."""
    return [job.address(c) for c in range(4 * BATCH)]


def c2_runner(vg, job, **kw):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.EthereumCreate2, frames=2, **kw)
    r.set_create2(job)
    return r


C2_COUNTS = [("zero-bytes>=2", 30), ("leading-zero-bytes>=1", 36), ("leading:0>=2", 36), ("leading:f>=2", 26), ("count:0>=8", 26), ("count:a>=7", 83)]


@pytest.mark.parametrize("term,n_hits", C2_COUNTS)
def test_create2_hit_counts(vg, job, c2, term, n_hits):
    spec = "score:" + term
    want = model_hits(spec, c2[:BATCH])
    assert len(want) == n_hits
    p = vg.Pattern(spec, fmt=vg.AddressFormat.EthereumCreate2)
    assert p.device_kind == 6
    r = c2_runner(vg, job)
    r.set_filter(p)
    r.dispatch_create2(0, 0)
    recs, n, tested = r.await_result(0)
    r.close()
    assert tested == BATCH and n == n_hits
    assert recs == want                       # indices ascending, payloads of exactly the hit lanes


def test_create2_conjunction_by_record_set(vg, job, c2):
    spec = "score:leading-zero-bytes>=1&zero-bytes>=2"
    r = c2_runner(vg, job)
    r.set_filter(vg.Pattern(spec, fmt=vg.AddressFormat.EthereumCreate2))
    for frame, first in ((0, 0), (1, 2 * BATCH)):
        r.dispatch_create2(first, frame)
    for frame, first in ((0, 0), (1, 2 * BATCH)):
        recs, n, _ = r.await_result(frame)
        want = model_hits(spec, c2[first:first + BATCH])
        assert n == len(want) and recs == want, first
    r.close()


def test_set_score_min_between_two_dispatches_changes_the_second_only(vg, job, c2):
    spec = "score:count:0>=6&zero-bytes>=0"
    p = vg.Pattern(spec, fmt=vg.AddressFormat.EthereumCreate2)
    low, high = model_hits(spec, c2[:BATCH]), model_hits("score:count:0>=8", c2[:BATCH])
    assert len(high) < len(low)
    r = c2_runner(vg, job)
    with pytest.raises(vg.VgenError) as e:    # no score filter installed yet
        r.set_score_min(3)
    assert e.value.status == -5
    r.set_filter(p)
    with pytest.raises(vg.VgenError) as e:
        r.set_score_min(41)
    assert e.value.status == -6
    r.dispatch_create2(0, 0)
    r.set_score_min(8)                        # while frame 0 is in flight: it keeps the threshold it was enqueued with
    r.dispatch_create2(0, 1)
    recs0, n0, _ = r.await_result(0)
    recs1, n1, _ = r.await_result(1)
    assert (n0, recs0) == (len(low), low) and (n1, recs1) == (len(high), high)
    r.set_filter(p)                           # resets the threshold to the filter's own
    r.dispatch_create2(0, 0)
    recs, n, _ = r.await_result(0)
    assert recs == low
    r.close()


def test_scan_create2_best_reports_every_new_best_score(vg, job, c2):
    best, want = -1, []
    for c, p in enumerate(c2):
        s = sv.metric(sv.COUNT_DIGIT, 0, p)
        if s >= 1 and s > best:
            best = s
            want.append((c, s))
    assert want == [(0, 7), (34, 9), (576, 10), (27478, 11)]
    for n_ctx in (1, 2):
        rs = [c2_runner(vg, job) for _ in range(n_ctx)]
        cfg = vg.ScanConfig(format=vg.AddressFormat.EthereumCreate2, count=None, max_batches=4 // n_ctx, best=True)
        res = vg.scan_create2("score:count:0>=1", job, cfg, rs)
        for r in rs:
            r.close()
        assert res.operations == 4 * BATCH
        assert [(int(m.hex[-16:], 16), vg.score("score:count:0>=1", m.address)) for m in res.matches] == want, n_ctx
        assert [bytes.fromhex(m.address[2:]) for m in res.matches] == [c2[c] for c, _ in want]


def test_scan_create2_threshold_equals_the_walk_and_best_refusals(vg, job, c2):
    r = c2_runner(vg, job)
    spec = "score:zero-bytes>=2"
    res = vg.scan_create2(spec, job, vg.ScanConfig(format=vg.AddressFormat.EthereumCreate2, count=None, max_batches=2), r)
    want = [i for i, p in enumerate(c2[:2 * BATCH]) if sv.accepts(spec, p)]
    assert 0 < len(want) and [int(m.hex[-16:], 16) for m in res.matches] == want
    with pytest.raises(vg.VgenError) as e:
        vg.scan_create2("^0x00", job, vg.ScanConfig(format=vg.AddressFormat.EthereumCreate2, count=1, best=True), r)
    assert e.value.status == -1
    with pytest.raises(vg.VgenError) as e:
        vg.scan_create2(spec, job, vg.ScanConfig(format=vg.AddressFormat.EthereumCreate2, count=1, best=True, checkpoint_path="/tmp/never.ckpt"), r)
    assert e.value.status == -8 and "checkpoint" in str(e.value)
    r.close()


def test_cli_generate_best(vg, c2):
    out = subprocess.run([CLI, "generate", "-f", "ethereum-create2", "-p", "score:count:0>=1", "--best", "-c", "3", "--deployer", "0x" + DEPLOYER.hex(),
                          "--init-code-hash", "0x" + vg.keccak256(b"\x00").hex(), "--gpu-batch-size", str(BATCH), "-o", "jsonl", "-q"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert [(int(r["private_key_hex"][-16:], 16), r["score"]) for r in rows] == [(0, 7), (34, 9), (576, 10)]
    assert [bytes.fromhex(r["address"][2:]) for r in rows] == [c2[0], c2[34], c2[576]]
    plain = subprocess.run([CLI, "generate", "-f", "ethereum-create2", "-p", "^0x00", "-c", "1", "--deployer", "0x" + DEPLOYER.hex(),
                            "--init-code-hash", "0x" + vg.keccak256(b"\x00").hex(), "--gpu-batch-size", str(BATCH), "-o", "jsonl", "-q"],
                           capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "score" not in json.loads(plain.stdout.splitlines()[0])   # the field appears for score searches only


def test_cli_range_estimate_and_the_csv_and_text_outputs(vg, vo):
    """`range` and `estimate` take a score specification; csv gets a last `score` column and text a `Score` line, for score searches
    only: the csv header and the text fields of a prefix search are what they were."""
    spec = "score:count:0>=6&zero-bytes>=1"
    acc = vo.payload_seq(vo.FMT_ETHEREUM, 1, 0x3FFF)
    want = [(1 + i, sv.metric(sv.COUNT_DIGIT, 0, acc[20 * i:20 * i + 20])) for i in range(0x3FFF) if sv.accepts(spec, acc[20 * i:20 * i + 20])]
    assert 0 < len(want) < 0x3FFF
    base = [CLI, "range", "--range", "1:3FFF", "-f", "ethereum", "-c", "0", "--gpu-batch-size", str(BATCH), "-q"]
    out = subprocess.run(base + ["-p", spec, "-o", "csv"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "address,wif,private_key_hex,format,pattern,operations,elapsed_secs,rate,score"
    rows = [ln.split(",") for ln in lines[1:]]
    assert [(int(r[2], 16), int(r[-1])) for r in rows] == want and all(len(r) == 9 and r[4] == spec for r in rows)
    text = subprocess.run(base + ["-p", spec, "-o", "text"], capture_output=True, text=True, timeout=120)
    assert text.returncode == 0 and [int(ln.split(":")[1]) for ln in text.stdout.splitlines() if ln.startswith("Score   :")] == [s for _, s in want]
    # a prefix search: no score anywhere, the header as it always was
    plain = subprocess.run(base + ["-p", "^0x00", "-o", "csv"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.splitlines()[0] == "address,wif,private_key_hex,format,pattern,operations,elapsed_secs,rate"
    assert all(len(ln.split(",")) == 8 for ln in plain.stdout.splitlines()) and len(plain.stdout.splitlines()) > 1
    ptext = subprocess.run(base + ["-p", "^0x00", "-o", "text"], capture_output=True, text=True, timeout=120)
    assert ptext.returncode == 0 and "Score" not in ptext.stdout and "Address :" in ptext.stdout
    est = subprocess.run([CLI, "estimate", "-p", "score:leading-zero-bytes>=2", "-f", "ethereum-create2"], capture_output=True, text=True, timeout=120)
    assert est.returncode == 0 and "Estimated difficulty: 1 in 65536\n" in est.stdout, est.stdout + est.stderr


# ---- formats 5 and 6: the per-key kernels dump, payload_score_kernel scores ----------------------------------------------------

LAMBDA = 0x5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72


def create0(vo, account):
    return vo.keccak256(b"\xd6\x94" + account + b"\x80")[12:]


def oracle_payload(vo, fmt, k):
    if not vo.key_valid(k):
        return bytes(20)
    acc = vo.payload(vo.FMT_ETHEREUM, k)
    return acc if fmt == 5 else create0(vo, acc)


_seq = {}


def oracle_seq(vo, fmt):
    """The oracle's payloads of the keys BASE_KEY .. BASE_KEY + 8191 (computed once per format)."""
    if fmt not in _seq:
        acc = vo.payload_seq(vo.FMT_ETHEREUM, BASE_KEY, BATCH)
        accs = [acc[20 * i:20 * i + 20] for i in range(BATCH)]
        _seq[fmt] = accs if fmt == 5 else [create0(vo, a) for a in accs]
    return _seq[fmt]


F5_COUNTS = [("zero-bytes>=2", 34), ("leading:0>=2", 40), ("count:0>=8", 20)]
SPECS56 = ["score:zero-bytes>=2", "score:leading:0>=2", "score:count:0>=8", "score:leading:f>=1&count:f>=4"]


@pytest.mark.parametrize("fmt", [5, 6])
def test_walk_against_the_oracle(vg, vo, fmt):
    payloads = oracle_seq(vo, fmt)
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(fmt), frames=2)
    before = r.memory()["mode_bytes"]
    for spec in SPECS56:
        want = model_hits(spec, payloads)
        if fmt == 5 and spec[6:] in dict(F5_COUNTS):
            assert len(want) == dict(F5_COUNTS)[spec[6:]]
        r.set_filter(vg.Pattern(spec, fmt=vg.AddressFormat(fmt)))
        r.dispatch(BASE_KEY, 1)
        recs, n, tested = r.await_result(1)
        assert tested == BATCH and n == len(want) and recs == want, spec
    assert r.memory()["mode_bytes"] >= before + 2 * BATCH * 20   # the frames' device-only payload buffers are accounted for
    r.close()


@pytest.mark.parametrize("fmt", [5, 6])
def test_six_images_against_key_variant_and_the_oracle(vg, vo, fmt):
    payloads = list(oracle_seq(vo, fmt))
    for v in range(1, 6):
        payloads += [oracle_payload(vo, fmt, vg.key_variant(BASE_KEY + i, v)) for i in range(BATCH)]
    assert vg.key_variant(BASE_KEY + 5, 1) == LAMBDA * (BASE_KEY + 5) % N
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(fmt), frames=2, endo=True, match_cap=8192)
    for spec in ("score:zero-bytes>=2", "score:leading:0>=2&count:0>=4"):
        want = model_hits(spec, payloads)
        r.set_filter(vg.Pattern(spec, fmt=vg.AddressFormat(fmt)))
        r.dispatch(BASE_KEY, 0)
        recs, n, tested = r.await_result(0)
        assert tested == 6 * BATCH and n == len(want) and recs == want, spec   # index = variant * batch + i
    r.close()


@pytest.mark.parametrize("fmt", [5, 6])
def test_uploaded_keys_with_the_scalars_0_and_n_and_a_ragged_count(vg, vo, fmt):
    spec = "score:zero-bytes>=1"
    keys = [BASE_KEY + 3 * i for i in range(700)]
    keys[0], keys[63], keys[64], keys[699] = 0, N, 0, N       # no key: the dump holds zeros there, which would score 20
    payloads = [oracle_payload(vo, fmt, k) for k in keys]
    assert payloads[0] == payloads[63] == bytes(20) and sv.accepts(spec, bytes(20))
    want = model_hits(spec, payloads)
    assert not {0, 63, 64, 699} & {i for i, _ in want}
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(fmt), frames=2)
    r.set_filter(vg.Pattern(spec, fmt=vg.AddressFormat(fmt)))
    r.dispatch(BASE_KEY, 0)                                     # a full dispatch first: the slots behind the ragged count hold its payloads
    full, _, _ = r.await_result(0)
    assert len(full) > len(want)
    r.dispatch_keys(keys, 0)
    recs, n, tested = r.await_result(0)
    r.close()
    assert tested == len(keys) and n == len(want) and recs == want


def test_random_keys_against_the_oracle(vg, vo):
    spec = "score:count:f>=6"
    seed, stream, first = 77, 3, 5 * BATCH
    payloads = [oracle_payload(vo, 5, vg.random_key(seed, stream, first + i) or 0) for i in range(BATCH)]
    want = model_hits(spec, payloads)
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.Ethereum, frames=2)
    r.set_filter(vg.Pattern(spec, fmt=vg.AddressFormat.Ethereum))
    r.dispatch_random(seed, stream, first, 1)
    recs, n, tested = r.await_result(1)
    r.close()
    assert tested == BATCH and n == len(want) and recs == want


@pytest.mark.parametrize("fmt", [5, 6])
def test_a_seeded_scan_returns_the_keys_of_the_prefix_scan(vg, fmt):
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat(fmt), frames=3)
    cfg = vg.ScanConfig(format=vg.AddressFormat(fmt), count=6, seed=42)
    a = vg.scan_gpu_with_runner("score:leading:0>=2", cfg, r)
    b = vg.scan_gpu_with_runner("^0x00", cfg, r)
    r.close()
    assert len(b.matches) == 6 and [(m.hex, m.address) for m in a.matches] == [(m.hex, m.address) for m in b.matches]
    assert all(m.address.startswith("0x00") for m in a.matches)


def test_a_seeded_best_scan_has_strictly_rising_scores_and_is_reproducible(vg, vo):
    spec = "score:count:0>=1"
    start = vo.seed_key(42, 0)
    payloads = vo.payload_seq(vo.FMT_ETHEREUM, start, 3 * BATCH)
    best, want = 0, []
    for i in range(3 * BATCH):
        s = sv.metric(sv.COUNT_DIGIT, 0, payloads[20 * i:20 * i + 20])
        if s > best:
            best = s
            want.append((start + i, s))
    assert len(want) >= 2
    for n_ctx in (1, 3):
        rs = [vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.Ethereum, frames=2) for _ in range(n_ctx)]
        cfg = vg.ScanConfig(format=vg.AddressFormat.Ethereum, count=None, seed=42, max_batches=3 // n_ctx, best=True)
        res = vg.scan_gpu_with_runner(spec, cfg, rs if n_ctx > 1 else rs[0])
        for r in rs:
            r.close()
        assert [(int(m.hex, 16), vg.score(spec, m.address)) for m in res.matches] == want, n_ctx
