"""CREATE3 jobs of the ethereum-create2 format (7) on the CPU: the address of the contract a CREATE3 factory deploys,
    proxy    = keccak256(0xff || factory || salt' || proxy_init_code_hash)[12:]
    contract = keccak256(0xd6 0x94 || proxy || 0x01)[12:]
with salt' the raw salt or keccak256(guard || salt), searched by salt.

Ground truth is the oracle's keccak256 over bytes written out here, the composition of two host functions pinned elsewhere
(contract_address(create2_address(factory, salt', proxy_hash), nonce 1)) and the values of tests/golden/create3.json, which were
computed with an independent Keccak.  Checked: the host functions and the job object, the two generated blocks of
device/hashgen.py in their Python model, the message builders of core/hash.h through a small host program, the ISA of the six
kernel symbols, that no format number or ABI version moved, and the command line's argument checks (no device needed)."""
import json
import os
import random
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vgen_amd", "csrc", "device"))
import hashgen as g  # noqa: E402
import vgen_amd as vg  # noqa: E402
from oracle import pyoracle as vo  # noqa: E402
from vgen_amd import api  # noqa: E402

FMT = 7
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "create3.json")))
PROXY_HASH = "21c35dbe1b344a2488cf3321d6ce542f8e9f305544ff09e4993a62319a497c1f"      # Solady's published constant
GUARD_LENS = [0, 1, 2, 3, 20, 32, 52, 63, 64]


def unhex(s):
    return bytes.fromhex(s[2:])


def create3(factory, salt, proxy_hash, guard):
    """(proxy, contract) over the oracle's Keccak; guard None = the raw salt goes in."""
    assert (len(factory), len(salt), len(proxy_hash)) == (20, 32, 32)
    s2 = salt if guard is None else vo.keccak256(guard + salt)
    proxy = vo.keccak256(b"\xff" + factory + s2 + proxy_hash)[12:]
    return proxy, vo.keccak256(b"\xd6\x94" + proxy + b"\x01")[12:]


# ---- host functions -------------------------------------------------------------------------------------------------------------

def test_the_default_proxy_hash_is_computed_and_is_soladys_constant():
    assert GOLDEN["proxy_init_code_hash"] == "0x" + PROXY_HASH
    assert vg.create3_proxy_hash().hex() == PROXY_HASH == vo.keccak256(unhex(GOLDEN["proxy_init_code"])).hex()
    assert unhex(GOLDEN["proxy_init_code"]).hex() == "67363d3d37363d34f03d5260086018f3"
    assert api._L.vgen_create3_proxy_hash(None) == api.E_INVALID
    # computed at run time from the 16 bytes: the 32 bytes of the digest are in no source file
    for path in ("cabi.cpp", "runtime.cpp", "scanner.cpp", "core/hash.h", "cli/vgen_hip_cli.cpp"):
        assert PROXY_HASH[:16] not in open(os.path.join(ROOT, "vgen_amd", "csrc", path)).read().lower().replace(", 0x", "")


def test_the_fixture():
    f, salt = unhex(GOLDEN["factory"]), unhex(GOLDEN["salt"])
    assert salt == bytes(24) + (5).to_bytes(8, "big") and len(GOLDEN["vectors"]) == 4
    assert [None if v["guard"] is None else len(unhex(v["guard"])) for v in GOLDEN["vectors"]] == [None, 0, 20, 64]
    assert GOLDEN["vectors"][0]["contract"] == "0x9fece057dbcf93f177f494d7570ca61992472b5f"
    assert GOLDEN["vectors"][3]["proxy"] == "0xa7782a37a241069ce77b9aca48a484c97fc223d8"
    for v in GOLDEN["vectors"]:
        guard = None if v["guard"] is None else unhex(v["guard"])
        want = (unhex(v["proxy"]), unhex(v["contract"]))
        assert create3(f, salt, bytes.fromhex(PROXY_HASH), guard) == want                    # the oracle agrees with the fixture
        assert vg.create3_address(f, salt, None, guard, with_proxy=True) == want            # ... and so does the host function
        assert vg.create3_address(GOLDEN["factory"], GOLDEN["salt"], "0x" + PROXY_HASH, guard) == want[1]
        # the composition of the two host functions pinned by the CREATE and CREATE2 tests
        s2 = salt if guard is None else vg.keccak256(guard + salt)
        assert vg.contract_address(vg.create2_address(f, s2, bytes.fromhex(PROXY_HASH)), 1) == want[1]
    assert GOLDEN["vectors"][0]["contract"] != GOLDEN["vectors"][1]["contract"]             # a guard of length 0 is not "no guard"


def test_host_function_on_random_jobs_against_the_composition():
    rng = random.Random(3)
    for k in range(300):
        f, s, h = rng.randbytes(20), rng.randbytes(32), rng.randbytes(32)
        guard = None if k % 4 == 0 else rng.randbytes(GUARD_LENS[k % len(GUARD_LENS)] if k % 2 else rng.randrange(65))
        proxy, contract = vg.create3_address(f, s, h, guard, with_proxy=True)
        assert (proxy, contract) == create3(f, s, h, guard)
        s2 = s if guard is None else vg.keccak256(guard + s)
        assert proxy == vg.create2_address(f, s2, h) and contract == vg.contract_address(proxy, 1)


def test_guard_len_validation():
    f, s, h = bytes(range(20)), bytes(range(32)), bytes(range(32, 64))
    out, proxy = api.ctypes.create_string_buffer(20), api.ctypes.create_string_buffer(20)
    call = api._L.vgen_create3_address
    assert call(f, s, h, None, -1, None, out) == api.OK and out.raw == create3(f, s, h, None)[1]         # proxy_out is optional
    assert call(f, s, h, None, 0, proxy, out) == api.OK and (proxy.raw, out.raw) == create3(f, s, h, b"")
    assert call(f, s, h, bytes(64), 64, proxy, out) == api.OK and (proxy.raw, out.raw) == create3(f, s, h, bytes(64))
    assert call(f, s, h, bytes(64), -1, proxy, out) == api.OK and out.raw == create3(f, s, h, None)[1]   # a guard nobody reads
    for guard, n in ((bytes(65), 65), (bytes(64), -2), (None, 1), (None, 64), (bytes(64), 2**31 - 1), (bytes(64), -2**31)):
        assert call(f, s, h, guard, n, proxy, out) == api.E_INVALID, n
    for args in ((None, s, h, None, -1, proxy, out), (f, None, h, None, -1, proxy, out), (f, s, None, None, -1, proxy, out), (f, s, h, None, -1, proxy, None)):
        assert call(*args) == api.E_INVALID
    assert api._L.vgen_set_create3(None, f, h, bytes(24), None, -1) == api.E_INVALID
    with pytest.raises(ValueError):
        vg.create3_address(f, s, h, bytes(65))


def test_job_object():
    f = bytes(range(1, 21))
    j = vg.Create3Job(f, salt_prefix=b"\xaa\xbb")
    assert j.proxy_init_code_hash.hex() == PROXY_HASH and j.salt_prefix == b"\xaa\xbb" + bytes(22) and j.guard is None and j.guard_len == -1
    salt = b"\xaa\xbb" + bytes(22) + (5).to_bytes(8, "big")
    assert j.salt(5) == j.guarded_salt(5) == salt
    assert (j.proxy(5), j.address(5)) == create3(f, salt, bytes.fromhex(PROXY_HASH), None)
    h = bytes(range(0x40, 0x60))
    for guard in (b"", bytes(range(20)), "0x" + "ab" * 64):
        gb = bytes.fromhex(guard[2:]) if isinstance(guard, str) else guard
        j = vg.Create3Job("0x" + f.hex(), "0x" + h.hex(), "0xaabb", guard)
        assert (j.guard, j.guard_len) == (gb, len(gb))
        assert j.salt(2**64 - 1) == b"\xaa\xbb" + bytes(22) + b"\xff" * 8 and j.guarded_salt(7) == vo.keccak256(gb + j.salt(7))
        assert (j.proxy(7), j.address(7)) == create3(f, j.salt(7), h, gb)
    for bad in (dict(salt_prefix=bytes(25)), dict(guard=bytes(65)), dict(proxy_init_code_hash=bytes(31))):
        with pytest.raises(ValueError):
            vg.Create3Job(f, **bad)
    with pytest.raises(ValueError):
        vg.Create3Job(bytes(19))


def test_format_number_and_abi_version_are_unchanged():
    assert vg.abi_version() == 4 and [int(x) for x in vg.AddressFormat] == list(range(8))
    hdr = open(os.path.join(ROOT, "include", "vgen_hip.h")).read()
    assert re.search(r"#define VGEN_ABI_VERSION 4\b", hdr) and re.search(r"VGEN_FMT_ETHEREUM_CREATE2\s*=\s*7\s", hdr)
    assert not re.search(r"VGEN_FMT_\w+\s*=\s*([89]|\d\d)\b", hdr) and "VGEN_FMT_ETHEREUM_CREATE3" not in hdr
    types = open(os.path.join(ROOT, "vgen_amd", "csrc", "device", "device_types.h")).read()
    assert not re.search(r"VGF_\w+\s*=\s*([89]|\d\d)\b", types)
    out = api.ctypes.create_string_buffer(128)
    for bad in (8, 9):
        assert api._L.vgen_address_from_payload(bad, bytes(20), out, 128) == api.E_UNSUPPORTED
    for fn in ("vgen_create3_proxy_hash", "vgen_create3_address", "vgen_set_create3", "vgen_scan_create3"):
        assert re.search(r"\bint %s\(" % fn, hdr), fn


# ---- the generated blocks ----------------------------------------------------------------------------------------------------------

SCHEDULES = [(False, 0, 1, 0), (True, 0, 1, 0), (False, 8, 1, 0), (False, 16, 2, 0), (False, 0, 1, 1), (False, 0, 1, 4), (False, 0, 1, 40), (True, 0, 1, 8)]


def scheduled(prog, grouped, window, distance, class_window):
    p, _, _ = prog(grouped)
    if window:
        g.spread(p, window, distance)
    if class_window:
        n = len(p.ins)
        runs = g.by_class(p, class_window)
        assert sum(runs) == n == len(p.ins)
    reg, nreg = g.allocate(p)
    if class_window <= 8:
        assert nreg <= 96
    return p, reg, nreg


def test_the_blocks_have_a_table_of_their_own():
    assert list(g.PROGRAMS_CREATE3) == ["keccak_create1_block", "keccak_guard_block"]
    assert not set(g.PROGRAMS_CREATE3) & (set(g.PROGRAMS) | set(g.OPTIONAL) | set(g.PROGRAMS_CONTRACT) | set(g.PROGRAMS_CREATE2))
    assert g.YIELDS["keccak_create1_block"] == g.YIELDS["keccak_guard_block"] == "none"
    older = g.generate() + g.generate_create2()
    assert "keccak_create1_block" not in older and "keccak_guard_block" not in older
    src = g.generate_create3()
    assert "void keccak_create1_block(const u32 a[5], u32 out[5])" in src and "void keccak_guard_block(const u32 w[26], u32 out[8])" in src
    assert src.count("void ") == 2 and "(a[4] >> 16) | 0x01010000u;" in src and "0x01800000u" not in src
    assert src.count("s_nop 0") == 0 and src.rstrip().splitlines()[-1] == "}"
    # main() writes the three texts one after another
    out = subprocess.run([sys.executable, os.path.join(ROOT, "vgen_amd", "csrc", "device", "hashgen.py")], capture_output=True, text=True, check=True).stdout
    assert out == older + src


@pytest.mark.parametrize("grouped,window,distance,class_window", SCHEDULES)
def test_create1_block_computes_the_nonce_one_contract_address(grouped, window, distance, class_window):
    rng = random.Random(hash((grouped, window, class_window)) & 0xFFFF)
    p, reg, nreg = scheduled(g.prog_keccak_create1, grouped, window, distance, class_window)
    assert len(p.inputs) == 6 and len(p.outputs) == 5 and sorted(reg[i] for i in p.inputs) == list(range(6))
    cases = [rng.randbytes(20) for _ in range(8)] + [unhex(v["proxy"]) for v in GOLDEN["vectors"]]
    for proxy in cases:
        msg = b"\xd6\x94" + proxy + b"\x01" + b"\x01"          # the RLP list [proxy, 1], then the padding's 0x01 at byte 23
        inputs = {f"m{i}": w for i, w in enumerate(struct.unpack("<6I", msg))}
        want = vo.keccak256(b"\xd6\x94" + proxy + b"\x01")[12:]
        assert want == vg.contract_address(proxy, 1)
        for out in (g.evaluate(p, inputs), g.evaluate_allocated(p, reg, nreg, inputs)):
            assert b"".join(struct.pack("<I", w) for w in out) == want
    assert [unhex(v["contract"]) for v in GOLDEN["vectors"]] == [vo.keccak256(b"\xd6\x94" + c + b"\x01")[12:] for c in cases[8:]]


@pytest.mark.parametrize("grouped,window,distance,class_window", SCHEDULES)
def test_guard_block_computes_the_whole_digest(grouped, window, distance, class_window):
    rng = random.Random(hash((grouped, window, class_window)) & 0xFFFF)
    p, reg, nreg = scheduled(g.prog_keccak_guard, grouped, window, distance, class_window)
    assert len(p.inputs) == 26 and len(p.outputs) == 8 and sorted(reg[i] for i in p.inputs) == list(range(26))
    for n in GUARD_LENS + [rng.randrange(65) for _ in range(3)]:
        msg = rng.randbytes(n + 32)
        inputs = {f"m{i}": w for i, w in enumerate(struct.unpack("<26I", (msg + b"\x01").ljust(104, b"\0")))}
        for out in (g.evaluate(p, inputs), g.evaluate_allocated(p, reg, nreg, inputs)):
            assert b"".join(struct.pack("<I", w) for w in out) == vo.keccak256(msg), n


# ---- the message builders of core/hash.h ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def words_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("create3") / "create3_words")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "create3_words.cpp")])
    return exe


def run_words(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return [int(x, 16) for x in r.stdout.split()]


PREFIX = bytes(range(0xA0, 0xB8))      # 24 distinct bytes
GUARD = bytes(range(0x10, 0x50))       # 64 distinct bytes, none of them in PREFIX


@pytest.mark.parametrize("n", GUARD_LENS)
def test_guarded_message_has_the_counter_and_the_padding_where_they_belong(words_exe, n):
    for counter in (0, 1, 0x0102030405060708, 2**32 - 1, 2**32, 2**64 - 1):
        out = run_words(words_exe, "guard", GUARD[:n].hex() or "-", PREFIX.hex(), str(counter))
        msg = GUARD[:n] + PREFIX + counter.to_bytes(8, "big")
        blob = b"".join(struct.pack("<I", w) for w in out[:26])
        assert blob == (msg + b"\x01").ljust(104, b"\0"), (n, hex(counter))
        assert blob[n + 24:n + 32] == counter.to_bytes(8, "big") and blob[n + 32] == 1 and not any(blob[n + 33:])
        assert b"".join(struct.pack("<I", w) for w in out[26:]) == vo.keccak256(msg)       # the twin of keccak_guard_block
    assert sorted({(k + 24) % 4 for k in GUARD_LENS}) == [0, 1, 2, 3] and (64 + 32) // 4 == 24


def test_digest_to_salt_shift_against_create2_message_of_the_same_bytes(words_exe):
    rng = random.Random(52)
    for _ in range(6):
        f, h, d = rng.randbytes(20), rng.randbytes(32), rng.randbytes(32)
        out = run_words(words_exe, "shift", f.hex(), h.hex(), d.hex())
        want = list(struct.unpack("<22I", b"\xff" + f + d + h + bytes(3)))      # tests/test_create2.py: words()
        assert out == want
    out = run_words(words_exe, "shift", (b"\x11" * 20).hex(), (b"\x22" * 32).hex(), bytes(32).hex())
    assert out[5] == 0x00000011 and out[13] == 0x22222200                      # the job's byte in word 5, its three bytes in word 13


# ---- ISA of the six kernel symbols ---------------------------------------------------------------------------------------------------

SYMS = {(d, gd): "_ZN2vg14create3_kernelILb%dELb%dEEEvNS_11Create3ArgsE" % (d, gd) for d in (1, 0) for gd in (0, 1)}      # (DUMP, GUARD)
SCORE_SYMS = {gd: "_ZN2vg20create3_score_kernelILb%dEEEvNS_16Create3ScoreArgsE" % gd for gd in (0, 1)}


@pytest.fixture(scope="module")
def isa():
    import test_isa_contract as t
    t.locked_make("-s", "-C", os.path.join(ROOT, "vgen_amd", "csrc"), "../../build/lib/device/kernels.s")
    return t.parse_isa(open(t.ISA).read())


def test_isa_of_the_create3_kernels(isa):
    import test_isa_contract as t
    every = {sym: gd for (_, gd), sym in SYMS.items()}
    every.update({sym: gd for gd, sym in SCORE_SYMS.items()})
    assert sorted(s for s in isa if "create3" in s) == sorted(every)
    assert sorted(s for s in isa if "create2_kernel" in s) == sorted("_ZN2vg14create2_kernelILb%dEEEvNS_11Create2ArgsE" % d for d in (1, 0))
    for sym, guarded in every.items():
        k = isa[sym]
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] == 0, (sym, k["vgpr"], k["scratch"], k["lds"])
        assert t.count(k["body"], "scratch_") == 0 and t.count(k["body"], "ds_") == 0, sym
        assert t.count(k["body"], "(global|flat|buffer)_atomic") == 0, sym
        assert t.count(k["body"], "v_mfma") == 0 and t.count(k["body"], "v_smfmac") == 0, sym
        assert t.count(k["body"], "v_alignbit_b32") >= (3 if guarded else 2) * 1351, (sym, t.count(k["body"], "v_alignbit_b32"))
    for sym in [SYMS[0, 0], SYMS[0, 1], SCORE_SYMS[0], SCORE_SYMS[1]]:          # the wave's ballot into the hit mask
        assert t.count(isa[sym]["body"], "global_store_dwordx2") == 1, sym
    for sym in (SYMS[1, 0], SYMS[1, 1]):
        assert t.count(isa[sym]["body"], "global_store_dwordx2") == 0, sym
    table = open(os.path.join(ROOT, "profiles", "r05_kernel_resources.txt")).read()
    for sym in every:
        assert sym.replace("_ZN2vg", "", 1) + "\t" in table, sym


def test_the_kernel_source_has_no_shared_memory_and_no_match_slot():
    src = open(os.path.join(ROOT, "vgen_amd", "csrc", "device", "kernels.hip")).read()
    body = src[src.index("void create3_chain("):]
    assert "match_slot" not in body and "__shared__" not in body and "atomic" not in body
    assert body.count("__global__") == 2 and "keccak_create2_block(m, proxy);" in body      # the proxy stage reuses CREATE2's block


# ---- command line (no device) ---------------------------------------------------------------------------------------------------

DEP, HASH = "0x" + "11" * 20, "0x" + "22" * 32
GOOD = ["generate", "-f", "ethereum-create3", "-p", "^0x0000", "--deployer", DEP]


def cli(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI, *args], capture_output=True, text=True, env=env, timeout=60)


def test_cli_names_the_format_and_gets_to_the_device():
    r = cli("generate", "-f", "nonsense", "-p", "^0xdead")
    assert r.returncode == 1 and "ethereum-create3" in [x.strip(" )\n") for x in r.stderr.split("(", 1)[1].split(",")]
    for extra in ([], ["--proxy-init-code-hash", HASH], ["--salt-guard-hash"], ["--salt-guard", "0x"], ["--salt-guard", "0x" + "ab" * 64],
                  ["--salt-guard", "ab" * 20, "--salt-prefix", "0x" + "cd" * 24, "--salt-start", "12345", "-c", "2", "-i"],
                  ["-p", "score:zero-bytes>=2", "--best"]):
        r = cli(*GOOD, *extra)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (extra, r.stderr)
    for extra in ([], ["--salt-guard-hash"]):
        r = cli("estimate", "-f", "ethereum-create3", "-p", "^0xdead", *extra)
        assert r.returncode == 1 and "no HIP device" in r.stderr and "--format" not in r.stderr, r.stderr


@pytest.mark.parametrize("args,names", [
    (GOOD[:5], "ethereum-create3"),                                                     # no factory
    (GOOD[:5] + ["--deployer", "0x1234"], "--deployer"),
    (GOOD + ["--proxy-init-code-hash", "0x1234"], "--proxy-init-code-hash"),
    (GOOD + ["--salt-guard", "0x" + "ab" * 65], "ethereum-create3"),                    # 65 bytes
    (GOOD + ["--salt-guard", "0xabc"], "ethereum-create3"),                             # odd number of digits
    (GOOD + ["--salt-guard", "0xzz"], "ethereum-create3"),
    (GOOD + ["--salt-guard", "0x00", "--salt-guard-hash"], "ethereum-create3"),
    (GOOD + ["--salt-prefix", "0x" + "ab" * 25], "--salt-prefix"),
    (GOOD + ["--salt-start", "-1"], "--salt-start"),
    (GOOD + ["--seed", "5"], "ethereum-create3"),
    (GOOD + ["--random-keys"], "ethereum-create3"),
    (GOOD + ["--checkpoint", "/tmp/never-written.ckpt"], "ethereum-create3"),
    (GOOD + ["--init-code-hash", HASH], "ethereum-create3"),
    (GOOD + ["--init-code-file", "/dev/null"], "ethereum-create3"),
    (["range", "--puzzle", "20"] + GOOD[1:], "ethereum-create3"),
    (["generate", "-f", "ethereum-create2", "-p", "^0xdead", "--deployer", DEP, "--init-code-hash", HASH, "--salt-guard-hash"], "ethereum-create3"),
    (["generate", "-f", "ethereum", "-p", "^0xdead", "--salt-guard", "0x00"], "ethereum-create3"),
    (["generate", "-f", "p2pkh", "-p", "^1A", "--proxy-init-code-hash", HASH], "ethereum-create3"),
])
def test_cli_argument_errors_come_before_the_device(args, names):
    r = cli(*args)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "no HIP device" not in r.stderr and names in r.stderr, r.stderr


def test_cli_refuses_a_patterns_file(tmp_path):
    f = tmp_path / "pats.txt"
    f.write_text("^0x00\n^0xab\n")
    r = cli("generate", "-f", "ethereum-create3", "--patterns-file", str(f), "--deployer", DEP)
    assert r.returncode == 1 and "--patterns-file" in r.stderr and "ethereum-create3" in r.stderr and "no HIP device" not in r.stderr, r.stderr
