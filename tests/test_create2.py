"""The CREATE2 format (VGEN_FMT_ETHEREUM_CREATE2 = 7) on the CPU: the address keccak256(0xff || deployer || salt || keccak256(init_code))[12:]
of EIP-1014, searched by salt.

Ground truth is the oracle's keccak256 over bytes written out here and the seven examples of EIP-1014 (tests/golden/eip1014.json),
never the code under test.  Checked: the general Keccak sponge and the address and salt helpers of the C ABI, the generated block
of device/hashgen.py in its Python model, the counter's place in the message, the filter compiler for the new format, the ISA of
the two kernel symbols, and the command line's argument checks (no device needed).

The job of a search travels through the C ABI as three byte arrays (deployer, init_code_hash, salt_prefix): the set of structures
of include/vgen_hip.h is fixed by tests/test_binding_matches_header.py.  The reference has no such format (src/address.rs:11-24)."""
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
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "eip1014.json")))["vectors"]


def unhex(s):
    return bytes.fromhex(s[2:])


def create2(deployer, salt, init_code_hash):
    """EIP-1014 over the oracle's Keccak."""
    assert (len(deployer), len(salt), len(init_code_hash)) == (20, 32, 32)
    return vo.keccak256(b"\xff" + deployer + salt + init_code_hash)[12:]


def words(deployer, salt, init_code_hash):
    """The 22 little-endian words of the 85-byte message (bytes 85..87 zero): what the block and its twin take."""
    return list(struct.unpack("<22I", b"\xff" + deployer + salt + init_code_hash + bytes(3)))


# ---- hash and address ---------------------------------------------------------------------------------------------------------

def test_the_fixture_is_eip_1014s_and_agrees_with_the_oracle():
    assert len(VECTORS) == 7
    assert VECTORS[0]["address"] == "0x4d1a2e2bb4f88f0250f26ffff098b0b30b26bf38" and VECTORS[6]["address"] == "0xe33c0c7f7df4809055c3eba6c09cfe4baf1bd9e0"
    for v in VECTORS:
        assert create2(unhex(v["deployer"]), unhex(v["salt"]), vo.keccak256(unhex(v["init_code"]))).hex() == v["address"][2:]


@pytest.mark.parametrize("n", [0, 1, 135, 136, 137, 271, 272, 1000])
def test_keccak256_of_any_length(n):
    rng = random.Random(n)
    data = rng.randbytes(n)
    assert vg.keccak256(data) == vo.keccak256(data)
    out = api.ctypes.create_string_buffer(32)
    assert api._L.vgen_keccak256(data, n, None) == api.E_INVALID
    assert api._L.vgen_keccak256(None, 0, out) == api.OK and out.raw == vo.keccak256(b"")


def test_create2_address_on_the_vectors_and_on_random_jobs():
    for v in VECTORS:
        h = vg.keccak256(unhex(v["init_code"]))
        assert vg.create2_address(unhex(v["deployer"]), unhex(v["salt"]), h).hex() == v["address"][2:]
        assert vg.create2_address(v["deployer"], v["salt"], "0x" + h.hex()).hex() == v["address"][2:]
    rng = random.Random(1014)
    for _ in range(300):
        d, s, h = rng.randbytes(20), rng.randbytes(32), rng.randbytes(32)
        assert vg.create2_address(d, s, h) == create2(d, s, h)
    out = api.ctypes.create_string_buffer(20)
    for args in ((None, bytes(32), bytes(32), out), (bytes(20), None, bytes(32), out), (bytes(20), bytes(32), None, out), (bytes(20), bytes(32), bytes(32), None)):
        assert api._L.vgen_create2_address(*args) == api.E_INVALID


def test_job_object():
    code = bytes.fromhex("6080604052")
    j = vg.Create2Job(bytes(range(1, 21)), init_code=code, salt_prefix=b"\xaa\xbb")
    assert j.init_code_hash == vo.keccak256(code) and j.salt_prefix == b"\xaa\xbb" + bytes(22)
    assert j.address(5) == create2(bytes(range(1, 21)), b"\xaa\xbb" + bytes(22) + (5).to_bytes(8, "big"), vo.keccak256(code))
    assert vg.Create2Job("0x" + "11" * 20, init_code_hash="0x" + "22" * 32).salt_prefix == bytes(24)
    for bad in (dict(), dict(init_code=b"", init_code_hash=bytes(32)), dict(init_code_hash=bytes(31)), dict(init_code=b"", salt_prefix=bytes(25))):
        with pytest.raises(ValueError):
            vg.Create2Job(bytes(20), **bad)


# ---- counter placement ----------------------------------------------------------------------------------------------------------

PREFIX = bytes(range(0xA0, 0xB8))      # 24 distinct bytes


@pytest.mark.parametrize("counter", [0, 1, 0xFF, 0x100, 0xFFFFFFFF, 0x100000000, 2**64 - 1])
def test_salt_is_prefix_then_the_counter_big_endian(counter):
    j = vg.Create2Job(bytes(20), init_code_hash=bytes(32), salt_prefix=PREFIX)
    assert j.salt(counter) == PREFIX + counter.to_bytes(8, "big")
    out = api.ctypes.create_string_buffer(32)
    assert api._L.vgen_create2_salt(None, counter, out) == api.E_INVALID and api._L.vgen_create2_salt(PREFIX, counter, None) == api.E_INVALID


def test_the_counter_straddles_lanes_5_and_6():
    """Message bytes 45..52 = words 11 (bytes 1..3), 12 and 13 (byte 0): the words the kernel ORs the counter into."""
    d, h = bytes(range(1, 21)), bytes(range(0x40, 0x60))
    base = words(d, PREFIX + bytes(8), h)
    for counter in (1, 0x0102030405060708, 2**64 - 1):
        w = words(d, PREFIX + counter.to_bytes(8, "big"), h)
        assert [i for i in range(22) if w[i] != base[i]] in ([13], [11, 12, 13])
        assert (w[11] & 0xFF, w[13] >> 8) == (base[11] & 0xFF, base[13] >> 8)
        assert (w[10], w[14]) == (base[10], base[14])


# ---- the generated block ---------------------------------------------------------------------------------------------------------

def case_keccak_create2(rng):
    d, s, h = rng.randbytes(20), rng.randbytes(32), rng.randbytes(32)
    return words(d, s, h), create2(d, s, h)


def test_the_block_has_a_table_of_its_own():
    assert list(g.PROGRAMS_CREATE2) == ["keccak_create2_block"]
    assert not set(g.PROGRAMS_CREATE2) & (set(g.PROGRAMS) | set(g.OPTIONAL) | set(g.PROGRAMS_CONTRACT))
    assert list(g.PROGRAMS_CONTRACT) == ["keccak_create_block"] and g.YIELDS["keccak_create2_block"] == "none"


@pytest.mark.parametrize("grouped,window,distance,class_window", [(False, 0, 1, 0), (True, 0, 1, 0), (False, 8, 1, 0), (False, 16, 2, 0),
                                                                  (False, 0, 1, 1), (False, 0, 1, 4), (False, 0, 1, 40), (True, 0, 1, 8)])
def test_block_computes_the_create2_address(grouped, window, distance, class_window):
    rng = random.Random(hash((grouped, window, class_window)) & 0xFFFF)
    p, _, _ = g.prog_keccak_create2(grouped)
    if window:
        g.spread(p, window, distance)
    if class_window:
        n = len(p.ins)
        runs = g.by_class(p, class_window)
        assert sum(runs) == n == len(p.ins)
    reg, nreg = g.allocate(p)
    if class_window <= 8:
        assert nreg <= 96
    assert len(p.inputs) == 22 and sorted(reg[i] for i in p.inputs) == list(range(22))
    cases = [case_keccak_create2(rng) for _ in range(8)]
    cases += [(words(unhex(v["deployer"]), unhex(v["salt"]), vo.keccak256(unhex(v["init_code"]))), unhex(v["address"])) for v in VECTORS]
    for m, want in cases:
        m = list(m)
        m[21] |= 0x100          # the prologue's OR: the 0x01 of the padding at message byte 85
        inputs = {f"m{i}": w for i, w in enumerate(m)}
        for out in (g.evaluate(p, inputs), g.evaluate_allocated(p, reg, nreg, inputs)):
            assert b"".join(struct.pack("<I", w) for w in out) == want


def test_the_instruction_count_of_the_block():
    """Pinned to what the generator produces: Keccak-f[1600] on eleven message lanes, the padding lane and thirteen zero lanes,
    pruned to the five output words (keccak_addr_block on eight message lanes: 4 195)."""
    p, _, _ = g.prog_keccak_create2()
    c = p.census()
    assert c == {"bitop3": 2795, "alignbit": 1351, "mov": 10, "xor": 35} and sum(c.values()) == 4191


def test_asm_text_shape_of_the_block():
    older = g.generate()
    assert "keccak_create2_block" not in older            # generate() is the text of the older tables, unchanged ...
    src = older + g.generate_create2()                    # ... and the file the Makefile writes is that text, then the new table
    assert "void keccak_create2_block(const u32 w[22], u32 out[5])" in src
    # emitted after every older function: the text slices the older blocks are cut out by stay what they were
    at = src.index("void keccak_create2_block(")
    assert all(src.index(f"void {n}(") < at for n in list(g.PROGRAMS) + list(g.PROGRAMS_CONTRACT))
    assert src.count("void keccak_create2_block(") == 1 and "void " not in src[at + 5:]
    body = src[at:]
    lines = re.findall(r'"([^"]*)\\n\\t"', body)
    assert sum(l.startswith("v_") for l in lines) == 4191
    assert "s_nop 0" not in lines
    for a, b in zip(lines, lines[1:]):
        assert not (a.startswith("s_setprio") and b.startswith("s_setprio"))
    level, changes = None, 0
    for l in lines:
        if l.startswith("s_setprio"):
            level, changes = int(l.split()[1]), changes + 1
        elif l.startswith("v_"):
            assert level == (1 if l.startswith(("v_alignbit_b32", "v_add3_u32", "v_perm_b32")) else 0), l
    assert lines[-1] == "s_setprio 1" and changes > 100
    for i, l in enumerate(lines):
        if l.startswith(("v_add3_u32", "v_bitop3_b32", "v_perm_b32", "v_alignbit_b32")):
            assert not re.search(r"0x[0-9a-f]{8}", l.split(" bitop3:")[0]), l
        if l.startswith("s_mov_b32"):
            assert "%[k]" in lines[i + 1], (l, lines[i + 1])
    assert "u32 m21 = w[21] | 0x00000100u;" in body and "u32 m11 = w[11];" in body and "bswap" not in body
    assert '"=&s"(k)' in body and body.count('"+v"') == 22


# ---- filter, format number, payload ------------------------------------------------------------------------------------------------

def test_format_number_and_abi_version():
    assert vg.abi_version() == 4 and int(vg.AddressFormat.EthereumCreate2) == FMT
    hdr = open(os.path.join(ROOT, "include", "vgen_hip.h")).read()
    assert re.search(r"VGEN_FMT_ETHEREUM_CREATE2\s*=\s*7\b", hdr) and re.search(r"#define VGEN_ABI_VERSION 4\b", hdr)
    types = open(os.path.join(ROOT, "vgen_amd", "csrc", "device", "device_types.h")).read()
    assert re.search(r"VGF_ETHEREUM_CREATE2\s*=\s*7\b", types)
    # the predicate for "hashes both coordinates" is not widened
    assert re.search(r"vgf_is_eth\(int fmt\) \{ return fmt == VGF_ETHEREUM \|\| fmt == VGF_ETHEREUM_CONTRACT; \}", types)
    assert vg.AddressFormat.EthereumCreate2.charset_name() == "Hex"


@pytest.mark.parametrize("pat,ci", [("^0xdead", False), ("dead$", False), ("ab", False), ("^0xDe", True)])
def test_filter_compilation_is_format_fives(pat, ci):
    p7, p5 = vg.Pattern(pat, ci, FMT), vg.Pattern(pat, ci, 5)
    assert p7.device_kind == p5.device_kind and p7.dfa_bytes == p5.dfa_bytes
    assert p7.estimate_difficulty() == p5.estimate_difficulty() and p7.validate_charset() == p5.validate_charset()
    # same device tests: a sample of payloads the two compiled filters are asked about through the host's own matcher
    rng = random.Random(7)
    rx = vo.Regex(pat, ci)
    addrs = [vo.eip55(rng.randbytes(20)) for _ in range(3000)] + [vo.eip55(bytes.fromhex("dead") + rng.randbytes(16) + bytes.fromhex("dead"))]
    assert [p7.matches(a) for a in addrs] == [rx.matches(a) for a in addrs] == [p5.matches(a) for a in addrs]
    assert any(vo.Regex(pat, True).matches(a) for a in addrs)
    if ci or pat == "ab":
        assert any(rx.matches(a) for a in addrs)


def test_pattern_list_compiles_for_the_format():
    pl = vg.PatternList(["^0x00", "^0xab"], fmt=FMT)
    assert pl.device_kind == 5 and pl.which("0x00" + "1" * 38) == [0] and pl.which("0xab" + "1" * 38) == [1] and pl.which("0x11" + "1" * 38) == []


def test_address_from_payload_is_eip55_and_no_key_owns_an_address():
    rng = random.Random(55)
    for _ in range(50):
        pl = rng.randbytes(20)
        assert vg.address_from_payload(FMT, pl) == vo.eip55(pl) == vg.address_from_payload(5, pl)
    out = api.ctypes.create_string_buffer(128)
    assert api._L.vgen_derive(FMT, (1).to_bytes(32, "big"), out, 128, None, 0) == api.E_UNSUPPORTED
    for bad in (8, 9):
        assert api._L.vgen_address_from_payload(bad, bytes(20), out, 128) == api.E_UNSUPPORTED


# ---- ISA of the two kernel symbols -----------------------------------------------------------------------------------------------

SYMS = ["_ZN2vg14create2_kernelILb%dEEEvNS_11Create2ArgsE" % d for d in (1, 0)]      # DUMP, !DUMP


@pytest.fixture(scope="module")
def isa():
    import test_isa_contract as t
    t.locked_make("-s", "-C", os.path.join(ROOT, "vgen_amd", "csrc"), "../../build/lib/device/kernels.s")
    return t.parse_isa(open(t.ISA).read())


def test_isa_of_the_create2_kernels(isa):
    import test_isa_contract as t
    assert sorted(s for s in isa if "create2_kernel" in s) == sorted(SYMS)
    for sym in SYMS:
        k = isa[sym]
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] == 0, (sym, k["vgpr"], k["scratch"], k["lds"])
        assert t.count(k["body"], "scratch_") == 0 and t.count(k["body"], "ds_") == 0, sym
        assert t.count(k["body"], "(global|flat|buffer)_atomic") == 0, sym
        assert t.count(k["body"], "v_mfma") == 0 and t.count(k["body"], "v_smfmac") == 0, sym
        assert t.count(k["body"], "v_alignbit_b32") >= 1351 and t.count(k["body"], "v_bitop3_b32") >= 2795, sym
    assert t.count(isa[SYMS[1]]["body"], "global_store_dwordx2") >= 1          # the wave's ballot into the hit mask
    # the block is in the assembly in the generator's order (modulo register names), in both kernels
    p, _, _ = g.prog_keccak_create2()
    g.by_class(p, g.DEFAULT_CLASS_WINDOW)
    reg, _ = g.allocate(p)
    prio = tuple(int(x) for x in g.DEFAULT_PRIO.split(":"))
    want = [re.sub(r"%\[\w+\]", "R", l) for l in g.asm_lines(p, reg, "none", prio)[0]]
    for sym in SYMS:
        norm = []
        for l in isa[sym]["body"]:
            l = l.split(";")[0].strip()
            if re.match(r"(v_|s_nop|s_mov_b32|s_setprio)", l):
                norm.append(re.sub(r"\b[vs]\d+\b", "R", l))
        first = next(i for i in range(len(norm)) if norm[i:i + 12] == want[:12])
        assert norm[first:first + len(want)] == want, sym
    table = open(os.path.join(ROOT, "profiles", "r05_kernel_resources.txt")).read()
    for sym in SYMS:
        assert sym.replace("_ZN2vg", "", 1) + "\t" in table, sym


def test_the_kernel_source_keeps_the_match_path_contract():
    src = open(os.path.join(ROOT, "vgen_amd", "csrc", "device", "kernels.hip")).read()
    body = src[src.index("void __launch_bounds__(256) create2_kernel("):]
    assert "match_slot" not in body and "atomic" not in body.split("hipError_t launch_create2")[0].replace("No atomics", "")
    assert "__shared__" not in body


# ---- command line (no device) ---------------------------------------------------------------------------------------------------

DEP, HASH = "0x" + "11" * 20, "0x" + "22" * 32
GOOD = ["generate", "-f", "ethereum-create2", "-p", "^0x0000", "--deployer", DEP, "--init-code-hash", HASH]


def cli(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI, *args], capture_output=True, text=True, env=env, timeout=60)


def test_cli_names_the_format_and_gets_to_the_device():
    r = cli("generate", "-f", "nonsense", "-p", "^0xdead")
    assert r.returncode == 1 and "ethereum-create2" in [x.strip(" )\n") for x in r.stderr.split("(", 1)[1].split(",")]
    for extra in ([], ["--salt-prefix", "0x" + "ab" * 24, "--salt-start", "12345", "-c", "2", "-i"], ["--salt-prefix", "abcd"]):
        r = cli(*GOOD, *extra)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (extra, r.stderr)
    r = cli("estimate", "-f", "ethereum-create2", "-p", "^0xdead")
    assert r.returncode == 1 and "no HIP device" in r.stderr and "--format" not in r.stderr, r.stderr


def test_cli_init_code_file(tmp_path):
    f = tmp_path / "code.bin"
    f.write_bytes(bytes.fromhex("deadbeef"))
    r = cli(*GOOD[:-2], "--init-code-file", str(f))
    assert r.returncode == 1 and "no HIP device" in r.stderr, r.stderr
    r = cli(*GOOD[:-2], "--init-code-file", str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "no HIP device" not in r.stderr and "init code file" in r.stderr, r.stderr


@pytest.mark.parametrize("args", [
    GOOD[:5] + ["--init-code-hash", HASH],                                            # no deployer
    GOOD[:5] + ["--deployer", "0x1234", "--init-code-hash", HASH],                    # malformed deployer
    GOOD[:5] + ["--deployer", "0x" + "zz" * 20, "--init-code-hash", HASH],
    GOOD[:7],                                                                         # neither init-code option
    GOOD + ["--init-code-file", "/dev/null"],                                         # both
    GOOD[:7] + ["--init-code-hash", "0x1234"],                                        # malformed hash
    GOOD + ["--salt-prefix", "0x" + "ab" * 25],                                       # over-long prefix
    GOOD + ["--salt-prefix", "0xabc"],                                                # odd number of digits
    GOOD + ["--salt-start", "-1"],
    GOOD + ["--seed", "5"],
    GOOD + ["--random-keys"],
    GOOD + ["--checkpoint", "/tmp/never-written.ckpt"],
    ["range", "--puzzle", "20"] + GOOD[1:],
    ["generate", "-f", "ethereum", "-p", "^0xdead", "--deployer", DEP],               # the new options with another format
    ["generate", "-f", "p2pkh", "-p", "^1A", "--salt-start", "5"],
    ["generate", "-f", "ethereum-contract", "-p", "^0xdead", "--init-code-hash", HASH],
])
def test_cli_argument_errors_come_before_the_device(args):
    r = cli(*args)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "no HIP device" not in r.stderr, r.stderr


def test_cli_refuses_a_patterns_file(tmp_path):
    f = tmp_path / "pats.txt"
    f.write_text("^0x00\n^0xab\n")
    r = cli("generate", "-f", "ethereum-create2", "--patterns-file", str(f), "--deployer", DEP, "--init-code-hash", HASH)
    assert r.returncode == 1 and "--patterns-file" in r.stderr and "no HIP device" not in r.stderr, r.stderr
