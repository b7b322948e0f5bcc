"""The Ethereum-contract format (VGEN_FMT_ETHEREUM_CONTRACT = 6) on the CPU: the address of the contract the key's account
creates with its first transaction, C = keccak256(0xd6 0x94 || A || 0x80)[12:] with A = keccak256(X || Y)[12:].

Ground truth is the oracle's keccak256 over bytes written out here, and tests/golden/eth_create.json (the widely published
deployer 0x6ac7ea33... vector, key 1, nonces of every RLP length) - never the code under test.  Checked: the generated second
Keccak block of device/hashgen.py in its Python model, the host helpers of the C ABI, the filter compiler and the pattern
front end for the new format, the ISA of the new kernel symbols, and the command line's format name.

(`vgen-hip estimate` benchmarks the device before it prints, so its difficulty line is checked in tests/test_gpu_eth_contract.py;
here the same number is asserted through vgen_pattern_difficulty, and `estimate -f ethereum-contract` is shown to get past the
format and the pattern to the device lookup.)
The reference has no such format (src/address.rs:11-24)."""
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

M = 0xFFFFFFFF
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
FMT = 6
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "eth_create.json")))


def create0(account):
    """The oracle formula of the issue: nonce 0."""
    return vo.keccak256(b"\xd6\x94" + account + b"\x80")[12:]


def rlp_create(deployer, nonce):
    """keccak256(rlp([deployer, nonce]))[12:] with the RLP written out by hand (test-side restatement)."""
    if nonce == 0:
        n = b"\x80"
    elif nonce < 0x80:
        n = bytes([nonce])
    else:
        b = nonce.to_bytes((nonce.bit_length() + 7) // 8, "big")
        n = bytes([0x80 + len(b)]) + b
    body = b"\x94" + deployer + n
    return vo.keccak256(bytes([0xC0 + len(body)]) + body)[12:]


# ---- the generated block ------------------------------------------------------------------------------------------------

def case_keccak_create(rng):
    acc = rng.randbytes(20)
    a = struct.unpack("<5I", acc)     # the five words keccak_addr_block leaves (memory order)
    m = [0x94D6 | ((a[0] << 16) & M)] + [(a[i - 1] >> 16) | ((a[i] << 16) & M) for i in range(1, 5)] + [(a[4] >> 16) | 0x01800000]
    assert struct.pack("<6I", *m) == b"\xd6\x94" + acc + b"\x80\x01"      # the prologue IS the padded message
    return m, create0(acc)


CASES = {"keccak_create_block": case_keccak_create}


def test_every_function_of_the_contract_table_has_a_case():
    assert set(CASES) == set(g.PROGRAMS_CONTRACT)
    assert not set(g.PROGRAMS_CONTRACT) & (set(g.PROGRAMS) | set(g.OPTIONAL))


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("grouped,window,distance,class_window", [(False, 0, 1, 0), (True, 0, 1, 0), (False, 8, 1, 0), (False, 16, 2, 0),
                                                                  (False, 0, 1, 1), (False, 0, 1, 4), (False, 0, 1, 40), (True, 0, 1, 8)])
def test_block_computes_the_contract_address(name, grouped, window, distance, class_window):
    rng = random.Random(hash((name, grouped, window)) & 0xFFFF)
    p, _, _ = g.PROGRAMS_CONTRACT[name](grouped)
    if window:
        g.spread(p, window, distance)
    if class_window:
        n = len(p.ins)
        runs = g.by_class(p, class_window)
        assert sum(runs) == n == len(p.ins)
    reg, nreg = g.allocate(p)
    if class_window <= 8:
        assert nreg <= 80
    assert sorted(reg[i] for i in p.inputs) == list(range(len(p.inputs)))
    for _ in range(12):
        m, want = CASES[name](rng)
        inputs = {f"m{i}": w for i, w in enumerate(m)}
        assert len(inputs) == len(p.inputs)
        for out in (g.evaluate(p, inputs), g.evaluate_allocated(p, reg, nreg, inputs)):
            assert b"".join(struct.pack("<I", w) for w in out) == want


def test_block_known_answers():
    p, _, _ = g.prog_keccak_create()
    for acc, want in ((GOLDEN["key_1"]["account"], GOLDEN["key_1"]["contract"]),
                      ("0x6ac7ea33f8831ea9dcc53393aaa88b25a785dbf0", "0xcd234a471b72ba2f1ccf0a70fcaba648a5eecd8d")):
        acc = bytes.fromhex(acc[2:])
        a = struct.unpack("<5I", acc)
        m = [0x94D6 | ((a[0] << 16) & M)] + [(a[i - 1] >> 16) | ((a[i] << 16) & M) for i in range(1, 5)] + [(a[4] >> 16) | 0x01800000]
        out = g.evaluate(p, {f"m{i}": w for i, w in enumerate(m)})
        assert b"".join(struct.pack("<I", w) for w in out).hex() == want[2:].lower()


def test_the_instruction_count_of_the_block():
    # Keccak-f[1600] on three message lanes, the padding lane and 21 zero lanes, pruned to the five output words; Program.bitop3
    # materialises a second constant with a mov instead of restricting the truth table, so the zero lanes buy little
    # (keccak_addr_block on its sixteen message words: 4 195)
    p, _, _ = g.prog_keccak_create()
    c = p.census()
    assert sum(c.values()) == 4217
    assert c == {"bitop3": 2787, "alignbit": 1347, "mov": 48, "xor": 35}


def test_asm_text_shape_of_the_block():
    src = g.generate()
    assert "void keccak_create_block(const u32 a[5], u32 out[5])" in src
    # emitted after every function of PROGRAMS: the text slices the older blocks are cut out by stay what they were
    assert all(src.index(f"void {n}(") < src.index("void keccak_create_block(") for n in g.PROGRAMS)
    body = src[src.index("void keccak_create_block("):]
    lines = re.findall(r'"([^"]*)\\n\\t"', body)
    assert sum(l.startswith("v_") for l in lines) == 4217
    assert "s_nop 0" not in lines                       # YIELDS = "none", as for keccak_addr_block
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
    # the prologue chains the two blocks with 16-bit funnel shifts of the first block's output words, no byte swap
    assert "u32 m0 = 0x94d6u | (a[0] << 16);" in body and "u32 m5 = (a[4] >> 16) | 0x01800000u;" in body and "bswap" not in body
    assert '"=&s"(k)' in body and body.count('"+v"') == 6


# ---- host helpers of the C ABI ----------------------------------------------------------------------------------------------

def test_abi_version_and_enumerator():
    assert vg.abi_version() == 4 and int(vg.AddressFormat.EthereumContract) == 6
    hdr = open(os.path.join(ROOT, "include", "vgen_hip.h")).read()
    assert re.search(r"VGEN_FMT_ETHEREUM_CONTRACT\s*=\s*6\b", hdr) and re.search(r"#define VGEN_ABI_VERSION 4\b", hdr)


def test_derive_address_and_key_against_the_oracle():
    rng = random.Random(606)
    keys = [1, 2, N - 1, 2**65 + 0x5EED0000] + [rng.randrange(1, N) for _ in range(220)]
    for k in keys:
        account = vo.payload(vo.FMT_ETHEREUM, k)
        want = create0(account)
        d = vg.derive(FMT, k)
        assert d.address == vo.eip55(want), k
        assert d.wif == "%064x" % k == vg.key_to_wif(FMT, k) == vg.key_to_wif(5, k)        # the key is shown as hex, as for Ethereum
        assert vg.address_from_payload(FMT, want) == vo.eip55(want) == vg.address_from_payload(5, want)
        assert vg.contract_address(account, 0) == want
        assert vg.derive(5, k).address == vo.eip55(account)                                  # the deployer is the key's account
    for bad in (0, N, N + 5, 2**256 - 1):
        assert vg.derive(FMT, bad) is None                                                    # VGEN_E_RANGE
        out = api.ctypes.create_string_buffer(128)
        assert api._L.vgen_derive(FMT, bad.to_bytes(32, "big"), out, 128, None, 0) == api.E_RANGE
        assert api._L.vgen_key_to_wif(FMT, bad.to_bytes(32, "big"), out, 128) == api.E_RANGE


def test_golden_vectors():
    k1 = GOLDEN["key_1"]
    assert k1["account"] == "0x7e5f4552091a69125d5dfcb7b8c2659029395bdf" and k1["contract"] == "0xF2E246BB76DF876Cef8b38ae84130F4F55De395b"
    assert vg.derive(5, 1).address.lower() == k1["account"] and vg.derive(FMT, 1).address == k1["contract"]
    seen = set()
    for row in GOLDEN["nonces"]:
        dep = bytes.fromhex(row["deployer"][2:])
        assert rlp_create(dep, row["nonce"]).hex() == row["address"][2:]                     # the fixture against the oracle's Keccak
        assert vg.contract_address(dep, row["nonce"]).hex() == row["address"][2:], row
        assert vg.contract_address(row["deployer"], row["nonce"]).hex() == row["address"][2:]
        seen.add((row["deployer"], row["nonce"]))
    pub = "0x6ac7ea33f8831ea9dcc53393aaa88b25a785dbf0"
    rows = {(r["deployer"], r["nonce"]): r["address"] for r in GOLDEN["nonces"]}
    assert rows[(pub, 0)] == "0xcd234a471b72ba2f1ccf0a70fcaba648a5eecd8d" and rows[(pub, 1)] == "0x343c43a37d37dff08ae8c4a11544c718abb4fcf8"
    assert {n for _, n in seen} >= {0, 1, 0x7F, 0x80, 0xFF, 0x100, 0xFFFF, 0x10000, 2**64 - 1}  # every RLP branch


def test_contract_address_rlp_against_the_oracle():
    rng = random.Random(9)
    for _ in range(300):
        dep = rng.randbytes(20)
        nonce = rng.choice([0, 1, 0x7F, 0x80, 0x81, 0xFF, 0x100, rng.getrandbits(rng.randrange(1, 65))])
        assert vg.contract_address(dep, nonce) == rlp_create(dep, nonce), (dep.hex(), nonce)
    out = api.ctypes.create_string_buffer(20)
    assert api._L.vgen_contract_address(None, 0, out) == api.E_INVALID and api._L.vgen_contract_address(bytes(20), 0, None) == api.E_INVALID


# ---- filters and the pattern front end -----------------------------------------------------------------------------------------

def test_filter_compile_device_kinds():
    for pat, ci in (("^0xdead", False), ("^0xdead", True), ("dead$", False), ("^0xDeAd", False), ("^0xDEAD", True), ("^0x0000", False)):
        p6, p5 = vg.Pattern(pat, ci, FMT), vg.Pattern(pat, ci, 5)
        assert p6.device_kind == 2 == p5.device_kind, pat
    p6 = vg.Pattern("de[0-9]d", False, FMT)
    assert p6.device_kind == 4 and p6.dfa_bytes == vg.Pattern("de[0-9]d", False, 5).dfa_bytes > 0
    for bad in (9, 17):
        d, n = api.ctypes.c_uint64(), api.ctypes.c_size_t()
        assert api._L.vgen_pattern_difficulty(b"a", 0, bad, api.ctypes.byref(d)) < 0
        assert api._L.vgen_pattern_invalid_chars(b"a", 0, bad, None, 0, api.ctypes.byref(n)) < 0
        assert api._L.vgen_format_charset_name(bad) is None
        out = api.ctypes.create_string_buffer(128)
        assert api._L.vgen_address_from_payload(bad, bytes(20), out, 128) == api.E_UNSUPPORTED
        assert api._L.vgen_derive(bad, (1).to_bytes(32, "big"), out, 128, None, 0) == api.E_UNSUPPORTED


def test_host_matching_is_format_fives():
    """Case folding, mixed-case patterns and -i behave as for Ethereum: the exact automaton judges the EIP-55 string."""
    rng = random.Random(17)
    addrs = [vo.eip55(create0(rng.randbytes(20))) for _ in range(4000)]
    for pat, ci in (("^0xd", False), ("^0xD", False), ("^0xd", True), ("a$", False), ("A$", False), ("a$", True), ("[0-9]e[A-F]", False)):
        rx = vo.Regex(pat, ci)
        p6, p5 = vg.Pattern(pat, ci, FMT), vg.Pattern(pat, ci, 5)
        want = [rx.matches(a) for a in addrs]
        assert [p6.matches(a) for a in addrs] == want == [p5.matches(a) for a in addrs], pat
        assert 0 < sum(want) < len(addrs)


def test_pattern_list_of_hex_prefixes():
    rng = random.Random(23)
    pats = sorted({"^0x" + "".join(rng.choice("0123456789abcdef") for _ in range(2)) for _ in range(40)}) + ["^0xAb1", "^0xdEaD"]
    plist = vg.PatternList(pats, fmt=FMT)
    assert plist.device_kind == 5 and len(plist) == len(pats)
    rxs = [vo.Regex(p) for p in pats]
    hits = 0
    for _ in range(6000):
        a = vo.eip55(create0(rng.randbytes(20)))
        want = [i for i, rx in enumerate(rxs) if rx.matches(a)]
        assert plist.which(a) == want, a
        assert plist.matches(a) == bool(want)
        hits += bool(want)
    assert hits > 300
    ci = vg.PatternList(["^0xAB", "^0xcd"], case_insensitive=True, fmt=FMT)
    for _ in range(3000):
        a = vo.eip55(create0(rng.randbytes(20)))
        assert ci.which(a) == [i for i, h in enumerate(("ab", "cd")) if a[2:4].lower() == h]


def test_pattern_front_end_equals_format_five():
    assert vg.AddressFormat.EthereumContract.charset_name() == "Hex" == vg.AddressFormat.Ethereum.charset_name()
    for pat in ("^0xdead", "^0xDEAD", "dead$", "^0xg00d", "^0xdeadbeef", "^1Cat", "de[0-9]d", "^0", "^0x", "beef", "^0XAB", "O0Il"):
        for ci in (False, True):
            p = vg.Pattern(pat, ci, FMT)
            assert p.estimate_difficulty() == p.estimate_difficulty(vg.AddressFormat.Ethereum), (pat, ci)
            assert p.validate_charset() == p.validate_charset(vg.AddressFormat.Ethereum), (pat, ci)
    assert vg.Pattern("^0xdead", False, FMT).estimate_difficulty() == 16 ** 4
    assert vg.Pattern("^0xg00d", False, FMT).validate_charset() == ["g"]


# ---- ISA of the new kernel symbols -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def isa():
    import test_isa_contract as t
    t.locked_make("-s", "-C", os.path.join(ROOT, "vgen_amd", "csrc"), "../../build/lib/device/kernels.s")
    return t.parse_isa(open(t.ISA).read())


def test_isa_of_the_contract_kernels(isa):
    """The per-key kernels of the format only write payloads (kernels.hip: DumpOnly): plain and six-image forms of the walk and
    of the arbitrary-scalar path.  They carry no match path - no atomic -; their filter is payload_filter_kernel (ballot stores
    into the hit mask, no atomic either) and the records are made by the list path's ptab_compact_kernel."""
    import test_isa_contract as t
    seq = ["_ZN2vg14seq_bwd_kernelILi6ELb0ELb%dELb0ELb0EEEvNS_7SeqArgsE" % endo for endo in (0, 1)]
    keys = ["_ZN2vg15keys_bwd_kernelILi6ELb0ELb%dEEEvNS_8KeysArgsE" % endo for endo in (0, 1)]
    assert sorted(s for s in isa if "kernelILi6E" in s) == sorted(seq + keys)     # no FULL forms, no one-frame twin
    for sym in seq + keys:
        k = isa[sym]
        # both generated Keccak bodies: 1 351 funnel shifts of keccak_addr_block + 1 347 of keccak_create_block
        assert t.count(k["body"], "v_alignbit_b32") >= 1351 + 1347, sym
        assert t.count(k["body"], "v_bitop3_b32") >= 2795 + 2787, sym
        assert k["scratch"] == 0 and t.count(k["body"], "scratch_") == 0, sym
        assert t.count(k["body"], "v_mfma") == 0
        assert t.count(k["body"], "(global|flat|buffer)_atomic") == 0, sym
        eth = isa[sym.replace("ILi6E", "ILi5E")]
        assert k["lds"] == eth["lds"], sym                                      # ypark / PARKI as for Ethereum
        assert k["vgpr"] <= 128, (sym, k["vgpr"])                               # four waves per SIMD, as Ethereum
    filt = [s for s in isa if "payload_filter_kernel" in s]
    assert len(filt) == 2
    for sym in filt:
        k = isa[sym]
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and t.count(k["body"], "(global|flat|buffer)_atomic") == 0, sym
        assert t.count(k["body"], "global_store_dwordx2") >= 1                  # the wave's ballot into the hit mask
    # the block is in the assembly in the generator's order (modulo register names)
    p, _, _ = g.prog_keccak_create()
    g.by_class(p, g.DEFAULT_CLASS_WINDOW)
    reg, _ = g.allocate(p)
    prio = tuple(int(x) for x in g.DEFAULT_PRIO.split(":"))
    want = [re.sub(r"%\[\w+\]", "R", l) for l in g.asm_lines(p, reg, "none", prio)[0]]
    norm = []
    for l in isa[seq[0]]["body"]:
        l = l.split(";")[0].strip()
        if re.match(r"(v_|s_nop|s_mov_b32|s_setprio)", l):
            norm.append(re.sub(r"\b[vs]\d+\b", "R", l))
    first = next(i for i in range(len(norm)) if norm[i:i + 12] == want[:12])
    assert norm[first:first + len(want)] == want


# ---- command line (no device) --------------------------------------------------------------------------------------------------

def test_cli_names_the_format():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([CLI, "generate", "-f", "ethereum-contracts", "-p", "^0xdead"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "invalid value 'ethereum-contracts' for '--format'" in r.stderr, r.stderr
    listed = r.stderr.split("(", 1)[1]
    assert "ethereum-contract" in [x.strip(" )\n") for x in listed.split(",")] and "ethereum" in listed and "p2tr" in listed
    # the name is known and the pattern compiles for it: estimate gets as far as asking for a device
    r = subprocess.run([CLI, "estimate", "-f", "ethereum-contract", "-p", "^0xdead"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "no HIP device" in r.stderr and "--format" not in r.stderr, r.stderr
    r = subprocess.run([CLI, "generate", "-f", "ethereum-contract", "-p", "^0x(dead"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "no HIP device" not in r.stderr, r.stderr
    # verify is left as it is: six addresses, no contract line
    r = subprocess.run([CLI, "verify", "-k", "%064x" % 1], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Ethereum address:   0x7E5F4552091A69125d5DfCb7b8C2659029395Bdf" in r.stdout and "ontract" not in r.stdout
