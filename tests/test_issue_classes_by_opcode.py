"""`tools/issue_classes.py --by-opcode`: the class X and class C instructions of the headline kernel's key loop outside the generated hash
block, by opcode (no GPU needed: the assembly of this build).  The table must add up with the census `bench.py` prices the steady state
against, and the census must hold what the key loop was trimmed to: at most 494 exclusive and 1 291 half-rate instructions per key."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "issue_classes.py")


def table():
    out, cls = {}, None
    for line in subprocess.check_output([sys.executable, TOOL, "--by-opcode"], text=True).splitlines():
        if line.startswith("class "):
            cls = line.split()[1]
            out[cls] = {}
        elif line.strip():
            op, n = line.split()
            out[cls][op] = float(n)
    return out


def test_the_table_adds_up_with_the_census():
    t = table()
    census = json.loads(subprocess.check_output([sys.executable, TOOL]))["per_key"]
    # the hash block has no exclusive instruction: all of class X is outside it
    assert sum(t["X"].values()) == census["exclusive_X"]
    # the block's half-rate instructions are its 868 funnel shifts, 370 three-input adds and 8 byte permutations (tests/test_hashgen.py)
    assert sum(t["C"].values()) == census["half_rate_C"] - (868 + 370 + 8)


def test_what_the_key_loop_was_trimmed_to():
    t = table()
    census = json.loads(subprocess.check_output([sys.executable, TOOL]))["per_key"]
    assert census["exclusive_X"] <= 494 and census["half_rate_C"] <= 1291
    # four products per key (two per pair of keys, lambda, the squaring and y3's): 3 x 115 + 79 multiply-adds, none for the addends
    assert t["X"]["v_mad_u64_u32"] <= 3 * 115 + 79
    # the squaring doubles its limbs at full rate: one left shift left (the ninth word of the key)
    assert t["C"].get("v_lshlrev_b32", 0) <= 1
