"""Pattern lists (vgen_filter_compile_list, device kind 5) on the host: the interval table is a superset of every pattern, the
attribution (vgen_filter_which) equals brute force over single-pattern filters, what a list refuses is refused with its line
number, and a 100 000-pattern list compiles and answers like str.startswith.  No GPU needed."""
import os
import random
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgen_amd", "csrc")
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BECH32 = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
HEX = "0123456789abcdef"

HARNESS = r"""
// Pattern-list lookup harness (tests/test_pattern_list.py): compiles a list, then, for payloads at every interval edge
// (lo - 1, lo, hi, hi + 1 in the top 64 bits) and random ones, checks
//   (a) through core/ptab_eval.h (the kernel's lookup): every pattern whose own automaton accepts the address is named by
//       the interval the payload falls in — the table is a superset;
//   (b) vg::filter_which == the patterns whose single-pattern filter (vg::filter_compile) accepts the address.
// usage: ptab_harness FORMAT CI SEED < list   -> prints "ok <checked> <hits>" or the first disagreement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "core/ptab_eval.h"
#include "host/encode.h"
#include "host/filter.h"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const uint32_t fmt = (uint32_t)atoi(argv[1]);
    const bool ci = atoi(argv[2]) != 0;
    std::mt19937_64 rng((uint64_t)atoll(argv[3]));
    std::string text((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
    vgen_filter list;
    std::string err;
    if (!vg::filter_compile_list(text, ci, fmt, list, err)) {
        printf("compile failed: %s\n", err.c_str());
        return 1;
    }
    const vg::PatternList &L = *list.list;
    std::vector<vgen_filter> single(L.patterns.size());
    for (size_t i = 0; i < L.patterns.size(); i++)
        if (!vg::filter_compile(L.patterns[i], ci, fmt, single[i], err)) {
            printf("single compile failed: %s\n", err.c_str());
            return 1;
        }
    const size_t plen = fmt == 3 ? 32 : 20;
    std::vector<uint64_t> xs;
    for (size_t j = 0; j < L.lo.size(); j++) {
        xs.push_back(L.lo[j] - 1);
        xs.push_back(L.lo[j]);
        xs.push_back(L.hi[j]);
        xs.push_back(L.hi[j] + 1);
    }
    for (int i = 0; i < 20000; i++) xs.push_back(rng());
    const vg::DevPtab view = L.view();
    size_t checked = 0, hits = 0;
    for (uint64_t x : xs) {
        for (int rep = 0; rep < 2; rep++) {
            uint8_t p[32];
            for (size_t k = 0; k < plen; k++) p[k] = (uint8_t)rng();
            for (int k = 0; k < 8; k++) p[k] = (uint8_t)(x >> (56 - 8 * k));
            const std::string addr = vg::address_from_payload(fmt, p);
            std::vector<uint32_t> want, got;
            for (uint32_t i = 0; i < single.size(); i++)
                if (single[i].dfa.is_match(addr)) want.push_back(i);
            uint32_t w[2];
            memcpy(w, p, 8);
            const int j = vg::ptab_find(view, vg::ptab_top64(w));
            for (uint32_t i : want) {
                bool named = false;
                for (uint32_t k = j < 0 ? 0 : L.pat_off[j]; j >= 0 && k < L.pat_off[j + 1]; k++) named = named || L.pat_idx[k] == i;
                if (!named) {
                    printf("superset broken: %s satisfies pattern %u (%s), interval %d does not name it\n", addr.c_str(), i, L.patterns[i].c_str(), j);
                    return 1;
                }
            }
            vg::filter_which(list, addr, nullptr, got);
            if (got != want) {
                printf("which differs on %s: %zu vs %zu patterns\n", addr.c_str(), got.size(), want.size());
                return 1;
            }
            checked++;
            hits += want.empty() ? 0 : 1;
        }
    }
    printf("ok %zu %zu\n", checked, hits);
    return 0;
}

"""


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    return vgen_amd


@pytest.fixture(scope="module")
def vo():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The lookup of core/ptab_eval.h (the header the list kernel compiles) built with g++ beside the host sources."""
    d = tmp_path_factory.mktemp("ptab")
    src = d / "ptab_harness.cpp"
    src.write_text(HARNESS)
    exe = d / "ptab_harness"
    host = [os.path.join(CSRC, "host", f) for f in ("filter.cpp", "regex_dfa.cpp", "encode.cpp", "host_ec.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           str(src), *host, "-o", str(exe), "-lpthread"])
    return str(exe)


def lists(seed):
    """Per format: (format, case_insensitive, list text) with short prefixes (frequent hits), a long one and classes."""
    rnd = random.Random(seed)
    out = []
    p2pkh = ["^1" + "".join(rnd.choice(B58) for _ in range(rnd.choice((1, 2)))) for _ in range(30)] + ["^1Cat", "^1[AB]x", "^11"]
    out.append((0, False, p2pkh))
    out.append((0, True, ["^1cat", "^1dog", "^1a", "^1Zz"]))
    out.append((4, False, ["^1" + rnd.choice(B58) + rnd.choice(B58) for _ in range(20)]))
    # (P2SH addresses are 3 + [2-9A-Q]...: the version byte 5 bounds the second character)
    out.append((2, False, ["^3" + rnd.choice("23456789ABCDEFGHJKLMNPQ") + "".join(rnd.choice(B58) for _ in range(rnd.choice((0, 1)))) for _ in range(30)]))
    out.append((1, False, ["^bc1q" + "".join(rnd.choice(BECH32) for _ in range(rnd.choice((1, 2, 3)))) for _ in range(30)] + ["^bc1q[02]"]))
    out.append((3, False, ["^bc1p" + "".join(rnd.choice(BECH32) for _ in range(rnd.choice((1, 2)))) for _ in range(30)]))
    out.append((5, False, ["^0x" + "".join(rnd.choice(HEX + "ABCDEF") for _ in range(rnd.choice((1, 2)))) for _ in range(30)] + ["^0xAb", "^0xab"]))
    out.append((5, True, ["^0xDE", "^0x0", "^0xbeef"]))
    return [(f, ci, list(dict.fromkeys(p))) for f, ci, p in out]


@pytest.mark.parametrize("case", range(8))
def test_lookup_is_a_superset_and_which_is_brute_force_at_every_interval_edge(harness, case):
    fmt, ci, pats = lists(11)[case]
    r = subprocess.run([harness, str(fmt), str(int(ci)), "5"], input="\n".join(pats), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    _, checked, hits = r.stdout.split()
    assert int(checked) > 40000 and int(hits) > 100, r.stdout


@pytest.mark.parametrize("case", range(8))
def test_which_equals_brute_force_on_oracle_addresses(vg, vo, case):
    fmt, ci, pats = lists(12)[case]
    plist = vg.PatternList(pats, case_insensitive=ci, fmt=vg.AddressFormat(fmt))
    assert len(plist) == len(pats) and plist.device_kind == 5
    singles = [vg.Pattern(p, ci, vg.AddressFormat(fmt)) for p in pats]
    hits = 0
    for k in range(1, 400):
        a = vo.generate(fmt, vo.seed_key(3, 0) + k * 7919)["address"]
        want = [i for i, s in enumerate(singles) if s.matches(a)]
        assert plist.which(a) == want, (a, want)
        assert plist.matches(a) == bool(want)
        hits += bool(want)
    assert hits > 0
    assert [plist.pattern(i) for i in range(len(plist))] == pats


def test_which_on_strings_that_are_not_addresses(vg):
    plist = vg.PatternList(["^1A", "^1B"])
    assert plist.which("1A") == [] and plist.which("1AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA") == []
    assert plist.which("bc1qqqqq") == [] and plist.which("") == []
    single = vg.Pattern("^1A")
    import ctypes
    from vgen_amd import api
    arr, n = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
    assert api._L.vgen_filter_which(single._h, b"1Abc", arr, 4, ctypes.byref(n)) == 0 and n.value == 1 and arr[0] == 0
    assert api._L.vgen_filter_which(single._h, b"1Bbc", arr, 4, ctypes.byref(n)) == 0 and n.value == 0


REJECT = [
    (0, "^1A\n1[Oo]ri\n", 2, "start-anchored prefix"),            # unanchored
    (0, "^1A\n\n# names\nabc$\n", 4, "start-anchored prefix"),     # suffix
    (0, "^1Cat.*z$\n", 1, "start-anchored prefix"),                # a trailing symbol
    (1, "^bc1qq\r\n^bc1q.{37}qq\r\n", 2, "start-anchored prefix"), # the checksum
    (0, "^1A\n^1\n", 2, "every address"),                          # every address
    (5, "^0x\n", 1, "every address"),
    (0, "^1A\n^1B\n^1A\n", 3, "duplicate of line 1"),
    (2, "^1A\n", 1, "no address"),                                 # P2SH addresses start with 3
    (0, "^1A\n^1[\n", 2, ""),                                      # invalid syntax
]


@pytest.mark.parametrize("fmt,text,line,why", REJECT)
def test_rejections_name_the_line(vg, fmt, text, line, why):
    with pytest.raises(vg.VgenError) as e:
        vg.PatternList(text, fmt=vg.AddressFormat(fmt))
    msg = str(e.value)
    assert f"line {line}:" in msg and why in msg, msg


def test_an_empty_list_is_refused(vg):
    for text in ("", "\n\n", "# only a comment\n\r\n"):
        with pytest.raises(vg.VgenError) as e:
            vg.PatternList(text)
        assert "empty" in str(e.value)


def test_comment_and_empty_lines_count_for_line_numbers_not_indices(vg):
    plist = vg.PatternList("# header\r\n\r\n^1A\n\n^1B\n")
    assert len(plist) == 2 and plist.pattern(0) == "^1A" and plist.pattern(1) == "^1B"


def test_a_hundred_thousand_prefixes(vg, vo):
    """100 000 random five-character P2PKH prefixes: compile time and the attribution of 10^5 oracle-encoded addresses
    against str.startswith."""
    rnd = random.Random(100)
    pats = set()
    while len(pats) < 100000:
        pats.add("1" + "".join(rnd.choice(B58) for _ in range(4)))
    pats = sorted(pats)
    t0 = time.time()
    plist = vg.PatternList(["^" + p for p in pats])
    secs = time.time() - t0
    assert len(plist) == 100000 and secs < 30, secs
    index = {p: i for i, p in enumerate(pats)}
    seen = 0
    for _ in range(100000):
        a = vo.address_from_hash160(vo.FMT_P2PKH, rnd.getrandbits(160).to_bytes(20, "big"))
        want = [index[a[:5]]] if a[:5] in index else []
        assert plist.which(a) == want, a
        seen += bool(want)
    assert seen > 100


CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")


@pytest.mark.parametrize("text,line,why", [
    ("^1A\n1[Oo]ri\n", 2, "start-anchored prefix"),
    ("^1A\n# provider\nboha:b1000:66\n", 3, "provider patterns"),
    ("^1A\n^1A\n", 2, "duplicate of line 1"),
    ("^1A\n^1\n", 2, "every address"),
    ("# nothing\n", None, "empty"),
])
@pytest.mark.parametrize("cmd", [["generate"], ["range", "--puzzle", "20"]])
def test_cli_refuses_a_bad_patterns_file_before_any_device(tmp_path, text, line, why, cmd):
    f = tmp_path / "names.txt"
    f.write_text(text)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")   # the list is checked before a device is asked for
    r = subprocess.run([CLI, *cmd, "--patterns-file", str(f)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1, r.stderr
    assert why in r.stderr and (line is None or f"line {line}:" in r.stderr), r.stderr


def test_cli_patterns_file_and_pattern_are_exclusive(tmp_path):
    f = tmp_path / "names.txt"
    f.write_text("^1A\n")
    r = subprocess.run([CLI, "generate", "--patterns-file", str(f), "-p", "^1B"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot be used with '--pattern'" in r.stderr, r.stderr
