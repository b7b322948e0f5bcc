"""Keys per second of the Ethereum-contract format (VGEN_FMT_ETHEREUM_CONTRACT: a second Keccak block per key) against the
Ethereum format of the same build, in the same run, on one MI355X.

`^0xdead -i` (kind 2: masked test inside seq_bwd_kernel), 2^20 keys per dispatch, 12 frames, a seeded walk.  Sustained legs
(>= --seconds each, two of every kind, alternated): eth (format 5), contract (format 6), then the six-image form of both
(VGEN_FLAG_ENDO).  The yardstick of the new format is NOT a fixed number but the instruction census of this build: expected
ratio = e / (e + b), e = VALU instructions of the per-key loop of seq_bwd_kernel<5> (build/lib/device/kernels.s, the loop
segment that holds the generated Keccak block) and b = the instructions of the second block, keccak_create_block, as
device/hashgen.py generates it (the contract kernels' own loops are laid out differently by the compiler - they only write
payloads -, so their segments do not line up with Ethereum's; the block is what a key costs more).  The filter and compaction
kernels that follow a contract dispatch are NOT in the expectation: they are what the measured ratio loses.  The summary line
prints measured ratio / expected ratio beside the target 0.9.  --formats 5 runs the Ethereum legs alone (the same script on a build without the new format: the +-3 % bar
on format 5's own rate).
usage: python tools/eth_contract_rate.py [--seconds 3] [--formats 5,6] > profiles/rNN_eth_contract_rate.jsonl
"""
import argparse
import collections
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "vgen_amd", "csrc", "device"))

import vgen_amd as vg  # noqa: E402
from oracle import pyoracle as vo  # noqa: E402

BATCH = 1 << 20
FRAMES = 12
ISA = os.path.join(ROOT, "build", "lib", "device", "kernels.s")
NAMES = {5: "eth", 6: "contract"}


def per_key_valu(txt, fmt, endo):
    """VALU instructions of the loop segment of seq_bwd_kernel<fmt, prefilter, endo> that holds the Keccak block(s): the code
    one key (one image, with endo) runs.  Segments are split at loop headers, as tools/isa_census.py does."""
    sym = "_ZN2vg14seq_bwd_kernelILi%dELb0ELb%dELb0ELb0EEEvNS_7SeqArgsE" % (fmt, int(endo))
    lines = txt.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0].split("\n")
    marks = [0] + [i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", l) and "Loop Header" in " ".join(lines[i:i + 3])] + [len(lines)]
    best = None
    for lo, hi in zip(marks, marks[1:]):
        c = collections.Counter()
        for l in lines[lo:hi]:
            m = re.match(r"^\s+(v_\w+)", l)
            if m:
                c[m.group(1)] += 1
        if best is None or c["v_bitop3_b32"] > best["v_bitop3_b32"]:
            best = c
    return {"valu": sum(best.values()), "alignbit": best["v_alignbit_b32"], "bitop3": best["v_bitop3_b32"], "mad_u64": best["v_mad_u64_u32"]}


def sustained(fmt, filt, seconds, endo=False):
    """Round-robin over the frames for `seconds`: dispatch, wait (the ring header only), dispatch again."""
    r = vg.GpuRunner(batch_size=BATCH, fmt=fmt, frames=FRAMES, match_cap=1 << 16, timing=False, endo=endo)
    r.set_filter(filt)
    key = [vo.seed_key(7, 0)]

    def go(f):
        r.dispatch(key[0], f)
        key[0] += BATCH

    for f in range(FRAMES):   # warm-up: every frame's stream and buffers exist
        go(f)
    for f in range(FRAMES):
        r.wait(f)
    t0 = time.perf_counter()
    issued = done = fw = cand = 0
    for f in range(FRAMES):
        go(f)
        issued += 1
    while done < issued:
        n, _ = r.wait(fw)
        cand += n
        done += 1
        if time.perf_counter() - t0 < seconds:
            go(fw)
            issued += 1
        fw = (fw + 1) % FRAMES
    dt = time.perf_counter() - t0
    r.close()
    keys = issued * BATCH * (6 if endo else 1)
    return {"keys": keys, "seconds": round(dt, 3), "mkeys_per_s": round(keys / dt / 1e6, 1), "dispatches": issued,
            "candidates_per_dispatch": round(cand / issued, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--formats", default="5,6")
    a = ap.parse_args()
    fmts = [int(x) for x in a.formats.split(",")]
    filt = {f: vg.Pattern("^0xdead", True, f) for f in fmts}
    census = None
    if os.path.exists(ISA):
        txt = open(ISA).read()
        census = {("endo_" if e else "") + "eth": per_key_valu(txt, 5, e) for e in (False, True)}
        if 6 in fmts:
            import hashgen
            census["keccak_create_block"] = len(hashgen.prog_keccak_create()[0].ins)
    print(json.dumps({"leg": "setup", "device": vg.device_name(0), "pattern": "^0xdead -i", "batch": BATCH, "frames": FRAMES,
                      "kinds": {NAMES[f]: filt[f].device_kind for f in fmts}, "per_key_census": census}), flush=True)
    rates = {}
    for endo in (False, True):
        for rep in range(2):
            for f in fmts:
                name = ("endo_" if endo else "") + NAMES[f]
                res = sustained(f, filt[f], a.seconds, endo)
                rates.setdefault(name, []).append(res["mkeys_per_s"])
                print(json.dumps({"leg": name, "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    out = {"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()}}
    if 5 in fmts and 6 in fmts:
        for pre in ("", "endo_"):
            got = mean[pre + "contract"] / mean[pre + "eth"]
            out[pre + "contract_over_eth"] = round(got, 3)
            if census:
                want = census[pre + "eth"]["valu"] / (census[pre + "eth"]["valu"] + census["keccak_create_block"])
                out[pre + "expected_from_census"] = round(want, 3)
                out[pre + "measured_over_expected"] = round(got / want, 3)
        out["target_measured_over_expected"] = 0.9
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
