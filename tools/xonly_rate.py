"""Keys per second of the Nostr format (VGEN_FMT_NOSTR: the x-only key is the payload, no hash) against P2PKH of the same build, in
the same run, on one MI355X.

2^20 keys per dispatch, 12 frames, a seeded walk (VGEN_FLAG_ENDO legs: the same walk with the images).  Sustained legs (>= --seconds
each, two of every kind, alternated in one process):
    p2pkh `^1Cat` | nostr `^npub1cat`            prefilter inside seq_bwd_kernel (match_slot) | inside xonly_bwd_kernel (hit mask), then ptab_compact_kernel<8>
    endo_p2pkh | endo_nostr                      the same pair with VGEN_FLAG_ENDO (six images / three images)
    nostr_list                                   a 1 000-line npub prefix list (payload form, ptab_lookup_kernel<8>, ptab_compact_kernel<8>)
    nostr_dfa                                    the unanchored pattern `cat` (payload form, payload_filter8_kernel<FULL>, the compaction)
The yardstick is the instruction census of this build, not a fixed number: VALU instructions per key of the two per-key kernels'
loops behind the product tree's barriers (build/lib/device/kernels.s; the head of the step loop, which serves two keys, counts half),
expected ratio nostr / p2pkh = census(p2pkh) / census(nostr).  What the census leaves out - the fwd / inv head of every dispatch,
the `pre` traffic, the compaction behind every dispatch (and, for lists and automata, 32 B per key written and read back) - is what measured / expected loses.
--formats 0,5 runs the P2PKH and Ethereum legs alone (the same script on a build without the format: the +-3 % bar on their rates).
usage: python tools/xonly_rate.py [--seconds 3] [--formats 0,10] > profiles/rNN_xonly_rate.jsonl
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vgen_amd as vg  # noqa: E402
from oracle import pyoracle as vo  # noqa: E402

BATCH = 1 << 20
FRAMES = 12
ISA = os.path.join(ROOT, "build", "lib", "device", "kernels.s")
SYMS = {"p2pkh": "_ZN2vg14seq_bwd_kernelILi0ELb0ELb0ELb0ELb0EEEvNS_7SeqArgsE", "endo_p2pkh": "_ZN2vg14seq_bwd_kernelILi0ELb0ELb1ELb0ELb0EEEvNS_7SeqArgsE",
        "nostr": "_ZN2vg16xonly_bwd_kernelILb1ELb0EEEvNS_7SeqArgsE", "endo_nostr": "_ZN2vg16xonly_bwd_kernelILb1ELb1EEEvNS_7SeqArgsE",
        "nostr_dump": "_ZN2vg16xonly_bwd_kernelILb0ELb0EEEvNS_7SeqArgsE"}
IMAGES = {0: 6, 5: 6, 10: 3}


def per_key_valu(txt, sym):
    """VALU instructions one key costs in a per-key kernel: the loop segments (split at loop headers, as tools/isa_census.py does)
    behind the last workgroup barrier - the head of the step loop, shared by the +R and -R keys, counted half, the rest in full
    (for an image loop: the cost of a point and its images, not divided)."""
    if ("\n" + sym + ":") not in txt:
        return None
    lines = txt.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0].split("\n")
    marks = [0] + [i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", l) and "Loop Header" in " ".join(lines[i:i + 3])] + [len(lines)]
    segs = [lines[lo:hi] for lo, hi in zip(marks, marks[1:])]
    last_barrier = max(i for i, s in enumerate(segs) if any("s_barrier" in l for l in s))
    valu = [sum(1 for l in s if re.match(r"^\s+v_\w+", l)) for s in segs]
    after = valu[last_barrier + 1:]
    if not after:
        return None
    return {"step_head": after[0], "per_key_rest": sum(after[1:]), "valu_per_key": after[0] // 2 + sum(after[1:])}


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
    keys = issued * BATCH * (IMAGES[fmt] if endo else 1)
    return {"keys": keys, "seconds": round(dt, 3), "mkeys_per_s": round(keys / dt / 1e6, 1), "dispatches": issued,
            "candidates_per_dispatch": round(cand / issued, 1)}


def npub_prefix_list(n):
    """n distinct three-symbol npub prefixes (of 32^3): one key in 32 768 / n is a candidate."""
    cs = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
    return ["^npub1" + cs[(i // 1024) % 32] + cs[(i // 32) % 32] + cs[i % 32] for i in range(0, 32768, 32768 // n)][:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--formats", default="0,10")
    a = ap.parse_args()
    fmts = [int(x) for x in a.formats.split(",")]
    legs = []   # (name, format, filter, endo)
    if 0 in fmts:
        p = vg.Pattern("^1Cat", False, 0)
        legs += [("p2pkh", 0, p, False), ("endo_p2pkh", 0, p, True)]
    if 5 in fmts:
        p5 = vg.Pattern("^0xdead", True, 5)
        legs += [("eth", 5, p5, False), ("endo_eth", 5, p5, True)]
    if 10 in fmts:
        p8, dfa, lst = vg.Pattern("^npub1cat", False, 10), vg.Pattern("cat", False, 10), vg.PatternList(npub_prefix_list(1000), False, 10)
        legs += [("nostr", 10, p8, False), ("endo_nostr", 10, p8, True), ("nostr_list", 10, lst, False), ("nostr_dfa", 10, dfa, False)]
    census = None
    if os.path.exists(ISA):
        txt = open(ISA).read()
        census = {k: per_key_valu(txt, s) for k, s in SYMS.items()}
    print(json.dumps({"leg": "setup", "device": vg.device_name(0), "batch": BATCH, "frames": FRAMES,
                      "kinds": {name: f.device_kind for name, _, f, _ in legs}, "per_key_census": census}), flush=True)
    rates = {}
    for rep in range(2):
        for name, fmt, filt, endo in legs:
            res = sustained(fmt, filt, a.seconds, endo)
            rates.setdefault(name, []).append(res["mkeys_per_s"])
            print(json.dumps({"leg": name, "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    out = {"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()}}
    if 0 in fmts and 10 in fmts:
        for pre in ("", "endo_"):
            got = mean[pre + "nostr"] / mean[pre + "p2pkh"]
            out[pre + "nostr_over_p2pkh"] = round(got, 3)
            # (no expectation for the image legs: their image loops run six and three times per point, which the static count does not see)
            if not pre and census and census.get("nostr") and census.get("p2pkh"):
                want = census["p2pkh"]["valu_per_key"] / census["nostr"]["valu_per_key"]
                out[pre + "expected_from_census"] = round(want, 3)
                out[pre + "measured_over_expected"] = round(got / want, 3)
        out["format_6_measured_over_expected"] = 0.94
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
