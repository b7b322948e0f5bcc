"""Keys per second of the pattern-list path (device kind 5) against a single prefix on one MI355X.

P2PKH, 2^20 keys per dispatch, 12 frames, a seeded walk.  Sustained legs (>= --seconds each, two of every kind, alternated):
  single     ^1Cat alone (kind 1: hash160 range test inside seq_bwd_kernel)
  list1k     1 000 random five-character prefixes as a pattern list (kind 5: dump into the frame's device buffer, then
             ptab_lookup_kernel + ptab_compact_kernel)
  list100k   100 000 such prefixes as a list
then the same 1 000 as ONE alternation through vgen_scan (today's kind-0 path: every payload to the host, a short window),
and on VGEN_FLAG_ENDO contexts (six keys per point) ^1Cat against the 1 000-prefix list.  Prints one JSON object per leg and
a summary line with list1k / single; --short runs one brief leg of each list kind (for a kernel trace under rocprofv3).
usage: python tools/list_rate.py [--seconds 3] [--short] > profiles/rNN_list_rate.jsonl
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vgen_amd as vg  # noqa: E402
from oracle import pyoracle as vo  # noqa: E402

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BATCH = 1 << 20
FRAMES = 12


def prefixes(n, seed):
    rnd = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add("1" + "".join(rnd.choice(B58) for _ in range(4)))
    return sorted(out)


def sustained(filt, seconds, endo=False):
    """Round-robin over the frames for `seconds`: dispatch, wait (the ring header only), dispatch again."""
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.P2pkh, frames=FRAMES, match_cap=1 << 16, timing=False, endo=endo)
    r.set_filter(filt)
    key = [vo.seed_key(7, 0)]

    def go(f):
        r.dispatch(key[0], f)
        key[0] += BATCH

    for f in range(FRAMES):   # warm-up: every frame's stream and buffers exist
        go(f)
    cand = 0
    for f in range(FRAMES):
        cand += r.wait(f)[0]
    t0 = time.perf_counter()
    issued = done = fw = 0
    cand = 0
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
    ap.add_argument("--short", action="store_true", help="one 1 s leg per list kind (kernel trace)")
    a = ap.parse_args()
    p1k, p100k = prefixes(1000, 1000), prefixes(100000, 100)
    single = vg.Pattern("^1Cat", False, vg.AddressFormat.P2pkh)
    t = time.perf_counter()
    l1k = vg.PatternList(["^" + p for p in p1k])
    t1k = time.perf_counter() - t
    t = time.perf_counter()
    l100k = vg.PatternList(["^" + p for p in p100k])
    t100k = time.perf_counter() - t
    print(json.dumps({"leg": "compile", "list1k_s": round(t1k, 3), "list100k_s": round(t100k, 3),
                      "kinds": {"single": single.device_kind, "list1k": l1k.device_kind, "list100k": l100k.device_kind}}), flush=True)
    if a.short:
        for name, f in (("list1k", l1k), ("list100k", l100k)):
            print(json.dumps({"leg": name, **sustained(f, 1.0)}), flush=True)
        return
    rates = {}
    for rep in range(2):
        for name, f in (("single", single), ("list1k", l1k), ("list100k", l100k)):
            res = sustained(f, a.seconds)
            rates.setdefault(name, []).append(res["mkeys_per_s"])
            print(json.dumps({"leg": name, "rep": rep, **res}), flush=True)
    # the same 1 000 prefixes as one alternation: kind 0, every payload to the host (vgen_scan's own loop)
    alt = "^(" + "|".join(p1k) + ")"
    r = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.P2pkh, frames=FRAMES, timing=False)
    res = vg.scan_gpu_with_runner(alt, vg.ScanConfig(format=vg.AddressFormat.P2pkh, count=None, seed=7, max_batches=24), r)
    r.close()
    rates["alternation_kind0"] = [round(res.operations / res.elapsed_secs / 1e6, 1)]
    print(json.dumps({"leg": "alternation_kind0", "kind": vg.Pattern(alt).device_kind, "keys": res.operations,
                      "seconds": round(res.elapsed_secs, 3), "mkeys_per_s": rates["alternation_kind0"][0],
                      "matches": len(res.matches)}), flush=True)
    for rep in range(2):
        for name, f in (("endo_single", single), ("endo_list1k", l1k)):
            res = sustained(f, a.seconds, endo=True)
            rates.setdefault(name, []).append(res["mkeys_per_s"])
            print(json.dumps({"leg": name, "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    print(json.dumps({"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()},
                      "list1k_over_single": round(mean["list1k"] / mean["single"], 3),
                      "list100k_over_single": round(mean["list100k"] / mean["single"], 3),
                      "endo_list1k_over_endo_single": round(mean["endo_list1k"] / mean["endo_single"], 3),
                      "target_list1k_over_single": 0.8}), flush=True)


if __name__ == "__main__":
    main()
