"""Keys per second of a split-key search (a runner with a base point, vgen_set_base_point) against the same search without a base,
in the same run, on one MI355X.

2^20 keys per dispatch, 12 frames.  Sustained legs (>= --seconds each, two of every kind, alternated in one process on one device):
    walk | walk_base              P2PKH `^1Cat`, the seeded sequential walk, without and with a base
    endo_walk | endo_walk_base    the same pair with VGEN_FLAG_ENDO (six images per point)
    random | random_base          P2PKH `^1Cat`, independent random keys (vgen_dispatch_random), without and with a base
The yardstick is the no-base leg of the SAME run.  The walked kernels are instruction-identical (the host folds the base into the
per-dispatch uniform points): anything beyond the spread of the repeated legs is host cost and wants explaining.  The random-key
path runs keys_fwd_base_kernel in keys_fwd_kernel's place: one complete mixed addition on top of a multiplication of about 21 300
instructions - a fraction of a percent is what to expect.
usage: python tools/splitkey_rate.py [--seconds 3] > profiles/rNN_splitkey_rate.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vgen_amd as vg  # noqa: E402
from oracle import pyoracle as vo  # noqa: E402

BATCH = 1 << 20
FRAMES = 12
SECRET = 0x51C2E7 << 216 | 0xA11CE


def sustained(filt, seconds, endo, random_keys, base):
    """Round-robin over the frames for `seconds`: dispatch, wait (the ring header only), dispatch again."""
    r = vg.GpuRunner(batch_size=BATCH, fmt=0, frames=FRAMES, match_cap=1 << 16, timing=False, endo=endo)
    if base:
        r.set_base(vo.pubkey(SECRET))
    r.set_filter(filt)
    key, index = [vo.seed_key(7, 0)], [0]

    def go(f):
        if random_keys:
            r.dispatch_random(7, 0, index[0], f)
            index[0] += BATCH
        else:
            r.dispatch(key[0], f)
            key[0] += BATCH

    for _ in range(2 if random_keys else 1):   # warm-up: every frame's stream and buffers exist (random keys: the generator table too)
        for f in range(FRAMES):
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
    table_bits = r.resources()["table_bits"]   # (the random-key legs: the generator table they ran on)
    r.close()
    keys = issued * BATCH * (6 if endo else 1)
    return {"keys": keys, "seconds": round(dt, 3), "mkeys_per_s": round(keys / dt / 1e6, 1), "dispatches": issued,
            "candidates_per_dispatch": round(cand / issued, 1), "table_bits": table_bits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    p = vg.Pattern("^1Cat", False, 0)
    legs = []   # (name, endo, random keys, base)
    for name, endo, rnd in (("walk", False, False), ("endo_walk", True, False), ("random", False, True)):
        legs += [(name, endo, rnd, False), (name + "_base", endo, rnd, True)]
    print(json.dumps({"leg": "setup", "device": vg.device_name(0), "batch": BATCH, "frames": FRAMES, "pattern": "^1Cat", "format": "p2pkh"}), flush=True)
    rates = {}
    for rep in range(2):
        for name, endo, rnd, base in legs:
            res = sustained(p, a.seconds, endo, rnd, base)
            rates.setdefault(name, []).append(res["mkeys_per_s"])
            print(json.dumps({"leg": name, "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    out = {"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()},
           "spread_of_repeats": {k: round(abs(v[0] - v[1]) / max(v), 4) for k, v in rates.items()}}
    for name in ("walk", "endo_walk", "random"):
        out[name + "_base_over_plain"] = round(mean[name + "_base"] / mean[name], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
