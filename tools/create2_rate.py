"""Salts per second of the CREATE2 format (VGEN_FMT_ETHEREUM_CREATE2: one Keccak block per candidate, no curve arithmetic)
against what the two older Ethereum formats of the same build, in the same run on the same MI355X, say a Keccak block costs.

`^0xdead` (kind 2) everywhere, 2^20 candidates per dispatch, 12 frames, sustained legs of >= --seconds each, two of every kind,
alternated: eth (format 5, seeded walk), contract (format 6: the same walk and one more Keccak block per key), create2 (format 7:
create2_kernel<false> with the prefilter inline, then the one-workgroup compaction).  None uses the six-image flag.

The yardstick is the single-block rate the first two imply, 1 / (1 / R_contract - 1 / R_eth): what the engine pays per key for
one more generated Keccak block inside its per-key kernel.  The target for R_create2 is 0.8 of it (the margin is the hit-mask
compaction, one workgroup per dispatch); the summary line records the ratio.  It also records Ethereum's rate against the one
committed for the parent build in profiles/r07_eth_contract_rate.jsonl (another run: a plausibility check, not an A/B).
usage: python tools/create2_rate.py [--seconds 3] > profiles/rNN_create2_rate.jsonl
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
NAMES = {5: "eth", 6: "contract", 7: "create2"}
PARENT_RECORD = os.path.join(ROOT, "profiles", "r07_eth_contract_rate.jsonl")


def sustained(fmt, filt, seconds):
    """Round-robin over the frames for `seconds`: dispatch, wait (the ring header only), dispatch again."""
    r = vg.GpuRunner(batch_size=BATCH, fmt=fmt, frames=FRAMES, match_cap=1 << 16, timing=False)
    if fmt == 7:
        r.set_create2(vg.Create2Job(bytes(range(1, 21)), init_code_hash=bytes(range(32, 64)), salt_prefix=bytes(range(128, 152))))
    r.set_filter(filt)
    pos = [vo.seed_key(7, 0) if fmt != 7 else 0]

    def go(f):
        if fmt == 7:
            r.dispatch_create2(pos[0], f)
        else:
            r.dispatch(pos[0], f)
        pos[0] += BATCH

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
    keys = issued * BATCH
    return {"keys": keys, "seconds": round(dt, 3), "mkeys_per_s": round(keys / dt / 1e6, 1), "dispatches": issued,
            "candidates_per_dispatch": round(cand / issued, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    fmts = (5, 6, 7)
    filt = {f: vg.Pattern("^0xdead", False, f) for f in fmts}
    print(json.dumps({"leg": "setup", "device": vg.device_name(0), "pattern": "^0xdead", "batch": BATCH, "frames": FRAMES,
                      "kinds": {NAMES[f]: filt[f].device_kind for f in fmts}}), flush=True)
    rates = {}
    for rep in range(2):
        for f in fmts:
            res = sustained(f, filt[f], a.seconds)
            rates.setdefault(NAMES[f], []).append(res["mkeys_per_s"])
            print(json.dumps({"leg": NAMES[f], "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    block = 1.0 / (1.0 / mean["contract"] - 1.0 / mean["eth"])
    out = {"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()}, "single_block_yardstick_mkeys_per_s": round(block, 1),
           "create2_over_yardstick": round(mean["create2"] / block, 3), "target": 0.8}
    if os.path.exists(PARENT_RECORD):
        for line in open(PARENT_RECORD):
            rec = json.loads(line)
            if rec.get("leg") == "summary":
                out["eth_parent_record_mkeys_per_s"] = rec["mkeys_per_s"]["eth"]
                out["eth_over_parent_record"] = round(mean["eth"] / rec["mkeys_per_s"]["eth"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
