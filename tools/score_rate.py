"""Keys (salts) per second of a score search against a prefix search of the same selectivity, same build, same run, same MI355X.

`score:leading:0>=4` (device kind 6) against `^0x0000` (kind 2): both accept exactly the addresses with four leading zero digits, one
candidate in 65 536.  The prefix legs run kernels this build shares with its parent instruction for instruction (seq_bwd_kernel with the
prefilter inline on format 5, create2_kernel<false> on format 7); the score legs run the deferred route on format 5 (seq_bwd_kernel in
dump form into the frame's device-only buffer - 20 B written and 20 B read per key -, then payload_score_kernel) and the fused
create2_score_kernel on format 7; the one-workgroup compaction follows every leg but the format-5 prefix one.
2^20 candidates per dispatch, 12 frames, sustained legs of >= --seconds each, two of every kind, alternated.  None uses the six-image flag.
Nothing is required of the ratios; the summary line records them (DESIGN.md quotes it).
usage: python tools/score_rate.py [--seconds 3] > profiles/rNN_score_rate.jsonl
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
NAMES = {5: "eth", 7: "create2"}
PATTERNS = {"prefix": "^0x0000", "score": "score:leading:0>=4"}


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
            "candidates_per_dispatch": round(cand / issued, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    filt = {(f, k): vg.Pattern(p, False, f) for f in NAMES for k, p in PATTERNS.items()}
    print(json.dumps({"leg": "setup", "device": vg.device_name(0), "patterns": PATTERNS, "batch": BATCH, "frames": FRAMES,
                      "kinds": {NAMES[f] + "_" + k: filt[(f, k)].device_kind for f, k in filt}}), flush=True)
    rates = {}
    for rep in range(2):
        for f in NAMES:
            for k in PATTERNS:
                res = sustained(f, filt[(f, k)], a.seconds)
                rates.setdefault(NAMES[f] + "_" + k, []).append(res["mkeys_per_s"])
                print(json.dumps({"leg": NAMES[f] + "_" + k, "rep": rep, **res}), flush=True)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    print(json.dumps({"leg": "summary", "mkeys_per_s": {k: round(v, 1) for k, v in mean.items()},
                      "eth_score_over_prefix": round(mean["eth_score"] / mean["eth_prefix"], 3),
                      "create2_score_over_prefix": round(mean["create2_score"] / mean["create2_prefix"], 3)}), flush=True)


if __name__ == "__main__":
    main()
