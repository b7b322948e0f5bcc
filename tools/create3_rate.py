"""Salts per second of the three salt kernels of the ethereum-create2 format on one MI355X, by the frames' kernel timers: CREATE2
(one Keccak block per salt), a CREATE3 job without a guard (two blocks, one after another) and one with a 20-byte guard (three).

`^0xdead` (device kind 2: the prefilter inline, then the one-workgroup compaction), 2^20 salts per dispatch, one dispatch in flight
at a time on a context created with VGEN_FLAG_TIMING; a sample is 2^20 / vgen_frame_kernel_ms of one dispatch.  Every leg runs in
a fresh child process - so that CREATE2 can also be measured with the library of another build of the project, --parent TREE, the
root of a built checkout of the commit to compare against - with --warmup dispatches that are not recorded and --samples that
are; the legs are alternated --reps times.  The summary line gives the median rate per leg and the two CREATE3 rates over
CREATE2's (by instruction count about 1/2 and 1/3), and CREATE2 of this build over the parent's (its kernels are untouched: 1.0
within the spread of the repetitions).
usage: python tools/create3_rate.py [--parent TREE] [--samples 40] [--reps 3] > profiles/rNN_create3_rate.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 1 << 20
PATTERN = "^0xdead"
FACTORY, HASH, PREFIX, GUARD = bytes(range(1, 21)), bytes(range(32, 64)), bytes(range(128, 152)), bytes(range(160, 180))


def leg(kind, tree, warmup, samples):
    """One leg in this (child) process, with the package of `tree`: the kernel milliseconds of `samples` dispatches."""
    sys.path.insert(0, tree)
    import vgen_amd as vg
    fmt = vg.AddressFormat(7)
    r = vg.GpuRunner(batch_size=BATCH, fmt=fmt, frames=2, match_cap=1 << 16, timing=True)
    if kind == "create2":
        r.set_create2(vg.Create2Job(FACTORY, init_code_hash=HASH, salt_prefix=PREFIX))
    else:
        r.set_create3(vg.Create3Job(FACTORY, HASH, PREFIX, GUARD if kind == "create3_guarded" else None))
    r.set_filter(vg.Pattern(PATTERN, False, 7))
    ms, cand = [], 0
    for k in range(warmup + samples):
        frame = k % 2
        r.dispatch_create2(k * BATCH, frame)
        n, _ = r.wait(frame)
        if k >= warmup:
            ms.append(r.kernel_ms(frame))
            cand += n
    r.close()
    print(json.dumps({"kernel_ms": [round(x, 4) for x in ms], "candidates_per_dispatch": round(cand / samples, 1), "device": vg.device_name(0),
                      "library": os.path.relpath(vg.library_path(), tree)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="root of a built checkout of the commit to compare CREATE2 against")
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, os.path.abspath(a.tree), a.warmup, a.samples)
    legs = ([("create2_parent", "create2", os.path.abspath(a.parent))] if a.parent else []) + \
        [("create2", "create2", ROOT), ("create3", "create3", ROOT), ("create3_guarded", "create3_guarded", ROOT)]
    print(json.dumps({"leg": "setup", "pattern": PATTERN, "batch": BATCH, "samples": a.samples, "warmup": a.warmup, "reps": a.reps,
                      "guard_bytes": len(GUARD), "timer": "vgen_frame_kernel_ms, one dispatch in flight"}), flush=True)
    rates = {}
    for rep in range(a.reps):
        for name, kind, tree in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--tree", tree, "--samples", str(a.samples), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.stderr.write(out.stderr)
                raise SystemExit("leg %s failed with status %d" % (name, out.returncode))
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            med = statistics.median(rec["kernel_ms"])
            rate = BATCH / med / 1e3      # salts per millisecond / 1e3 = Msalts/s
            rates.setdefault(name, []).append(rate)
            print(json.dumps({"leg": name, "rep": rep, "median_kernel_ms": round(med, 4), "msalts_per_s": round(rate, 1), **rec}), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    out = {"leg": "summary", "msalts_per_s": {k: round(v, 1) for k, v in med.items()},
           "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in rates.items()},
           "create3_over_create2": round(med["create3"] / med["create2"], 3), "create3_guarded_over_create2": round(med["create3_guarded"] / med["create2"], 3),
           "expected_by_instruction_count": [0.5, 0.333]}
    if "create2_parent" in med:
        out["create2_over_parent"] = round(med["create2"] / med["create2_parent"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
