"""Keys per second of the onion format (format 13: the Ed25519 walk, a handful of field products per key) beside Solana (`^So1`: SHA-512
and a fixed-base multiplication per candidate) and Nostr (`^npub1cat`: the secp256k1 walk, hash-free) in the same run, and the static
VALU count per key of the walk's kernels.  2^20 keys per dispatch, 12 frames, one device, legs of at least 3 s, two of each kind
alternated, every leg in a child process of its own (one context per process, as a search has).
Condition (the issue's): measured(onion) / measured(Solana) >= 0.5 x (51 808 / onion's count), 51 808 being Solana's static count
(tools/solana_rate.py --static-only).
usage: python tools/onion_rate.py [--seconds 3] > profiles/r14_onion_rate.jsonl
       python tools/onion_rate.py --static-only [--rates ONION,SOLANA] >> profiles/r14_onion_rate.jsonl   (no GPU: the count per key from
       the build's assembly, and the ratio of the counts beside the ratio of the measured rates)"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, FRAMES = 1 << 20, 12
ONION_S = 32                                     # device_types.h: keys per lane and sign
SOLANA_VALU_PER_CANDIDATE = 51808                # profiles/r12_solana_rate.jsonl
SQR_TRIPS = [2, 5, 10, 20, 10, 50, 100, 50, 5]   # fe25_inv's runs of squarings (core/fe25519.h), in program order


def leg(r, dispatch, pattern, fmt, seconds):
    """Keeps every frame in flight for `seconds`; -> (keys per second, candidates reported)."""
    r.set_filter(vg.Pattern(pattern, False, fmt))
    nxt = 0
    for f in range(FRAMES):
        dispatch(r, nxt, f)
        nxt += 1
    for f in range(FRAMES):   # (warm-up: the first round creates the streams)
        r.wait(f)
        dispatch(r, nxt, f)
        nxt += 1
    done = found = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for f in range(FRAMES):
            n, tested = r.wait(f)
            done += tested
            found += n
            dispatch(r, nxt, f)
            nxt += 1
    dt = time.perf_counter() - t0
    for f in range(FRAMES):
        r.wait(f)
    return done / dt, found


def valu(lines):
    return sum(1 for l in lines if re.match(r"\s+v_", l))


def kernel_body(txt, symbol_part):
    sym = next(s for s in re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M) if symbol_part in s)
    return txt.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0].split("\n")


def back_branches(body):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    out = []
    for i, l in enumerate(body):
        m = re.match(r"\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(2), i) < i:
            out.append((labels[m.group(2)], i))
    return out


def static_count():
    """VALU instructions per key of one dispatch, from the build's assembly.  A lane of onion_fwd_kernel / onion_bwd_kernel<filter> runs
    its main loop ONION_S times for 2 ONION_S keys; the forward kernel's section between its two barriers (the inversion, with its nine
    squaring loops at their trip counts) is executed by one wave of the workgroup's eight.  The backward kernel's loop is counted up to
    its first branch back to the head - the path of a pair without a hit; the code behind it (x for hit lanes, the payload stores) runs
    for about one pair in 32^k and is reported beside the count, not in it.  The filter's loop over tests counts one trip.
    onion_points_kernel runs 32 lanes a dispatch: its share per key is reported and included."""
    txt = open(os.path.join(ROOT, "build", "lib", "device", "kernels.s")).read()
    fwd = kernel_body(txt, "onion_fwd_kernel")
    barriers = [i for i, l in enumerate(fwd) if re.match(r"\s+s_barrier", l)]
    assert len(barriers) == 2, barriers
    bb = back_branches(fwd)
    head = min(a for a, b in bb if b < barriers[0])
    end = max(b for a, b in bb if a == head)
    sqr = [(a, b) for a, b in bb if barriers[0] < a and b < barriers[1]]
    assert len(sqr) == len(SQR_TRIPS) and len({valu(fwd[a:b]) for a, b in sqr}) == 1, sqr
    inv_wave = valu(fwd[barriers[0]:barriers[1]]) + sum((t - 1) * valu(fwd[a:b]) for t, (a, b) in zip(SQR_TRIPS, sqr))
    fwd_loop = valu(fwd[head:end])
    fwd_rest = valu(fwd[:head]) + valu(fwd[end:barriers[0]]) + valu(fwd[barriers[1]:])
    fwd_lane = fwd_rest + ONION_S * fwd_loop + inv_wave / 8
    bwd = kernel_body(txt, "onion_bwd_kernelILb0")
    bb = back_branches(bwd)
    head = min(a for a, b in bb)
    first_back = min(b for a, b in bb if a == head)
    last_back = max(b for a, b in bb if a == head)
    bwd_loop, bwd_hit = valu(bwd[head:first_back]), valu(bwd[first_back:last_back])
    bwd_rest = valu(bwd[:head]) + valu(bwd[last_back:])
    bwd_lane = bwd_rest + ONION_S * bwd_loop
    pts = kernel_body(txt, "onion_points_kernel")
    bb = back_branches(pts)
    window = [(a, b) for a, b in bb if any("global_load" in l for l in pts[a:b])]
    assert len(window) == 1, window
    psq = [(a, b) for a, b in bb if (a, b) != window[0]]
    assert len(psq) == len(SQR_TRIPS), psq
    pts_lane = valu(pts) + 31 * valu(pts[window[0][0]:window[0][1]]) + sum((t - 1) * valu(pts[a:b]) for t, (a, b) in zip(SQR_TRIPS, psq))
    pts_share = pts_lane * 64 / BATCH            # one wave a dispatch, whatever its 32 live lanes
    per_key = (fwd_lane + bwd_lane) / (2 * ONION_S) + pts_share
    return {"valu_per_key": round(per_key, 1), "fwd_loop_per_pair": fwd_loop, "bwd_loop_per_pair_no_hit": bwd_loop, "bwd_hit_path_per_pair": bwd_hit,
            "fwd_outside_loop_per_lane": fwd_rest, "bwd_outside_loop_per_lane": bwd_rest, "inverting_wave_valu": inv_wave,
            "inversion_share_per_key": round(inv_wave / 8 / (2 * ONION_S), 1), "points_kernel_share_per_key": round(pts_share, 2),
            "keys_per_lane": 2 * ONION_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--leg", default="", help="(internal) run one leg in this process: onion, solana, nostr or timers")
    ap.add_argument("--rates", default="", help="--static-only: the measured rates ONION,SOLANA (keys/s) to set the count ratio against")
    a = ap.parse_args()
    if a.static_only:
        rec = {"static": True, **static_count(), "solana_valu_per_candidate": SOLANA_VALU_PER_CANDIDATE}
        rec["count_ratio_expected_rate_ratio"] = SOLANA_VALU_PER_CANDIDATE / rec["valu_per_key"]
        rec["condition_rate_ratio_at_least"] = 0.5 * rec["count_ratio_expected_rate_ratio"]
        if a.rates:
            on, sol = (float(x) for x in a.rates.split(","))
            rec["rate_ratio"] = on / sol
            rec["measured_over_expected"] = rec["rate_ratio"] / rec["count_ratio_expected_rate_ratio"]
            rec["condition_met"] = rec["rate_ratio"] >= rec["condition_rate_ratio_at_least"]
        print(json.dumps(rec), flush=True)
        return
    global vg
    if not a.leg:
        # every leg in a process of its own, alternated twice: a process that holds several contexts spreads their streams over the same
        # twelve hardware queues, and which frames then share a queue depends on how many streams exist (measured: 15.0 against 9.4 Gkeys/s
        # for this leg, either way round) - a leg has the device's queues to itself, as a search has
        import subprocess
        rates = {"onion": [], "solana": [], "nostr": []}
        for rep in range(2):
            for name in rates:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--seconds", str(a.seconds)], capture_output=True, text=True,
                                     timeout=120)
                if out.returncode != 0:
                    sys.exit("leg %s failed: %s" % (name, out.stderr[-2000:]))
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                rec["rep"] = rep
                rates[name].append(rec["keys_per_s"])
                print(json.dumps(rec), flush=True)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "timers"], capture_output=True, text=True, timeout=120)
        if out.returncode != 0:
            sys.exit("timers failed: %s" % out.stderr[-2000:])
        sys.stdout.write(out.stdout)
        m = {k: sum(v) / len(v) for k, v in rates.items()}
        print(json.dumps({"summary": True, "onion_keys_per_s": m["onion"], "solana_keys_per_s": m["solana"], "nostr_keys_per_s": m["nostr"],
                          "onion_over_solana": m["onion"] / m["solana"], "onion_over_nostr": m["onion"] / m["nostr"]}), flush=True)
        return
    import vgen_amd as vg
    base = int.from_bytes(vg.onion_base(20261021, 0), "little")
    key0 = 0x1234567 << 200
    if a.leg == "timers":
        # where a dispatch's time goes: the frames' event timers, alone (1 frame in flight) and in the full pipeline
        t = vg.GpuRunner(batch_size=BATCH, fmt=vg.FORMAT_ONION, device=0, frames=FRAMES, timing=True)
        t.set_filter(vg.Pattern("^cat", False, vg.FORMAT_ONION))
        for depth in (1, FRAMES):
            tot, back = [], []
            for rnd in range(6):
                for f in range(depth):
                    t.dispatch_onion(base, (rnd * depth + f) * BATCH, f)
                for f in range(depth):
                    t.wait(f)
                    if rnd >= 2:
                        tot.append(t.dispatch_ms(f))
                        back.append(t.kernel_ms(f))
            print(json.dumps({"timers": True, "frames_in_flight": depth, "dispatch_ms": sum(tot) / len(tot), "bwd_and_compaction_ms": sum(back) / len(back),
                              "points_and_fwd_ms": (sum(tot) - sum(back)) / len(tot)}), flush=True)
        t.close()
        return
    fmt, pat, dispatch = {"onion": (vg.FORMAT_ONION, "^cat", lambda r, n, f: r.dispatch_onion(base, n * BATCH, f)),
                          "solana": (vg.FORMAT_SOLANA, "^So1", lambda r, n, f: r.dispatch_random(20261021, 0, n * BATCH, f)),
                          "nostr": (vg.FORMAT_NOSTR, "^npub1cat", lambda r, n, f: r.dispatch(key0 + n * BATCH, f))}[a.leg]
    r = vg.GpuRunner(batch_size=BATCH, fmt=fmt, device=0, frames=FRAMES, timing=False)
    rate, found = leg(r, dispatch, pat, fmt, a.seconds)
    print(json.dumps({"leg": a.leg, "pattern": pat, "keys_per_s": rate, "candidates": found, "batch": BATCH, "frames": FRAMES, "seconds": a.seconds,
                      "device": vg.device_name(0)}), flush=True)
    r.close()


if __name__ == "__main__":
    main()
