"""Keys per second of the Solana format (format 12: SHA-512 + an Ed25519 fixed-base multiplication per candidate) against the
secp256k1 random-key P2PKH path in the same run, beside the static VALU count per candidate of ed_keys_kernel<PRE>.
`^So1` / `^1Cat`, 2^20 candidates per dispatch, 12 frames, one device, two legs of each kind alternated in one process, and one leg
of a pattern the device cannot filter (kind 0: dumps, confirmed on the host).  A first measurement: no pass bar.
usage: python tools/solana_rate.py [--seconds 3] > profiles/r12_solana_rate.jsonl
       python tools/solana_rate.py --static-only [--rates SOLANA,P2PKH] >> profiles/r12_solana_rate.jsonl   (no GPU: the count per candidate
       from the build's assembly, its split, and the ratio of the counts beside the ratio of the measured rates)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, FRAMES = 1 << 20, 12


def dispatch_leg(r, pattern, fmt, seconds):
    """Keeps every frame in flight for `seconds`; -> (keys per second, candidates reported)."""
    r.set_filter(vg.Pattern(pattern, False, fmt))
    nxt = 0
    for f in range(FRAMES):
        r.dispatch_random(20261020, 0, nxt * BATCH, f)
        nxt += 1
    # (warm-up: the first round builds streams and tables)
    for f in range(FRAMES):
        r.wait(f)
        r.dispatch_random(20261020, 0, nxt * BATCH, f)
        nxt += 1
    done = found = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for f in range(FRAMES):
            n, tested = r.wait(f)
            done += tested
            found += n
            r.dispatch_random(20261020, 0, nxt * BATCH, f)
            nxt += 1
    dt = time.perf_counter() - t0
    for f in range(FRAMES):
        r.wait(f)
    return done / dt, found


SQR_TRIPS = [2, 5, 10, 20, 10, 50, 100, 50, 5]   # fe25_inv's runs of squarings (core/fe25519.h), in program order
# the yardstick's count per key, from the documents: 21 300 instructions for the secp256k1 multiplication over its wide table
#  and 2 957 executed VALU for the per-key tail of the P2PKH kernel (profiles/pmc_valu.json)
P2PKH_RANDOM_VALU_PER_KEY = 21300 + 2957


def valu(lines):
    return sum(1 for l in lines if re.match(r"\s+v_", l))


def kernel_body(txt, symbol_part):
    sym = next(s for s in re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M) if symbol_part in s)
    return txt.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0].split("\n")


def static_count():
    """VALU instructions one candidate executes in ed_keys_kernel<PRE>, from the build's assembly: straight-line code as it stands, the
    window loop (the one loop that loads the table) x 32, the nine squaring loops of the inversion x their trip counts, and the region
    between the two barriers - which one wave of the workgroup's eight executes - divided by 8.  The filter's loops count one trip
    (one range or residue).  The head (draw + SHA-512) and the tail (products, encoding, filter) are interleaved by the compiler:
    tools/ed_count.hip compiles the pieces alone, and their counts give the split."""
    body = kernel_body(open(os.path.join(ROOT, "build", "lib", "device", "kernels.s")).read(), "ed_keys_kernelILb1")
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    barriers = [i for i, l in enumerate(body) if re.match(r"\s+s_barrier", l)]
    assert len(barriers) == 2, barriers
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(2), i) < i and not any(labels[m.group(2)] < b < i for b in barriers):
            loops.append((labels[m.group(2)], i))
    window = [lp for lp in loops if any("global_load" in l for l in body[lp[0]:lp[1]])]
    assert len(window) == 1 and window[0][1] < barriers[0], window
    w0, w1 = window[0]
    sqr = [lp for lp in loops if barriers[0] < lp[0] and lp[1] < barriers[1]]
    assert len(sqr) == len(SQR_TRIPS) and len({valu(body[a:b]) for a, b in sqr}) == 1, sqr
    inv_wave = valu(body[barriers[0]:barriers[1]]) + sum((t - 1) * valu(body[a:b]) for t, (a, b) in zip(SQR_TRIPS, sqr))
    head, mult = valu(body[:w0]), 32 * valu(body[w0:w1])
    tree_up, tail = valu(body[w1:barriers[0]]), valu(body[barriers[1]:])
    pieces = {}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ed_count.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "--cuda-device-only", "-S",
                               os.path.join(ROOT, "tools", "ed_count.hip"), "-o", out], stderr=subprocess.DEVNULL)
        ptxt = open(out).read()
        for name in ("draw", "sha512", "encode", "filter", "mul"):
            pieces[name] = valu(kernel_body(ptxt, "count_" + name))
    total = head + mult + tree_up + inv_wave / 8 + tail
    return {"valu_per_candidate": round(total), "window_step": valu(body[w0:w1]), "squaring": valu(body[sqr[0][0]:sqr[0][1]]),
            "split": {"seed_draw_sha256": pieces["draw"], "sha512_and_clamp": head - pieces["draw"], "multiplication_32_steps": mult,
                      "inversion_share": round(tree_up + inv_wave / 8 + pieces["mul"]), "of_which_inverting_wave_over_8": round(inv_wave / 8),
                      "affine_and_encoding": tail - pieces["filter"] - pieces["mul"], "filter_one_test": pieces["filter"]},
            "pieces_compiled_alone": pieces, "inverting_wave_valu": inv_wave, "kernel_text_valu": valu(body)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--rates", default="", help="--static-only: the measured rates SOLANA,P2PKH_RANDOM (keys/s) to set the count ratio against")
    a = ap.parse_args()
    if a.static_only:
        rec = {"static": True, **static_count(), "p2pkh_random_valu_per_key": P2PKH_RANDOM_VALU_PER_KEY,
               "p2pkh_random_source": "21 300 instructions per multiplication (DESIGN.md 4) + 2 957 executed VALU of the per-key tail (profiles/pmc_valu.json)"}
        rec["count_ratio_expected_rate_ratio"] = P2PKH_RANDOM_VALU_PER_KEY / rec["valu_per_candidate"]
        if a.rates:
            sol, p2 = (float(x) for x in a.rates.split(","))
            rec["rate_ratio"] = sol / p2
            rec["measured_over_expected"] = rec["rate_ratio"] / rec["count_ratio_expected_rate_ratio"]
        print(json.dumps(rec), flush=True)
        return
    global vg
    import vgen_amd as vg
    sol = vg.GpuRunner(batch_size=BATCH, fmt=vg.FORMAT_SOLANA, device=0, frames=FRAMES, timing=False)
    p2 = vg.GpuRunner(batch_size=BATCH, fmt=vg.AddressFormat.P2pkh, device=0, frames=FRAMES, timing=False)
    rates = {"solana": [], "p2pkh_random": []}
    for rep in range(2):
        for name, r, pat, fmt in (("solana", sol, "^So1", vg.FORMAT_SOLANA), ("p2pkh_random", p2, "^1Cat", vg.AddressFormat.P2pkh)):
            rate, found = dispatch_leg(r, pat, fmt, a.seconds)
            rates[name].append(rate)
            print(json.dumps({"leg": name, "rep": rep, "pattern": pat, "keys_per_s": rate, "candidates": found, "batch": BATCH, "frames": FRAMES}), flush=True)
    t0 = time.perf_counter()
    res = vg.scan_gpu_with_runner("So1", vg.ScanConfig(format=vg.FORMAT_SOLANA, count=None, seed=1, max_batches=8), sol)
    print(json.dumps({"leg": "solana_kind0_scan", "pattern": "So1", "keys_per_s": res.operations / (time.perf_counter() - t0), "matches": len(res.matches)}), flush=True)
    m = {k: sum(v) / len(v) for k, v in rates.items()}
    print(json.dumps({"summary": True, "solana_keys_per_s": m["solana"], "p2pkh_random_keys_per_s": m["p2pkh_random"],
                      "ratio": m["solana"] / m["p2pkh_random"], "device": vg.device_name(0)}), flush=True)
    sol.close()
    p2.close()


if __name__ == "__main__":
    main()
