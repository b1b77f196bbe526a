#!/usr/bin/env python3
"""Tile pairs per second of SimulateTileStitching at the reference's size (289^3, synthetic.measured_like_psf(51), overlap 0.2, snr 8);
prints one JSON line.

  host      SimulateTileStitching(resident=False).getNextPair: each tile cropped on the host, uploaded, sampled, downloaded
  resident  resident=True: both convolved phantoms stay in HBM, a pair is one mvsim_extract_intervals call with two jobs
  batch16   resident=True, getNextPairs with 16 pairs: 32 jobs in one call, fresh arrays for every call
  batch16_reuse  the same into the arrays of the first call (getNextPairs(snrs, out=...)): without the page faults of 225 MB of fresh
                 output per call, which cost several times the call itself

Each leg is a child process of its own under its own time limit (--limit seconds); a leg that fails or runs out of time ends the run:
nothing more is started on the GPU.  Per leg: the object is built and --warmup pairs are drawn, then every pair (batch16: every call of
16) is timed by the host clock around the synchronous call; the rate is 1 / the median time per pair over --pairs pairs (at least 20).
The legs draw the same seeds, and the run fails unless their first pairs are bit-identical.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("host", "resident", "batch16", "batch16_reuse")
SNR = 8.0


def leg(name, pairs, warmup):
    sys.path.insert(0, ROOT)
    mvs = importlib.import_module("multiview-simulation_amd")
    synth = importlib.import_module("multiview-simulation_amd.synthetic")
    t0 = time.perf_counter()
    sim = mvs.SimulateTileStitching(mvs.JavaRandom(5), True, (0.2,) * 3, None, psf=synth.measured_like_psf(51), resident=name != "host")
    init_s = time.perf_counter() - t0
    per_call = 16 if name.startswith("batch16") else 1
    kept = []

    def draw():
        if per_call == 1:
            return [sim.getNextPair(SNR)]
        if name != "batch16_reuse":
            return sim.getNextPairs([SNR] * 16)
        if not kept:
            kept.append(sim.getNextPairs([SNR] * 16))
            return kept[0]
        return sim.getNextPairs([SNR] * 16, out=kept[0])

    first = draw()[0]
    crc = zlib.crc32(first[1].tobytes(), zlib.crc32(first[0].tobytes()))
    shape = list(first[0].shape)
    for _ in range(max(0, -(-warmup // per_call) - 1)):
        draw()
    times = []
    for _ in range(-(-pairs // per_call)):
        t0 = time.perf_counter()
        draw()
        times.append((time.perf_counter() - t0) / per_call)
    sim.close()
    med = float(np.median(times))
    print(json.dumps({"leg": name, "pairs_per_s": round(1.0 / med, 2), "ms_per_pair": round(1e3 * med, 3),
                      "ms_per_pair_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)], "pairs_timed": len(times) * per_call,
                      "init_s": round(init_s, 2), "tile_shape": shape, "first_pair_crc32": crc}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32, help="pairs timed per leg (at least 20)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one leg, seconds")
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent starts)")
    args = ap.parse_args()
    if args.pairs < 20:
        ap.error("--pairs must be at least 20")
    if args.leg:
        leg(args.leg, args.pairs, args.warmup)
        return 0
    out = {"metric": "tile_pairs", "size": 289, "psf": "measured_like_psf(51)", "overlap": 0.2, "snr": SNR}
    for name in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--pairs", str(args.pairs), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"leg {name}: no result within {args.limit} s; stopping", file=sys.stderr)
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"leg {name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    crcs = {out[name].pop("first_pair_crc32") for name in LEGS}
    out["first_pairs_identical"] = len(crcs) == 1
    out["resident_over_host"] = round(out["resident"]["pairs_per_s"] / out["host"]["pairs_per_s"], 2)
    out["batch16_over_host"] = round(out["batch16"]["pairs_per_s"] / out["host"]["pairs_per_s"], 2)
    out["batch16_reuse_over_host"] = round(out["batch16_reuse"]["pairs_per_s"] / out["host"]["pairs_per_s"], 2)
    print(json.dumps(out))
    return 0 if out["first_pairs_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
