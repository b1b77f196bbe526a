#!/usr/bin/env python3
"""Procedural phantom (procedural.hip) timings at the size of HypersphereCollectionRealRandomAccessible.main; prints one JSON line and
writes it to --out (default profiles/phantoms_bench.json).

  perlin_raster     the 1024 x 1024 x 256 Perlin field of main (scales 256, 1024 / 1.5, 256; 100 vectors), raw, device resident
  big_raster        the 400 big spheres (radius 20 .. 40) into that volume
  small_raster      the 20 000 small spheres (radius 2 .. 4), combined with Math.max
  sample_big        400 points against the thresholded Perlin field
  sample_small      20 000 points against the 400 big spheres

Every figure is the median wall clock of a call that ends in a device synchronise (the samplers synchronise by themselves), after a
warm-up call of the same shape.  Rasters also get Gvoxel/s and the share of 8 TB/s that their 4 bytes per voxel would take in that time;
the Perlin raster gets the fp64 operations per second at PERLIN_FLOP operations per voxel, counted from perlin_value in procedural.hip.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mvs = importlib.import_module("multiview-simulation_amd")
PEAK_BYTES = 8.0e12
# per voxel: 3 divisions; 8 neighbours x (3 subtractions + 3 multiplications + 3 additions); 7 smoothsteps x 12 operations
PERLIN_FLOP = 3 + 8 * 9 + 7 * 12


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t)), 1e3 * float(np.max(t))


def raster_record(t, vox):
    ms = t[0]
    return {"ms": round(ms, 3), "ms_min": round(t[1], 3), "ms_max": round(t[2], 3), "gvox_per_s": round(vox / ms / 1e6, 2),
            "store_frac_of_8TBps": round(vox * 4 / (ms * 1e-3) / PEAK_BYTES, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dim", type=int, nargs=3, default=[1024, 1024, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phantoms_bench.json"))
    args = ap.parse_args()
    dim = [int(d) for d in args.dim]
    vox = dim[0] * dim[1] * dim[2]
    interval = ((0, 0, 0), tuple(d - 1 for d in dim))
    out = {"metric": "procedural_phantom", "dim": dim}
    ctx = mvs.default_context()
    P, H, S, PRS = (mvs.PerlinNoiseRealRandomAccessible, mvs.HypersphereCollectionRealRandomAccessible,
                    mvs.SimpleCalculatedRealRandomAccessible, mvs.PointRejectionSampling)

    def fork(rnd):
        r = mvs.JavaRandom(0)
        r._s, r._pending = rnd._s, rnd._pending
        return r

    # main's sequence (:201-255), each sampling call timed from the generator state it starts at
    rnd = mvs.JavaRandom(42)
    perlin = P((dim[0] // 4, dim[1] / 1.5, dim[2]), (15, 15, 15), 100, rnd)
    thr = S.threshold(perlin, 0.1)
    r0 = fork(rnd)
    t = timed(lambda: PRS.sampleRealPoints(interval, 400, thr, fork(r0)), args.reps)
    big_pos, trials = ctx.rejection_sample(interval[0], interval[1], 400, thr._struct(), rnd)
    out["sample_big"] = {"ms": round(t[0], 3), "ms_min": round(t[1], 3), "ms_max": round(t[2], 3), "samples": 400, "trials": trials}
    density, big, small = H(3, 0.0), H(3, 0.0), H(3, 0.0)
    radii = [20.0 + rnd.nextDouble() * 20.0 for _ in range(400)]
    for c, r in zip(big_pos, radii):
        density.addSphere(c, r, 1.0)
    r1 = fork(rnd)
    t = timed(lambda: PRS.sampleRealPoints(interval, 20000, density, fork(r1)), args.reps)
    small_pos, trials = ctx.rejection_sample(interval[0], interval[1], 20000, density._struct(), rnd)
    out["sample_small"] = {"ms": round(t[0], 3), "ms_min": round(t[1], 3), "ms_max": round(t[2], 3), "samples": 20000, "trials": trials}
    for sp in small_pos:
        small.addSphere(sp, 2.0 + rnd.nextDouble() * 2.0, np.float32(4.0 + rnd.nextDouble() * 2.0))
    for c, r in zip(big_pos, radii):
        big.addSphere(c, r, np.float32(float(np.float32(1.2)) + rnd.nextDouble() * float(np.float32(2.4) - np.float32(1.2))))

    d = ctx.dev_alloc(4 * vox)
    try:
        fs, bs, ss = perlin._struct(), big._struct(), small._struct()

        def run(fn):
            def f():
                fn()
                ctx.synchronize()
            return f
        t = timed(run(lambda: ctx.perlin_raster_dev(fs, dim, (0, 0, 0), d)), args.reps)
        out["perlin_raster"] = raster_record(t, vox)
        out["perlin_raster"]["fp64_tflops_at_%d_per_voxel" % PERLIN_FLOP] = round(vox * PERLIN_FLOP / (t[0] * 1e-3) / 1e12, 2)
        t = timed(run(lambda: ctx.spheres_raster_dev(bs, dim, (0, 0, 0), d)), args.reps)
        out["big_raster"] = raster_record(t, vox)
        t = timed(run(lambda: ctx.spheres_raster_dev(ss, dim, (0, 0, 0), d, combine=True)), args.reps)
        out["small_raster"] = raster_record(t, vox)
    finally:
        ctx.dev_free(d)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
