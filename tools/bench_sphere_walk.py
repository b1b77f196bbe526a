#!/usr/bin/env python3
"""Host walk against device walk (option sphere_walk, csrc/sphere_walk.hip) at the reference's 580^3 canvas and at 1160^3; prints one
JSON line and writes it to --out (default profiles/sphere_walk_bench.json).

  draw_spheres_host / draw_spheres_device   mvsim_draw_spheres_dev (scale 2, half-pixel offset off, new Random(464232194)) on a device
                                            canvas, the walk on the host and on the device.  The compositing kernels are the same in
                                            both, so the difference of the two is the difference of the walks.
  phantom                                   Context.simulate_aberration_phantom on synthetic.index_block(n): upload of the canvas, noise,
                                            multiSpheres (device walk), both down-samplings, download of the two results.

Every figure is the median wall clock of a call that ends in a device synchronise, after a warm-up call of the same shape; the two walks
alternate call by call.  Both walks must leave the same image bits, sphere count and generator state at the size timed (--no-verify skips
the image comparison, which downloads the canvas twice).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mvs = importlib.import_module("multiview-simulation_amd")
synthetic = importlib.import_module("multiview-simulation_amd.synthetic")
SEED = 464232194


def record(t):
    return {"ms": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * min(t), 3), "ms_max": round(1e3 * max(t), 3)}


def draw(ctx, canvas, n, how):
    """one drawSpheres call with the walk `how`: (seconds, spheres, state)"""
    dim = (C.c_int64 * 3)(n, n, n)
    st, count = C.c_uint64((SEED ^ 0x5DEECE66D) & ((1 << 48) - 1)), C.c_int64(0)
    ctx.set_option("sphere_walk", how)
    t0 = time.perf_counter()
    mvs._lib.check(ctx._L.mvsim_draw_spheres_dev(ctx._h, C.c_void_p(canvas), dim, 0.0, 1.0, 2, 0, C.byref(st), C.byref(count)))
    ctx.synchronize()
    return time.perf_counter() - t0, int(count.value), int(st.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[580, 1160])
    ap.add_argument("--phantom-sizes", type=int, nargs="*", default=[580, 1160])
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_walk_bench.json"))
    args = ap.parse_args()
    ctx = mvs.default_context()
    chunk, entries = ctx.sphere_walk_geometry()
    out = {"metric": "sphere_walk", "reps": args.reps, "chunk_positions": chunk, "entry_offsets": entries, "sizes": {}}
    for n in args.sizes:
        rec = {}
        canvas = ctx.dev_alloc(4 * n ** 3)
        try:
            images = {}
            for how in ("host", "device_only"):                      # warm-up, and the comparison of what the two walks leave
                mvs._lib.check(ctx._L.mvsim_dev_memset(ctx._h, canvas, 0, 4 * n ** 3))
                _, rec["spheres_" + how], rec["state_" + how] = draw(ctx, canvas, n, how)
                if not args.no_verify:
                    images[how] = ctx.download(canvas, (n, n, n)).view(np.uint32)
            same = rec["spheres_host"] == rec["spheres_device_only"] and rec["state_host"] == rec["state_device_only"]
            if not args.no_verify:
                same = same and bool(np.array_equal(images["host"], images["device_only"]))
            images.clear()
            rec["identical"] = same
            if not same:
                raise SystemExit(f"host and device walk differ at {n}^3: {rec}")
            times = {"host": [], "device_only": []}
            for _ in range(args.reps):
                for how in times:
                    times[how].append(draw(ctx, canvas, n, how)[0])
            rec["draw_spheres_host"], rec["draw_spheres_device"] = record(times["host"]), record(times["device_only"])
            rec["host_over_device"] = round(rec["draw_spheres_host"]["ms"] / rec["draw_spheres_device"]["ms"], 2)
        finally:
            ctx.set_option("sphere_walk", "auto")
            ctx.dev_free(canvas)
        if n in args.phantom_sizes:
            block = synthetic.index_block(n)
            t = []
            for i in range(1 + min(args.reps, 3)):
                t0 = time.perf_counter()
                img, ri = ctx.simulate_aberration_phantom(block, mvs.JavaRandom(SEED), scale=2)
                if i:
                    t.append(time.perf_counter() - t0)
            rec["phantom"] = record(t)
            rec["phantom"]["out_shape"] = list(img.shape)
            del block, img, ri
        out["sizes"][str(n)] = rec
        print(f"{n}^3: {json.dumps(rec)}", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
