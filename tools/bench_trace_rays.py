#!/usr/bin/env python3
"""The general tracer (raytrace.hip) beside refract3d (aberrations.hip) on the same resident volumes, in one process; prints one
JSON line.

  refract3d   200 000 light-sheet rays through a 289^3 index volume (the inputs of tools/bench_aberrations.py), tracing only
  trace_rays  mvsim_trace_rays_dev given refract3d's 200 000 starts (host lists, uploaded by every call), the map (1, 1.1),
              max_moves = Nz and the image as value source, tracing only: the same rays, the same moves
  The legs alternate; each figure is the median of --reps runs after one warm-up, with the fastest and slowest run beside it,
  so that the ratio can be read against the run-to-run spread of the same session.  Two more legs say where the difference goes:
  trace_rays with its start lists in page-locked memory, and the upload of the two lists (48 bytes per ray) alone.

  drawMultipleRays   the sandbox's bundle of 200 000 rays through a 289^3 raw index image in [1, 1.33] (host entry point: the volume
                     crosses to the device, image and weight come back)
  renderDifferentNAs the reference's stack of wedge scenes at 300 x 300 x 10 (na = 1.0; na <= 2; na += 0.01 -- 100 scenes: the fp64 sum
                     passes 2 before the 101st)
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
synth = importlib.import_module("multiview-simulation_amd.synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=289)
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tracers-only", action="store_true", help="skip the sandbox legs (drawMultipleRays, renderDifferentNAs)")
    args = ap.parse_args()
    n, z = args.size, 176 * args.size // 289
    img = synth.smooth_blobs(n, seed=3, count=8, sigma=(0.18, 0.3))
    ri_img = synth.smooth_blobs(n, seed=4)
    out = {"metric": "trace_rays", "size": n, "rays": args.rays}
    with mvs.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        d_img, d_ri = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(img.nbytes)
        d_starts = 0
        try:
            ctx.upload(d_img, img)
            ctx.upload(d_ri, ri_img)
            dim = (C.c_int64 * 3)(n, n, n)
            abc = mvs.Lightsheet(n / 2.0, 1.0, float(n), 3.0)
            pos, vec = ctx.refract3d_ray_starts((n, n, n), False, z, (abc.a, abc.b, abc.c), args.rays, mvs.JavaRandom(2423))
            moves = np.zeros(args.rays, np.int32)
            steps = mvs._lib.RaySteps(args.rays * n, 0, None, None, moves.ctypes.data_as(C.POINTER(C.c_int32)))

            def refract(with_steps=False):
                state = C.c_uint64((2423 ^ 0x5DEECE66D) & ((1 << 48) - 1))
                mvs._lib.check(L.mvsim_refract3d_dev(h, C.c_void_p(d_img), C.c_void_p(d_ri), dim, 0, z, 1.0, 3.0, 1.1, args.rays, C.byref(state),
                                                     None, None, C.byref(steps) if with_steps else None))
                ctx.synchronize()

            tp = mvs._lib.TraceParams()
            mvs._lib.check(L.mvsim_trace_params_default(dim, C.byref(tp)))
            tp.n_a, tp.n_b, tp.max_moves = 1.0, 1.1, n
            dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
            moves2 = np.zeros(args.rays, np.int32)
            steps2 = mvs._lib.RaySteps(args.rays * n, 0, None, None, moves2.ctypes.data_as(C.POINTER(C.c_int32)))

            def trace(with_steps=False, p=pos, v=vec):
                mvs._lib.check(L.mvsim_trace_rays_dev(h, C.c_void_p(d_ri), C.c_void_p(d_img), dim, dp(p), dp(v), None, args.rays,
                                                      C.byref(tp), None, None, C.byref(steps2) if with_steps else None, None, None, None))
                ctx.synchronize()

            # where the general tracer's extra time goes: the same start lists in page-locked memory, and their upload alone
            pin_pos, pin_vec = ctx.pinned_empty(pos.shape, np.float64), ctx.pinned_empty(vec.shape, np.float64)
            pin_pos[...], pin_vec[...] = pos, vec
            d_starts = ctx.dev_alloc(pos.nbytes)

            def upload_starts():
                ctx.upload(d_starts, pos)
                ctx.upload(d_starts, vec)
                ctx.synchronize()

            refract(True)
            nmoves = int(moves.sum())
            trace(True)
            same = np.array_equal(moves2, moves)
            t = {"refract3d": [], "trace_rays": [], "trace_rays_pinned_starts": [], "starts_upload": []}
            for k in range(args.reps + 1):
                for name, fn in (("refract3d", refract), ("trace_rays", trace), ("trace_rays_pinned_starts", lambda: trace(False, pin_pos, pin_vec)),
                                 ("starts_upload", upload_starts)):
                    t0 = time.perf_counter()
                    fn()
                    if k:
                        t[name].append(time.perf_counter() - t0)
            med = {k: float(np.median(v)) for k, v in t.items()}
            for k, v in t.items():
                out[k] = {"s": round(med[k], 5), "fastest_s": round(min(v), 5), "slowest_s": round(max(v), 5)}
                if k != "starts_upload":
                    out[k]["moves_per_s"] = round(nmoves / med[k])
            out["moves"] = nmoves
            out["same_move_counts"] = bool(same)
            out["trace_rays_over_refract3d"] = round(med["trace_rays"] / med["refract3d"], 4)
        finally:
            ctx.dev_free(d_img)
            ctx.dev_free(d_ri)
            if d_starts:
                ctx.dev_free(d_starts)
        if args.tracers_only:
            print(json.dumps(out))
            return
        raw = synth.smooth_blobs(n, seed=4, count=40, sigma=(0.04, 0.07), lo=1.0, hi=1.33)
        runs = []
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            inj = mvs.RayTracingTest.drawMultipleRays(raw, n // 2, n // 2, args.rays, ctx=ctx)
            if k:
                runs.append(time.perf_counter() - t0)
        out["drawMultipleRays"] = {"s": round(float(np.median(runs)), 4), "rays_per_s": round(args.rays / float(np.median(runs))),
                                   "weight_max": float(inj.getWeight().max())}
        t0 = time.perf_counter()
        stack = mvs.RayTracingTest.renderDifferentNAs(ctx=ctx)
        out["renderDifferentNAs"] = {"scenes": int(stack.shape[0]), "s": round(time.perf_counter() - t0, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
