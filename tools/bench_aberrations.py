#!/usr/bin/env python3
"""Refraction simulator (aberrations.hip) timings at the reference's size; prints one JSON line.

  refract3d        200 000 light-sheet rays through a 289^3 index volume (smooth blobs, multiview-simulation_amd/synthetic.py), plane
                   z = 176, lsMiddle 1, lsEdge 3, ri 1.1, volumes resident on the device: once tracing only (no image / weight), once
                   with the injection; the difference is the injection
  projectToCamera  --pixels camera rows of the 289 x 289 image at 500 rays per pixel (the whole image is 41.8 M rays; a band of rows
                   has the same per-ray work), on the refracted volume of the run above

Rates are rays/s and moves/s (a move = one Hessian, eigenpair and possibly refraction); moves are counted from the step list.
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


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=289)
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--rows", type=int, default=16, help="camera rows traced by the projectToCamera leg")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n, z = args.size, 176 * args.size // 289
    img = synth.smooth_blobs(n, seed=3, count=8, sigma=(0.18, 0.3))
    ri_img = synth.smooth_blobs(n, seed=4)
    out = {"metric": "aberrations", "size": n, "rays": args.rays}
    with mvs.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        nbytes = img.nbytes
        d_img, d_ri, d_image, d_weight = (ctx.dev_alloc(nbytes) for _ in range(4))
        try:
            ctx.upload(d_img, img)
            ctx.upload(d_ri, ri_img)
            dim = (C.c_int64 * 3)(n, n, n)
            moves = np.zeros(args.rays, np.int32)
            steps = mvs._lib.RaySteps(args.rays * n, 0, None, None, moves.ctypes.data_as(C.POINTER(C.c_int32)))

            def refract(inject, with_steps=False):
                state = C.c_uint64((2423 ^ 0x5DEECE66D) & ((1 << 48) - 1))
                if inject:
                    mvs._lib.check(L.mvsim_dev_memset(h, C.c_void_p(d_image), 0, nbytes))
                    mvs._lib.check(L.mvsim_dev_memset(h, C.c_void_p(d_weight), 0, nbytes))
                mvs._lib.check(L.mvsim_refract3d_dev(h, C.c_void_p(d_img), C.c_void_p(d_ri), dim, 0, z, 1.0, 3.0, 1.1, args.rays, C.byref(state),
                                                     C.c_void_p(d_image) if inject else None, C.c_void_p(d_weight) if inject else None,
                                                     C.byref(steps) if with_steps else None))
                ctx.synchronize()

            refract(False, True)
            nmoves = int(moves.sum())
            t_trace = timed(lambda: refract(False), args.reps)
            t_all = timed(lambda: refract(True), args.reps)
            out["refract3d"] = {"moves": nmoves, "trace_s": round(t_trace, 4), "trace_and_inject_s": round(t_all, 4),
                                "inject_s": round(t_all - t_trace, 4), "trace_rays_per_s": round(args.rays / t_trace),
                                "trace_moves_per_s": round(nmoves / t_trace), "inject_steps_per_s": round(nmoves / max(t_all - t_trace, 1e-9))}
            # the camera on a band of rows: a volume of the same x and z extent whose y extent is the band
            rows = min(args.rows, n)
            y0 = (n - rows) // 2
            refr = ctx.download(d_image, img.shape)
            band_ri = np.ascontiguousarray(ri_img[:, y0:y0 + rows, :])
            band_refr = np.ascontiguousarray(refr[:, y0:y0 + rows, :])
            rays = rows * n * 500
            t_cam = timed(lambda: ctx.project_to_camera(band_ri, band_refr, z, 500), max(1, args.reps - 1))
            out["projectToCamera"] = {"rows": rows, "rays": rays, "s": round(t_cam, 4), "rays_per_s": round(rays / t_cam),
                                      "moves_per_s_upper": round(rays * (n - 1) / t_cam)}
        finally:
            for p in (d_img, d_ri, d_image, d_weight):
                ctx.dev_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
