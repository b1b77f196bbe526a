#!/usr/bin/env python3
"""The reference's ray sandbox, raytracing/RayTracingTest.java, on the GPU: the wedge of Raytrace.drawSimpleImage, the weight plane of
drawRays(img, 5, 8) through it, and the stack of renderDifferentNAs, written as ImageJ float TIFFs (wedge.tif, rays_weight.tif,
different_nas.tif).  The reference's constants are the defaults: 300 x 300 x 10, low 1.0, high 1.33, z = 5, one ray every 8 voxels,
NA 1.0 .. 2 in steps of 0.01.  A last leg launches rays the reference cannot: a converging bundle through the wedge, with
Context.trace_rays (converging_weight.tif).

    python examples/trace_rays.py [--size 300 300 10] [--high 1.33] [--na-to 2.0] [--out DIR]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[300, 300, 10], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--high", type=float, default=1.33)
    ap.add_argument("--z", type=int, default=None, help="plane of the rays (default: Nz // 2)")
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--na-to", type=float, default=2.0)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    nx, ny, nz = args.size
    z = nz // 2 if args.z is None else args.z
    os.makedirs(args.out, exist_ok=True)

    def save(name, a):
        path = os.path.join(args.out, name)
        mvs.Tools.save(np.ascontiguousarray(a, dtype=np.float32), path)
        print(f"{path}: {' x '.join(str(d) for d in np.shape(a)[::-1])}, max {float(np.max(a)):.4g}")

    wedge = np.zeros((nz, ny, nx), np.float32)
    mvs.Raytrace.drawSimpleImage(wedge, 1.0, args.high)
    save("wedge.tif", wedge)
    t0 = time.perf_counter()
    rays = mvs.RayTracingTest.drawRays(wedge, z, args.spacing)
    print(f"drawRays: {nx // args.spacing} rays, {time.perf_counter() - t0:.3f} s")
    save("rays_weight.tif", mvs.RayTracingTest.getProcessor(rays.getWeight(), z))
    t0 = time.perf_counter()
    stack = mvs.RayTracingTest.renderDifferentNAs(size=(nx, ny, nz), naTo=args.na_to, z=z, spacing=args.spacing)
    print(f"renderDifferentNAs: {len(stack)} scenes, {time.perf_counter() - t0:.3f} s")
    save("different_nas.tif", stack)

    # a bundle converging on the middle of the volume from the top edge
    ctx = mvs.default_context()
    n = 2000
    x0 = np.linspace(1.0, nx - 2.0, n)
    pos = np.stack([x0, np.full(n, ny - 1.0), np.full(n, float(z))], axis=1)
    aim = np.array([nx / 2.0, ny / 4.0, float(z)])
    out = ctx.trace_rays(wedge, pos, aim - pos, normalize_dirs=True)
    print(f"converging bundle: {n} rays, {out['n_capped']} still inside after the move cap")
    save("converging_weight.tif", out["weight"][z])
    print("done.")


if __name__ == "__main__":
    main()
