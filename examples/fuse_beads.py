#!/usr/bin/env python3
"""Fuse the bead views from their registrations: render the four views of SimulateBeads.main on the GPU, detect the beads in every
view, register each view against view 0 and fuse all four into view 0's interval -- the matrices go from the registration to the
fusion in device memory, and nothing is downloaded on the way.

    python examples/fuse_beads.py                                       # 1000 beads in 512 x 512 x 200, as SimulateBeads.main
    python examples/fuse_beads.py --size 128 128 96 --beads 60 --out /tmp/fused
    python examples/fuse_beads.py --size 128 128 96 --beads 60 --deconvolve 10

Writes fused.tif and, beside it, fused_true.tif: the same fusion with the simulator's true transforms.  --deconvolve N instead
aligns the views, their weights and their Gaussian PSFs into view 0's frame, normalises the weights and runs N iterations of
MultiViewDeconvolution on them (deconvolved.tif).
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gaussian_psf(sigma, radius):
    ax = [np.arange(-r, r + 1, dtype=np.float64) for r in radius]
    g = [np.exp(-(a * a) / (2.0 * s * s)) for a, s in zip(ax, sigma)]
    return (g[2][:, None, None] * g[1][None, :, None] * g[0][None, None, :]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=5.0, help="on the DoG of the unnormalised images (beads of amplitude 1000)")
    ap.add_argument("--blend", type=float, default=8.0)
    ap.add_argument("--u16", action="store_true", help="fuse the unsigned-short images the image loaders serve")
    ap.add_argument("--deconvolve", type=int, default=0, metavar="N", help="align views, weights and PSFs and run N iterations")
    ap.add_argument("--out", default=".")
    a = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    angles = [0, 45, 90, 135]
    sigma = [1, 1, 3]
    rng = ((0, 0, 0), tuple(s - 1 for s in a.size))                # FinalInterval(size)
    sb = mvs.SimulateBeads(angles, 0, a.beads, rng, rng, sigma)
    det = mvs.DifferenceOfGaussian(sigma=1.8, threshold=a.threshold, capacity=max(1024, 4 * a.beads))
    params = mvs.fuse_params(blend=a.blend)
    os.makedirs(a.out, exist_ok=True)
    fused, regs, fused_true = sb.fuse(reference=0, detector=det, u16=a.u16, params=params)
    for v, r in enumerate(regs):
        if r is not None:
            print(f"view {angles[v]:3d} -> view 0: {r['n_candidates']} candidates, {r['n_inliers']} inliers, flags {r['flags']}, "
                  f"inlier error mean {r['mean_error']:.4f}")
    diff = np.abs(fused - fused_true)
    print(f"fused {fused.shape[::-1]}: largest value {fused.max():.1f}; against the fusion with the true matrices: largest difference "
          f"{diff.max():.3f}, mean {diff.mean():.5f}")
    mvs.Tools.save(fused, os.path.join(a.out, "fused.tif"))
    mvs.Tools.save(fused_true, os.path.join(a.out, "fused_true.tif"))
    if a.deconvolve > 0:
        ctx = mvs.default_context()
        eye = np.hstack([np.eye(3), np.zeros((3, 1))])
        mats = [eye if r is None else r["m"].reshape(3, 4) for r in regs]
        views = sb.getImgs()
        dim = views[0].shape[::-1]
        aligned, weights = ctx.align_views(views, mats, (0, 0, 0), dim, params)
        radius = [3 * s for s in sigma]
        psf = gaussian_psf(sigma, radius)
        side = 2 * max(radius) + 3
        psfs = [mvs.transform_psf(psf, m, (side, side, side), ctx=ctx) for m in mats]
        n = dim[0] * dim[1] * dim[2]
        ptrs = [ctx.dev_alloc(4 * n) for _ in weights]
        try:
            for d, w in zip(ptrs, weights):
                ctx.upload(d, w)
            ctx.normalize_weights_dev(ptrs, n, 1.0)
            weights = [ctx.download(d, w.shape) for d, w in zip(ptrs, weights)]
        finally:
            for d in ptrs:
                ctx.dev_free(d)
        psi = mvs.MultiViewDeconvolution(ctx=ctx, iterations=a.deconvolve).run(aligned, psfs, weights)
        print(f"deconvolved, {a.deconvolve} iterations: largest value {psi.max():.1f}")
        mvs.Tools.save(psi, os.path.join(a.out, "deconvolved.tif"))
    print("done.")


if __name__ == "__main__":
    main()
