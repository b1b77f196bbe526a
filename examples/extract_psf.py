#!/usr/bin/env python3
"""Measure every view's PSF from its beads: render the four views of SimulateBeads.main on the GPU, detect the beads in every view,
register each view against view 0 and average the neighbourhoods of the registration's inliers into one PSF per view, sampled through
the inverse of the registration so that every PSF comes out in view 0's frame -- what the deconvolution takes.

    python examples/extract_psf.py                                       # 1000 beads in 512 x 512 x 200, as SimulateBeads.main
    python examples/extract_psf.py --size 128 128 96 --beads 60 --out /tmp/psf
    python examples/extract_psf.py --size 128 128 96 --beads 60 --deconvolve 10

Writes psf_<angle>.tif.  --deconvolve N aligns the views into view 0's frame and deconvolves them with the extracted PSFs; beside
every iteration's NRMSE against the bead cloud rendered as points (sigma 0.5) it prints the NRMSE of the same run with the
renderer's own Gaussian brought into the frame by transform_psf.  (On device buffers the same chain is psf_use_from_matches_dev and
extract_psf_dev with the registration's matrix read from device memory; tests/test_psf.py runs it.)
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def nrmse(estimate, truth):
    """RMS difference of the two volumes, each scaled to unit sum, over the range of the truth."""
    e, t = estimate.astype(np.float64), truth.astype(np.float64)
    e, t = e / e.sum(), t / t.sum()
    return float(np.sqrt(np.mean((e - t) ** 2)) / (t.max() - t.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=5.0, help="on the DoG of the unnormalised images (beads of amplitude 1000)")
    ap.add_argument("--kdim", type=int, nargs=3, default=[15, 15, 21], metavar=("KX", "KY", "KZ"))
    ap.add_argument("--deconvolve", type=int, default=0, metavar="N", help="align the views and run N iterations with the extracted PSFs")
    ap.add_argument("--out", default=".")
    a = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    ctx = mvs.default_context()
    angles = [0, 45, 90, 135]
    sigma = [1, 1, 3]
    rng = ((0, 0, 0), tuple(s - 1 for s in a.size))                # FinalInterval(size)
    sb = mvs.SimulateBeads(angles, 0, a.beads, rng, rng, sigma)
    det = mvs.DifferenceOfGaussian(sigma=1.8, threshold=a.threshold, capacity=max(1024, 4 * a.beads))
    reg = mvs.BeadRegistration()
    extraction = mvs.PsfExtraction(kdim=a.kdim, min_separation=a.kdim)
    os.makedirs(a.out, exist_ok=True)
    views = sb.getImgs()
    peaks = [det.detect(v)[0] for v in views]
    mats, psfs = [], []
    for v, angle in enumerate(angles):
        m, use = None, None
        if v > 0:
            r, cand, mask = reg.register(peaks[v]["pos"], peaks[0]["pos"])
            m = r["m"].reshape(3, 4)
            use = np.zeros(len(peaks[v]), np.uint8)
            use[cand["a"][mask == 1]] = 1
            print(f"view {angle:3d} -> view 0: {r['n_candidates']} candidates, {r['n_inliers']} inliers, flags {r['flags']}")
        psf, rec = extraction.extract(views[v], peaks[v], m=m, use=use)
        print(f"view {angle:3d}: {rec['n_listed']} detections, {rec['n_used']} used ({rec['n_masked']} no inliers, {rec['n_outside']} too near "
              f"a face, {rec['n_crowded']} crowded), background {rec['minimum']:.3f}, flags {rec['flags']}")
        mvs.Tools.save(psf, os.path.join(a.out, f"psf_{angle}.tif"))
        mats.append(np.hstack([np.eye(3), np.zeros((3, 1))]) if m is None else m)
        psfs.append(psf)
    if a.deconvolve > 0:
        dim = views[0].shape[::-1]
        aligned, weights = ctx.align_views(views, mats, (0, 0, 0), dim, mvs.fuse_params())
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
        truth = ctx.render_beads(sb.points, rng, [0.5, 0.5, 0.5], matrices=sb.matrices()[:1])["f32"][0]
        known = [mvs.transform_psf(mvs.gaussian_psf(sigma, a.kdim).astype(np.float32), m, ctx=ctx) for m in mats]
        psi = {"extracted": None, "renderer": None}
        for it in range(a.deconvolve):
            line = []
            for name, ks in (("extracted", psfs), ("renderer", known)):
                p = mvs.decon_params(iterations=1, init_from_psi=0 if psi[name] is None else 1)
                psi[name] = ctx.deconvolve(aligned, ks, weights, p, psi=psi[name])
                line.append(f"{name} PSFs {nrmse(psi[name], truth):.5f}")
            print(f"iteration {it + 1:3d}: NRMSE " + ", ".join(line))
        mvs.Tools.save(psi["extracted"], os.path.join(a.out, "deconvolved.tif"))
    print("done.")


if __name__ == "__main__":
    main()
