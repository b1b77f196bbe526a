#!/usr/bin/env python3
"""Close the loop on the bead images: render the four views of SimulateBeads.main on the GPU, detect the beads in every view
there (difference of Gaussians, sub-voxel fit; no image is downloaded), and recover each view's matrix from the detections.

    python examples/detect_beads.py                                   # 1000 beads in 512 x 512 x 200, as SimulateBeads.main
    python examples/detect_beads.py --size 128 128 96 --beads 60      # a smaller cloud

Per view: the detections found, the true beads that lie inside the image (at least --margin voxels from every face), how many of
them have a detection within one voxel, the mean and the largest distance of those pairs, and the view's 3 x 4 matrix recovered
by a least-squares fit from (true untransformed position -> detection) beside the true one.  Beads closer to each other than
the detector can separate, or cut by a face, stay unpaired; they are counted, not hidden.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=5.0, help="on the DoG of the unnormalised images (beads of amplitude 1000)")
    ap.add_argument("--margin", type=float, default=8.0)
    ap.add_argument("--u16", action="store_true", help="detect in the unsigned-short images the image loaders serve")
    a = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    angles = [0, 45, 90, 135]
    rng = ((0, 0, 0), tuple(s - 1 for s in a.size))                # FinalInterval(size)
    sb = mvs.SimulateBeads(angles, 0, a.beads, rng, rng, [1, 1, 3])
    det = mvs.DifferenceOfGaussian(sigma=1.8, threshold=a.threshold, capacity=max(1024, 4 * a.beads))
    mats = sb.matrices()
    np.set_printoptions(precision=4, suppress=True, linewidth=140)
    for v, angle in enumerate(angles):
        peaks, found, truth = sb.detect(v, det, u16=a.u16)
        hi = np.array([s - 2 for s in a.size], dtype=np.float64)   # the image has one voxel less than the interval per axis
        inside = np.all((truth >= a.margin) & (truth <= hi - a.margin), axis=1)
        pos = peaks["pos"]
        pairs = []
        for i in np.nonzero(inside)[0]:
            if len(pos):
                d = np.linalg.norm(pos - truth[i], axis=1)
                j = int(np.argmin(d))
                if d[j] <= 1.0:
                    pairs.append((i, j, d[j]))
        print(f"view {angle:3d} degrees: {found} detections, {int(inside.sum())} beads inside the image, {len(pairs)} paired within one voxel")
        if len(pairs) < 4:
            print("  too few pairs for a fit")
            continue
        dist = np.array([p[2] for p in pairs])
        print(f"  distance true bead -> detection: mean {dist.mean():.4f}, largest {dist.max():.4f} voxel")
        src = np.hstack([sb.points[[p[0] for p in pairs]], np.ones((len(pairs), 1))])
        dst = pos[[p[1] for p in pairs]] + np.array(rng[0], dtype=np.float64)
        fit, *_ = np.linalg.lstsq(src, dst, rcond=None)
        print("  recovered matrix                                  true matrix")
        for r in range(3):
            print("  " + np.array2string(fit.T[r]).ljust(50) + np.array2string(mats[v][r]))
        print(f"  largest difference of a matrix entry: {np.max(np.abs(fit.T - mats[v])):.2e}")
    print("done.")


if __name__ == "__main__":
    main()
