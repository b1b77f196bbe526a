#!/usr/bin/env python3
"""Register the bead views from their detections alone: render the four views of SimulateBeads.main on the GPU, detect the beads in
every view there, and register each view against view 0 by geometric descriptors, RANSAC and an affine refit -- no image and no
detection list is downloaded on the way, and nothing but the detections is known to the registration.

    python examples/register_beads.py                                   # 1000 beads in 512 x 512 x 200, as SimulateBeads.main
    python examples/register_beads.py --size 128 128 96 --beads 60      # a smaller cloud

Per view: the matrix view -> view 0 that the registration found beside the true one, the candidates, the inliers and how many inliers
pair a bead with itself, and -- for comparison -- the fit that examples/detect_beads.py gets by pairing every detection with the
simulator's true bead position, which no user could do.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def nearest_bead(truth, pos, limit=1.0):
    """For every detection the index of the true bead within `limit` voxel, or -1."""
    if len(pos) == 0:
        return np.zeros(0, np.int64)
    d = np.linalg.norm(pos[:, None, :] - truth[None, :, :], axis=2)
    j = np.argmin(d, axis=1)
    return np.where(d[np.arange(len(pos)), j] <= limit, j, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=5.0, help="on the DoG of the unnormalised images (beads of amplitude 1000)")
    ap.add_argument("--redundancy", type=int, default=1)
    ap.add_argument("--max-epsilon", type=float, default=5.0)
    ap.add_argument("--u16", action="store_true", help="detect in the unsigned-short images the image loaders serve")
    a = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    angles = [0, 45, 90, 135]
    rng = ((0, 0, 0), tuple(s - 1 for s in a.size))                # FinalInterval(size)
    sb = mvs.SimulateBeads(angles, 0, a.beads, rng, rng, [1, 1, 3])
    det = mvs.DifferenceOfGaussian(sigma=1.8, threshold=a.threshold, capacity=max(1024, 4 * a.beads))
    reg = mvs.BeadRegistration(redundancy=a.redundancy, max_epsilon=a.max_epsilon)
    np.set_printoptions(precision=4, suppress=True, linewidth=140)
    peaks0, _, truth0 = sb.detect(0, det, u16=a.u16)
    bead0 = nearest_bead(truth0, peaks0["pos"])
    for v, angle in enumerate(angles[1:], start=1):
        res, cand, mask, true_m = sb.register(v, 0, det, reg, u16=a.u16)
        peaks, _, truth = sb.detect(v, det, u16=a.u16)
        bead = nearest_bead(truth, peaks["pos"])
        inl = mask.astype(bool)
        same = (bead[cand["a"]] == bead0[cand["b"]]) & (bead[cand["a"]] >= 0)
        print(f"view {angle:3d} -> view 0: {res['n_a']} / {res['n_b']} described points, {res['n_candidates']} candidates "
              f"({int(same.sum())} true), {res['n_inliers']} inliers ({int(same[inl].sum())} true), refits {res['refits']}, flags {res['flags']}, "
              f"inlier error mean {res['mean_error']:.4f} largest {res['max_error']:.4f}")
        m = res["m"].reshape(3, 4)
        print("  registered matrix                                 true matrix")
        for r in range(3):
            print("  " + np.array2string(m[r]).ljust(50) + np.array2string(true_m[r]))
        print(f"  largest difference of a matrix entry: {np.max(np.abs(m - true_m)):.2e}")
        # the fit from truth pairing: detections of the same bead in both views
        common = [(i, int(np.nonzero(bead0 == b)[0][0])) for i, b in enumerate(bead) if b >= 0 and np.any(bead0 == b)]
        if len(common) >= 4:
            src = np.hstack([peaks["pos"][[c[0] for c in common]], np.ones((len(common), 1))])
            fit, *_ = np.linalg.lstsq(src, peaks0["pos"][[c[1] for c in common]], rcond=None)
            print(f"  truth-paired fit over {len(common)} beads: largest difference of a matrix entry {np.max(np.abs(fit.T - true_m)):.2e}")
    print("done.")


if __name__ == "__main__":
    main()
