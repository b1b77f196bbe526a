#!/usr/bin/env python3
"""SimulateBeads.main (SimulateBeads.java:207-224): 1000 random beads (new Random(535)) in 512 x 512 x 200, seen at 0, 45, 90 and
135 degrees about x, rendered as Gaussians of sigma (1, 1, 3) on the GPU and written as Angle_<a>.tif (ImageJ float stacks of
511 x 511 x 199, one voxel less than the interval per axis, as the reference renders them).

    python examples/simulate_beads.py [--out DIR]
"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    mvs = importlib.import_module("multiview-simulation_amd")
    angles = [0, 45, 90, 135]
    rng = ((0, 0, 0), (511, 511, 199))                     # FinalInterval(512, 512, 200)
    sb = mvs.SimulateBeads(angles, 0, 1000, rng, rng, [1, 1, 3])
    os.makedirs(args.out, exist_ok=True)
    for i, a in enumerate(angles):
        path = os.path.join(args.out, f"Angle_{a}.tif")
        mvs.Tools.save(sb.getImgs()[i], path)
        back = mvs.Tools.open(path)
        print(f"{path}: {back.shape[2]} x {back.shape[1]} x {back.shape[0]}, max {float(back.max()):.1f}")
    print("done.")


if __name__ == "__main__":
    main()
