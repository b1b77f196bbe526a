#!/usr/bin/env python3
"""Bead renderer (beads.hip) timings; prints one JSON line.

  a  SimulateBeads.main: 1000 beads, 512 x 512 x 200 interval (511 x 511 x 199 images), 4 angles about x, float, host buffers
  b  the defaults of the loader dialog (SimulatedBeadsImgLoader2.java:249-268): 2000 beads in [-512, 512]^3, viewport 0..256 x 256 x 100,
     angles 0 and 90 about y, float, host buffers
  c  10^6 beads in 2048 x 2048 x 512, 4 angles, float and uint16 images resident on the device

Per case: ms per view (wall clock of the call / views), Gvoxel/s, and the fraction of 8 TB/s that the bytes written (4 or 6 B per
voxel) plus the bead-list traffic would take at that time.  Case a also gets the CPU time of the sequential numpy restatement
(tests/beads_restatement.py) for one view.
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
PEAK = 8.0e12


def record(ms_per_view, vox, bytes_per_voxel, list_bytes):
    return {"ms_per_view": round(ms_per_view, 4), "gvox_per_s": round(vox / ms_per_view / 1e6, 2),
            "frac_of_8TBps": round((vox * bytes_per_voxel + list_bytes) / (ms_per_view * 1e-3) / PEAK, 4)}


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    out = {"metric": "bead_render"}
    with mvs.Context(0) as ctx:
        # a
        rng = ((0, 0, 0), (511, 511, 199))
        pts = mvs.SimulateBeads.randomPoints(1000, rng, mvs.JavaRandom(535))
        sb = mvs.SimulateBeads([0, 45, 90, 135], 0, 1000, rng, rng, [1, 1, 3])
        mats = sb.matrices()
        ms = timed(lambda: ctx.render_beads(pts, rng, (1, 1, 3), matrices=mats), args.reps) / 4
        out["a_main"] = record(ms, 511 * 511 * 199, 4, 1000 * 64)
        if not args.skip_cpu:
            from tests import beads_restatement as R
            lst = R.apply(mats[1], pts)
            t0 = time.perf_counter()
            R.render(lst, rng, (1, 1, 3))
            out["a_main"]["cpu_restatement_ms_per_view"] = round(1e3 * (time.perf_counter() - t0), 1)
        # b
        rngs = ((-512, -512, -512), (512, 512, 512))
        view = ((0, 0, 0), (256, 256, 100))
        ptsb = mvs.SimulateBeads.randomPoints(2000, rngs, mvs.JavaRandom(535))
        mb = np.stack([mvs.AffineTransform3D().rotate(1, mvs.beads.to_radians(a)).m for a in (0, 90)])
        ms = timed(lambda: ctx.render_beads(ptsb, view, (1, 1, 3), matrices=mb), args.reps) / 2
        out["b_dialog"] = record(ms, 256 * 256 * 100, 4, 2000 * 64)
        # c
        nx, ny, nz = 2048, 2048, 512
        big = ((0, 0, 0), (nx, ny, nz))
        ptsc = mvs.SimulateBeads.randomPoints(1_000_000, big, mvs.JavaRandom(535))
        mc = np.stack([mvs.SimulateMultiViewDataset.axisRotation((nx + 1, ny + 1, nz + 1), 0, a) for a in (0, 45, 90, 135)])
        nv = nx * ny * nz
        f = [ctx.dev_alloc(4 * nv) for _ in range(4)]
        u = [ctx.dev_alloc(2 * nv) for _ in range(4)]
        try:
            def run():
                ctx.render_beads_dev(ptsc, big, (1, 1, 3), f, u, matrices=mc)
                ctx.synchronize()
            ms = timed(run, max(1, args.reps // 2)) / 4
            out["c_dense"] = record(ms, nv, 6, 1_000_000 * 64)
        finally:
            for p in f + u:
                ctx.dev_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
