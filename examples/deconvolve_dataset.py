#!/usr/bin/env python3
"""Close the loop on the simulated dataset: a weighted, sequential (OSEM) multi-view Richardson-Lucy deconvolution of the
aligned views with their PSFs and normalised weights, and its error against the ground truth per iteration.

    python examples/deconvolve_dataset.py --size 64 --views 7                  # simulates the dataset in memory first
    python examples/deconvolve_dataset.py --dataset /tmp/mvsim_out/dataset.npz  # what examples/simulate_dataset.py --out wrote

Printed: the NRMSE (root mean square error over the ground truth's range, after the least-squares scale of the estimate) of
the weighted average of the aligned views -- the baseline a reconstruction has to beat -- and of the estimate after every
iteration.  Every iteration continues from the previous estimate (init_from_psi), so the figures are those of one run.
"""
import argparse
import importlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")


def nrmse(est, truth):
    e, t = est.astype(np.float64).ravel(), truth.astype(np.float64).ravel()
    s = float(e @ t) / max(float(e @ e), 1e-300)
    return float(np.sqrt(np.mean((s * e - t) ** 2)) / (t.max() - t.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default=None, metavar="NPZ", help="dataset.npz of examples/simulate_dataset.py (default: simulate in memory)")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--views", type=int, default=7)
    ap.add_argument("--psf", type=int, default=15)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--tikhonov", type=float, default=0.0)
    ap.add_argument("--method", type=int, default=0, help="0 auto, 1 FFT, 2 stencil")
    a = ap.parse_args()

    if a.dataset:
        data = dict(np.load(a.dataset))
    else:
        import simulate_dataset
        data = simulate_dataset.simulate(argparse.Namespace(size=a.size, views=a.views, psf=a.psf, reference_inputs=None))
    angles = sorted(int(m.group(1)) for k in data if (m := re.fullmatch(r"aligned_view_(\d+)", k)))
    views = [data[f"aligned_view_{g}"] for g in angles]
    psfs = [data[f"aligned_view_psf_{g}"] for g in angles]
    weights = [data[f"aligned_view_weights{g}"] for g in angles]
    truth = data["groundtruth"]
    planes = min([v.shape[0] for v in views] + [w.shape[0] for w in weights] + [truth.shape[0]])
    if any(x.shape[0] != planes for x in views + weights + [truth]):
        print(f"makeIsotropic returns {views[0].shape[0]} planes, weights and ground truth have {truth.shape[0]}: every input cropped to the first {planes}")
        views, weights, truth = [v[:planes] for v in views], [w[:planes] for w in weights], truth[:planes]
    views = [np.ascontiguousarray(v, dtype=np.float32) for v in views]
    weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]

    wsum = np.sum(weights, axis=0, dtype=np.float64)
    avg = np.sum([w.astype(np.float64) * v for v, w in zip(views, weights)], axis=0) / np.maximum(wsum, 1e-12)
    print(f"{len(views)} views of {views[0].shape}, PSFs of {psfs[0].shape}")
    print(f"NRMSE weighted average of the views: {nrmse(avg, truth):.4f}")

    ctx = mvs.default_context()
    line, psi = [], None
    for it in range(a.iterations):
        p = mvs.decon_params(iterations=1, method=a.method, lambda_=a.tikhonov, init_from_psi=0 if psi is None else 1)
        psi = ctx.deconvolve(views, psfs, weights, p, psi=psi)
        line.append(nrmse(psi, truth))
    print("NRMSE per iteration: " + " ".join(f"{v:.4f}" for v in line))


if __name__ == "__main__":
    main()
