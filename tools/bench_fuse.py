"""View fusion: milliseconds per call and per stage, the algorithmic bytes per second they amount to, and the same job done with
torch.nn.functional.grid_sample and a weighted sum -- what a user has without the library:
    python tools/bench_fuse.py [--size 512 512 200] [--rounds 5] [--json profiles/bench_fuse.json]
Four views of --size under 0 / 45 / 90 / 135 degrees about x (SimulateBeads.main's angles) are fused into view 0's interval, blend 8.
Every figure is the median over --rounds of host wall time around work enqueued on the context's stream and one synchronise.
  prepare  a call with a one-voxel interval: the prepare launches that invert the matrices, and a fuse launch of one brick
  fuse     mvsim_fuse_views_dev with the sum of weights
  align    mvsim_align_views_dev with every view's resampled volume and weight volume
Algorithmic bytes: every source once plus the outputs (the gathers of an oblique view touch lines more than once; those re-reads
are the kernel's business, not the algorithm's).  For comparison: the copy ceiling of the chip, 6.3 TB/s.
The baseline resamples value and weight volumes with grid_sample (float32 positions, so it is not the same bits; its grids are built
beforehand and their time is reported apart)."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")

COPY_CEILING_TBS = 6.3
ANGLES = (0, 45, 90, 135)


def timed(sync, rounds, reps, fn):
    fn()
    sync()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out), min(out)


def torch_baseline(views, mats, dim, blend, rounds):
    """grid_sample of value and weight volumes plus the weighted sum, on the same device."""
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    nx, ny, nz = dim
    t0 = time.perf_counter()
    zz, yy, xx = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float32), torch.arange(ny, device=dev, dtype=torch.float32),
                                torch.arange(nx, device=dev, dtype=torch.float32), indexing="ij")
    grids, vols, wvols = [], [], []
    for src, m in zip(views, mats):
        inv = np.linalg.inv(np.vstack([m, [0, 0, 0, 1]]))[:3]
        p = [inv[r, 0] * xx + inv[r, 1] * yy + inv[r, 2] * zz + inv[r, 3] for r in range(3)]
        g = torch.stack([2 * p[0] / (nx - 1) - 1, 2 * p[1] / (ny - 1) - 1, 2 * p[2] / (nz - 1) - 1], dim=-1)[None]
        grids.append(g)
        vols.append(torch.from_numpy(src).to(dev)[None, None])
        ramps = []
        for n in (nz, ny, nx):
            e = torch.minimum(torch.arange(n, device=dev, dtype=torch.float32), (n - 1) - torch.arange(n, device=dev, dtype=torch.float32))
            q = torch.clamp(e / blend, max=1.0)
            ramps.append(q * q * (3 - 2 * q))
        wvols.append((ramps[0][:, None, None] * ramps[1][None, :, None] * ramps[2][None, None, :])[None, None])
    torch.cuda.synchronize()
    grid_ms = (time.perf_counter() - t0) * 1e3

    def run():
        num = torch.zeros((1, 1, nz, ny, nx), device=dev)
        den = torch.zeros_like(num)
        for vol, w, g in zip(vols, wvols, grids):
            s = F.grid_sample(vol, g, mode="bilinear", padding_mode="zeros", align_corners=True)
            ws = F.grid_sample(w, g, mode="bilinear", padding_mode="zeros", align_corners=True)
            num += ws * s
            den += ws
        return torch.where(den > 0, num / den, torch.zeros_like(num))

    med, best = timed(torch.cuda.synchronize, rounds, 1, run)
    return {"baseline_ms": med, "baseline_ms_min": best, "baseline_setup_ms": grid_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blend", type=float, default=8.0)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not a.no_baseline:
        import torch                                       # before the library is loaded: one HIP runtime in the process, torch's
        torch.cuda.init()
    dim = tuple(a.size)
    n = dim[0] * dim[1] * dim[2]
    V = len(ANGLES)
    rng = np.random.default_rng(0)
    views = [rng.random((dim[2], dim[1], dim[0]), dtype=np.float32) for _ in range(V)]
    rot = [mvs.SimulateMultiViewDataset.axisRotation(dim, 0, ang) for ang in ANGLES]
    mats = [mvs.registration.true_transform(r, rot[0], (0, 0, 0)) for r in rot]
    p = mvs.fuse_params(blend=a.blend)
    res = {"size": list(dim), "views": V, "angles": list(ANGLES), "blend": a.blend, "geometry": mvs.fusion_geometry(),
           "copy_ceiling_TBs": COPY_CEILING_TBS}
    with mvs.Context(0) as ctx:
        src = [ctx.dev_alloc(4 * n) for _ in range(V)]
        for d, v in zip(src, views):
            ctx.upload(d, v)
        out = [ctx.dev_alloc(4 * n) for _ in range(2 * V)]
        dims = [dim] * V
        prep = timed(ctx.synchronize, a.rounds, 20, lambda: ctx.fuse_views_dev(src, dims, mats, (0, 0, 0), (1, 1, 1), out[0], params=p))
        fuse = timed(ctx.synchronize, a.rounds, 3, lambda: ctx.fuse_views_dev(src, dims, mats, (0, 0, 0), dim, out[0], out[1], params=p))
        fuse0 = timed(ctx.synchronize, a.rounds, 3,
                      lambda: ctx.fuse_views_dev(src, dims, mats, (0, 0, 0), dim, out[0], out[1], params=mvs.fuse_params(blend=0.0)))
        den = ctx.download(out[1], (dim[2], dim[1], dim[0]))
        align = timed(ctx.synchronize, a.rounds, 3, lambda: ctx.align_views_dev(src, dims, mats, (0, 0, 0), dim, out[:V], out[V:], params=p))
        for d in src + out:
            ctx.dev_free(d)
    fuse_bytes, align_bytes = 4.0 * n * (V + 2), 4.0 * n * (V + 2 * V)
    res.update({"prepare_ms": prep[0], "fuse_ms": fuse[0], "fuse_ms_min": fuse[1], "fuse_blend0_ms": fuse0[0], "align_ms": align[0],
                "align_ms_min": align[1], "fuse_bytes": fuse_bytes, "align_bytes": align_bytes, "fuse_TBs": fuse_bytes / fuse[0] / 1e9,
                "align_TBs": align_bytes / align[0] / 1e9, "covered_share": float((den > 0).mean()), "mean_sum_of_weights": float(den.mean()),
                "fuse_ns_per_voxel_and_view": fuse[0] * 1e6 / (n * V)})
    print(f"{V} views of {dim[0]} x {dim[1]} x {dim[2]} into view 0's interval, blend {a.blend}:")
    print(f"  prepare (one-voxel call) {prep[0]:8.3f} ms")
    print(f"  fuse + sum of weights    {fuse[0]:8.3f} ms (min {fuse[1]:.3f})  {res['fuse_TBs']:.3f} TB/s of {fuse_bytes / 1e9:.2f} GB algorithmic")
    print(f"  fuse, blend 0            {fuse0[0]:8.3f} ms")
    print(f"  align, values + weights  {align[0]:8.3f} ms (min {align[1]:.3f})  {res['align_TBs']:.3f} TB/s of {align_bytes / 1e9:.2f} GB algorithmic")
    print(f"  for comparison: copy ceiling {COPY_CEILING_TBS} TB/s")
    if not a.no_baseline:
        res.update(torch_baseline(views, mats, dim, a.blend, a.rounds))
        print(f"  grid_sample + weighted sum {res['baseline_ms']:8.3f} ms (grids and weight volumes built beforehand in {res['baseline_setup_ms']:.1f} ms)")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
