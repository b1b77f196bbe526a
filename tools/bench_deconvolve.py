"""Multi-view deconvolution: milliseconds per view-iteration, split into its two convolutions and its two elementwise kernels,
next to two plain mvsim_convolve_dev calls timed in the same process:
    python tools/bench_deconvolve.py [--size 512] [--psf 31] [--views 7] [--iterations 2] [--rounds 5] [--json out.json]
Every figure is the median over --rounds of host wall time around work enqueued on the context's stream and one synchronise
(the launches are milliseconds long at 512^3, the enqueue costs microseconds).  The parts are timed one kernel kind at a time on the
volumes of the run; `convolve x2` is mvsim_convolve_dev with the PSF and with its flipped twin (it normalises and uploads the
31^3 PSF on every call, which the deconvolution does once).  `elementwise share` = (ratio + update) / view-iteration."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")
synth = importlib.import_module("multiview-simulation_amd.synthetic")


def timed(ctx, rounds, reps, fn):
    fn()
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--psf", type=int, default=31)
    ap.add_argument("--views", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--method", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.size ** 3
    dim = (a.size, a.size, a.size)
    rng = np.random.default_rng(1)
    with mvs.Context(0) as ctx:
        gt = synth.sphere_phantom(a.size)
        psfs = [synth.gaussian_psf(a.psf, sigma=(a.psf / 8.0 + 0.1 * v, a.psf / 7.0, a.psf / 4.0)) for v in range(a.views)]
        d_gt = ctx.dev_alloc(gt.nbytes); ctx.upload(d_gt, gt)
        d_views, d_weights = [], []
        w = rng.random(gt.shape, dtype=np.float32)
        for v in range(a.views):                               # views: the phantom blurred by each PSF; weights: one random volume per view
            d = ctx.dev_alloc(gt.nbytes); ctx.convolve_dev(d_gt, dim, psfs[v].copy(), d, method=a.method); d_views.append(d)
            d = ctx.dev_alloc(gt.nbytes); ctx.upload(d, np.roll(w, v, axis=0)); d_weights.append(d)
        d_psi, d_b, d_c = (ctx.dev_alloc(gt.nbytes) for _ in range(3))
        p = mvs.decon_params(iterations=a.iterations, method=a.method)
        steps = a.iterations * a.views
        whole = timed(ctx, a.rounds, 1, lambda: ctx.deconvolve_dev(d_views, dim, psfs, d_psi, d_weights, p))
        flipped = mvs.flip_psf(psfs[0])
        conv_p = timed(ctx, a.rounds, 3, lambda: ctx.convolve_dev(d_psi, dim, psfs[0].copy(), d_b, method=a.method))
        conv_f = timed(ctx, a.rounds, 3, lambda: ctx.convolve_dev(d_b, dim, flipped.copy(), d_c, method=a.method))
        ratio = timed(ctx, a.rounds, 10, lambda: ctx.decon_ratio_dev(d_views[0], d_b, n, 1e-6, d_b))
        update = timed(ctx, a.rounds, 10, lambda: ctx.decon_update_dev(d_psi, d_c, d_weights[0], n, 1e-4, 0.0))
        update_l = timed(ctx, a.rounds, 10, lambda: ctx.decon_update_dev(d_psi, d_c, d_weights[0], n, 1e-4, 0.006))
        for d in d_views + d_weights + [d_gt, d_psi, d_b, d_c]:
            ctx.dev_free(d)
    per = whole[0] / steps
    res = {"size": a.size, "psf": a.psf, "views": a.views, "iterations": a.iterations, "method": a.method,
           "view_iteration_ms": per, "view_iteration_ms_min": whole[1] / steps,
           "convolve_psf_ms": conv_p[0], "convolve_flipped_ms": conv_f[0], "two_convolve_dev_ms": conv_p[0] + conv_f[0],
           "ratio_ms": ratio[0], "update_ms": update[0], "update_tikhonov_ms": update_l[0],
           "ratio_GBps": 12.0 * n / ratio[0] / 1e6, "update_GBps": 16.0 * n / update[0] / 1e6,
           "elementwise_share": (ratio[0] + update[0]) / per}
    print(f"{a.size}^3, {a.psf}^3 PSFs, {a.views} views, {a.iterations} iterations, method {a.method}")
    print(f"view-iteration        {per:8.3f} ms (min {whole[1] / steps:.3f})")
    print(f"  convolve  P         {conv_p[0]:8.3f} ms")
    print(f"  convolve  flipped P {conv_f[0]:8.3f} ms     convolve x2 {conv_p[0] + conv_f[0]:8.3f} ms")
    print(f"  ratio               {ratio[0]:8.3f} ms  ({res['ratio_GBps']:.0f} GB/s of 12 B/voxel)")
    print(f"  update              {update[0]:8.3f} ms  ({res['update_GBps']:.0f} GB/s of 16 B/voxel);  with Tikhonov {update_l[0]:.3f} ms")
    print(f"  elementwise share   {res['elementwise_share']:.1%}")
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
