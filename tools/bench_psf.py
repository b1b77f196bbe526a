"""PSF extraction: milliseconds per stage and per call, the sampled voxels per second they amount to, and the same job done with
torch.nn.functional.grid_sample over the stacked windows plus a mean -- what a user has without the library:
    python tools/bench_psf.py [--size 512 512 200] [--rounds 5] [--json profiles/bench_psf.json]
One view of --size, 1 000 and 20 000 beads whose windows lie inside it, PSFs of 15^3, 31^3 and 51^3 (51^3 is the size of the
reference's own PSFs), under the identity and under 45 degrees about x.  Every figure is the median over --rounds of host wall time
around work enqueued on the context's stream and one synchronise.
  select   mvsim_psf_select_dev with the default separation of 15 voxels (the all-pairs crowding pass) and without one
  gather   mvsim_psf_gather_dev over status bytes that use every bead: the hot kernel and the addition of its partials
  finish   mvsim_psf_finish_dev
  extract  mvsim_extract_psf_dev, separation 0: the three stages on one stream
A sampled voxel is one trilinear sample (eight loads) of one tap of one bead.  The baseline builds its sampling grid (float32
positions, so it is not the same bits) inside the timed region, in slices of at most 2^26 samples, because the grid of a whole call
does not fit the device; it is given only the used beads."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")

COUNTS, KDIMS, ANGLES = (1000, 20000), (15, 31, 51), (0, 45)
SLICE = 1 << 26


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


def torch_baseline(vol, pos, off, dim, rounds):
    """grid_sample over the windows of all beads, summed slice by slice, then the mean; vol: (1, 1, Nz, Ny, Nx) on the device."""
    import torch
    import torch.nn.functional as F
    dev = vol.device
    nx, ny, nz = dim
    kz, ky, kx = off.shape[:3]
    taps = kz * ky * kx
    o = torch.from_numpy(off.reshape(taps, 3).astype(np.float32)).to(dev)
    p = torch.from_numpy(pos.astype(np.float32)).to(dev)
    scale = torch.tensor([2.0 / (nx - 1), 2.0 / (ny - 1), 2.0 / (nz - 1)], device=dev)
    per = max(1, SLICE // taps)

    def run():
        acc = torch.zeros(taps, device=dev)
        for b0 in range(0, len(p), per):
            q = p[b0:b0 + per]
            g = ((q[:, None, :] + o[None, :, :]) * scale - 1.0)[None, :, :, None, :]          # (1, beads, taps, 1, 3)
            acc += F.grid_sample(vol, g, mode="bilinear", padding_mode="border", align_corners=True)[0, 0, :, :, 0].sum(dim=0)
        return acc / len(p)

    return timed(torch.cuda.synchronize, rounds, 1, run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 200], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not a.no_baseline:
        import torch                                       # before the library is loaded: one HIP runtime in the process, torch's
        torch.cuda.init()
    dim = tuple(a.size)
    n = dim[0] * dim[1] * dim[2]
    rng = np.random.default_rng(0)
    view = rng.random((dim[2], dim[1], dim[0]), dtype=np.float32)
    res = {"size": list(dim), "geometry": mvs.psf_geometry(), "rounds": a.rounds, "cases": []}
    with mvs.Context(0) as ctx:
        img = ctx.dev_alloc(4 * n)
        ctx.upload(img, view)
        tvol = None
        if not a.no_baseline:
            tvol = torch.from_numpy(view).to("cuda")[None, None]
        cap = max(COUNTS)
        lst, cnt, st, rec = ctx.dev_alloc(24 * cap), ctx.dev_alloc(8), ctx.dev_alloc(cap), ctx.dev_alloc(72)
        tot, out = ctx.dev_alloc(8 * max(KDIMS) ** 3), ctx.dev_alloc(4 * max(KDIMS) ** 3)
        for k in KDIMS:
            for angle in ANGLES:
                m = np.asarray(mvs.SimulateMultiViewDataset.axisRotation(dim, 0, angle), np.float64).reshape(3, 4) if angle else None
                margin = np.array([k // 2 + 1, 0.75 * k + 1, 0.75 * k + 1])
                for count in COUNTS:
                    pos = margin + rng.random((count, 3)) * (np.array(dim) - 1 - 2 * margin)
                    ctx.upload(lst, pos)
                    ctx.upload(cnt, np.array([count], np.int64))
                    p0 = mvs.psf_params(kdim=k, min_separation=0)
                    p15 = mvs.psf_params(kdim=k)
                    args = (lst, 24, cnt, count)
                    sel15 = timed(ctx.synchronize, a.rounds, 3, lambda: ctx.psf_select_dev(*args, dim, st, rec, m=m, params=p15))
                    sel0 = timed(ctx.synchronize, a.rounds, 3, lambda: ctx.psf_select_dev(*args, dim, st, rec, m=m, params=p0))
                    record = ctx.download(rec, (1,), mvs.psf.PSF_RESULT_DTYPE)[0]
                    reps = 3 if count * k ** 3 < 1 << 30 else 1
                    gat = timed(ctx.synchronize, a.rounds, reps, lambda: ctx.psf_gather_dev(img, dim, *args, st, tot, m=m, params=p0))
                    fin = timed(ctx.synchronize, a.rounds, 3, lambda: ctx.psf_finish_dev(tot, out, rec, p0))
                    ctx.psf_select_dev(*args, dim, st, rec, m=m, params=p0)                   # the record again as the selection leaves it
                    whole = timed(ctx.synchronize, a.rounds, reps, lambda: ctx.extract_psf_dev(img, dim, *args, out, rec, m=m, params=p0))
                    samples = float(record["n_used"]) * k ** 3
                    case = {"kdim": k, "angle": angle, "beads": count, "n_used": int(record["n_used"]), "select_sep15_ms": sel15[0],
                            "select_sep0_ms": sel0[0], "gather_ms": gat[0], "gather_ms_min": gat[1], "finish_ms": fin[0], "extract_ms": whole[0],
                            "extract_ms_min": whole[1], "sampled_voxels": samples, "gather_Gsamples_per_s": samples / gat[0] / 1e6,
                            "extract_Gsamples_per_s": samples / whole[0] / 1e6}
                    if tvol is not None:
                        base = torch_baseline(tvol, pos, mvs.psf_offsets(m, (k, k, k)), dim, a.rounds)
                        case.update({"baseline_ms": base[0], "baseline_ms_min": base[1]})
                    res["cases"].append(case)
                    print(f"kdim {k:2d}^3 angle {angle:2d} beads {count:5d} (used {case['n_used']:5d}): select {sel15[0]:7.3f} ms (no separation "
                          f"{sel0[0]:.3f}), gather {gat[0]:8.3f} ms = {case['gather_Gsamples_per_s']:7.1f} Gsamples/s, finish {fin[0]:6.3f} ms, "
                          f"whole call {whole[0]:8.3f} ms" + (f", grid_sample + mean {case['baseline_ms']:9.3f} ms" if tvol is not None else ""), flush=True)
        for d in (img, lst, cnt, st, rec, tot, out):
            ctx.dev_free(d)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
