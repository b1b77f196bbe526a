"""Bead detection: milliseconds per kernel kind and for the whole call, with the bytes per second each pass reaches on its algorithmic
traffic:
    python tools/bench_detect.py [--size 512] [--beads 20000] [--rounds 5] [--json out.json]
A float volume of size^3 with `beads` Gaussians of sigma (1, 1, 3) on a Poisson background, default sigmas, threshold 5.  Every figure is
the median over --rounds of host wall time around work enqueued on the context's stream and one synchronise.  Each kernel kind is
timed alone in the same process (option dog_pass = xy | z launches one DoG kernel without the other), then the whole call.
Algorithmic bytes per voxel: xy 4 read + 8 written, z 8 read + 4 written, peaks 4 read + 1/4 for the ballot words written and
read back (the 26 neighbours of a candidate come from cache), the halos not counted.  Beside them: the 4.7-5.0 TB/s of the library's elementwise
kernels and the 6.3 TB/s copy ceiling."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")


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
    ap.add_argument("--beads", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.size ** 3
    dim = (a.size,) * 3
    interval = ((0, 0, 0), dim)
    cap = 4 * a.beads
    item = mvs.detection.PEAK_DTYPE.itemsize
    p = mvs.dog_params(threshold=5.0)
    with mvs.Context(0) as ctx:
        pts = mvs.SimulateBeads.randomPoints(a.beads, interval, mvs.JavaRandom(535))
        d_img, d_u16, d_dog = ctx.dev_alloc(4 * n), ctx.dev_alloc(2 * n), ctx.dev_alloc(4 * n)
        d_list, d_peaks = ctx.dev_alloc(8 * cap + 8), ctx.dev_alloc(item * cap + 8)
        ctx.render_beads_dev(pts, interval, [1, 1, 3], [d_img], [d_u16])
        ctx.synchronize()
        res = {"size": a.size, "beads": a.beads, "capacity": cap}
        whole = timed(ctx, a.rounds, 3, lambda: ctx.detect_beads_dev(d_img, np.float32, dim, cap, d_peaks, d_peaks + item * cap, p))
        whole16 = timed(ctx, a.rounds, 3, lambda: ctx.detect_beads_dev(d_u16, np.uint16, dim, cap, d_peaks, d_peaks + item * cap, p))
        res["found"] = int(ctx.download(d_peaks + item * cap, (1,), np.int64)[0])
        dog = timed(ctx, a.rounds, 5, lambda: ctx.dog_dev(d_img, np.float32, dim, d_dog, p))
        ctx.set_option("dog_pass", "xy")
        xy = timed(ctx, a.rounds, 5, lambda: ctx.dog_dev(d_img, np.float32, dim, d_dog, p))
        xy16 = timed(ctx, a.rounds, 5, lambda: ctx.dog_dev(d_u16, np.uint16, dim, d_dog, p))
        ctx.set_option("dog_pass", "z")
        z = timed(ctx, a.rounds, 5, lambda: ctx.dog_dev(d_img, np.float32, dim, d_dog, p))
        ctx.set_option("dog_pass", "both")
        ctx.dog_dev(d_img, np.float32, dim, d_dog, p)
        peaks = timed(ctx, a.rounds, 5, lambda: ctx.find_peaks_dev(d_dog, dim, 5.0, cap, d_list, d_list + 8 * cap))
        loc = timed(ctx, a.rounds, 5, lambda: ctx.localise_peaks_dev(d_dog, dim, d_list, d_list + 8 * cap, cap, 4, d_peaks))
        for d in (d_img, d_u16, d_dog, d_list, d_peaks):
            ctx.dev_free(d)
    tb = lambda bytes_per_voxel, ms: bytes_per_voxel * n / ms / 1e9
    res.update({"detect_ms": whole[0], "detect_ms_min": whole[1], "detect_u16_ms": whole16[0], "dog_ms": dog[0],
                "xy_ms": xy[0], "xy_TBps": tb(12, xy[0]), "xy_u16_ms": xy16[0], "xy_u16_TBps": tb(10, xy16[0]),
                "z_ms": z[0], "z_TBps": tb(12, z[0]), "peaks_ms": peaks[0], "peaks_TBps": tb(4.25, peaks[0]), "localise_ms": loc[0],
                "reference_elementwise_TBps": [4.7, 5.0], "reference_copy_TBps": 6.3})
    print(f"{a.size}^3 float, {a.beads} beads, default sigmas, {res['found']} found (capacity {cap})")
    print(f"detect (whole call)   {whole[0]:8.3f} ms (min {whole[1]:.3f});  uint16 source {whole16[0]:.3f} ms")
    print(f"  DoG, both kernels   {dog[0]:8.3f} ms")
    print(f"    xy kernel         {xy[0]:8.3f} ms  ({res['xy_TBps']:.2f} TB/s of 12 B/voxel);  uint16 {xy16[0]:.3f} ms ({res['xy_u16_TBps']:.2f} TB/s of 10 B/voxel)")
    print(f"    z kernel          {z[0]:8.3f} ms  ({res['z_TBps']:.2f} TB/s of 12 B/voxel)")
    print(f"  peaks (count, scan, emit) {peaks[0]:8.3f} ms  ({res['peaks_TBps']:.2f} TB/s of 4.25 B/voxel)")
    print(f"  localise            {loc[0]:8.3f} ms  ({cap} lanes, {min(res['found'], cap)} fits)")
    print("  for comparison: elementwise kernels of the deconvolution 4.7-5.0 TB/s, copy ceiling 6.3 TB/s")
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
