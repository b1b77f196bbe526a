"""Bead registration: milliseconds per stage and for the whole call, with the fp64 operations per second the two all-pairs kernels
reach:
    python tools/bench_register.py [--beads 1000 20000] [--size 512] [--rounds 5] [--json out.json]
Per bead count: SimulateBeads' cloud in size^3 rendered under 0 and 45 degrees about x and detected on the device (default sigmas,
threshold 5); the two detection lists stay there.  Every figure is the median over --rounds of host wall time around work enqueued on
the context's stream and one synchronise.  Each stage is timed alone on the outputs of the stage before it, then the whole call.  The
capacities are the numbers of detections (a capacity far above the count still gives the same bits, but the split of the small lists
over blocks is planned from the capacity).
Counted operations, none fused: a pair of points costs k_knn 8 (3 - , 3 x, 2 +), a pair of descriptors costs k_match 17 (6 -, 6 x, 5 +);
comparisons and the bookkeeping of the sorted lists are not counted.  Beside them: what 256 CUs x 4 SIMDs issue at the 4.5 - 4.9 cycles
per fp64 wave instruction of profiles/r04_f64_rate.txt (64 lanes per instruction, 2.4 GHz): 32 - 35 T operations per second."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mvs = importlib.import_module("multiview-simulation_amd")

CEILING_TOPS = [256 * 4 * 64 * 2.4e9 / c / 1e12 for c in (4.92, 4.54)]


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


def one(ctx, beads, size, rounds, redundancy):
    dim = (size,) * 3
    interval = ((0, 0, 0), dim)
    n = size ** 3
    item = mvs.detection.PEAK_DTYPE.itemsize
    mreg = mvs.registration
    p = mvs.match_params(redundancy=redundancy)
    K = 3 + redundancy
    S = len(mvs.descriptor_subsets(redundancy))
    det = mvs.dog_params(threshold=5.0)
    pts = mvs.SimulateBeads.randomPoints(beads, interval, mvs.JavaRandom(535))
    mats = [mvs.SimulateMultiViewDataset.axisRotation(dim, 0, a) for a in (0, 45)]
    cap0 = 4 * beads
    d_img = ctx.dev_alloc(4 * n)
    peaks = [ctx.dev_alloc(item * cap0 + 8) for _ in range(2)]
    found = []
    for m, pk in zip(mats, peaks):
        ctx.render_beads_dev(pts, interval, [1, 1, 3], [d_img], None, matrices=np.asarray(m)[None])
        ctx.detect_beads_dev(d_img, np.float32, dim, cap0, pk, pk + item * cap0, det)
        found.append(int(ctx.download(pk + item * cap0, (1,), np.int64)[0]))
    detect = timed(ctx, rounds, 3, lambda: ctx.detect_beads_dev(d_img, np.float32, dim, cap0, peaks[1], peaks[1] + item * cap0, det))
    ctx.dev_free(d_img)
    cap = [max(1, min(f, mreg.MVSIM_REG_MAX_POINTS)) for f in found]
    cnt = [pk + item * cap0 for pk in peaks]
    idx = [ctx.dev_alloc(4 * K * c) for c in cap]
    d2 = [ctx.dev_alloc(8 * K * c) for c in cap]
    desc = [ctx.dev_alloc(48 * S * c) for c in cap]
    misc = ctx.dev_alloc(1024 + 25 * cap[0])
    n_desc, n_cand, d_res, d_cand, d_mask = misc, misc + 16, misc + 256, misc + 1024, misc + 1024 + 24 * cap[0]
    knn = timed(ctx, rounds, 5, lambda: ctx.knn_dev(peaks[0], item, cnt[0], cap[0], redundancy, idx[0], d2[0]))
    ctx.knn_dev(peaks[1], item, cnt[1], cap[1], redundancy, idx[1], d2[1])
    dsc = timed(ctx, rounds, 5, lambda: ctx.bead_descriptors_dev(peaks[0], item, cnt[0], cap[0], redundancy, idx[0], desc[0], n_desc))
    ctx.bead_descriptors_dev(peaks[1], item, cnt[1], cap[1], redundancy, idx[1], desc[1], n_desc + 8)
    match = timed(ctx, rounds, 3, lambda: ctx.match_descriptors_dev(desc[0], cnt[0], cap[0], desc[1], cnt[1], cap[1], redundancy, p.ratio, cap[0],
                                                                   d_cand, n_cand))
    ransac = timed(ctx, rounds, 3, lambda: ctx.ransac_affine_dev(peaks[0], item, cnt[0], cap[0], peaks[1], item, cnt[1], cap[1], d_cand, n_cand,
                                                                 cap[0], d_res, d_mask, p))
    whole = timed(ctx, rounds, 3, lambda: ctx.register_beads_dev(peaks[0], item, cnt[0], cap[0], peaks[1], item, cnt[1], cap[1], d_res, d_cand,
                                                                 d_mask, p))
    res = ctx.download(d_res, (1,), mreg.REGISTRATION_DTYPE)[0]
    described = ctx.download(n_desc, (2,), np.int64)
    for d in peaks + idx + d2 + desc + [misc]:
        ctx.dev_free(d)
    true = mreg.true_transform(mats[0], mats[1], (0, 0, 0))
    knn_ops = 8.0 * found[0] * found[0]
    match_ops = 17.0 * S * S * float(described[0]) * float(described[1])
    out = {"beads": beads, "size": size, "redundancy": redundancy, "found": found, "described": [int(v) for v in described],
           "candidates": int(res["n_candidates"]), "inliers": int(res["n_inliers"]), "flags": int(res["flags"]), "refits": int(res["refits"]),
           "mean_error": float(res["mean_error"]), "largest_matrix_entry_error": float(np.abs(res["m"].reshape(3, 4) - true).max()),
           "detect_ms": detect[0], "knn_ms": knn[0], "descriptors_ms": dsc[0], "match_ms": match[0], "ransac_ms": ransac[0],
           "register_ms": whole[0], "register_ms_min": whole[1], "knn_Tops": knn_ops / knn[0] / 1e9, "match_Tops": match_ops / match[0] / 1e9,
           "geometry": mvs.match_geometry(cap[0], cap[1], redundancy)}
    print(f"{beads} beads in {size}^3, redundancy {redundancy}: {found[0]} / {found[1]} detections, {out['described']} described, "
          f"{out['candidates']} candidates, {out['inliers']} inliers, flags {out['flags']}, matrix within {out['largest_matrix_entry_error']:.2e}")
    print(f"  detect one view       {detect[0]:8.3f} ms")
    print(f"  register (whole call) {whole[0]:8.3f} ms (min {whole[1]:.3f})")
    print(f"    k_knn + merge, A    {knn[0]:8.3f} ms  ({out['knn_Tops']:.3f} T fp64 operations per second)")
    print(f"    descriptors, A      {dsc[0]:8.3f} ms")
    print(f"    match A -> B        {match[0]:8.3f} ms  ({out['match_Tops']:.3f} T fp64 operations per second)")
    print(f"    RANSAC + refit      {ransac[0]:8.3f} ms  ({p.hypotheses} hypotheses)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beads", type=int, nargs="+", default=[1000, 20000])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--redundancy", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    with mvs.Context(0) as ctx:
        runs = [one(ctx, b, a.size, a.rounds, a.redundancy) for b in a.beads]
    res = {"runs": runs, "fp64_issue_ceiling_Tops": CEILING_TOPS}
    print(f"  for comparison: fp64 vector issue of the whole chip {CEILING_TOPS[0]:.1f} - {CEILING_TOPS[1]:.1f} T operations per second")
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
