"""The bead registration without a GPU: the library's host helpers (rank triples, defaults, struct sizes, geometry, mvsim_fit_affine,
every refusal) against the restatement of tests/register_reference.py, and the recipe on its own through the restatement -- a planted
affine under outliers, a rotated and cropped cloud, and detections of the detector's restatement registered from the detections alone."""
import ctypes as C
import math

import numpy as np
import pytest

from . import dog_reference as D
from . import register_reference as R

F64 = np.float64
LOOP_SEED, LOOP_BEADS, LOOP_INTERVAL = 11, 40, ((0, 0, 0), (128, 128, 96))


def loop_cloud(mvs):
    """The cloud of the closed loop (here and in tests/test_register.py): LOOP_BEADS beads at least 12 voxels apart and 8 from every face
    of 128 x 128 x 96 under the identity and under 45 degrees about x.  Returns (points, [matrix A, matrix B])."""
    mats = [np.asarray(mvs.SimulateMultiViewDataset.axisRotation((128, 128, 96), 0, a), F64).reshape(3, 4) for a in (0, 45)]
    hi = np.array([127.0, 127.0, 95.0])

    def keeps_margin(p):
        return all(np.all(q >= 8) and np.all(q <= hi - 8) for q in (mvs.beads.apply_affine(m, p) for m in mats))

    return D.draw_positions((96, 128, 128), LOOP_BEADS, np.random.default_rng(LOOP_SEED), accept=keeps_margin), mats


def true_pairs(cand, perm):
    """perm[b] = the point of A that point b of B is: which candidates pair a point with itself."""
    return perm[cand["b"]] == cand["a"]


# ---- host helpers ----------------------------------------------------------------------------------------------------------------------
def test_subsets_defaults_sizes_and_geometry(mvs):
    for r, S in ((0, 1), (1, 4), (2, 10)):
        got = mvs.descriptor_subsets(r)
        assert got.dtype == np.int32 and np.array_equal(got, R.subsets(3 + r)) and len(got) == S
    p = mvs.match_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    q = mvs.match_params(redundancy=2, seed=-5, ratio=2.0)
    assert (q.redundancy, q.seed, q.ratio, q.hypotheses) == (2, -5, 2.0, 10000)
    with pytest.raises(TypeError):
        mvs.match_params(bogus=1)
    reg = mvs.registration
    assert C.sizeof(mvs.MatchParams) == 48
    assert C.sizeof(mvs._lib.Match) == 24 == reg.MATCH_DTYPE.itemsize == R.MATCH_DTYPE.itemsize
    assert C.sizeof(mvs._lib.Registration) == 160 == reg.REGISTRATION_DTYPE.itemsize == R.REGISTRATION_DTYPE.itemsize
    assert reg.MATCH_DTYPE == R.MATCH_DTYPE and reg.REGISTRATION_DTYPE == R.REGISTRATION_DTYPE
    assert (mvs._lib.MVSIM_REG_MAX_POINTS, mvs._lib.MVSIM_REG_FIT_CHUNK) == (R.MAX_POINTS, R.FIT_CHUNK)
    assert (mvs._lib.MVSIM_REG_FEW_CANDIDATES, mvs._lib.MVSIM_REG_NO_MODEL, mvs._lib.MVSIM_REG_CAPPED, mvs._lib.MVSIM_REG_FEW_INLIERS) == \
           (R.FEW_CANDIDATES, R.NO_MODEL, R.CAPPED, R.FEW_INLIERS)
    # the split rule of the header, restated
    for cap_a, cap_b, r in ((1, 1, 0), (64, 65, 1), (1000, 1000, 1), (2048, 2048, 0), (2049, 700, 2), (65536, 65536, 2), (20000, 30000, 1)):
        g = mvs.match_geometry(cap_a, cap_b, r)
        assert g["queries"] == 64 and g["knn_tile"] >= 16 and g["match_tile"] >= 8 and g["ransac_tile"] >= 64
        S = (3 + r) * (2 + r) * (1 + r) // 6
        for lanes, pts, tile, key in ((cap_a, cap_a, g["knn_tile"], "knn"), (cap_a * S, cap_b, g["match_tile"], "match")):
            Q, T = -(-lanes // g["queries"]), -(-pts // tile)
            want = min(T, max(1, -(-1024 // Q)))
            per = -(-T // want)
            assert (g[key + "_splits"], g[key + "_tiles_per_split"]) == (-(-T // per), per), (cap_a, cap_b, r, key)
    assert mvs._lib.load().mvsim_match_geometry(8, 8, 1, None) == mvs._lib.MVSIM_EINVAL


def test_java_random_draws_of_the_restatement(mvs):
    """The vectorised generator of the restatement against the package's JavaRandom, bounds that are and are not powers of two."""
    for seed, M in ((0, 4), (7, 5), (-3, 256), (2 ** 40 + 1, 2000), (99, 3 << 29)):
        h = np.arange(6)
        idx, void = R.draw4(seed, h, M)
        for k in h:
            rnd, have = mvs.JavaRandom(seed + int(k)), []
            for _ in range(R.MAX_DRAWS):
                v = rnd.nextInt(M)
                if v not in have:
                    have.append(v)
                if len(have) == 4:
                    break
            assert bool(void[k]) == (len(have) < 4)
            if len(have) == 4:
                assert sorted(have) == idx[k].tolist(), (seed, M, k)


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 1000])
def test_fit_affine_equals_the_restatement_bit_for_bit(mvs, n):
    rng = np.random.default_rng(n)
    p = rng.uniform(0, 500, (n, 3))
    A = np.array([[0.9, -0.3, 0.1], [0.2, 1.1, -0.4], [0.05, 0.3, 0.8]])
    q = p @ A.T + np.array([10.0, -20.0, 5.0]) + rng.normal(0, 0.1, (n, 3))
    masks = [None, np.ones(n, np.uint8)]
    if n > 8:
        masks += [(rng.random(n) < 0.5).astype(np.uint8), (np.arange(n) >= n - 5).astype(np.uint8), (np.arange(n) % 97 == 0).astype(np.uint8)]
    for mask in masks:
        got, want = mvs.fit_affine(p, q, mask), R.fit_affine(p, q, mask)
        if want is None:
            assert got is None
        else:
            assert got is not None and R.same_bits(got.reshape(-1), want)
    full = mvs.fit_affine(p, q)
    assert np.abs(full[:, :3] - A).max() < 0.05 if n >= 255 else True
    assert mvs.fit_affine(p, q, np.zeros(n, np.uint8)) is None            # fewer than 4 selected


def test_fit_affine_without_a_model(mvs):
    rng = np.random.default_rng(1)
    flat = rng.uniform(0, 100, (50, 3))
    flat[:, 2] = 7.0                                                      # coplanar: Sm is singular
    same = np.tile(rng.uniform(0, 100, (1, 3)), (30, 1))                  # repeated: Sm is zero
    q = rng.uniform(0, 100, (50, 3))
    for p in (flat, same, flat[:3]):
        assert R.fit_affine(p, q[:len(p)]) is None and mvs.fit_affine(p, q[:len(p)]) is None
    bad = flat.copy()
    bad[3, 1] = np.nan
    assert R.fit_affine(bad, q) is None and mvs.fit_affine(bad, q) is None
    L = mvs._lib.load()
    m, has, buf = (C.c_double * 12)(), C.c_int(0), (C.c_double * 12)()
    ptr = C.c_void_p(C.addressof(buf))
    for args in ((None, ptr, None, 4, m, C.byref(has)), (ptr, None, None, 4, m, C.byref(has)), (ptr, ptr, None, 4, None, C.byref(has)),
                 (ptr, ptr, None, 4, m, None), (ptr, ptr, None, -1, m, C.byref(has)), (ptr, ptr, None, R.MAX_POINTS + 1, m, C.byref(has))):
        assert L.mvsim_fit_affine(*args) == mvs._lib.MVSIM_EINVAL


def test_every_refusal_is_reachable_without_a_device(mvs):
    """A null context is the LAST thing every entry point looks at."""
    L, EINVAL = mvs._lib.load(), mvs._lib.MVSIM_EINVAL
    buf = (C.c_char * 64)()
    ptr = C.c_void_p(C.addressof(buf))                     # never dereferenced: no call gets as far as a launch

    def msg():
        return (L.mvsim_last_error() or b"").decode()

    def refused(fn, good, bad_sets):
        assert fn(None, *good) == EINVAL and "ctx" in msg(), (fn.__name__, msg())
        for at, values in bad_sets.items():
            for v in values:
                args = list(good)
                args[at] = v
                assert fn(None, *args) == EINVAL, (fn.__name__, at, v)
                assert "ctx" not in msg(), (fn.__name__, at, v, msg())

    strides, caps = (0, 16, 23, 28, -24), (0, -1, R.MAX_POINTS + 1)
    ok = mvs.match_params()
    bad_params = [None] + [C.byref(mvs.match_params(**kw)) for kw in (
        dict(redundancy=-1), dict(redundancy=3), dict(ratio=0.99), dict(ratio=math.nan), dict(ratio=math.inf), dict(max_epsilon=0.0),
        dict(max_epsilon=-1.0), dict(max_epsilon=math.nan), dict(max_epsilon=math.inf), dict(min_inlier_ratio=math.nan),
        dict(min_inlier_ratio=math.inf), dict(hypotheses=0), dict(hypotheses=-4), dict(max_refits=-1), dict(max_refits=4097), dict(min_inliers=3))]
    refused(L.mvsim_knn_dev, (ptr, 24, ptr, 8, 1, ptr, ptr), {0: [None], 1: strides, 2: [None], 3: caps, 4: [-1, 3], 5: [None], 6: [None]})
    refused(L.mvsim_bead_descriptors_dev, (ptr, 40, ptr, 8, 1, ptr, ptr, ptr),
            {0: [None], 1: strides, 2: [None], 3: caps, 4: [-1, 3], 5: [None], 6: [None], 7: [None]})
    refused(L.mvsim_match_descriptors_dev, (ptr, ptr, 8, ptr, ptr, 8, 1, 3.0, 8, ptr, ptr),
            {0: [None], 1: [None], 2: caps, 3: [None], 4: [None], 5: caps, 6: [-1, 3], 7: [0.5, math.nan, math.inf], 8: caps, 9: [None], 10: [None]})
    refused(L.mvsim_ransac_affine_dev, (ptr, 24, ptr, 8, ptr, 40, ptr, 8, ptr, ptr, 8, C.byref(ok), ptr, None),
            {0: [None], 1: strides, 2: [None], 3: caps, 4: [None], 5: strides, 6: [None], 7: caps, 8: [None], 9: [None], 10: caps,
             11: bad_params, 12: [None]})
    refused(L.mvsim_register_beads_dev, (ptr, 24, ptr, 8, ptr, 40, ptr, 8, C.byref(ok), ptr, None, None),
            {0: [None], 1: strides, 2: [None], 3: caps, 4: [None], 5: strides, 6: [None], 7: caps, 8: bad_params, 9: [None]})
    refused(L.mvsim_register_beads, (ptr, 24, 2, ptr, 40, 1, C.byref(ok), ptr, None, None),
            {0: [None], 1: strides, 2: [-1, R.MAX_POINTS + 1], 3: [None], 4: strides, 5: [-1, R.MAX_POINTS + 1], 6: bad_params, 7: [None]})
    n = C.c_int(0)
    assert L.mvsim_descriptor_subsets(3, (C.c_int32 * 30)(), C.byref(n)) == EINVAL
    assert L.mvsim_descriptor_subsets(1, None, C.byref(n)) == EINVAL and L.mvsim_descriptor_subsets(1, (C.c_int32 * 30)(), None) == EINVAL


# ---- the recipe on its own ----------------------------------------------------------------------------------------------------------------
def planted(rng, M, outlier_share, noise=0.05):
    """M candidates over M + M points: the inliers follow one affine with Gaussian noise, the planted outliers go anywhere."""
    A = np.array([[0.8, -0.5, 0.1], [0.45, 0.85, -0.2], [0.0, 0.25, 0.95]])
    t = np.array([30.0, -12.0, 4.0])
    pa = rng.uniform(0, 400, (M, 3))
    pb = pa @ A.T + t + rng.normal(0, noise, (M, 3))
    out = rng.random(M) < outlier_share
    pb[out] = rng.uniform(-200, 600, (int(out.sum()), 3))
    cand = np.zeros(M, R.MATCH_DTYPE)
    cand["a"] = cand["b"] = np.arange(M)
    return pa, pb, cand, ~out, np.hstack([A, t[:, None]])


def test_planted_affine_is_recovered_under_outliers():
    rng = np.random.default_rng(5)
    pa, pb, cand, inlier, truth = planted(rng, 300, 0.3)
    res, mask = R.ransac_refit(pa, pb, cand, R.params(hypotheses=200, max_epsilon=1.0))
    print(f"{int(mask.sum())} inliers of {int(inlier.sum())} planted, refits {res['refits']}, flags {res['flags']}, best {res['best_hypothesis']}")
    assert res["flags"] == 0 and np.array_equal(mask.astype(bool), inlier) and res["n_inliers"] == inlier.sum()
    assert np.abs(res["m"].reshape(3, 4) - truth).max() < 0.05 and res["max_error"] <= 1.0 and 0 < res["mean_error"] < 0.3


def rotated_cloud(seed=2, n=60, box=(128, 128, 96), deg=45.0, noise=0.03):
    """n random points in `box`; view A sees those 8 voxels inside the box, view B those that are after a rotation about x through the
    centre; positions carry Gaussian noise, B's list is shuffled.  Returns (A, B, perm): perm[b] = index in A of B's point b, or -1."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, (n, 3)) * (np.array(box, F64) - 1)
    rot = R.apply(R.rotation_x(deg, (np.array(box, F64) - 1) / 2), pts)
    in_a, in_b = R.inside(pts, box, 8), R.inside(rot, box, 8)
    A = pts[in_a] + rng.normal(0, noise, (int(in_a.sum()), 3))
    ids_a = np.nonzero(in_a)[0]
    order = rng.permutation(int(in_b.sum()))
    B = (rot[in_b] + rng.normal(0, noise, (int(in_b.sum()), 3)))[order]
    ids_b = np.nonzero(in_b)[0][order]
    where = {int(g): i for i, g in enumerate(ids_a)}
    return A, B, np.array([where.get(int(g), -1) for g in ids_b])


def test_rotated_cropped_cloud_registers_from_true_pairs_only():
    A, B, perm = rotated_cloud()
    common = int((perm >= 0).sum())
    out = R.register(A, B, R.params(max_epsilon=1.0, hypotheses=300, min_inliers=4))
    cand, res, mask = out["candidates"], out["result"], out["mask"].astype(bool)
    true = true_pairs(cand, perm)
    print(f"{len(A)} / {len(B)} points, {common} common, {len(cand)} candidates ({int(true.sum())} true), {int(mask.sum())} inliers, flags {res['flags']}")
    assert len(cand) >= 8 and res["n_inliers"] >= 8 and not res["flags"] & (R.NO_MODEL | R.FEW_CANDIDATES)
    assert np.all(true[mask]), "an inlier is no true pair"
    # points without a partner in the other view: at least 4 have no candidate or are dropped
    lonely = np.setdiff1d(np.arange(len(A)), perm[perm >= 0])
    assert len(lonely) >= 4
    kept = set(cand["a"][mask].tolist())
    assert sum(1 for a in lonely if a not in kept) >= 4 and not kept & set(lonely.tolist())


def test_detections_of_the_detector_restatement_register(mvs):
    """Two numpy-rendered volumes of one cloud, the second turned by 90 degrees about x (a 96 x 80 x 80 box maps onto itself), through the
    detector's restatement and then the registration's: the rotation comes back from the detections alone."""
    shape = (80, 80, 96)
    rng = np.random.default_rng(21)
    pts = D.draw_positions(shape, 24, rng)
    turn = R.rotation_x(90.0, (47.5, 39.5, 39.5))
    views = [pts, R.apply(turn, pts)]
    det = [D.detect(D.render_beads(shape, v), threshold=5)[0] for v in views]
    assert len(det[0]) == len(det[1]) == 24
    out = R.register(det[0]["pos"], det[1]["pos"], R.params(max_epsilon=1.0, hypotheses=200))
    res, cand, mask = out["result"], out["candidates"], out["mask"].astype(bool)
    print(f"{len(cand)} candidates, {int(mask.sum())} inliers, mean error {res['mean_error']:.4f}, flags {res['flags']}")
    assert res["flags"] == 0 and res["n_inliers"] >= 12
    moved = R.apply(res["m"], views[0])
    assert np.abs(moved - views[1]).max() < 0.5
    near_a = np.argmin(((det[0]["pos"][:, None] - views[0][None]) ** 2).sum(-1), axis=1)
    near_b = np.argmin(((det[1]["pos"][:, None] - views[1][None]) ** 2).sum(-1), axis=1)
    assert np.all(near_a[cand["a"][mask]] == near_b[cand["b"][mask]]), "an inlier pairs two different beads"


def test_loop_cloud_gives_enough_true_candidates_from_true_positions(mvs):
    """The cloud of the GPU closed loop, checked here: from the TRUE positions of both views the restatement finds at least 16
    candidates and every one is a true pair."""
    pts, mats = loop_cloud(mvs)
    views = [mvs.beads.apply_affine(m, pts) for m in mats]
    sep = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1) + np.eye(len(pts)) * 1e9).min()
    assert len(pts) == LOOP_BEADS and sep >= 12
    K = 3 + R.DEFAULTS["redundancy"]
    desc = [R.descriptors(v, R.knn(v, K)[0]) for v in views]
    cand = R.match(desc[0], desc[1], R.DEFAULTS["ratio"])
    print(f"{len(cand)} candidates from {LOOP_BEADS} beads")
    assert len(cand) >= 16 and np.all(cand["a"] == cand["b"])
