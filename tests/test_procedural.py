"""The procedural phantom on the GPU (procedural.hip) against the literal restatement (tests/procedural_restatement.py), bit for bit:
Perlin values and rasters, sphere values and rasters, the rejection sampler and HypersphereCollectionRealRandomAccessible.main."""
import numpy as np
import pytest

from tests import procedural_restatement as R

pytestmark = pytest.mark.gpu

DIM, ORIGIN = (50, 19, 21), (-7, 0, -3)
SCALES = (3.0, 19 / 1.5, 5.25)            # x crosses the loop wrap at 45; negative positions take the mod + b branch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module", params=[((15, 15, 15), 100), ((3, 5, 2), 7)], ids=["ext15_n100", "ext352_n7"])
def perlin(request, mvs):
    ext, n = request.param
    field = mvs.PerlinNoiseRealRandomAccessible(SCALES, ext, n, mvs.JavaRandom(42))
    grad, perm = R.perlin_init(n, R.Lcg(42))
    grid = R.perlin_value(R.grid_positions(DIM, ORIGIN), SCALES, ext, grad, perm)
    return field, ext, grad, perm, grid


def test_perlin_at_bit_exact(ctx, perlin):
    field, ext, grad, perm, grid = perlin
    pos = R.grid_positions(DIM, ORIGIN)
    got = ctx.perlin_at(field._struct(), pos)
    assert np.array_equal(bits(got), bits(grid))
    rng = np.random.default_rng(5)
    far = rng.uniform(-1.0e4, 1.0e4, size=(2000, 3))
    want = R.perlin_value(far, SCALES, ext, grad, perm)
    assert np.array_equal(bits(ctx.perlin_at(field._struct(), far)), bits(want))
    assert np.ptp(want) > 0.1                                          # a field, not a constant
    assert field.get(far[3]) == want[3]                                # the mirror's get() is the same call
    assert len(ctx.perlin_at(field._struct(), np.zeros((0, 3)))) == 0


def test_perlin_raster_bit_exact(ctx, perlin):
    field, ext, grad, perm, grid = perlin
    got = ctx.perlin_raster(field._struct(), DIM, ORIGIN)
    assert got.shape == (DIM[2], DIM[1], DIM[0])
    assert np.array_equal(bits(got.ravel()), bits(grid.astype(np.float32)))
    # the device form writes the same volume
    d = ctx.dev_alloc(got.nbytes)
    try:
        ctx.perlin_raster_dev(field._struct(), DIM, ORIGIN, d)
        assert np.array_equal(bits(ctx.download(d, got.shape)), bits(got))
    finally:
        ctx.dev_free(d)


def test_perlin_threshold_raster(ctx, perlin):
    field, ext, grad, perm, grid = perlin
    assert np.abs(grid - 0.1).min() > 1e-12                            # no value on the edge: the test can neither pass nor fail by luck
    got = ctx.perlin_raster(field._struct(0.1), DIM, ORIGIN).ravel()
    assert np.array_equal(got, (grid > 0.1).astype(np.float32))
    # the reference compares the FloatType's value, (float)value > 0.1: here the same voxels
    assert np.array_equal(got, R.perlin_field(R.grid_positions(DIM, ORIGIN), SCALES, ext, grad, perm, 0.1).astype(np.float32))
    assert 0 < got.sum() < got.size
    at = ctx.perlin_at(field._struct(0.1), R.grid_positions(DIM, ORIGIN))
    assert np.array_equal(at, got.astype(np.float64))


# ---- spheres -----------------------------------------------------------------------------------------------------------------
SDIM, SORIGIN = (45, 19, 37), (0, 0, 0)                                # no multiples of the 32 x 8 x 16 brick


@pytest.fixture(scope="module")
def spheres(mvs):
    rng = np.random.default_rng(11)
    n = 300
    c = rng.uniform((-8, -6, -8), (53, 25, 45), size=(n, 3))           # partly outside the volume
    r = rng.uniform(0.0, 6.0, size=n)
    v = rng.uniform(1.0, 9.0, size=n).astype(np.float32)
    c[0], r[0], v[0] = (10.0, 5.0, 7.0), 0.0, 20.0                     # radius exactly 0 on an integer centre
    c[20:80] = rng.uniform((1, 1, 1), (30, 7, 15), size=(60, 3))       # 60 spheres in the first brick: more than one LDS chunk of 32
    r[20:80] = rng.uniform(0.5, 2.0, size=60)
    c[101], c[103] = c[100], c[102]                                    # two pairs with identical centres and different values
    r[101], r[103] = r[100], r[102] + 1.0
    c[150], r[150], v[150] = (22.0, 9.0, 18.0), 40.0, 0.5              # covers everything: lower indices win inside it, higher ones never show
    h = mvs.HypersphereCollectionRealRandomAccessible(3, -1.0)
    for i in range(n):
        h.addSphere(c[i], r[i], v[i])
    want = R.spheres_value(R.grid_positions(SDIM, SORIGIN), c, r, v, -1.0)
    return h, c, r, v, want


def test_spheres_reference_has_the_cases(spheres):
    h, c, r, v, want = spheres
    vol = want.reshape(SDIM[2], SDIM[1], SDIM[0])
    assert vol[7, 5, 10] == np.float32(20.0)                           # the radius-0 sphere owns exactly its voxel
    assert not np.any(want == -1.0)                                    # sphere 150 covers the rest ...
    assert not np.any(np.isin(want, v[151:]) & ~np.isin(want, v[:151]))   # ... so nothing behind it shows
    assert np.count_nonzero(want == np.float32(0.5)) > 100 and len(np.unique(want)) > 50


def test_spheres_at_bit_exact(ctx, spheres):
    h, c, r, v, want = spheres
    got = ctx.spheres_at(h._struct(), R.grid_positions(SDIM, SORIGIN))
    assert np.array_equal(bits(got), bits(want))
    rng = np.random.default_rng(12)
    pos = rng.uniform((-60, -60, -60), (100, 80, 100), size=(1500, 3))    # non-integer, also outside every sphere
    w2 = R.spheres_value(pos, c, r, v, -1.0)
    assert np.any(w2 == -1.0)
    assert np.array_equal(bits(ctx.spheres_at(h._struct(), pos)), bits(w2))
    assert h.get(pos[0]) == w2[0]


@pytest.mark.parametrize("cap", [1 << 28, 1024], ids=["one_range", "pair_cap_1024"])
def test_spheres_raster_bit_exact(ctx, spheres, cap):
    h, c, r, v, want = spheres
    ctx.set_option("beads_pair_cap", cap)
    try:
        got = ctx.spheres_raster(h._struct(), SDIM, SORIGIN)
        assert np.array_equal(bits(got.ravel()), bits(want))
        # Math.max over a volume that is there already
        rng = np.random.default_rng(13)
        pre = rng.uniform(-3.0, 10.0, size=got.shape).astype(np.float32)
        out = pre.copy()
        ctx.spheres_raster(h._struct(), SDIM, SORIGIN, out=out, combine=True)
        assert np.array_equal(bits(out), bits(np.maximum(pre, want.reshape(pre.shape))))
        # a raster that starts elsewhere: the positions are origin + l
        o2, d2 = (-5, 3, 9), (33, 9, 17)
        w2 = R.spheres_value(R.grid_positions(d2, o2), c, r, v, -1.0)
        assert np.array_equal(bits(ctx.spheres_raster(h._struct(), d2, o2).ravel()), bits(w2))
    finally:
        ctx.set_option("beads_pair_cap", 1 << 28)


def _pairs(c, r, dim):
    """(brick, sphere) pairs the raster bins: each sphere's box with one voxel to spare per side, in 32 x 8 x 16 bricks."""
    total = 0
    for ci, ri in zip(c, r):
        n = 1
        for d, b in enumerate((32, 8, 16)):
            lo, hi = max(int(np.floor(ci[d] - ri)) - 1, 0), min(int(np.ceil(ci[d] + ri)) + 1, dim[d] - 1)
            n *= (hi // b - lo // b + 1) if lo <= hi else 0
        total += n
    return total


@pytest.mark.parametrize("cover", [True, False], ids=["covered", "with_background"])
def test_spheres_raster_in_sphere_ranges(ctx, mvs, cover):
    """More pairs than beads_pair_cap: the raster runs in sphere ranges, and a later range must not replace a voxel an earlier one
    owns -- sphere 400 covers the volume, sphere 780 again with another value.  Without the two, the background shows, which only
    the last range may write."""
    dim, n = (70, 30, 40), 800
    rng = np.random.default_rng(31)
    c = rng.uniform((-4, -4, -4), (74, 34, 44), size=(n, 3))
    r = rng.uniform(0.0, 6.0, size=n)
    v = rng.uniform(1.0, 9.0, size=n).astype(np.float32)
    if cover:
        c[400], r[400], v[400] = (35.0, 15.0, 20.0), 50.0, 0.25
        c[780], r[780], v[780] = (35.0, 15.0, 20.0), 60.0, 0.75
    assert _pairs(c[:400], r[:400], dim) > 1024 and _pairs(c[401:780], r[401:780], dim) > 1024     # 400 and 780 in later ranges, and not in the same
    h = mvs.HypersphereCollectionRealRandomAccessible(3, -1.0)
    for i in range(n):
        h.addSphere(c[i], r[i], v[i])
    want = R.spheres_value(R.grid_positions(dim), c, r, v, -1.0)
    if cover:
        assert not np.any(want == np.float32(0.75)) and np.any(want == np.float32(0.25)) and not np.any(want == -1.0)
    else:
        assert np.any(want == -1.0) and np.any(want != -1.0)
    pre = rng.uniform(-3.0, 10.0, size=(dim[2], dim[1], dim[0])).astype(np.float32)
    res = {}
    for cap in (1 << 28, 1024):
        ctx.set_option("beads_pair_cap", cap)
        try:
            out = pre.copy()
            res[cap] = (ctx.spheres_raster(h._struct(), dim), ctx.spheres_raster(h._struct(), dim, out=out, combine=True))
        finally:
            ctx.set_option("beads_pair_cap", 1 << 28)
        assert np.array_equal(bits(res[cap][0].ravel()), bits(want))
        assert np.array_equal(bits(res[cap][1]), bits(np.maximum(pre, want.reshape(pre.shape))))


def test_spheres_without_the_covering_sphere_and_empty_set(ctx, mvs, spheres):
    """Background where no sphere reaches (bricks with an empty list included), and the empty set."""
    h, c, r, v, want = spheres
    keep = [i for i in range(len(r)) if i != 150 and not 20 <= i < 80 and c[i][2] < 20]
    g = mvs.HypersphereCollectionRealRandomAccessible(3, 2.5)
    for i in keep:
        g.addSphere(c[i], r[i], v[i])
    dim = (70, 19, 53)                                                 # bricks nothing reaches: x >= 64, z >= 32
    w = R.spheres_value(R.grid_positions(dim), c[keep], r[keep], v[keep], 2.5)
    assert np.any(w == 2.5) and np.any(w != 2.5)
    assert np.array_equal(bits(ctx.spheres_raster(g._struct(), dim).ravel()), bits(w))
    pre = np.random.default_rng(14).uniform(0.0, 5.0, size=(dim[2], dim[1], dim[0])).astype(np.float32)
    out = pre.copy()
    ctx.spheres_raster(g._struct(), dim, out=out, combine=True)
    assert np.array_equal(bits(out), bits(np.maximum(pre, w.reshape(pre.shape))))
    e = mvs.HypersphereCollectionRealRandomAccessible(3, 7.0)
    assert np.all(ctx.spheres_raster(e._struct(), SDIM) == np.float32(7.0))
    assert np.all(ctx.spheres_at(e._struct(), np.zeros((5, 3))) == np.float32(7.0))
    out = pre.copy()
    ctx.spheres_raster(e._struct(), dim, out=out, combine=True)
    assert np.array_equal(out, np.maximum(pre, np.float32(7.0)))


# ---- rejection sampling ------------------------------------------------------------------------------------------------------
MDIM = (96, 80, 24)
RMIN, RMAX = (0.0, 0.0, 0.0), (95.0, 79.0, 23.0)


@pytest.fixture(scope="module")
def sampler_cases(mvs):
    """name -> (density struct of the package, points, trials and final state of the sequential loop from new Random(7))."""
    scales, ext = (24.0, 80 / 1.5, 24.0), (15, 15, 15)
    field = mvs.PerlinNoiseRealRandomAccessible(scales, ext, 100, mvs.JavaRandom(42))
    grad, perm = R.perlin_init(100, R.Lcg(42))
    rng = np.random.default_rng(21)
    c = rng.uniform((0, 0, 0), MDIM, size=(12, 3))
    r = rng.uniform(8.0, 16.0, size=12)
    h = mvs.HypersphereCollectionRealRandomAccessible(3, 0.0)
    for i in range(12):
        h.addSphere(c[i], r[i], 1.0 if i % 2 else 0.5)                 # half the spheres accept every second trial inside them
    vals = [1.0 if i % 2 else 0.5 for i in range(12)]
    cases = {}
    for name, struct, dens, n in (("perlin_threshold", field._struct(0.1), R.perlin_density(scales, ext, grad, perm, 0.1), 50),
                                  ("perlin_raw", field._struct(), R.perlin_density(scales, ext, grad, perm), 20),
                                  ("spheres", h._struct(), R.spheres_density(c, r, vals), 300)):
        ref = R.Lcg(7)
        pts, trials = R.sample_points(RMIN, RMAX, n, dens, ref)
        cases[name] = (struct, n, pts, trials, ref.s)
    return cases


@pytest.mark.parametrize("batch", ["64", "auto"])
@pytest.mark.parametrize("name", ["perlin_threshold", "perlin_raw", "spheres"])
def test_sampler_equals_the_sequential_loop(ctx, mvs, sampler_cases, name, batch):
    struct, n, pts, trials, state = sampler_cases[name]
    assert trials > n                                                  # some trials are rejected
    if name == "spheres":
        assert trials > 5 * 64 and trials % 64 != 0                    # several batches of 64, the last one overshooting
    ctx.set_option("reject_batch", batch)
    try:
        rnd = mvs.JavaRandom(7)
        got, t = ctx.rejection_sample(RMIN, RMAX, n, struct, rnd)
        assert np.array_equal(bits(got), bits(pts)) and t == trials and rnd._s == state
        # nothing to sample: nothing drawn
        rnd = mvs.JavaRandom(7)
        s0 = rnd._s
        got, t = ctx.rejection_sample(RMIN, RMAX, 0, struct, rnd)
        assert got.shape == (0, 3) and t == 0 and rnd._s == s0
    finally:
        ctx.set_option("reject_batch", "auto")


@pytest.mark.parametrize("batch", ["64", "auto"])
def test_sampler_gives_up_after_max_trials(ctx, mvs, batch):
    e = mvs.HypersphereCollectionRealRandomAccessible(3, 0.0)          # background everywhere: the reference would never return
    ctx.set_option("reject_batch", batch)
    try:
        rnd = mvs.JavaRandom(7)
        s0 = rnd._s
        with pytest.raises(ValueError, match="max_trials"):
            ctx.rejection_sample(RMIN, RMAX, 3, e._struct(), rnd, max_trials=1000)
        assert rnd._s == s0
    finally:
        ctx.set_option("reject_batch", "auto")


def test_sampler_mirror_takes_the_loop_for_other_generators(mvs, sampler_cases):
    struct, n, pts, trials, state = sampler_cases["spheres"]

    class Plain:
        def __init__(self):
            self.r = mvs.JavaRandom(7)

        def nextDouble(self):
            return self.r.nextDouble()
    h = mvs.HypersphereCollectionRealRandomAccessible(3, 0.0)
    c, r, v = struct._keep
    for i in range(len(r)):
        h.addSphere(c[i], r[i], v[i])
    p = Plain()
    got = mvs.PointRejectionSampling.sampleRealPoints((RMIN, RMAX), 20, h, p)
    assert np.array_equal(bits(got), bits(pts[:20]))
    rnd = mvs.JavaRandom(7)
    assert np.array_equal(bits(mvs.PointRejectionSampling.sampleRealPoints((RMIN, RMAX), n, h, rnd)), bits(pts)) and rnd._s == state


def test_main_at_reduced_size(mvs):
    """HypersphereCollectionRealRandomAccessible.main through the mirror: the draws, both samplers and both rasters in sequence."""
    want, _ = R.phantom_main(MDIM, 42, 12, 200)
    got = mvs.HypersphereCollectionRealRandomAccessible.main(dim=MDIM, seed=42, nBigSpheres=12, nSmallSamples=200)
    assert got.shape == (MDIM[2], MDIM[1], MDIM[0]) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(got)) > 20 and np.any(got == 0.0) and got.max() > 4.0       # background, big and small spheres
