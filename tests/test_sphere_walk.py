"""The device-side walk of drawSpheres / multiSpheres (csrc/sphere_walk.hip, option sphere_walk) and the phantom of the refraction
simulator (mvsim_ri_noise, mvsim_multi_spheres, Context.simulate_aberration_phantom) against the host walk, the oracle's drawSpheres and
the Python restatement of tests/aberr_phantom_restatement.py.  Everything is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import aberr_phantom_restatement as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _walk:
    """the context's sphere_walk option for a block; `auto` comes back on every exit"""

    def __init__(self, ctx, how):
        self.ctx, self.how = ctx, how

    def __enter__(self):
        self.ctx.set_option("sphere_walk", self.how)

    def __exit__(self, *exc):
        self.ctx.set_option("sphere_walk", "auto")


def _draw(ctx, mvs, how, shape, scale, half, state, calls=2):
    """`calls` drawSpheres on one image and one generator: [(image bits, spheres, state)] after each"""
    img = np.zeros(shape, dtype=np.float32)
    rnd = mvs.JavaRandom(0)
    rnd._s = state
    out = []
    with _walk(ctx, how):
        for _ in range(calls):
            n = ctx.draw_spheres(img, 0.0, 1.0, scale, half, rnd)
            out.append((img.view(np.uint32).copy(), n, rnd._s))
    return out


def _assert_same_draw(ctx, mvs, shape, scale, half, state, orc=None):
    host = _draw(ctx, mvs, "host", shape, scale, half, state)
    for how in ("device", "device_only"):          # device_only: the device walk itself, no host walk behind it
        dev = _draw(ctx, mvs, how, shape, scale, half, state)
        for (hb, hn, hs), (db, dn, ds) in zip(host, dev):
            assert hn == dn and hs == ds
            assert np.array_equal(hb, db)
    if orc is not None:
        img = np.zeros(shape, dtype=np.float32)
        rnd = orc.JRandom(0)
        rnd.st.s = state
        for hb, hn, hs in host:
            assert orc.draw_spheres(img, 0.0, 1.0, scale, half, rnd) == hn
            assert rnd.st.s == hs and np.array_equal(img.view(np.uint32), hb)
    return host


@pytest.mark.parametrize("shape,scale,half", [((128, 128, 128), 1, False), ((140, 128, 130), 1, False), ((236, 236, 236), 2, True),
                                              ((96, 96, 96), 1, False)])
def test_draw_spheres_device_walk_equals_host_walk_and_oracle(ctx, mvs, orc, shape, scale, half):
    """128^3 (about 50 spheres), a canvas with three different extents, 236^3 at scale 2 with the half-pixel offset, and 96^3 whose large
    sphere has radius 0 (one voxel): image bits, sphere count and generator state, for a second call on the same image and generator too."""
    host = _assert_same_draw(ctx, mvs, shape, scale, half, R.scramble(464232194), orc)
    if shape == (128, 128, 128):
        assert 20 <= host[0][1] <= 100
    if shape == (96, 96, 96):
        assert R.large_radius(shape, 1) == 0


def _retry_state(m, scale=1, rule="draw"):
    """a generator state whose voxel m retries nextInt once while no earlier voxel is an event: the state after 3 m + 1 steps is
    ((2^31 - 1) << 17) | low, stepped backwards with the inverse multiplier"""
    inv = pow(R.MUL, -1, 1 << 48)
    for low in range(1 << 17):
        s = (((1 << 31) - 1) << 17) | low
        for _ in range(3 * m + 1):
            s = ((s - R.ADD) * inv) & R.MASK
        rnd = R.Rnd(s)
        plain = True
        for _ in range(m):
            before = rnd.steps
            rnd.nextInt(10 * scale)
            rv = rnd.nextDouble()
            plain = plain and rnd.steps - before == 3 and np.floor(rv * 10000 + 0.5) % (7 * scale) ** 3 != 0
        before = rnd.steps
        rnd.nextInt(10 * scale)
        if plain and rnd.steps - before == 2:
            return s
    raise AssertionError(f"no retry state for voxel {m} within low < 2^17")


def test_nextint_retry_at_the_chunk_boundary(ctx, mvs, orc):
    """Voxel m retries nextInt (the JDK's overflow test) for m = 0, 1 and the three values around chunk / 3, the library's real chunk."""
    chunk, entries = ctx.sphere_walk_geometry()
    assert chunk >= 512 and entries >= 6
    for m in (0, 1, chunk // 3 - 1, chunk // 3, chunk // 3 + 1):
        assert m < R.sphere_size(R.large_radius((128, 128, 128), 1))
        _assert_same_draw(ctx, mvs, (128, 128, 128), 1, False, _retry_state(m), orc)


def test_accepted_voxel_straddling_a_chunk_boundary(ctx, mvs, orc):
    """A seed whose walk accepts a voxel whose five steps lie on both sides of a chunk boundary, found with the restatement."""
    chunk, _ = ctx.sphere_walk_geometry()
    radius = R.large_radius((128, 128, 128), 1)
    for seed in range(1, 201):
        hits = [a for a in R.walk(R.Rnd(R.scramble(seed)), radius, 1, "draw") if a[4] // chunk != (a[4] + a[5] - 1) // chunk]
        if hits:
            break
    else:
        raise AssertionError("no seed in 1..200 has an accepted voxel across a chunk boundary")
    _assert_same_draw(ctx, mvs, (128, 128, 128), 1, False, R.scramble(seed), orc)


def test_ri_noise_bit_for_bit(ctx, mvs):
    """23 x 19 x 37 voxels around 0.02 (the clamp at 0 acts): the restatement's bits, the state 2 n steps on, n = 0, device == host form."""
    rng = np.random.default_rng(5)
    ri0 = (0.02 + 0.01 * rng.standard_normal((23, 19, 37))).astype(np.float32)
    state = R.scramble(7)
    want = ri0.copy()
    ref = R.Rnd(state)
    R.ri_noise(want, ref)
    assert (want == 0).sum() > 100 and (want > 0).sum() > 100
    got = ri0.copy()
    rnd = mvs.JavaRandom(7)
    ctx.ri_noise(got, rnd)
    assert np.array_equal(_bits(got), _bits(want))
    assert rnd._s == ref.s == R.jump(state, 2 * ri0.size)
    empty = np.zeros((0,), dtype=np.float32)
    ctx.ri_noise(empty, rnd)
    assert rnd._s == ref.s
    d = ctx.dev_alloc(ri0.nbytes)
    try:
        ctx.upload(d, ri0)
        st = C.c_uint64(state)
        mvs._lib.check(ctx._L.mvsim_ri_noise_dev(ctx._h, C.c_void_p(d), ri0.size, C.byref(st)))
        assert st.value == ref.s
        assert np.array_equal(_bits(ctx.download(d, ri0.shape)), _bits(want))
        mvs._lib.check(ctx._L.mvsim_ri_noise_dev(ctx._h, None, 0, C.byref(st)))
        assert st.value == ref.s
    finally:
        ctx.dev_free(d)


def _multi_canvas():
    """160^3: the index canvas pre-filled with 1.05, a box of exact 5.0 that cuts through the sphere edges, a few voxels one ulp above
    5.0; the image non-zero in one octant"""
    ri = np.full((160, 160, 160), 1.05, dtype=np.float32)
    ri[60:101, 50:90, 70:125] = np.float32(5.0)
    ri[70:80:3, 60:70:3, 80:90:3] = np.nextafter(np.float32(5.0), np.float32(6.0))
    img = np.zeros((160, 160, 160), dtype=np.float32)
    img[80:, 80:, 80:] = np.float32(0.8)
    return img, ri


@functools.lru_cache(maxsize=None)
def _multi_reference(seed):
    """the restatement's two calls on the 160^3 canvases, computed once: [(image, ri, spheres, state)]"""
    img, ri = _multi_canvas()
    rnd = R.Rnd(R.scramble(seed))
    out = []
    radii = []
    for _ in range(2):
        radii.append(R.multi_spheres(img, ri, 1, rnd))
        out.append((img.copy(), ri.copy(), len(radii[-1]), rnd.s))
    return out, radii[0]


@pytest.mark.parametrize("seed", [28, 41])
def test_multi_spheres_bit_for_bit(ctx, mvs, seed):
    """Scale 1 on 160^3 (large-sphere radius 32, 131 305 voxels): image, index volume, count and state against the restatement, for a second
    call on the same volumes too; sphere_walk = host and device_only give the same bits."""
    assert R.large_radius((160, 160, 160), 1) == 32 and R.sphere_size(32) == 131305
    want, radii = _multi_reference(seed)
    assert len(radii) >= 3 and {9, 10} <= set(radii)
    for how in ("auto", "host", "device_only"):
        img, ri = _multi_canvas()
        rnd = mvs.JavaRandom(seed)
        with _walk(ctx, how):
            for w_img, w_ri, w_n, w_s in want:
                assert ctx.multi_spheres(img, ri, 1, rnd) == w_n
                assert rnd._s == w_s
                assert np.array_equal(_bits(img), _bits(w_img))
                assert np.array_equal(_bits(ri), _bits(w_ri))


def test_multi_spheres_rejects_a_canvas_without_a_large_sphere(ctx, mvs):
    img, ri = np.zeros((64, 64, 64), np.float32), np.ones((64, 64, 64), np.float32)
    rnd = mvs.JavaRandom(1)
    with pytest.raises(ValueError, match="too small"):
        ctx.multi_spheres(img, ri, 1, rnd)
    assert rnd._s == R.scramble(1) and not img.any() and (ri == 1).all()


@functools.lru_cache(maxsize=None)
def _phantom_seed():
    """a seed for which simulate(rnd, dir) draws at least one sphere on a 236^3 canvas at scale 2: multiSpheres starts 2 * 236^3 steps in"""
    radius = R.large_radius((236, 236, 236), 2)
    for seed in range(1, 41):
        if R.walk(R.Rnd(R.jump(R.scramble(seed), 2 * 236 ** 3)), radius, 2, "multi"):
            return seed
    raise AssertionError("no seed in 1..40 draws a sphere")


def test_simulate_aberration_phantom_is_the_composition_of_its_steps(ctx, mvs, synth):
    canvas = synth.index_block(236)
    assert canvas.shape == (236, 236, 236) and (canvas == 5.0).any() and (canvas == 1.0).any()
    seed = _phantom_seed()
    rnd = mvs.JavaRandom(seed)
    img, ri = ctx.simulate_aberration_phantom(canvas, rnd, scale=2)
    assert img.shape == ri.shape == (117, 117, 117)
    step = mvs.JavaRandom(seed)
    ri1 = canvas.copy()
    ctx.ri_noise(ri1, step)
    img1 = np.zeros_like(ri1)
    assert ctx.multi_spheres(img1, ri1, 2, step) >= 1
    assert step._s == rnd._s
    assert np.array_equal(_bits(img), _bits(ctx.downsample2x(img1)))
    assert np.array_equal(_bits(ri), _bits(ctx.downsample2x(ri1)))
    assert img.max() >= 0.5


def test_facade_returns_what_the_context_returns(ctx, mvs, tmp_path):
    """SimulateMultiViewAberrations.multiSpheres / .simulatePhantom (canvas given, or block4.tif opened through Tools.open)."""
    A = mvs.SimulateMultiViewAberrations
    want, _ = _multi_reference(28)
    img, ri = _multi_canvas()
    rnd = mvs.JavaRandom(28)
    assert A.multiSpheres(img, ri, 1, rnd, ctx=ctx) == want[0][2] and rnd._s == want[0][3]
    assert np.array_equal(_bits(img), _bits(want[0][0])) and np.array_equal(_bits(ri), _bits(want[0][1]))
    _, canvas = _multi_canvas()
    a = ctx.simulate_aberration_phantom(canvas, mvs.JavaRandom(3), scale=1)
    r1, r2 = mvs.JavaRandom(3), mvs.JavaRandom(3)
    b = A.simulatePhantom(r1, ri=canvas, scale=1, ctx=ctx)
    mvs.Tools.save(canvas, str(tmp_path / "block4.tif"))
    c = A.simulatePhantom(r2, dir=str(tmp_path) + "/", scale=1, ctx=ctx)
    for got in (b, c):
        assert np.array_equal(_bits(got[0]), _bits(a[0])) and np.array_equal(_bits(got[1]), _bits(a[1]))
    assert r1._s == r2._s == R.jump(R.scramble(3), 2 * canvas.size + _steps_of_multi(canvas.shape, 1, R.jump(R.scramble(3), 2 * canvas.size)))
    with pytest.raises(ValueError):
        A.simulatePhantom(mvs.JavaRandom(1))


def _steps_of_multi(shape, scale, state):
    rnd = R.Rnd(state)
    R.walk(rnd, R.large_radius(shape, scale), scale, "multi")
    return rnd.steps
