"""Host logic of the procedural phantom (no GPU): nextGaussian() over the restated fdlibm logarithm, Collections.shuffle, the Perlin
constructor, the bound of the one deliberate difference (Math.pow as products) and the argument checks of the entry points."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import procedural_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_next_gaussian_known_answers(mvs):
    """The widely published JDK values; the first tells fdlibm's logarithm from glibc's (1.141905315473055)."""
    assert mvs.JavaRandom(42).nextGaussian() == 1.1419053154730547
    assert mvs.JavaRandom(0).nextGaussian() == 0.8025330637390305
    assert R.Lcg(42).next_gaussian() == 1.1419053154730547
    assert R.Lcg(0).next_gaussian() == 0.8025330637390305


def test_next_gaussian_sequence_matches_the_restatement(mvs):
    a, b = mvs.JavaRandom(535), R.Lcg(535)
    got = np.array([a.nextGaussian() for _ in range(1000)])
    want = np.array([b.next_gaussian() for _ in range(1000)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert a._s == b.s
    # the cached second value belongs to the state: a draw in between does not disturb it, setSeed drops it
    a, b = mvs.JavaRandom(7), R.Lcg(7)
    assert a.nextGaussian() == b.next_gaussian() and a.nextDouble() == b.next_double() and a.nextGaussian() == b.next_gaussian()
    a.nextGaussian()
    a.setSeed(7)
    assert a._pending is None and a.nextGaussian() == R.Lcg(7).next_gaussian()
    for x in (1e-300, 5e-324, 0.3, 0.9999999, 1.0, 1.0000001, 2.0, 1e10):
        assert mvs.phantoms.strict_log(x) == R.fdlibm_log(x) and abs(R.fdlibm_log(x) - math.log(x)) <= 2e-16 * max(1.0, abs(math.log(x)))


def test_shuffle_is_collections_shuffle(mvs):
    for n in (1, 2, 7, 100):
        a, b = mvs.JavaRandom(99), mvs.JavaRandom(99)
        got = list(range(n))
        a.shuffle(got)
        want = list(range(n))
        i = n
        while i > 1:                                                   # for i = size; i > 1; i--: swap(i - 1, rnd.nextInt(i))
            j = b.nextInt(i)
            want[i - 1], want[j] = want[j], want[i - 1]
            i -= 1
        assert got == want and a._s == b._s and sorted(got) == list(range(n))


@pytest.mark.parametrize("n", [100, 7])
def test_perlin_init_matches_the_restatement(mvs, n):
    """mvsim_perlin_init: gradients, permutation, final state and the cached Gaussian (7 vectors draw 21: the 22nd is pending)."""
    rnd, ref = mvs.JavaRandom(42), R.Lcg(42)
    p = mvs.PerlinNoiseRealRandomAccessible((3.0, 4.0, 5.0), (15, 15, 15), n, rnd)
    grad, perm = R.perlin_init(n, ref)
    assert np.array_equal(p.gradients.view(np.uint64), grad.view(np.uint64))
    assert np.array_equal(p.permutation, perm)
    assert rnd._s == ref.s
    assert (rnd._pending is None) == (ref.pending is None) == (n % 2 == 0)
    assert rnd.nextGaussian() == ref.next_gaussian() and rnd._s == ref.s
    # a generator that is no JavaRandom is drawn from in Python: the same tables

    class Plain:
        def __init__(self):
            self.r = mvs.JavaRandom(42)

        def nextGaussian(self):
            return self.r.nextGaussian()

        def nextInt(self, bound):
            return self.r.nextInt(bound)
    q = mvs.PerlinNoiseRealRandomAccessible((3.0, 4.0, 5.0), (15, 15, 15), n, Plain())
    assert np.array_equal(q.gradients.view(np.uint64), grad.view(np.uint64)) and np.array_equal(q.permutation, perm)


def test_pow_as_products_stays_below_the_bound():
    """The one deliberate difference: Math.pow(p, 3) * (10 - 15 p + 6 Math.pow(p, 2)) as products.  pow is within one ulp, so the
    weight moves by at most about four ulp of 1.0 on a factor |a2 - a1| <= 2 sqrt(3), over three levels: below 1e-15."""
    rnd = R.Lcg(42)
    grad, perm = R.perlin_init(100, rnd)
    scales, ext = (256.0, 1024 / 1.5, 256.0), (15, 15, 15)
    pos = np.array([[rnd.next_double() * 1023, rnd.next_double() * 1023, rnd.next_double() * 255] for _ in range(20000)])
    a = R.perlin_value(pos, scales, ext, grad, perm)
    b = R.perlin_value(pos, scales, ext, grad, perm, use_pow=True)
    diff = np.abs(a - b)
    print(f"pow vs products: {np.count_nonzero(diff) / len(diff):.4%} of values differ, max {diff.max():.3e}; field {a.min():.3f} .. {a.max():.3f}; "
          f"nearest value to 0.1: {np.abs(a - 0.1).min():.3e}")
    assert diff.max() < 1e-15
    assert np.abs(a).max() < 1.0


def test_entry_points_reject_bad_arguments(mvs):
    L = mvs._lib.load()
    chk = mvs._lib.check
    i3 = lambda *v: (C.c_int64 * 3)(*v)                                # noqa: E731
    rnd = mvs.JavaRandom(1)
    p = mvs.PerlinNoiseRealRandomAccessible((2.0, 2.0, 2.0), (15, 15, 15), 5, rnd)
    xyz = (C.c_double * 3)(0, 0, 0)
    out = (C.c_double * 8)()
    good = p._struct()
    with pytest.raises(ValueError, match="ctx is null"):               # a well-formed call gets as far as the context
        chk(L.mvsim_perlin_at(None, C.byref(good), xyz, 1, out))

    def perlin(**kw):
        f = p._struct(kw.pop("threshold", None))
        for k, v in kw.items():
            if k in ("scales", "loop_extents"):
                getattr(f, k)[:] = v
            else:
                setattr(f, k, v)
        return f
    for kw, msg in ((dict(n_vectors=0), "n_vectors"), (dict(n_vectors=-3), "n_vectors"), (dict(n_vectors=100000), "LDS"),
                    (dict(loop_extents=[15, 0, 15]), "extents"), (dict(loop_extents=[15, 15, 1 << 30]), "flatIndex"),
                    (dict(scales=[2.0, 0.0, 2.0]), "scale"), (dict(scales=[math.nan, 1.0, 2.0]), "scale"),
                    (dict(gradients=None), "null"), (dict(permutation=None), "null")):
        f = perlin(**kw)
        for call in (lambda: L.mvsim_perlin_at(None, C.byref(f), xyz, 1, out), lambda: L.mvsim_perlin_at_dev(None, C.byref(f), xyz, 1, out),
                     lambda: L.mvsim_perlin_raster(None, C.byref(f), i3(0, 0, 0), i3(2, 2, 2), out),
                     lambda: L.mvsim_perlin_raster_dev(None, C.byref(f), i3(0, 0, 0), i3(2, 2, 2), out)):
            with pytest.raises(ValueError, match=msg):
                chk(call())
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_perlin_at(None, None, xyz, 1, out))
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_perlin_at(None, C.byref(good), None, 1, out))
    with pytest.raises(ValueError, match="negative"):
        chk(L.mvsim_perlin_at(None, C.byref(good), xyz, -1, out))
    with pytest.raises(ValueError, match="finite"):
        chk(L.mvsim_perlin_at(None, C.byref(good), (C.c_double * 3)(0, math.inf, 0), 1, out))
    for dim, origin, msg in (((2, 0, 2), (0, 0, 0), "dimensions"), ((2, 2, -1), (0, 0, 0), "dimensions"), ((2, 2, 2), (0, 1 << 41, 0), "origin")):
        with pytest.raises(ValueError, match=msg):
            chk(L.mvsim_perlin_raster(None, C.byref(good), i3(*origin), i3(*dim), out))
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_perlin_raster(None, C.byref(good), i3(0, 0, 0), i3(2, 2, 2), None))
    st = C.c_uint64(5)
    g, pm = (C.c_double * 3)(), (C.c_int32 * 1)()
    with pytest.raises(ValueError, match="n_vectors"):
        chk(L.mvsim_perlin_init(C.byref(st), 0, g, pm, None))
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_perlin_init(None, 1, g, pm, None))
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_perlin_init(C.byref(st), 1, None, pm, None))
    assert st.value == 5

    def spheres(radii=(1.0, 2.0), centres=((0, 0, 0), (1, 1, 1))):
        h = mvs.HypersphereCollectionRealRandomAccessible(3, 0.0)
        for c, r in zip(centres, radii):
            h.addSphere(c, r, 1.0)
        return h._struct()
    fo = (C.c_float * 8)()
    s = spheres()
    with pytest.raises(ValueError, match="ctx is null"):
        chk(L.mvsim_spheres_at(None, C.byref(s), xyz, 1, fo))
    with pytest.raises(ValueError, match="ctx is null"):
        chk(L.mvsim_spheres_raster(None, C.byref(s), i3(0, 0, 0), i3(2, 2, 2), 1, fo))
    for s, msg in ((spheres(radii=(1.0, -0.5)), "radius"), (spheres(radii=(math.nan, 1.0)), "radius"),
                   (spheres(centres=((0, 0, 0), (0, math.inf, 0))), "centre")):
        for call in (lambda: L.mvsim_spheres_at(None, C.byref(s), xyz, 1, fo), lambda: L.mvsim_spheres_at_dev(None, C.byref(s), xyz, 1, fo),
                     lambda: L.mvsim_spheres_raster(None, C.byref(s), i3(0, 0, 0), i3(2, 2, 2), 0, fo),
                     lambda: L.mvsim_spheres_raster_dev(None, C.byref(s), i3(0, 0, 0), i3(2, 2, 2), 0, fo)):
            with pytest.raises(ValueError, match=msg):
                chk(call())
    s = spheres()
    with pytest.raises(ValueError, match="combine"):
        chk(L.mvsim_spheres_raster(None, C.byref(s), i3(0, 0, 0), i3(2, 2, 2), 2, fo))
    with pytest.raises(ValueError, match="dimensions"):
        chk(L.mvsim_spheres_raster(None, C.byref(s), i3(0, 0, 0), i3(0, 2, 2), 0, fo))
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_spheres_raster(None, None, i3(0, 0, 0), i3(2, 2, 2), 0, fo))
    s.values = None
    with pytest.raises(ValueError, match="null"):
        chk(L.mvsim_spheres_at(None, C.byref(s), xyz, 1, fo))

    s = spheres()
    d = mvs._lib.Density()
    d.kind, d.spheres = 1, C.pointer(s)
    d3 = lambda *v: (C.c_double * 3)(*v)                               # noqa: E731
    st, tr = C.c_uint64(77), C.c_int64(-1)

    def sample(state=C.byref(st), rmin=d3(0, 0, 0), rmax=d3(1, 1, 1), n=1, dens=C.byref(d), max_trials=10, dst=xyz):
        return chk(L.mvsim_rejection_sample(None, state, rmin, rmax, n, dens, max_trials, dst, C.byref(tr)))
    with pytest.raises(ValueError, match="ctx is null"):
        sample()
    for kw, msg in ((dict(state=None), "null"), (dict(dens=None), "null"), (dict(dst=None), "null"), (dict(n=-1), "n_samples"),
                    (dict(max_trials=-1), "max_trials"), (dict(rmax=d3(1, math.inf, 1)), "interval"), (dict(rmin=None), "null")):
        with pytest.raises(ValueError, match=msg):
            sample(**kw)
    d.kind = 2
    with pytest.raises(ValueError, match="kind"):
        sample()
    d.kind = 0                                                         # a Perlin density without a field
    with pytest.raises(ValueError, match="null"):
        sample()
    assert st.value == 77 and tr.value == -1


def test_procedural_host_leg_under_sanitizers(tmp_path):
    """tests/c_abi/procedural_host.c built with ASan + UBSan against libmvsim.so: mvsim_perlin_init and the argument checks, in a
    program of its own (nothing sanitized is loaded into Python)."""
    pkg = os.path.join(ROOT, "multiview-simulation_amd")
    exe = str(tmp_path / "procedural_host")
    cmd = [shutil.which("gcc") or "gcc", "-std=c99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "procedural_host.c"),
           "-L" + pkg, "-lmvsim", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lm", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0")   # the ROCm runtime keeps process-lifetime blocks
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "procedural host sanitizer run ok" in r.stdout, r.stdout + r.stderr
