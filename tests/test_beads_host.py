"""Host logic of the bead simulators (no GPU): java.util.Random replay, Java rounding, kernel diameters, isInsideAdjust, the
restated AffineTransform3D and the argument checks of the bead entry points."""
import ctypes as C
import math

import numpy as np
import pytest


def _jdk_next_double(seed, count):
    """java.util.Random.nextDouble() from the JDK specification, written out independently of the package."""
    s = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)
    out = []
    for _ in range(count):
        parts = []
        for bits in (26, 27):
            s = (s * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
            parts.append(s >> (48 - bits))
        out.append(((parts[0] << 27) + parts[1]) / float(1 << 53))
    return out, s


def test_random_points_replay_java_util_random(mvs):
    rng = ((-512, -512, -512), (512, 512, 512))
    u, state = _jdk_next_double(535, 30)
    want = np.array([u[3 * i + d] * 1024.0 + (-512.0) for i in range(10) for d in range(3)]).reshape(10, 3)
    r1 = mvs.JavaRandom(535)
    got = mvs.SimulateBeads.randomPoints(10, rng, r1)                  # native replay
    assert np.array_equal(got, want)
    assert r1._s == state

    class Plain:                                                       # any object with nextDouble(): drawn in Python
        def __init__(self):
            self.r = mvs.JavaRandom(535)

        def nextDouble(self):
            return self.r.nextDouble()
    p = Plain()
    assert np.array_equal(mvs.SimulateBeads.randomPoints(10, rng, p), want)
    assert p.r._s == state
    # the C ABI advances the caller's state exactly as far
    L = mvs._lib.load()
    st = C.c_uint64(mvs.JavaRandom(535)._s)
    xyz = (C.c_double * 30)()
    assert L.mvsim_beads_random_points(C.byref(st), 10, (C.c_int64 * 3)(*rng[0]), (C.c_int64 * 3)(*rng[1]), xyz) == 0
    assert st.value == state and np.array_equal(np.array(xyz).reshape(10, 3), want)
    # SimulateBeads.main's first point: new Random(535), range 512 x 512 x 200
    first = mvs.SimulateBeads.randomPoints(1, ((0, 0, 0), (511, 511, 199)), mvs.JavaRandom(535))[0]
    assert np.array_equal(first, [u[0] * 511.0, u[1] * 511.0, u[2] * 199.0])


def test_java_round(mvs):
    jr = mvs.beads.java_round
    assert [jr(v) for v in (2.5, -2.5, 0.5, -0.5, 1.5, -1.5)] == [3, -2, 1, 0, 2, -1]
    assert jr(0.49999999999999994) == 0 and jr(-0.49999999999999994) == 0
    assert jr(float("nan")) == 0 and jr(1e300) == (1 << 63) - 1 and jr(-1e300) == -(1 << 63)
    jf = mvs.beads.java_round_float
    got = jf(np.array([2.5, -2.5, 0.5, -0.5, np.float32(0.49999997), np.nan, 3e9, -3e9, 65535.5], dtype=np.float32))
    assert got.tolist() == [3, -2, 1, 0, 0, 0, 2147483647, -2147483648, 65536]
    assert mvs.beads.to_unsigned_short(np.array([65535.5, 70000.2, -1.0], dtype=np.float32)).tolist() == [0, 4464, 65535]


def test_kernel_diameter(mvs):
    kd = mvs.beads.kernel_diameter
    assert [kd(s) for s in (0.3, 0.5, 1.0, 3.0, 6.2)] == [3, 5, 7, 19, 39]
    assert kd(0.0) == 3 and kd(-1.0) == 3


def test_is_inside_adjust_mutates_up_to_the_first_failing_axis(mvs):
    sb = mvs.SimulateBeads
    interval = ((2, 3, 4), (12, 13, 14))
    p = [5.0, 100.0, 9.0]
    assert not sb.isInsideAdjust(p, interval)
    assert p == [3.0, 97.0, 9.0]                                       # z untouched: the check stopped at y
    p = [12.0, 13.0, 14.0]                                             # exactly max: kept (p - min == max - min)
    assert sb.isInsideAdjust(p, interval) and p == [10.0, 10.0, 10.0]
    p = [1.9, 5.0, 5.0]
    assert not sb.isInsideAdjust(p, interval) and p == [-0.10000000000000009, 5.0, 5.0]
    arr = np.array([[5.0, 100.0, 9.0], [12.0, 13.0, 14.0]])
    assert np.array_equal(mvs.beads._adjust(arr, *interval), [[3.0, 97.0, 9.0], [10.0, 10.0, 10.0]])


def test_affine_transform3d(mvs):
    A = mvs.AffineTransform3D
    t = A().translate([10.5, -3.25, 7.0])
    inv = t.inverse()
    assert np.array_equal(inv.m, [[1, 0, 0, -10.5], [0, 1, 0, 3.25], [0, 0, 1, -7.0]])
    r = A().rotate(1, mvs.beads.to_radians(90))
    c, s = math.cos(90 * 0.017453292519943295), math.sin(90 * 0.017453292519943295)
    assert np.array_equal(r.m, [[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0]])
    assert mvs.beads.to_radians(90) == 1.5707963267948966
    # SimulateBeads2 composes tp -> angle -> channel -> illumination -> tile, each pre-concatenated: T = tile * ill * ch * angle * tp
    sb = mvs.SimulateBeads2.__new__(mvs.SimulateBeads2)
    sb.tpTransforms, sb.angleTransforms, sb.channelTransforms, sb.illumTransforms, sb.tileTransforms = {}, {}, {}, {}, {}
    sb.addTimepoint(0, [1, 0, 0])
    sb.addAngle(0, 2, 90)
    sb.addChannel(0, [0, 2, 0])
    sb.addIllumination(0, [0, 0, 3])
    sb.addTile(0, [5, 0, 0])
    m = sb.transform(0, 0, 0, 0, 0).m
    full = lambda a: np.vstack([a, [0, 0, 0, 1]])                      # noqa: E731
    parts = [sb.tpTransforms[0], sb.angleTransforms[0], sb.channelTransforms[0], sb.illumTransforms[0], sb.tileTransforms[0]]
    want = np.eye(4)
    for p in parts:
        want = full(p.m) @ want
    assert np.allclose(m, want[:3], atol=1e-15)
    # the point (0, 0, 0): +x 1 (tp), rotate about z by 90 deg -> (0, 1, 0), +y 2, +z 3, tile -5 in x
    assert np.allclose(mvs.beads.apply_affine(m, np.zeros((1, 3)))[0], [-5, 3, 3], atol=1e-12)
    assert sb.getTilesExtent.__doc__


def test_bead_entry_points_reject_bad_arguments(mvs):
    L = mvs._lib.load()
    i3 = lambda *v: (C.c_int64 * 3)(*v)                               # noqa: E731
    d3 = lambda *v: (C.c_double * 3)(*v)                              # noqa: E731
    xyz = (C.c_double * 3)(1, 1, 1)
    out = (C.c_void_p * 1)(1234)

    def call(mn=(0, 0, 0), mx=(8, 8, 8), sigma=(1, 1, 1), offs=None, nviews=1, n=1, m12=None):
        return mvs._lib.check(L.mvsim_render_beads(None, xyz, offs, n, m12, nviews, i3(*mn), i3(*mx), d3(*sigma), out, None))
    with pytest.raises(ValueError, match="ctx is null"):
        call()
    st = C.c_uint64(0)
    with pytest.raises(ValueError, match="negative"):
        mvs._lib.check(L.mvsim_beads_random_points(C.byref(st), -1, i3(0, 0, 0), i3(1, 1, 1), xyz))
    # argument errors are reported before the context is looked at
    for kw, msg in ((dict(mx=(8, 0, 8)), "dimension"), (dict(mn=(3, 0, 0), mx=(3, 8, 8)), "dimension"),
                    (dict(sigma=(1, 0, 1)), "sigma"), (dict(sigma=(1, float("nan"), 1)), "sigma"), (dict(sigma=(-1, 1, 1)), "sigma"),
                    (dict(sigma=(1, float("inf"), 1)), "sigma"), (dict(nviews=0), "view"),
                    (dict(offs=(C.c_int64 * 2)(0, 2)), "view_offsets"), (dict(offs=(C.c_int64 * 2)(1, 0)), "view_offsets"),
                    (dict(m12=(C.c_double * 12)(*([1.0] * 11 + [float("nan")]))), "non-finite")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="no output"):
        mvs._lib.check(L.mvsim_render_beads(None, xyz, None, 1, None, 1, i3(0, 0, 0), i3(4, 4, 4), d3(1, 1, 1), None, None))
