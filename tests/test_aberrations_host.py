"""The refraction simulator without a GPU: known answers of the sequential restatement (tests/aberrations_restatement.py), of the
library's host-only entry points and of the Python mirror's host helpers, and the divergence twin on the GPU tests' inputs."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R


def _unit(deg):
    """A ray in the x-y plane hitting the plane y = 0 (normal (0, 1, 0)) at `deg` degrees from the normal, travelling towards -y."""
    return [math.sin(math.radians(deg)), -math.cos(math.radians(deg)), 0.0]


# ------------------------------------------------------------------------------------------------ Raytrace
def test_snell_reproduces_the_reference_recorded_angles():
    """SimulateMultiViewAberrations.java:690-692 records 45 degrees at 1.0 -> 1.1 giving 40.00274776305653 degrees, and that angle at
    1.1 -> 1.2 giving 36.10420471349619 degrees."""
    i = [math.sqrt(0.5), -math.sqrt(0.5), 0.0]
    theta_i, n = R.incident_angle(i, [0.0, 1.0, 0.0])
    assert abs(math.degrees(theta_i) - 45.0) <= 1e-12
    theta_t, t = R.refract(i, n, 1.0, 1.1, theta_i)
    assert abs(math.degrees(theta_t) - 40.00274776305653) <= 1e-12
    theta_t2, _ = R.refract(t, n, 1.1, 1.2, theta_t)
    assert abs(math.degrees(theta_t2) - 36.10420471349619) <= 1e-12
    # the refracted ray leaves at thetaT from the (flipped) normal and keeps its length up to rounding
    assert abs(math.degrees(math.acos(np.dot(t, n) / np.linalg.norm(t))) - 40.00274776305653) <= 1e-9


def test_snell_in_the_python_mirror(mvs):
    i = [math.sqrt(0.5), -math.sqrt(0.5), 0.0]
    n = [0.0, 1.0, 0.0]
    theta_i = mvs.Raytrace.incidentAngle(i, n)
    assert n == [-0.0, -1.0, -0.0]
    t = [0.0, 0.0, 0.0]
    theta_t = mvs.Raytrace.refract(i, n, 1.0, 1.1, theta_i, t)
    assert abs(math.degrees(theta_t) - 40.00274776305653) <= 1e-12
    want_t, want = R.refract(i, n, 1.0, 1.1, theta_i)
    assert theta_t == want_t and np.array_equal(t, want)
    # total reflection: NaN, t untouched
    t2 = [7.0, 7.0, 7.0]
    assert math.isnan(mvs.Raytrace.refract(_unit(80), [0.0, 1.0, 0.0], 1.5, 1.0, math.radians(80), t2)) and t2 == [7.0, 7.0, 7.0]
    assert math.isnan(R.refract(_unit(80), [0.0, 1.0, 0.0], 1.5, 1.0, math.radians(80))[0])
    v = [3.0, 4.0, 12.0]
    mvs.Raytrace.norm(v)
    assert v == [3.0 / 13.0, 4.0 / 13.0, 12.0 / 13.0] and mvs.Raytrace.length([3.0, 4.0, 12.0]) == 13.0


def test_reflect_keeps_the_length():
    rng = np.random.default_rng(2)
    for _ in range(50):
        i = rng.standard_normal(3)
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        r = R.reflect(i, n)
        assert abs(np.linalg.norm(r) - np.linalg.norm(i)) <= 1e-14 * np.linalg.norm(i)
        assert abs(np.dot(r, n) + np.dot(i, n)) <= 1e-14 * np.linalg.norm(i)


def test_incident_angle_quirk_is_pinned():
    """thetaI >= pi / 2 flips the normal and SUBTRACTS pi / 2 (Raytrace.java:79-90): a ray at 120 degrees from the normal is reported
    at 30 degrees -- not at the 60 degrees it makes with the flipped normal."""
    i = [math.sin(math.radians(120)), math.cos(math.radians(120)), 0.0]
    theta, n = R.incident_angle(i, [0.0, 1.0, 0.0])
    assert abs(math.degrees(theta) - 30.0) <= 1e-12
    assert np.array_equal(n, [-0.0, -1.0, -0.0])
    theta2, n2 = R.incident_angle([math.sin(math.radians(60)), math.cos(math.radians(60)), 0.0], [0.0, 1.0, 0.0])
    assert abs(math.degrees(theta2) - 60.0) <= 1e-12 and np.array_equal(n2, [0.0, 1.0, 0.0])


# ------------------------------------------------------------------------------------------------ Lightsheet
@pytest.mark.parametrize("n,middle,edge", [(289, 1.0, 3.0), (48, 1.0, 3.0), (40, 2.5, 0.5)])
def test_lightsheet_predicts_its_three_thicknesses(mvs, n, middle, edge):
    abc = R.lightsheet_fit(n / 2.0, middle, float(n), edge)
    ls = mvs.Lightsheet(n / 2.0, middle, float(n), edge)
    assert (ls.getA(), ls.getB(), ls.getC()) == abc                      # the library's fit is the restatement's, bit for bit
    for x, want in ((n / 2.0, middle), (0.0, edge), (float(n), edge)):
        assert abs(ls.predict(x) - want) <= 1e-9 * abs(want)
    assert mvs.Lightsheet(1.0, 2.0, 3.0).predict(2.0) == 1.0 * 2.0 * 2.0 + 2.0 * 2.0 + 3.0


def test_lightsheet_singular_input_raises(mvs):
    with pytest.raises(ValueError):
        R.lightsheet_fit(10.0, 1.0, 0.0, 3.0)          # the three points share one x
    with pytest.raises(ValueError, match="invert"):
        mvs.Lightsheet(10.0, 1.0, 0.0, 3.0)
    with pytest.raises(ValueError):
        mvs.Lightsheet(float("nan"), 1.0, 4.0, 3.0)


# ------------------------------------------------------------------------------------------------ Hessian, eigenpair
def _field(f, shape=(12, 11, 10)):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.ascontiguousarray(f(x, y, z), dtype=np.float32)


def test_hessian_of_known_fields_is_exact():
    pts = [(3.0, 4.0, 5.0), (6.0, 2.0, 8.0), (2.0, 7.0, 3.0)]
    m, _, _ = R.hessian_at(_field(lambda x, y, z: x * x), pts)
    assert np.array_equal(m, np.broadcast_to(np.diag([2.0, 0.0, 0.0]), m.shape))
    m, vec, val = R.hessian_at(_field(lambda x, y, z: y * z), pts)
    want = np.zeros((3, 3))
    want[1, 2] = want[2, 1] = 1.0
    assert np.array_equal(m, np.broadcast_to(want, m.shape))
    assert np.allclose(np.abs(val), 1.0, rtol=0, atol=1e-15) and np.allclose(vec[:, 0], 0.0, atol=1e-15)
    m, vec, val = R.hessian_at(_field(lambda x, y, z: 0 * x + 3.5), pts)
    assert np.array_equal(m, np.zeros_like(m)) and np.array_equal(val, np.zeros(3))
    # between the samples the interpolant of x^2 is piecewise linear: its second difference over +-1 is still 2
    m, _, _ = R.hessian_at(_field(lambda x, y, z: x * x), [(3.25, 4.5, 5.75)])
    assert m[0, 0, 0] == 2.0 and m[0, 1, 1] == 0.0 and m[0, 2, 2] == 0.0
    # the images: integer positions through the mirror
    val_img, vec_img = R.hessian_images(_field(lambda x, y, z: x * x))
    assert val_img[5, 5, 5] == 2.0 and abs(vec_img[0, 5, 5, 5]) == 1.0 and vec_img[1, 5, 5, 5] == 0.0


def test_eigen_decomposition_residuals_and_tie_rule():
    rng = np.random.default_rng(7)
    mats = [rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-6, 6) for _ in range(3000)]
    mats += [np.diag(rng.standard_normal(3)) for _ in range(20)]                               # diagonal
    for _ in range(20):                                                                         # already tridiagonal
        a = np.diag(rng.standard_normal(3))
        a[0, 1], a[1, 2] = rng.standard_normal(2)
        mats.append(a)
    mats += [np.zeros((3, 3)), np.ones((3, 3)), np.eye(3)]
    for a in mats:
        a = np.triu(a) + np.triu(a, 1).T
        d, V = R.eig_all(a)
        norm = np.linalg.norm(a)
        assert d[0] <= d[1] <= d[2]
        for k in range(3):
            assert np.linalg.norm(a @ V[:, k] - d[k] * V[:, k]) <= 1e-14 * norm
            assert abs(np.linalg.norm(V[:, k]) - 1.0) <= 1e-14
        ev, vec = R.largest_eigen(a)
        k = 0 if abs(d[0]) >= max(abs(d[1]), abs(d[2])) else (1 if abs(d[1]) >= abs(d[2]) else 2)   # first wins on ties
        assert ev == d[k] and np.array_equal(vec, V[:, k])
    # the tie: -3 and 3 have the same magnitude, ascending order puts -3 first
    ev, vec = R.largest_eigen(np.diag([3.0, -3.0, 1.0]))
    assert ev == -3.0 and np.array_equal(np.abs(vec), [0.0, 1.0, 0.0])
    ev, _ = R.largest_eigen(np.diag([1.0, 2.0, -2.0]))
    assert ev == -2.0


# ------------------------------------------------------------------------------------------------ VolumeInjection
def test_injection_geometry_and_sum_of_weights(mvs):
    size, sum_weights, num_pixels = R.inject_info((0.5, 0.5, 0.5))
    assert size == [5, 5, 5] and num_pixels == 125                       # getSuggestedKernelDiameter(0.5) = 5
    want = 0.0
    for z in range(-2, 3):
        for y in range(-2, 3):
            for x in range(-2, 3):
                want += ((1 * math.exp(-(x * x) / 0.5)) * math.exp(-(y * y) / 0.5)) * math.exp(-(z * z) / 0.5)
    assert abs(sum_weights - want) <= 4e-16 * want                       # exp of numpy / libm / Python may differ in the last bit
    v = mvs.VolumeInjection(None, None, [0.5, 0.5, 0.5])
    assert v.getSize() == [5, 5, 5] and v.getNumPixels() == 125 and v.getSumWeights() == sum_weights
    assert R.inject_info((1.0, 0.7, 2.0))[0] == [7, 5, 13]
    with pytest.raises(ValueError, match="sigma"):
        mvs.VolumeInjection(None, None, [0.5, 0.0, 0.5])
    # one Gaussian in the middle of a small volume: the weights sum to sumWeights (as floats), the image to the intensity
    img, w = np.zeros((9, 9, 9), np.float32), np.zeros((9, 9, 9), np.float32)
    R.inject(img, w, (0.5, 0.5, 0.5), [(4.0, 4.0, 4.0)], [3.0], normalized=True)
    assert abs(float(w.sum(dtype=np.float64)) - sum_weights) <= 1e-6 and abs(float(img.sum(dtype=np.float64)) - 3.0) <= 1e-6
    # a point on the face loses the part of its box outside the volume; x.5 rounds up
    img, w = np.zeros((9, 9, 9), np.float32), np.zeros((9, 9, 9), np.float32)
    R.inject(img, w, (0.5, 0.5, 0.5), [(0.0, 4.5, 8.0)], [1.0])
    assert np.count_nonzero(w) == 3 * 5 * 3 and w[8, 5, 0] == np.float32(math.exp(-0.25 / 0.5)) and w[:, 2, :].max() == 0


def test_normalize_and_project_restatement():
    img = np.array([[[2.0, 0.0]], [[4.0, 0.0]]], np.float32)            # (Nz, Ny, Nx) = (2, 1, 2)
    w = np.array([[[2.0, 5.0]], [[0.5, 5.0]]], np.float32)
    assert np.array_equal(R.normalize(img, w), np.array([[[1.0, 0.0]], [[4.0, 0.0]]], np.float32))
    p = R.project(img, w)
    assert p[0, 0] == np.float32((2.0 * 2.0 + 4.0 * 0.5) / 2.5) and np.isnan(p[0, 1])


# ------------------------------------------------------------------------------------------------ java.util.Random
def test_ray_starts_replay_java_util_random(mvs):
    rnd = mvs.JavaRandom(2423)
    abc = R.lightsheet_fit(20.0, 1.0, 40.0, 3.0)
    pos, vec, state = R.refract3d_ray_starts(R.seed_state(2423), (33, 56, 40), 1, 16, abc, 5)
    for k in range(5):
        x = rnd.nextDouble() * 39
        th = abc[0] * x * x + abc[1] * x + abc[2]
        z = 16 + (rnd.nextDouble() * th) - th / 2.0
        v = [(rnd.nextDouble() - 0.5) / 5, -1.0, 0.0]
        mvs.Raytrace.norm(v)
        assert list(pos[k]) == [x, 55.0, z] and list(vec[k]) == v
    assert state == rnd._s
    rnd = mvs.JavaRandom(464232194)
    pos, state = R.camera_ray_starts(R.seed_state(464232194), (4, 3, 5), 2)
    assert list(pos[0]) == [0 + (rnd.nextDouble() - 0.5), 0 + (rnd.nextDouble() - 0.5), 1.0]
    for _ in range(2 * (2 * 5 + 1) - 2 + 2):      # to ray 0 of pixel (x 1, y 1): pixels are x fastest
        rnd.nextDouble()
    assert list(pos[2 * 6]) == [1 + (rnd.nextDouble() - 0.5), 1 + (rnd.nextDouble() - 0.5), 1.0]


# ------------------------------------------------------------------------------------------------ the divergence twin
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("shape", cases.TRACE_SHAPES)
def test_divergence_twin_of_refract3d(shape, illum):
    """One ulp in every libm result must not send more than 0.1 % of the rays elsewhere, and must move the others by far less
    than a voxel: the GPU tests accept 16 D_twin per position, which has to stay below 1e-6 voxel."""
    img, ri_img = cases.trace_inputs(shape)
    base, share, d_twin = cases.twin_refract3d(img, ri_img, illum, shape[0] // 2)
    straight = R.refract3d(img, np.full(shape, 0.5, np.float32), illum, shape[0] // 2, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI,
                           cases.TRACE_RAYS, inject=False)
    bent = float(np.mean(base["moves"] != straight["moves"]))
    print(f"refract3d twin {shape} illum={illum}: rays that differ {100 * share:.4f} %, D_twin {d_twin:.3e} voxel, "
          f"steps {len(base['xyz'])}, rays whose move count the refraction changes {100 * bent:.2f} %")
    assert share <= 1e-3
    assert 0.0 < d_twin and 16 * d_twin <= 1e-6
    assert bent > 0.01, "the index field must refract for the twin to mean anything"


@pytest.mark.parametrize("rays_per_pixel", [7, 500])
def test_divergence_twin_of_project_to_camera(rays_per_pixel):
    ri_img, refr = cases.camera_inputs()
    base, share, e_twin = cases.twin_project_to_camera(ri_img, refr, cases.CAMERA_SHAPE[0] // 2, rays_per_pixel)
    print(f"projectToCamera twin, {rays_per_pixel} rays per pixel: rays that differ {100 * share:.4f} %, E_twin {e_twin:.3e} of the range")
    assert share <= 1e-3
    assert e_twin <= 1e-6
    assert np.isfinite(base["proj"]).all() and base["proj"].max() > base["proj"].min()
