"""The refraction simulator on the GPU (aberrations.hip) against its sequential restatement (tests/aberrations_restatement.py), through
the C ABI and the Python mirror.

What is exact is compared bit for bit: ray starts, the Hessian and its eigenpair, the injection of a given step list, normalize, project,
and everything on inputs without index contrast.  What passes through acos / asin / sin / cos cannot be: there the tests cut at the
step list and measure against the divergence twin (the restatement with every libm result moved by one ulp), see DESIGN.md section 11."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_traces = {}
_cameras = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _trace(ctx, shape, illum):
    """The GPU's refract3d with its step list on a trace input, computed once and shared by the tests."""
    key = (shape, illum)
    if key not in _traces:
        img, ri_img = cases.trace_inputs(shape)
        _traces[key] = ctx.refract3d(img, ri_img, illum, shape[0] // 2, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, cases.TRACE_RAYS, steps=True)
    return _traces[key]


def _camera(ctx, rays_per_pixel):
    if rays_per_pixel not in _cameras:
        ri_img, refr = cases.camera_inputs()
        _cameras[rays_per_pixel] = ctx.project_to_camera(ri_img, refr, cases.CAMERA_SHAPE[0] // 2, rays_per_pixel)
    return _cameras[rays_per_pixel]


# ------------------------------------------------------------------------------------------------ 1. ray starts
@pytest.mark.parametrize("illum", [False, True])
def test_refract3d_ray_starts_are_bit_exact(ctx, mvs, illum):
    """200 000 rays: the last one jumps the generator 1 199 994 steps (draw 600 000) ahead of the caller's state."""
    shape = (289, 289, 289)
    abc = R.lightsheet_fit(289 / 2.0, 1.0, 289.0, 3.0)
    for z in (0, 144, 288):
        rnd = mvs.JavaRandom(2423)
        pos, vec = ctx.refract3d_ray_starts(shape, illum, z, abc, 200000, rnd)
        want_pos, want_vec, state = R.refract3d_ray_starts(R.seed_state(2423), shape, illum, z, abc, 200000)
        assert _same(pos, want_pos) and _same(vec, want_vec)
        assert rnd._s == state
    # a state in the middle of a stream, a non-cubic volume
    rnd = mvs.JavaRandom(1)
    for _ in range(77):
        rnd.nextDouble()
    s0 = rnd._s
    pos, vec = ctx.refract3d_ray_starts((33, 56, 40), illum, 16, R.lightsheet_fit(20.0, 1.0, 40.0, 3.0), 1000, rnd)
    want_pos, want_vec, state = R.refract3d_ray_starts(s0, (33, 56, 40), illum, 16, R.lightsheet_fit(20.0, 1.0, 40.0, 3.0), 1000)
    assert _same(pos, want_pos) and _same(vec, want_vec) and rnd._s == state


@pytest.mark.parametrize("rays_per_pixel", [7, 500])
def test_camera_ray_starts_are_bit_exact(ctx, mvs, rays_per_pixel):
    rnd = mvs.JavaRandom(464232194)
    pos = ctx.camera_ray_starts(cases.CAMERA_SHAPE, rays_per_pixel, rnd)
    want, state = R.camera_ray_starts(R.seed_state(464232194), cases.CAMERA_SHAPE, rays_per_pixel)
    assert _same(pos, want) and rnd._s == state


# ------------------------------------------------------------------------------------------------ 2., 3. Hessian
def test_hessian_at_real_positions_is_bit_exact(ctx):
    rng = np.random.default_rng(12)
    shape = (17, 20, 24)
    img = (rng.random(shape) ** 2).astype(np.float32)
    dims = np.array([24, 20, 17], dtype=np.float64)
    inside = rng.random((8000, 3)) * (dims - 1)
    far = (rng.random((3000, 3)) - 0.5) * 8 * (2 * dims - 2)            # several periods of the mirror on either side
    small = (rng.random((1500, 3)) - 0.5) * 2                            # |p| < 1: (p + 1) - 1 is not always p
    edge = np.array([[0, 0, 0], [23, 19, 16], [-1, -1, -1], [0.5, 19.5, -0.5], [23.999999, 1e-17, -1e-17], [1e6 + 0.25, -1e6 - 0.75, 5]])
    grid = np.floor(rng.random((500, 3)) * dims)
    pts = np.concatenate([inside, far, small, edge, grid])
    m, vec, val = ctx.hessian_at(img, pts)
    wm, wvec, wval = R.hessian_at(img, pts)
    assert _same(m, wm)
    assert _same(val, wval)
    assert _same(vec, wvec)                                              # sign included: it decides incidentAngle's flip
    # a smooth field as the tracers see it
    img, ri_img = cases.trace_inputs(cases.TRACE_SHAPES[1])
    pts = rng.random((4000, 3)) * (np.array([40, 56, 33]) - 1.0)
    got, want = ctx.hessian_at(ri_img, pts), R.hessian_at(ri_img, pts)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert np.mean(np.abs(want[2]) > 0.01) > 0.05                        # positions where the tracer would refract


def test_hessian_images_are_bit_exact(ctx, mvs):
    rng = np.random.default_rng(13)
    img = rng.random((17, 20, 24)).astype(np.float32)                    # 24 x 20 x 17
    val, vec = ctx.hessian_images(img)
    wval, wvec = R.hessian_images(img)
    assert _same(val, wval) and _same(vec, wvec)
    val2, vec2 = mvs.Hessian.largestEigenVector(R.smooth_blobs((17, 20, 24), 5))
    wval2, wvec2 = R.hessian_images(R.smooth_blobs((17, 20, 24), 5))
    assert _same(val2, wval2) and _same(vec2, wvec2)


# ------------------------------------------------------------------------------------------------ 4. the trace
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("shape", cases.TRACE_SHAPES)
def test_trace_agrees_with_the_restatement_within_the_twin(ctx, shape, illum):
    """A ray agrees if its move count matches and every position is within 16 D_twin (the device's functions may be off by two ulp
    where the twin moves one, and errors add over up to maxMoves refractions); valueIm of agreeing rays within 1e-6 of the range.
    At most 0.5 % of the rays may disagree."""
    img, ri_img = cases.trace_inputs(shape)
    base, share_twin, d_twin = cases.twin_refract3d(img, ri_img, illum, shape[0] // 2)
    assert share_twin <= 1e-3 and 16 * d_twin <= 1e-6, (share_twin, d_twin)
    got = _trace(ctx, shape, illum)
    assert got["moves"].shape == base["moves"].shape and int(got["moves"].sum()) == len(got["xyz"]) == len(got["value"])
    og, ob = cases.offsets(got["moves"]), cases.offsets(base["moves"])
    vrange = float(img.max()) - float(img.min())
    disagree, worst_pos, worst_val = 0, 0.0, 0.0
    for k in range(cases.TRACE_RAYS):
        if got["moves"][k] != base["moves"][k]:
            disagree += 1
            continue
        dp = np.abs(got["xyz"][og[k]:og[k + 1]] - base["xyz"][ob[k]:ob[k + 1]])
        if dp.size and dp.max() > 16 * d_twin:
            disagree += 1
            continue
        if dp.size:
            worst_pos = max(worst_pos, float(dp.max()))
            worst_val = max(worst_val, float(np.abs(got["value"][og[k]:og[k + 1]].astype(np.float64) - base["value"][ob[k]:ob[k + 1]]).max()))
    share = disagree / cases.TRACE_RAYS
    print(f"trace {shape} illum={illum}: D_twin {d_twin:.3e}, disagreeing rays {100 * share:.4f} %, largest position difference of the "
          f"agreeing rays {worst_pos:.3e} voxel, largest valueIm difference {worst_val / vrange:.3e} of the range")
    assert share <= 5e-3
    assert worst_val <= 1e-6 * vrange


# ------------------------------------------------------------------------------------------------ 5. injection
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("shape", cases.TRACE_SHAPES)
def test_injection_of_the_gpu_step_list_is_bit_exact(ctx, shape, illum):
    """The GPU's OWN step list fed to the restatement's sequential addNormalizedGaussian: image and weight equal as uint32."""
    got = _trace(ctx, shape, illum)
    image, weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    R.inject(image, weight, (0.5, 0.5, 0.5), got["xyz"], got["value"].astype(np.float64), normalized=True)
    assert weight.max() > 1.0
    assert _same(got["weight"], weight)
    assert _same(got["image"], image)


def _points(rng, shape, n):
    dims = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)
    pts = -4.0 + rng.random((n, 3)) * (dims + 8.0)                       # inside and a little outside
    half = np.floor(rng.random((n // 4, 3)) * dims) + 0.5                # x.5: Math.round goes up
    faces = rng.random((n // 4, 3)) * (dims - 1)
    faces[np.arange(len(faces)), rng.integers(0, 3, len(faces))] = 0.0
    faces[::2, 0] = dims[0] - 1
    away = np.array([[-100.0, 5, 5], [5, 1e12, 5], [5, 5, -1e15], [-2.5, -2.5, -2.5], [dims[0] + 1.49, 3, 3]])
    return np.concatenate([pts, half, faces, away])


@pytest.mark.parametrize("sigma", [(0.5, 0.5, 0.5), (1.0, 0.7, 2.0)])
@pytest.mark.parametrize("normalized", [False, True])
def test_volume_inject_is_bit_exact_on_random_point_lists(ctx, sigma, normalized):
    rng = np.random.default_rng(21)
    shape = (21, 33, 40)
    pts = _points(rng, shape, 3000)
    inten = rng.standard_normal(len(pts)) * 3.0
    image = rng.random(shape).astype(np.float32)                         # the injection continues from what the volumes hold
    weight = rng.random(shape).astype(np.float32)
    want_i, want_w = image.copy(), weight.copy()
    ctx.volume_inject(image, weight, sigma, pts, inten, normalized)
    R.inject(want_i, want_w, sigma, pts, inten, normalized)
    assert _same(image, want_i) and _same(weight, want_w)


def test_volume_inject_of_points_that_reach_no_voxel_leaves_the_volumes_as_they_are(ctx):
    """A non-empty list whose every box misses the volume (no multiple of the 32 x 8 x 16 brick): no pair at all, every brick's list
    is empty, image and weight keep their bits.  With one NaN coordinate added the C ABI refuses the list before it touches either
    volume (mvsim.h: positions must be finite) -- the cull's own NaN guard cannot be reached from outside -- and again both keep their bits."""
    rng = np.random.default_rng(23)
    shape = (21, 33, 40)
    dims = np.array(shape[::-1], dtype=np.float64)
    far = np.concatenate([dims + 20.0 + rng.random((200, 3)) * 50.0,                 # boxes beyond the last voxel on every axis
                          -20.0 - rng.random((200, 3)) * 50.0,                      # boxes in front of the first
                          (rng.random((200, 3)) - 0.5) * 1.0e12 + 3.0e12,           # beyond the cull's 1e9: no box is formed
                          np.array([[10.0, 10.0, -30.0], [10.0, 80.0, 10.0], [-7.0, 10.0, 10.0]])])   # inside on two axes
    inten = rng.standard_normal(len(far)) * 3.0
    image = rng.random(shape).astype(np.float32) + 0.5
    weight = rng.random(shape).astype(np.float32) + 0.5
    want_i, want_w = image.copy(), weight.copy()
    for normalized in (False, True):
        ctx.volume_inject(image, weight, (1.0, 0.7, 2.0), far, inten, normalized)
        assert _same(image, want_i) and _same(weight, want_w)
    with_nan = far.copy()
    with_nan[17, 1] = np.nan
    with pytest.raises(ValueError):
        ctx.volume_inject(image, weight, (1.0, 0.7, 2.0), with_nan, inten)
    assert _same(image, want_i) and _same(weight, want_w)


def test_volume_inject_honours_the_order_and_hides_its_chunks(mvs):
    rng = np.random.default_rng(22)
    shape = (36, 40, 48)
    pts = np.array([20.3, 17.8, 15.1]) + (rng.random((3000, 3)) - 0.5) * 4.0
    inten = rng.random(len(pts)) * 5.0
    sigma = (1.0, 0.7, 2.0)
    fwd_i, fwd_w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    rev_i, rev_w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    R.inject(fwd_i, fwd_w, sigma, pts, inten)
    R.inject(rev_i, rev_w, sigma, pts[::-1], inten[::-1])
    assert not np.array_equal(fwd_i, rev_i) and not np.array_equal(fwd_w, rev_w), "forward and reverse sums must differ somewhere"
    with mvs.Context(0) as c:
        a_i, a_w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        c.volume_inject(a_i, a_w, sigma, pts, inten)
        c.set_option("beads_pair_cap", 4096)                             # ranges of the list in sequence
        b_i, b_w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        c.volume_inject(b_i, b_w, sigma, pts, inten)
    assert _same(a_i, fwd_i) and _same(a_w, fwd_w)
    assert _same(b_i, fwd_i) and _same(b_w, fwd_w)


# ------------------------------------------------------------------------------------------------ 6. no index contrast
@pytest.mark.parametrize("illum", [False, True])
def test_refract3d_without_index_contrast_is_bit_exact_end_to_end(ctx, illum):
    shape = cases.TRACE_SHAPES[1]
    img, _ = cases.trace_inputs(shape)
    ri_img = np.full(shape, 0.37, np.float32)
    got = ctx.refract3d(img, ri_img, illum, 11, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, 3000, steps=True)
    want = R.refract3d(img, ri_img, illum, 11, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, 3000)
    assert np.array_equal(got["moves"], want["moves"])
    assert _same(got["xyz"], want["xyz"]) and _same(got["value"], want["value"])
    assert _same(got["weight"], want["weight"]) and _same(got["image"], want["image"])
    # every ray straight: the direction never changes
    o = cases.offsets(got["moves"])
    k = int(np.argmax(got["moves"]))
    steps = np.diff(got["xyz"][o[k]:o[k + 1]], axis=0)
    assert np.abs(steps - steps[0]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 7. projectToCamera
@pytest.mark.parametrize("rays_per_pixel", [7, 500])
def test_project_to_camera_within_the_twin(ctx, rays_per_pixel):
    """Within 4 E_twin of the restatement, range-normalised (a pixel averages its rays)."""
    ri_img, refr = cases.camera_inputs()
    base, share_twin, e_twin = cases.twin_project_to_camera(ri_img, refr, cases.CAMERA_SHAPE[0] // 2, rays_per_pixel)
    got = _camera(ctx, rays_per_pixel)
    rng = float(base["proj"].max()) - float(base["proj"].min())
    err = float(np.abs(got.astype(np.float64) - base["proj"].astype(np.float64)).max()) / rng
    print(f"projectToCamera, {rays_per_pixel} rays per pixel: E_twin {e_twin:.3e}, twin rays that differ {100 * share_twin:.4f} %, "
          f"GPU against the restatement {err:.3e} of the range, pixels that differ {int(np.sum(got != base['proj']))} of {got.size}")
    assert share_twin <= 1e-3
    assert err <= 4 * e_twin


@pytest.mark.parametrize("rays_per_pixel", [7, 500])
def test_project_to_camera_without_index_contrast_is_bit_exact(ctx, mvs, rays_per_pixel):
    _, refr = cases.camera_inputs()
    ri_img = np.full(cases.CAMERA_SHAPE, 0.5, np.float32)
    rnd = mvs.JavaRandom(99)
    got = ctx.project_to_camera(ri_img, refr, 9, rays_per_pixel, rnd)
    want = R.project_to_camera(ri_img, refr, 9, rays_per_pixel, R.seed_state(99))
    assert _same(got, want["proj"]) and rnd._s == want["state"]


# ------------------------------------------------------------------------------------------------ 8. normalize, project
def test_normalize_and_project_are_bit_exact(ctx, mvs):
    got = _trace(ctx, cases.TRACE_SHAPES[1], True)
    assert _same(ctx.volume_normalize(got["image"], got["weight"]), R.normalize(got["image"], got["weight"]))
    proj, want = ctx.volume_project(got["image"], got["weight"]), R.project(got["image"], got["weight"])
    assert _same(proj, want)
    assert np.isnan(want).any() and np.isfinite(want).any()              # columns no ray reached: 0 / 0, as the reference
    v = mvs.VolumeInjection(got["image"], got["weight"], [0.5, 0.5, 0.5], ctx=ctx)
    assert _same(v.normalize(), R.normalize(got["image"], got["weight"])) and _same(v.project(), want)
    rng = np.random.default_rng(3)
    image = (rng.random((9, 14, 30)) - 0.3).astype(np.float32)
    weight = (rng.random((9, 14, 30)) * 2).astype(np.float32)
    image[:, 3, 4] = -1.0                                                # an empty column
    assert _same(ctx.volume_normalize(image, weight), R.normalize(image, weight))
    proj = ctx.volume_project(image, weight)
    assert np.isnan(proj[3, 4]) and _same(proj, R.project(image, weight))


# ------------------------------------------------------------------------------------------------ 9. determinism
def test_runs_are_bit_identical(ctx, mvs):
    shape = cases.TRACE_SHAPES[0]
    img, ri_img = cases.trace_inputs(shape)
    first = _trace(ctx, shape, False)
    with mvs.Context(0) as c:
        c.set_option("beads_pair_cap", 8192)                             # rays in many ranges: the same lists, the same sums
        again = c.refract3d(img, ri_img, False, shape[0] // 2, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, cases.TRACE_RAYS, steps=True)
    for key in ("image", "weight", "xyz", "value"):
        assert _same(first[key], again[key]), key
    assert np.array_equal(first["moves"], again["moves"])
    ri_cam, refr = cases.camera_inputs()
    for rays_per_pixel in (7, 500):
        assert _same(_camera(ctx, rays_per_pixel), ctx.project_to_camera(ri_cam, refr, cases.CAMERA_SHAPE[0] // 2, rays_per_pixel))


# ------------------------------------------------------------------------------------------------ 10. errors, C ABI, mirror
def test_error_paths_return_einval(ctx, mvs):
    L = mvs._lib.load()
    EINVAL = mvs._lib.MVSIM_EINVAL
    img = np.zeros((8, 8, 8), np.float32)
    out_i, out_w = np.zeros_like(img), np.zeros_like(img)
    dim = (C.c_int64 * 3)(8, 8, 8)
    state = C.c_uint64(1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    d3 = lambda *v: (C.c_double * 3)(*v)

    def refract(dim=dim, middle=1.0, edge=3.0, ri=1.1, rays=4, state_p=C.byref(state)):
        return L.mvsim_refract3d(ctx._h, p(img), p(img), dim, 0, 4, middle, edge, ri, rays, state_p, p(out_i), p(out_w), None)

    assert refract() == 0
    assert refract(rays=-1) == EINVAL and b"rays" in L.mvsim_last_error()
    assert refract(middle=float("nan")) == EINVAL and refract(ri=float("inf")) == EINVAL
    assert refract(dim=(C.c_int64 * 3)(8, 1, 8)) == EINVAL
    assert refract(state_p=None) == EINVAL
    small = mvs._lib.RaySteps(3, 0, None, None, None)
    assert L.mvsim_refract3d(ctx._h, p(img), p(img), dim, 0, 4, 1.0, 3.0, 1.1, 4, C.byref(state), None, None, C.byref(small)) == EINVAL
    assert b"capacity" in L.mvsim_last_error()
    pts, inten = np.array([[1.0, 2.0, 3.0]]), np.array([1.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    inject = lambda sigma, pts=pts, inten=inten: L.mvsim_volume_inject(ctx._h, p(out_i), p(out_w), dim, sigma, dp(pts), dp(inten), 1, 0)
    assert inject(d3(0.5, 0.5, 0.5)) == 0
    for bad in (d3(0.5, 0.0, 0.5), d3(-1.0, 0.5, 0.5), d3(0.5, 0.5, float("nan"))):
        assert inject(bad) == EINVAL
    assert inject(d3(0.5, 0.5, 0.5), pts=np.array([[1.0, float("nan"), 3.0]])) == EINVAL
    assert inject(d3(0.5, 0.5, 0.5), inten=np.array([float("inf")])) == EINVAL
    proj = np.zeros((8, 8), np.float32)
    camera = lambda rays: L.mvsim_project_to_camera(ctx._h, p(img), p(img), dim, 4, rays, C.byref(state), p(proj))
    assert camera(3) == 0 and camera(0) == EINVAL and camera(5000) == EINVAL
    assert L.mvsim_hessian_at(ctx._h, p(img), dim, dp(np.array([[1.0, float("nan"), 1.0]])), 1, None, None, None) == EINVAL
    assert L.mvsim_hessian_at(ctx._h, p(img), dim, dp(np.array([[1.0, 2.0 ** 31, 1.0]])), 1, None, None, None) == EINVAL
    abc = d3(0, 0, 0)
    assert L.mvsim_lightsheet_fit(4.0, 1.0, 0.0, 3.0, abc) == EINVAL and L.mvsim_lightsheet_fit(4.0, 1.0, 8.0, 3.0, abc) == 0
    with pytest.raises(ValueError):
        ctx.refract3d(img, np.zeros((8, 8, 9), np.float32), False, 4, 1, 3, 1.1, 4)
    with pytest.raises(ValueError):
        ctx.volume_inject(out_i, out_w, (0.5, -0.5, 0.5), pts, inten)


def test_python_mirror_equals_the_c_abi(ctx, mvs):
    shape = cases.TRACE_SHAPES[1]
    img, ri_img = cases.trace_inputs(shape)
    got = _trace(ctx, shape, True)
    inj = mvs.SimulateMultiViewAberrations.refract3d(img, ri_img, True, shape[0] // 2, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI,
                                                     numRays=cases.TRACE_RAYS, ctx=ctx)
    assert _same(inj.getImage(), got["image"]) and _same(inj.getWeight(), got["weight"])
    assert inj.getSize() == [5, 5, 5] and inj.getNumPixels() == 125
    assert mvs.SimulateMultiViewAberrations.inside([0.0, 55.0, 32.0], img) and not mvs.SimulateMultiViewAberrations.inside([0.0, 55.1, 3.0], img)
    # device-resident form: same volumes, added to zeroed outputs
    n = img.size * 4
    d = [ctx.dev_alloc(n) for _ in range(4)]
    try:
        ctx.upload(d[0], img)
        ctx.upload(d[1], ri_img)
        mvs._lib.check(ctx._L.mvsim_dev_memset(ctx._h, C.c_void_p(d[2]), 0, n))
        mvs._lib.check(ctx._L.mvsim_dev_memset(ctx._h, C.c_void_p(d[3]), 0, n))
        state = C.c_uint64(R.seed_state(2423))
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        mvs._lib.check(ctx._L.mvsim_refract3d_dev(ctx._h, C.c_void_p(d[0]), C.c_void_p(d[1]), dim, 1, shape[0] // 2, cases.LS_MIDDLE,
                                                  cases.LS_EDGE, cases.RI, cases.TRACE_RAYS, C.byref(state), C.c_void_p(d[2]),
                                                  C.c_void_p(d[3]), None))
        image, weight = ctx.download(d[2], shape), ctx.download(d[3], shape)
        assert _same(image, got["image"]) and _same(weight, got["weight"])
        want_state = R.refract3d_ray_starts(R.seed_state(2423), shape, 1, 0, (0.0, 0.0, 1.0), cases.TRACE_RAYS)[2]
        assert state.value == want_state
    finally:
        for q in d:
            ctx.dev_free(q)
    # the camera through the facade draws from the class's generator, as the reference's static rnd
    ri_cam, refr = cases.camera_inputs()
    mvs.SimulateMultiViewAberrations.rnd = mvs.JavaRandom(464232194)
    proj = mvs.SimulateMultiViewAberrations.projectToCamera(ri_cam, refr, 1.1, cases.CAMERA_SHAPE[0] // 2, raysPerPixel=7, ctx=ctx)
    assert _same(proj, _camera(ctx, 7))
    assert mvs.SimulateMultiViewAberrations.rnd._s == R.camera_ray_starts(R.seed_state(464232194), cases.CAMERA_SHAPE, 7)[1]


def test_plain_c_consumer(tmp_path, mvs):
    """tests/c_abi/aberr.c: the new entry points from C99, no Python, no C++."""
    pkg = os.path.join(ROOT, "multiview-simulation_amd")
    exe = str(tmp_path / "c_abi_aberr")
    cmd = [shutil.which("gcc") or "gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "aberr.c"), "-L" + pkg, "-lmvsim", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "aberrations c abi ok" in r.stdout, r.stdout + r.stderr
