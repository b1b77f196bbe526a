"""The general tracer and the ray sandbox on the GPU (raytrace.hip) against the sequential restatement
(tests/raytrace_restatement.py) and against refract3d on the same device, through the C ABI and the Python mirror.

Exact and compared bit for bit: ray starts, the wedge, the Hessian plane, refract3d's results when the general tracer is given
refract3d's rays, everything on inputs without index contrast, the injection of the GPU's own step list, ranges.  What passes through
acos / asin / sin / cos is measured against the divergence twin."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R
from tests import raytrace_restatement as T
from tests import trace_rays_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_wedges = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _wedge(ctx, k):
    """The GPU's trace of a wedge case with its step list, computed once."""
    if k not in _wedges:
        img, pos, vec = TC.wedge_case(*TC.WEDGES[k])
        _wedges[k] = ctx.trace_rays(img, pos, vec, steps=True)
    return _wedges[k]


# ------------------------------------------------------------------------------------------------ 1. starts, wedge, Hessian plane
def test_sandbox_bundle_is_bit_exact(ctx, mvs):
    rnd = mvs.JavaRandom(1)
    for _ in range(77):
        rnd.nextDouble()
    s0 = rnd._s
    pos, vec = ctx.sandbox_ray_starts((33, 56, 40), 17, 9, 1000, rnd)
    want_pos, want_vec, state = T.sandbox_ray_starts(s0, (33, 56, 40), 17, 9, 1000)
    assert _same(pos, want_pos) and _same(vec, want_vec) and rnd._s == state
    # the reference's generator; the last ray jumps it 799 996 steps ahead
    rnd = mvs.JavaRandom(234345)
    pos, vec = ctx.sandbox_ray_starts((300, 300, 300), 150, 150, 200000, rnd)
    want_pos, want_vec, state = T.sandbox_ray_starts(R.seed_state(234345), (300, 300, 300), 150, 150, 200000)
    assert _same(pos, want_pos) and _same(vec, want_vec) and rnd._s == state


@pytest.mark.parametrize("nx", [24, 25])
@pytest.mark.parametrize("ny", [25, 26])
def test_grid_starts_are_bit_exact(ctx, nx, ny):
    shape = (4, ny, nx)
    pos, vec = ctx.grid_ray_starts(shape, 2, 8)
    want_pos, want_vec = T.grid_ray_starts(shape, 2, 8)
    assert len(pos) == 3 and _same(pos, want_pos) and _same(vec, want_vec)
    got = ctx.trace_rays(np.ones(shape, np.float32), pos, vec, steps=True)
    want = T.trace_rays(np.ones(shape, np.float32), want_pos, want_vec)
    assert np.array_equal(got["moves"], want["moves"]) and got["moves"].tolist() == [ny - 24, ny - 24, 0 if nx == 24 else ny - 24]


@pytest.mark.parametrize("shape", [(5, 41, 37), (10, 64, 64)])
def test_wedge_is_bit_exact(ctx, mvs, shape):
    assert _same(ctx.draw_simple_image(shape, 1.0, 1.33), T.draw_simple_image(shape, 1.0, 1.33))
    a = np.zeros(shape, np.float32)
    mvs.Raytrace.drawSimpleImage(a, 0.5, 2.0, ctx=ctx)
    assert _same(a, T.draw_simple_image(shape, 0.5, 2.0))


def test_hessian_plane_is_the_plane_of_hessian_images(ctx, mvs):
    rng = np.random.default_rng(13)
    img = rng.random((17, 20, 24)).astype(np.float32)
    val, vec = ctx.hessian_images(img)
    for z in (0, 8, 16):
        pv, pvec = ctx.hessian_plane(img, z, vectors=True)
        assert _same(pv, val[z]) and _same(pvec, np.ascontiguousarray(vec[:, z]))
        assert _same(ctx.hessian_plane(img, z), val[z])
        h = mvs.RayTracingTest.hessian(img, z, ctx=ctx)
        assert _same(h[z], val[z]) and _same(np.delete(h, z, axis=0), np.delete(img, z, axis=0))
    val2, vec2 = ctx.hessian_images(img)                                   # the whole-volume entry point keeps its results
    wval, wvec = R.hessian_images(img)
    assert _same(val2, wval) and _same(vec2, wvec)


# ------------------------------------------------------------------------------------------------ 2. GPU against GPU
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("shape", cases.TRACE_SHAPES)
def test_trace_rays_given_refract3d_rays_returns_refract3d(ctx, mvs, shape, illum):
    """refract3d's starts, the map (1, ri), max_moves = Nz, the image as value source: the step list, move counts, image and weight of
    refract3d on the same device.  No tolerance."""
    img, ri_img = cases.trace_inputs(shape)
    z = shape[0] // 2
    want = ctx.refract3d(img, ri_img, illum, z, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, cases.TRACE_RAYS, steps=True)
    abc = R.lightsheet_fit(shape[2] / 2.0, cases.LS_MIDDLE, float(shape[2]), cases.LS_EDGE)
    pos, vec = ctx.refract3d_ray_starts(shape, illum, z, abc, cases.TRACE_RAYS, mvs.JavaRandom(2423))
    got = ctx.trace_rays(ri_img, pos, vec, img=img, n_a=1.0, n_b=cases.RI, max_moves=shape[0], steps=True)
    assert np.array_equal(got["moves"], want["moves"])
    assert _same(got["xyz"], want["xyz"]) and _same(got["value"], want["value"])
    assert _same(got["image"], want["image"]) and _same(got["weight"], want["weight"])
    assert got["weight"].max() > 1.0


# ------------------------------------------------------------------------------------------------ 3. no index contrast
@pytest.mark.parametrize("source", ["image", "intensity", "constant"])
def test_without_index_contrast_is_bit_exact_end_to_end(ctx, source):
    shape = cases.TRACE_SHAPES[1]
    rng = np.random.default_rng(31)
    pos, vec = TC.random_rays(shape, TC.RAYS, seed=6)
    vec *= 0.25 + 2.0 * rng.random((TC.RAYS, 1))                           # directions as given: any length
    vec[0], vec[1], vec[2], vec[3], vec[4], vec[5] = (1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, 0, 0), (0, 0, 0), (0, 0.5, 0)
    assert (vec < 0).any()
    ri_img = np.full(shape, 1.2, np.float32)
    img, _ = cases.trace_inputs(shape)
    kw = dict(max_moves=97, n_a=1.0, n_b=1.33)
    if source == "image":
        kw["img"] = img
        kw["intensity"] = rng.random(TC.RAYS).astype(np.float32)            # the image wins
    elif source == "intensity":
        kw["intensity"] = (rng.random(TC.RAYS) * 3).astype(np.float32)
    else:
        kw["constant_value"] = 0.75
    got = ctx.trace_rays(ri_img, pos, vec, steps=True, **kw)
    want = T.trace_rays(ri_img, pos, vec, **kw)
    assert np.array_equal(got["moves"], want["moves"]) and got["moves"][4] == 97
    assert got["n_capped"] == want["n_capped"] >= 1
    assert _same(got["xyz"], want["xyz"]) and _same(got["value"], want["value"])
    assert _same(got["end_pos"], want["end_pos"]) and _same(got["end_dir"], want["end_dir"]) and _same(got["end_dir"], vec)
    assert _same(got["weight"], want["weight"]) and _same(got["image"], want["image"])
    assert got["weight"].max() > 1.0


# ------------------------------------------------------------------------------------------------ 4. within the twin
@pytest.mark.parametrize("name", TC.TWIN_NAMES)
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_trace_rays_agrees_with_the_restatement_within_the_twin(ctx, shape, name):
    """The rule of test_trace_agrees_with_the_restatement_within_the_twin (tests/test_aberrations.py): a ray agrees if its move count
    matches and every position is within 16 D_twin; at most 0.5 % of the rays may disagree.  Precondition: twin share <= 1e-3 and
    16 D_twin <= 1e-6."""
    ri_img, pos, vec, kw = TC.twin_cases(shape)[name]
    base, share_twin, d_twin = TC.twin_of(shape, name)
    assert share_twin <= 1e-3 and 16 * d_twin <= 1e-6, (share_twin, d_twin)
    gkw = dict(kw)
    if "total_reflection" in gkw:
        gkw["total_reflection"] = "reflect" if gkw["total_reflection"] == T.REFLECT else "keep"
    got = ctx.trace_rays(ri_img, pos, vec, steps=True, inject=False, **gkw)
    assert got["moves"].shape == base["moves"].shape and int(got["moves"].sum()) == len(got["xyz"]) == len(got["value"])
    assert got["n_capped"] == 0 and np.all(got["value"] == np.float32(1.0))
    og, ob = cases.offsets(got["moves"]), cases.offsets(base["moves"])
    disagree, worst = 0, 0.0
    for k in range(len(pos)):
        if got["moves"][k] != base["moves"][k]:
            disagree += 1
            continue
        dp = np.abs(got["xyz"][og[k]:og[k + 1]] - base["xyz"][ob[k]:ob[k + 1]])
        if dp.size and dp.max() > 16 * d_twin:
            disagree += 1
            continue
        if dp.size:
            worst = max(worst, float(dp.max()))
    share = disagree / len(pos)
    print(f"trace_rays {shape} {name}: D_twin {d_twin:.3e}, disagreeing rays {100 * share:.4f} %, largest position difference of the "
          f"agreeing rays {worst:.3e} voxel")
    assert share <= 5e-3


# ------------------------------------------------------------------------------------------------ 5. the sandbox's own scene
@pytest.mark.parametrize("k", range(len(TC.WEDGES)))
def test_wedge_scene_ray_by_ray_outside_the_ties(ctx, k):
    """Integer starts on a piecewise-constant image sit on exact ties (acos(0) = pi / 2 at the >= test): rays whose decisions the twin
    flips are printed and left out, no more than one in five.  The others agree in their move counts and in every position within
    16 max(D_twin, moves * 2^-52): D_twin of a dozen rays can be smaller than what a direction that is one ulp off carries to the end
    of the longest ray, so that path error is the floor."""
    shape, spacing, high = TC.WEDGES[k]
    img, pos, vec = TC.wedge_case(shape, spacing, high)
    base, share_twin, d_twin = TC.twin_trace(img, pos, vec)
    left_out = np.nonzero(base["differs"])[0]
    print(f"wedge {shape} spacing {spacing} high {high}: rays left out {left_out.tolist()} of {len(pos)}, D_twin {d_twin:.3e}")
    assert len(left_out) <= len(pos) / 5
    got = _wedge(ctx, k)
    tol = 16 * max(d_twin, int(base["moves"].max()) * 2.0 ** -52)
    og, ob = cases.offsets(got["moves"]), cases.offsets(base["moves"])
    for r in np.nonzero(~base["differs"])[0]:
        assert got["moves"][r] == base["moves"][r], (r, got["moves"][r], base["moves"][r])
        if got["moves"][r]:
            dp = float(np.abs(got["xyz"][og[r]:og[r + 1]] - base["xyz"][ob[r]:ob[r + 1]]).max())
            assert dp <= tol, (r, dp, tol)
    assert got["n_capped"] == 0


@pytest.mark.parametrize("k", range(len(TC.WEDGES)))
def test_wedge_scene_injection_and_determinism_on_all_rays(ctx, mvs, k):
    """Whatever the ties decide: the GPU's own step list injected by the restatement's sequential addNormalizedGaussian equals the
    GPU's image and weight, two runs are bit-identical, and the sandbox mirror returns the same volumes."""
    shape, spacing, high = TC.WEDGES[k]
    img, pos, vec = TC.wedge_case(shape, spacing, high)
    got = _wedge(ctx, k)
    image, weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    T.inject(image, weight, (0.5, 0.5, 0.5), got["xyz"], got["value"].astype(np.float64), normalized=True)
    assert weight.max() > 0 and _same(got["weight"], weight) and _same(got["image"], image)
    again = ctx.trace_rays(img, pos, vec, steps=True)
    for key in ("image", "weight", "xyz", "value", "end_pos", "end_dir"):
        assert _same(got[key], again[key]), key
    assert np.array_equal(got["moves"], again["moves"])
    inj = mvs.RayTracingTest.drawRays(img, shape[0] // 2, spacing, ctx=ctx)
    assert _same(inj.getWeight(), got["weight"]) and _same(inj.getImage(), got["image"])


# ------------------------------------------------------------------------------------------------ 6. ranges are hidden
def test_ranges_are_hidden(mvs):
    """4096 rays with max_moves = 4096: the default cap of 2^25 step records gives one range of 4096 rays, "beads_pair_cap" = 2^26
    (2^23 records) two ranges of 2048 rays, 98304 (12288 records) ranges of three rays: the same bits."""
    shape = cases.TRACE_SHAPES[1]
    ri_img = TC.field_b(shape)
    pos, vec = TC.random_rays(shape)
    vec[7] = 0.0                                                            # one ray fills its 4096 slots
    kw = dict(max_moves=4096, steps=True)
    with mvs.Context(0) as c:
        one = c.trace_rays(ri_img, pos, vec, **kw)
        c.set_option("beads_pair_cap", 1 << 26)
        many = c.trace_rays(ri_img, pos, vec, **kw)
        c.set_option("beads_pair_cap", 8 * 4096 * 3)                        # three rays per range
        few = c.trace_rays(ri_img, pos[:100], vec[:100], **kw)
    assert one["n_capped"] == many["n_capped"] == 1 and one["moves"][7] == 4096
    for key in ("image", "weight", "xyz", "value", "end_pos", "end_dir"):
        assert _same(one[key], many[key]), key
    assert np.array_equal(one["moves"], many["moves"])
    o = cases.offsets(one["moves"])
    assert np.array_equal(few["moves"], one["moves"][:100]) and _same(few["xyz"], one["xyz"][:o[100]])
    assert _same(few["end_pos"], one["end_pos"][:100]) and few["n_capped"] == 1


# ------------------------------------------------------------------------------------------------ 7. surfaces and errors
def test_error_paths_return_einval(ctx, mvs):
    L = mvs._lib.load()
    EINVAL = mvs._lib.MVSIM_EINVAL
    shape = (8, 8, 8)
    vol = np.ones(shape, np.float32)
    pos, vec = np.array([[3.0, 3.0, 3.0], [4.0, 7.0, 4.0]]), np.array([[0.0, -1.0, 0.0], [0.0, -1.0, 0.0]])
    ok = ctx.trace_rays(vol, pos, vec, steps=True)
    assert ok["moves"].tolist() == [4, 8] and ok["n_capped"] == 0
    dim = (C.c_int64 * 3)(8, 8, 8)
    tp = mvs._lib.TraceParams()
    assert L.mvsim_trace_params_default(dim, C.byref(tp)) == 0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    small = mvs._lib.RaySteps(11, 0, None, None, None)                      # twelve steps are needed
    assert L.mvsim_trace_rays(ctx._h, C.c_void_p(vol.ctypes.data), None, dim, dp(pos), dp(vec), None, 2, C.byref(tp), None, None,
                              C.byref(small), None, None, None) == EINVAL and b"capacity" in L.mvsim_last_error()
    exact = mvs._lib.RaySteps(12, 0, None, None, None)
    assert L.mvsim_trace_rays(ctx._h, C.c_void_p(vol.ctypes.data), None, dim, dp(pos), dp(vec), None, 2, C.byref(tp), None, None,
                              C.byref(exact), None, None, None) == 0 and exact.n == 12
    for bad in (dict(max_moves=0), dict(max_moves=(1 << 20) + 1), dict(ev_threshold=-1.0), dict(n_b=float("nan")), dict(sigma=(0.5, 0, 0.5)),
                dict(constant_value=float("inf")), dict(total_reflection="absorb"), dict(intensity=[1.0, float("nan")])):
        with pytest.raises(ValueError):
            ctx.trace_rays(vol, pos, vec, **bad)
    with pytest.raises(ValueError):
        ctx.trace_rays(vol, pos, np.zeros((2, 3)), normalize_dirs=True)
    with pytest.raises(ValueError):
        ctx.trace_rays(vol, [[3.0, float("nan"), 3.0]], [[0.0, -1.0, 0.0]])
    with pytest.raises(ValueError):
        ctx.trace_rays(np.ones((8, 1, 8), np.float32), pos, vec)
    with pytest.raises(ValueError):
        ctx.trace_rays(vol, pos, vec, img=np.ones((8, 8, 9), np.float32))
    with pytest.raises(ValueError):
        ctx.grid_ray_starts(shape, 4, 0)
    with pytest.raises(ValueError):
        ctx.hessian_plane(vol, 8)
    with pytest.raises(ValueError):
        ctx.draw_simple_image(shape, float("nan"), 1.0)
    # the sandbox mirror refuses a result that is not the reference's
    with pytest.raises(RuntimeError):
        mvs.RayTracingTest._trace(vol, [[3.0, 3.0, 3.0]], [[0.0, 0.0, 0.0]], ctx, None)


def test_python_mirror_equals_the_c_abi(ctx, mvs):
    shape = TC.SHAPES[1]
    ri_img = TC.field_b(shape)
    x, z = TC.bundle_x(shape), shape[0] // 2
    pos, vec = ctx.sandbox_ray_starts(shape, x, z, 1000)
    host = ctx.trace_rays(ri_img, pos, vec, steps=True)
    inj = mvs.RayTracingTest.drawMultipleRays(ri_img, z, x, 1000, ctx=ctx)
    assert _same(inj.getImage(), host["image"]) and _same(inj.getWeight(), host["weight"]) and inj.getSize() == [5, 5, 5]
    mapped = mvs.RayTracingTest.drawMultipleRays(TC.field_a(shape), z, x, 200, ctx=ctx, riMap=mvs.RefractiveIndexMap(1.0, 1.33))
    want = ctx.trace_rays(TC.field_a(shape), pos[:200], vec[:200], n_a=1.0, n_b=1.33)
    assert _same(mapped.getWeight(), want["weight"])
    # device-resident form: the same volumes, added to zeroed outputs; then added to again
    n = ri_img.size * 4
    d = [ctx.dev_alloc(n) for _ in range(3)]
    try:
        ctx.upload(d[0], ri_img)
        for q in d[1:]:
            mvs._lib.check(ctx._L.mvsim_dev_memset(ctx._h, C.c_void_p(q), 0, n))
        dev = ctx.trace_rays_dev(d[0], shape, pos, vec, image_dev=d[1], weight_dev=d[2], steps=True)
        assert _same(ctx.download(d[1], shape), host["image"]) and _same(ctx.download(d[2], shape), host["weight"])
        for key in ("xyz", "value", "end_pos", "end_dir"):
            assert _same(dev[key], host[key]), key
        assert np.array_equal(dev["moves"], host["moves"]) and dev["n_capped"] == host["n_capped"] == 0
        ctx.trace_rays_dev(d[0], shape, pos, vec, image_dev=d[1], weight_dev=d[2])
        twice_i, twice_w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        for _ in range(2):
            T.inject(twice_i, twice_w, (0.5, 0.5, 0.5), host["xyz"], host["value"].astype(np.float64), normalized=True)
        assert _same(ctx.download(d[2], shape), twice_w) and _same(ctx.download(d[1], shape), twice_i)
        wedge = ctx.dev_alloc(n)
        d.append(wedge)
        mvs._lib.check(ctx._L.mvsim_draw_simple_image_dev(ctx._h, C.c_void_p(wedge), (C.c_int64 * 3)(shape[2], shape[1], shape[0]), 1.0, 1.33))
        assert _same(ctx.download(wedge, shape), T.draw_simple_image(shape, 1.0, 1.33))
        plane = ctx.dev_alloc(4 * shape[1] * shape[2] * 4)
        d.append(plane)
        mvs._lib.check(ctx._L.mvsim_hessian_plane_dev(ctx._h, C.c_void_p(d[0]), (C.c_int64 * 3)(shape[2], shape[1], shape[0]), 5,
                                                      C.c_void_p(plane), C.c_void_p(plane + shape[1] * shape[2] * 4)))
        pv, pvec = ctx.hessian_plane(ri_img, 5, vectors=True)
        assert _same(ctx.download(plane, (4,) + shape[1:]), np.concatenate([pv[None], pvec]))
    finally:
        for q in d:
            ctx.dev_free(q)


def test_draw_single_ray_frames_equal_cumulative_injection(ctx, mvs):
    shape, spacing, high = TC.WEDGES[0]
    img = T.draw_simple_image(shape, 1.0, high)
    z, x = shape[0] // 2, 2 * spacing
    frames = mvs.RayTracingTest.drawSingleRay(img, z, x, ctx=ctx)
    one = ctx.trace_rays(img, [[x, shape[1] - 25, z]], [[0, -1, 0]], steps=True)
    assert len(frames) == one["moves"][0] == len(one["xyz"]) >= shape[1] - 24
    image, weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for k in range(len(frames)):
        T.inject(image, weight, (0.5, 0.5, 0.5), one["xyz"][k:k + 1], one["value"][k:k + 1].astype(np.float64), normalized=True)
        assert _same(frames[k], weight[z]), k
    assert _same(one["weight"], weight)
    assert _same(mvs.RayTracingTest.getProcessor(one["weight"], z), weight[z])


def test_render_different_nas_equals_separate_calls(ctx, mvs):
    stack = mvs.RayTracingTest.renderDifferentNAs(size=(40, 48, 6), naFrom=1.0, naTo=1.025, naStep=0.01, z=3, spacing=3, ctx=ctx)
    assert stack.shape == (3, 48, 40)
    na = 1.0
    for k in range(3):
        wedge = T.draw_simple_image((6, 48, 40), 1.0, np.float32(na))
        assert _same(stack[k], mvs.RayTracingTest.drawRays(wedge, 3, 3, ctx=ctx).getWeight()[3]), k
        na += 0.01
    assert not _same(stack[0], stack[2])


def test_plain_c_consumer(tmp_path, mvs):
    """tests/c_abi/trace_rays.c: the new header block from C99, no Python, no C++."""
    pkg = os.path.join(ROOT, "multiview-simulation_amd")
    exe = str(tmp_path / "c_abi_trace_rays")
    cmd = [shutil.which("gcc") or "gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "trace_rays.c"), "-L" + pkg, "-lmvsim", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "trace rays c abi ok" in r.stdout, r.stdout + r.stderr
