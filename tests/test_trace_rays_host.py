"""The general tracer and the ray sandbox without a GPU: the generic restatement (tests/raytrace_restatement.py) anchored to
refract3d's restatement bit for bit, the start arithmetic and the wedge against independent statements, the argument checks of the C
ABI that run before a device is touched, and the divergence twin on the GPU tests' inputs."""
import ctypes as C

import numpy as np
import pytest

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R
from tests import raytrace_restatement as T
from tests import trace_rays_cases as TC


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the yardstick's anchor
@pytest.mark.parametrize("illum", [False, True])
@pytest.mark.parametrize("shape", cases.TRACE_SHAPES)
def test_generic_restatement_equals_refract3d_restatement(shape, illum):
    """refract3d's starts, the map (1, ri), max_moves = Nz and the image as value source: steps, values, moves, decisions, image and
    weight of R.refract3d, bit for bit."""
    img, ri_img = cases.trace_inputs(shape)
    z = shape[0] // 2
    want = R.refract3d(img, ri_img, illum, z, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, cases.TRACE_RAYS)
    abc = R.lightsheet_fit(shape[2] / 2.0, cases.LS_MIDDLE, float(shape[2]), cases.LS_EDGE)
    pos, vec, state = R.refract3d_ray_starts(R.seed_state(2423), shape, illum, z, abc, cases.TRACE_RAYS)
    assert state == want["state"]
    got = T.trace_rays(ri_img, pos, vec, img=img, n_a=1.0, n_b=cases.RI, max_moves=shape[0])
    assert np.array_equal(got["moves"], want["moves"]) and np.array_equal(got["decisions"], want["decisions"])
    assert _same(got["xyz"], want["xyz"]) and _same(got["value"], want["value"])
    assert _same(got["image"], want["image"]) and _same(got["weight"], want["weight"])
    assert got["weight"].max() > 1.0 and got["n_reflected"] == 0


def test_value_sources_and_policies_of_the_restatement():
    shape = (9, 12, 10)
    rng = np.random.default_rng(1)
    ri_img = np.full(shape, 1.2, np.float32)
    img = rng.random(shape).astype(np.float32)
    pos, vec = TC.random_rays(shape, 64, seed=2)
    vec[3] = 0.0                                                          # a ray that never leaves
    inten = rng.random(64).astype(np.float32)
    a = T.trace_rays(ri_img, pos, vec, img=img, intensity=inten, max_moves=40)
    b = T.trace_rays(ri_img, pos, vec, intensity=inten, max_moves=40)
    c = T.trace_rays(ri_img, pos, vec, constant_value=0.75, max_moves=40)
    assert np.array_equal(a["moves"], b["moves"]) and np.array_equal(b["moves"], c["moves"]) and _same(a["xyz"], c["xyz"])
    assert a["moves"][3] == 40 and a["n_capped"] == 1 and np.array_equal(a["end_pos"][3], pos[3])
    assert np.array_equal(b["value"], np.repeat(inten, b["moves"])) and np.all(c["value"] == np.float32(0.75))
    assert not np.array_equal(a["value"], b["value"])
    # constant field: no refraction, straight rays, the end is the first position outside
    k = int(np.argmax(np.where(a["moves"] < 40, a["moves"], 0)))
    assert np.array_equal(a["end_dir"][k], vec[k])
    assert not all(0 <= a["end_pos"][k][d] <= shape[2 - d] - 1 for d in range(3))
    # normalize_dirs applies Raytrace.norm once
    d = T.trace_rays(ri_img, pos[:3], 3.0 * vec[:3], normalize_dirs=True, max_moves=40)
    want = 3.0 * vec[:3]
    want = want / np.sqrt((want * want).sum(axis=1))[:, None]
    assert np.abs(d["end_dir"] - want).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ starts, wedge
def test_sandbox_bundle_arithmetic_against_java_random(mvs):
    """RayTracingTest :110-123 with the package's JavaRandom: two nextDouble() per ray."""
    shape = (10, 30, 20)
    rnd = mvs.JavaRandom(234345)
    pos, vec, state = T.sandbox_ray_starts(R.seed_state(234345), shape, 7, 4, 500)
    for k in range(500):
        assert pos[k, 0] == 7 + rnd.nextDouble() - 0.5
        assert pos[k, 1] == 29.0
        assert pos[k, 2] == 4 + rnd.nextDouble() - 0.5
    assert rnd._s == state
    assert np.array_equal(vec, np.tile([0.0, -1.0, 0.0], (500, 1)))


@pytest.mark.parametrize("shape,spacing,count", [((4, 40, 24), 8, 3), ((4, 40, 25), 8, 3), ((4, 40, 24), 5, 4), ((4, 25, 24), 8, 3),
                                                 ((4, 26, 24), 1, 24)])
def test_grid_starts_and_their_quirks(shape, spacing, count):
    pos, vec = T.grid_ray_starts(shape, 2, spacing)
    assert len(pos) == count == shape[2] // spacing
    assert np.array_equal(pos[:, 0], spacing * np.arange(1, count + 1)) and np.all(pos[:, 1] == shape[1] - 25) and np.all(pos[:, 2] == 2)
    out = T.trace_rays(np.ones(shape, np.float32), pos, vec)
    inside = pos[:, 0] <= shape[2] - 1
    assert np.all(out["moves"][inside] == shape[1] - 24) and np.all(out["moves"][~inside] == 0)
    assert (~inside).any() == (shape[2] % spacing == 0)                   # x = Nx is a ray that is not inside


def test_grid_quirk_ny_25_and_26():
    """Ny = 25 starts at y = 0 (inside: one move), Ny = 24 below the image (no move), Ny = 26 at y = 1 (two moves)."""
    for ny, moves in ((24, 0), (25, 1), (26, 2)):
        pos, vec = T.grid_ray_starts((4, ny, 24), 2, 5)
        assert np.all(T.trace_rays(np.ones((4, ny, 24), np.float32), pos, vec)["moves"] == moves)


@pytest.mark.parametrize("shape", [(5, 41, 37), (10, 64, 64), (3, 9, 2), (3, 4, 7)])
def test_wedge_against_a_numpy_statement(mvs, shape):
    nz, ny, nx = shape
    x, y = np.meshgrid(np.arange(nx), np.arange(ny))
    rule = np.where(x < nx // 2, x > y, nx - x > y)
    want = np.broadcast_to(np.where(rule, np.float32(1.33), np.float32(1.0)), shape)
    assert _same(T.draw_simple_image(shape, 1.0, 1.33), np.ascontiguousarray(want))
    assert rule.any() and not rule.all()


def test_index_maps(mvs):
    m = mvs.RefractiveIndexMap(1.0, 1.33)
    assert m.getRI(0.0) == 1.0 and m.getRI(0.5) == (1.33 - 1.0) * 0.5 + 1.0
    assert mvs.RefractiveIndexMap().getRI(1.2345) == 1.2345               # (0, 1): 1 * i + 0 is i
    assert mvs.ClearingMap().getRI(7.0) == 0 and isinstance(mvs.ClearingMap(), mvs.RefractiveIndexMap)
    assert "Out of scope, as in the C ABI: ``RayTracingTest``" not in mvs.aberrations.__doc__


# ------------------------------------------------------------------------------------------------ argument checks before the device
def test_einval_paths_that_need_no_gpu(mvs):
    L = mvs._lib.load()
    EINVAL = mvs._lib.MVSIM_EINVAL
    dim = (C.c_int64 * 3)(8, 8, 8)
    tp = mvs._lib.TraceParams()
    assert L.mvsim_trace_params_default(dim, C.byref(tp)) == 0
    assert (tp.n_a, tp.n_b, tp.ev_threshold, tp.max_moves, tp.total_reflection, tp.normalize_dirs, tp.constant_value, tp.normalized) == \
        (0.0, 1.0, 0.01, 96, 0, 0, 1.0, 1) and list(tp.sigma) == [0.5, 0.5, 0.5]
    assert L.mvsim_trace_params_default(dim, None) == EINVAL
    assert L.mvsim_trace_params_default((C.c_int64 * 3)(8, 1, 8), C.byref(tp)) == EINVAL
    n = C.c_int64(-1)
    assert L.mvsim_grid_ray_starts(None, dim, 4, 3, 0, None, None, C.byref(n)) == 0 and n.value == 2
    assert L.mvsim_grid_ray_starts(None, dim, 4, 0, 0, None, None, C.byref(n)) == EINVAL and b"spacing" in L.mvsim_last_error()
    buf = np.zeros((1, 3))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mvsim_grid_ray_starts(None, dim, 4, 3, 1, dp(buf), dp(buf), C.byref(n)) == EINVAL      # two rays, room for one

    vol = np.ones((8, 8, 8), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    pos, vec = np.array([[3.0, 3.0, 3.0]]), np.array([[0.0, -1.0, 0.0]])

    def trace(ri=vol, dim=dim, pos=pos, vec=vec, inten=None, image=None, weight=None, steps=None, **kw):
        q = mvs._lib.TraceParams()
        assert L.mvsim_trace_params_default((C.c_int64 * 3)(8, 8, 8), C.byref(q)) == 0
        for k, v in kw.items():
            if k == "sigma":
                q.sigma[0], q.sigma[1], q.sigma[2] = v
            else:
                setattr(q, k, v)
        return L.mvsim_trace_rays(None, None if ri is None else p(ri), None, dim, dp(pos), dp(vec),
                                  None if inten is None else inten.ctypes.data_as(C.POINTER(C.c_float)), len(pos), C.byref(q),
                                  None if image is None else p(image), None if weight is None else p(weight), steps, None, None, None)

    assert trace(max_moves=0) == EINVAL and b"max_moves" in L.mvsim_last_error()
    assert trace(max_moves=(1 << 20) + 1) == EINVAL
    assert trace(ev_threshold=-0.01) == EINVAL and b"ev_threshold" in L.mvsim_last_error()
    for name in ("n_a", "n_b", "ev_threshold", "constant_value"):
        assert trace(**{name: float("nan")}) == EINVAL and trace(**{name: float("inf")}) == EINVAL
    assert trace(sigma=(0.5, 0.0, 0.5)) == EINVAL and trace(sigma=(0.5, 0.5, -1.0)) == EINVAL
    assert trace(total_reflection=2) == EINVAL
    assert trace(dim=(C.c_int64 * 3)(8, 8, 1)) == EINVAL
    assert trace(ri=None) == EINVAL and b"null volume" in L.mvsim_last_error()
    assert trace(image=vol) == EINVAL                                      # image without weight
    assert trace(pos=np.array([[3.0, float("nan"), 3.0]])) == EINVAL
    assert trace(vec=np.array([[0.0, float("inf"), 0.0]])) == EINVAL
    assert trace(vec=np.zeros((1, 3)), normalize_dirs=1) == EINVAL and b"zero direction" in L.mvsim_last_error()
    assert trace(inten=np.array([float("nan")], np.float32)) == EINVAL
    assert trace(steps=C.byref(mvs._lib.RaySteps(-1, 0, None, None, None))) == EINVAL
    assert L.mvsim_draw_simple_image(None, None, dim, 1.0, 1.33) == EINVAL
    assert L.mvsim_draw_simple_image(None, p(vol), dim, float("nan"), 1.33) == EINVAL
    assert L.mvsim_hessian_plane(None, p(vol), dim, 8, p(vol), None) == EINVAL and L.mvsim_hessian_plane(None, p(vol), dim, -1, p(vol), None) == EINVAL
    assert L.mvsim_sandbox_ray_starts(None, None, dim, 4, 4, 1, dp(buf), dp(buf)) == EINVAL


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("name", TC.TWIN_NAMES)
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_twin_preconditions_hold(shape, name):
    """What tests/test_trace_rays.py relies on: the twin changes the decisions of at most 1e-3 of the rays, moves the others by
    16 D_twin <= 1e-6 voxel, no ray comes near the move cap, and a sizeable share of the moves refracts (measured on the
    restatement: twin share 0 everywhere, D_twin 1.7e-13 .. 5.0e-13, refracting moves 11 .. 34 %, longest ray 95 of >= 516 moves)."""
    ri_img, pos, vec, kw = TC.twin_cases(shape)[name]
    base, share_twin, d_twin = TC.twin_of(shape, name)
    refr = TC.refracting_share(ri_img, base["xyz"])
    print(f"{shape} {name}: twin share {share_twin:.2e}, D_twin {d_twin:.3e}, refracting moves {100 * refr:.1f} %, longest ray "
          f"{int(base['moves'].max())} of {T.default_max_moves(shape)} moves")
    assert share_twin <= 1e-3 and 16 * d_twin <= 1e-6
    assert base["n_capped"] == 0 and 2 * int(base["moves"].max()) < T.default_max_moves(shape)
    assert refr >= 0.05


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_reflect_policy_takes_its_branch(shape):
    """Case (a) at 1.33 with total_reflection = reflect: rays do meet total reflection (563 and 642 reflections measured), and the
    policy changes their paths."""
    ri_img, pos, vec, kw = TC.twin_cases(shape)["a_1.33_reflect"]
    refl = T.trace_rays(ri_img, pos, vec, inject=False, **kw)
    keep = T.trace_rays(ri_img, pos, vec, inject=False, **dict(kw, total_reflection=T.KEEP))
    assert refl["n_reflected"] >= 1 and keep["n_reflected"] == 0
    assert not np.array_equal(refl["moves"], keep["moves"]) or not _same(refl["xyz"], keep["xyz"])
    # with the reference's policy and threshold the loop is bend_ray itself: the same bits as a threshold that is 0.01 by another route
    other = T.trace_rays(ri_img, pos, vec, inject=False, **dict(kw, total_reflection=T.KEEP, ev_threshold=0.1 * 0.1))
    assert 0.1 * 0.1 != 0.01 and np.array_equal(other["moves"], keep["moves"]) and _same(other["xyz"], keep["xyz"])


@pytest.mark.parametrize("shape,spacing,high", TC.WEDGES)
def test_wedge_ties_leave_enough_rays(shape, spacing, high):
    """The sandbox's own scene sits on exact ties (integer starts on a piecewise-constant image: acos(0) = pi / 2 at the >= test);
    the twin may flip their decisions, and such rays are left out of the ray-by-ray comparison -- no more than one in five."""
    img, pos, vec = TC.wedge_case(shape, spacing, high)
    base, share, d_twin = TC.twin_trace(img, pos, vec)
    print(f"wedge {shape} spacing {spacing} high {high}: {int(base['differs'].sum())} of {len(pos)} rays flip in the twin, D_twin {d_twin:.3e}")
    assert len(pos) == shape[2] // spacing and share <= 0.2 and 16 * d_twin <= 1e-6 and base["n_capped"] == 0
