"""Inputs shared by the general tracer's tests (tests/test_trace_rays_host.py, tests/test_trace_rays.py) and its divergence twin: the
restatement run twice on the same rays, as it is and with every libm result moved by one ulp."""
import numpy as np

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R
from tests import raytrace_restatement as T

SHAPES = cases.TRACE_SHAPES          # (Nz, Ny, Nx): 48^3 and 40 x 56 x 33 (x, y, z)
RAYS = 4096
WEDGES = [((6, 48, 40), 3, 1.33), ((5, 41, 37), 2, 1.33), ((5, 41, 37), 2, 2.0), ((10, 64, 64), 8, 1.33)]   # shape, spacing, high

_memo = {}


def random_rays(shape, n=RAYS, seed=5):
    """Uniform starts inside the volume and isotropic unit directions (normalised normal deviates)."""
    rng = np.random.default_rng(seed)
    dims = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)
    pos = rng.random((n, 3)) * (dims - 1)
    vec = rng.standard_normal((n, 3))
    vec /= np.sqrt((vec * vec).sum(axis=1))[:, None]
    return pos, vec


def field_a(shape):
    """The index field of refract3d's tests, in [0, 1]: to be mapped by (1, 1.1) or (1, 1.33)."""
    return R.smooth_blobs(shape, 4, **cases.RI_BLOBS)


def field_b(shape):
    """A raw index image in [1, 1.33] for the identity map (0, 1): many narrow blobs, so that the curvature passes the threshold."""
    return R.smooth_blobs(shape, 4, count=40, sigma=(0.04, 0.07), lo=1.0, hi=1.33)


def bundle_x(shape):
    """x = Nx // 2, except at 40 x 56 x 33: there the bundle at x = 20 holds one ray (2253 of 4096) that the twin moves by 2.5e-5
    voxel through field_b without changing a decision, so that 16 D_twin <= 1e-6 fails; at x = 21 D_twin is 4.1e-13 (at 19, 22, 18,
    23: 7.8e-13, 1.7e-13, 2.0e-13, 2.8e-13)."""
    return shape[2] // 2 + (1 if tuple(shape) == (33, 56, 40) else 0)


def bundle(shape, n=RAYS):
    """The sandbox bundle at x = bundle_x, z = Nz // 2 from new Random(234345)."""
    pos, vec, _ = T.sandbox_ray_starts(R.seed_state(234345), shape, bundle_x(shape), shape[0] // 2, n)
    return pos, vec


def twin_cases(shape):
    """name -> (index volume, positions, directions, keyword arguments of trace_rays)"""
    pos, vec = random_rays(shape)
    bpos, bvec = bundle(shape)
    return {
        "a_1.1": (field_a(shape), pos, vec, dict(n_a=1.0, n_b=1.1)),
        "a_1.33": (field_a(shape), pos, vec, dict(n_a=1.0, n_b=1.33)),
        "b_identity": (field_b(shape), pos, vec, dict(n_a=0.0, n_b=1.0)),
        "c_bundle": (field_b(shape), bpos, bvec, dict(n_a=0.0, n_b=1.0)),
        "a_1.33_reflect": (field_a(shape), pos, vec, dict(n_a=1.0, n_b=1.33, total_reflection=T.REFLECT)),
    }


TWIN_NAMES = ["a_1.1", "a_1.33", "b_identity", "c_bundle", "a_1.33_reflect"]


def twin_trace(ri_img, pos, vec, **kw):
    """(base run, share of rays whose move count or any decision differs in the twin, D_twin = the largest position difference at
    any move over the other rays, share of moves that refract)."""
    base = T.trace_rays(ri_img, pos, vec, inject=False, **kw)
    T.twin(True)
    try:
        tw = T.trace_rays(ri_img, pos, vec, inject=False, **kw)
    finally:
        T.twin(False)
    differs = (base["moves"] != tw["moves"]) | (base["decisions"] != tw["decisions"])
    ob, ot = cases.offsets(base["moves"]), cases.offsets(tw["moves"])
    d_twin = 0.0
    for k in np.nonzero(~differs)[0]:
        if base["moves"][k]:
            d_twin = max(d_twin, float(np.abs(base["xyz"][ob[k]:ob[k + 1]] - tw["xyz"][ot[k]:ot[k + 1]]).max()))
    base["differs"] = differs
    return base, float(differs.mean()), d_twin


def twin_of(shape, name):
    """twin_trace of a named case, computed once per process."""
    key = (shape, name)
    if key not in _memo:
        ri_img, pos, vec, kw = twin_cases(shape)[name]
        _memo[key] = twin_trace(ri_img, pos, vec, **kw)
    return _memo[key]


def refracting_share(ri_img, xyz, threshold=0.01):
    """The share of the steps at which the tracer refracts: |largest eigenvalue| above the threshold."""
    return float(np.mean(np.abs(R.hessian_at(ri_img, xyz)[2]) > threshold)) if len(xyz) else 0.0


def wedge_case(shape, spacing, high):
    """(the wedge, grid positions, grid directions) of drawRays(img, Nz // 2, spacing)."""
    img = T.draw_simple_image(shape, 1.0, high)
    pos, vec = T.grid_ray_starts(shape, shape[0] // 2, spacing)
    return img, pos, vec
