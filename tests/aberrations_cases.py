"""Inputs shared by the refraction simulator's tests (tests/test_aberrations_host.py, tests/test_aberrations.py) and the divergence
twin: the restatement run twice on the same input, as it is and with every libm result moved by one ulp."""
import numpy as np

from tests import aberrations_restatement as R

# (Nz, Ny, Nx): 48 x 48 x 48 and, non-cubic on purpose, 40 x 56 x 33 (x, y, z)
TRACE_SHAPES = [(48, 48, 48), (33, 56, 40)]
TRACE_RAYS = 4096
CAMERA_SHAPE = (32, 20, 24)          # 24 x 20 x 32 (x, y, z)
LS_MIDDLE, LS_EDGE, RI = 1.0, 3.0, 1.1
RI_BLOBS = dict(count=14, sigma=(0.08, 0.14))      # curvature well above the tracer's |eigenvalue| > 0.01 threshold


def trace_inputs(shape):
    """A smooth image and a smooth refractive-index field in [0, 1]."""
    return R.smooth_blobs(shape, 3, count=8), R.smooth_blobs(shape, 4, **RI_BLOBS)


def camera_inputs(shape=CAMERA_SHAPE):
    return R.smooth_blobs(shape, 7, **RI_BLOBS), R.smooth_blobs(shape, 8, count=8)


def offsets(moves):
    return np.concatenate([[0], np.cumsum(moves, dtype=np.int64)])


def twin_refract3d(img, ri_img, illum, z, num_rays=TRACE_RAYS):
    """(base run, share of rays whose move count or any decision differs in the twin, D_twin = the largest position difference at
    any move over the other rays)."""
    base = R.refract3d(img, ri_img, illum, z, LS_MIDDLE, LS_EDGE, RI, num_rays, inject=False)
    R.twin(True)
    try:
        tw = R.refract3d(img, ri_img, illum, z, LS_MIDDLE, LS_EDGE, RI, num_rays, inject=False)
    finally:
        R.twin(False)
    differs = (base["moves"] != tw["moves"]) | (base["decisions"] != tw["decisions"])
    ob, ot = offsets(base["moves"]), offsets(tw["moves"])
    d_twin = 0.0
    for k in np.nonzero(~differs)[0]:
        if base["moves"][k]:
            d_twin = max(d_twin, float(np.abs(base["xyz"][ob[k]:ob[k + 1]] - tw["xyz"][ot[k]:ot[k + 1]]).max()))
    return base, float(differs.mean()), d_twin


def twin_project_to_camera(ri_img, refr, current_z, rays_per_pixel):
    """(base run, share of rays that differ in the twin, E_twin = the largest pixel difference over the image's range)."""
    base = R.project_to_camera(ri_img, refr, current_z, rays_per_pixel)
    R.twin(True)
    try:
        tw = R.project_to_camera(ri_img, refr, current_z, rays_per_pixel)
    finally:
        R.twin(False)
    differs = (base["moves"] != tw["moves"]) | (base["decisions"] != tw["decisions"])
    rng = float(base["proj"].max()) - float(base["proj"].min())
    e_twin = float(np.abs(base["proj"].astype(np.float64) - tw["proj"].astype(np.float64)).max()) / rng
    return base, float(differs.mean()), e_twin
