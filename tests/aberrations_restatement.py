"""Sequential restatement of the refraction simulator (SimulateMultiViewAberrations.java, Hessian.java, raytracing/Raytrace.java,
raytracing/Lightsheet.java, VolumeInjection.java): the yardstick of aberrations.hip.  The inner loops live in
tests/aberr_restatement.c (one ray after the other, a literal java.util.Random), compiled here with gcc; volumes are (Nz, Ny, Nx)
float32 arrays, positions (n, 3) float64 with x first.

``twin(True)`` moves every acos / asin / sin / cos / exp result by one ulp, alternating up and down: what a different but equally
good libm would do to the rays (the divergence twin of the tests)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

_f = C.POINTER(C.c_float)
_d = C.POINTER(C.c_double)
_i64 = C.POINTER(C.c_int64)
_u64 = C.POINTER(C.c_uint64)
_i32 = C.POINTER(C.c_int32)


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="aberr_restatement_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "aberr_restatement.so")
        subprocess.check_call([shutil.which("gcc") or "gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                               "-shared", "-fPIC", os.path.join(HERE, "aberr_restatement.c"), "-lm", "-o", so])
        L = C.CDLL(so)
        L.rs_largest_eigen.restype = C.c_double
        L.rs_incident_angle.restype = C.c_double
        L.rs_refract.restype = C.c_double
        L.rs_refract.argtypes = [_d, _d, C.c_double, C.c_double, C.c_double, _d]
        L.rs_lightsheet_fit.argtypes = [C.c_double] * 4 + [_d]
        L.rs_refract3d.restype = C.c_int64
        L.rs_refract3d.argtypes = [_f, _f, _i64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int64, _u64, _f, _f, _d, _f,
                                   _i32, _u64, C.c_int]
        L.rs_refract3d_ray_starts.argtypes = [_u64, _i64, C.c_int, C.c_int, _d, C.c_int64, _d, _d]
        L.rs_camera_ray_starts.argtypes = [_u64, _i64, C.c_int, _d]
        L.rs_project_to_camera.argtypes = [_f, _f, _i64, C.c_int, C.c_int, _u64, _f, _i32, _u64]
        L.rs_inject.argtypes = [_f, _f, _i64, _d, _d, _d, C.c_int64, C.c_int]
        L.rs_hessian_at.argtypes = [_f, _i64, _d, C.c_int64, _d, _d, _d]
        L.rs_hessian_images.argtypes = [_f, _i64, _f, _f]
        L.rs_normalize.argtypes = [_f, _f, C.c_int64, _f]
        L.rs_project.argtypes = [_f, _f, _i64, _f]
        L.rs_inject_info.argtypes = [_d, _i32, _d, _i32]
        _lib = L
    return _lib


def twin(on):
    lib().rs_set_twin(1 if on else 0)


def seed_state(seed):
    """The 48-bit state of ``new java.util.Random(seed)``."""
    return (int(seed) ^ 0x5DEECE66D) & ((1 << 48) - 1)


def _vol(a):
    v = np.ascontiguousarray(a, dtype=np.float32)
    assert v.ndim == 3
    return v


def _dim(v):
    return (C.c_int64 * 3)(v.shape[2], v.shape[1], v.shape[0])


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _vec(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def largest_eigen(matrix):
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(9)
    vec = np.zeros(3)
    ev = lib().rs_largest_eigen(_p(m, _d), _p(vec, _d))
    return ev, vec


def eig_all(matrix):
    """Eigenvalues ascending and the eigenvectors as columns."""
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(9)
    d, V = np.zeros(3), np.zeros((3, 3))
    lib().rs_eig_all(_p(m, _d), _p(d, _d), _p(V, _d))
    return d, V


def hessian_at(img, xyz):
    v = _vol(img)
    pts = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    m, vec, val = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n)
    lib().rs_hessian_at(_p(v, _f), _dim(v), _p(pts, _d), n, _p(m, _d), _p(vec, _d), _p(val, _d))
    return m, vec, val


def hessian_images(img):
    v = _vol(img)
    val = np.zeros(v.shape, dtype=np.float32)
    vec = np.zeros((3,) + v.shape, dtype=np.float32)
    lib().rs_hessian_images(_p(v, _f), _dim(v), _p(val, _f), _p(vec, _f))
    return val, vec


def incident_angle(i, n):
    """Returns (thetaI, the normal as incidentAngle leaves it)."""
    nn = _vec(n)
    t = lib().rs_incident_angle(_vec(i), nn)
    return t, np.array(nn[:])


def refract(i, n, n0, n1, theta_i):
    t = (C.c_double * 3)()
    theta_t = lib().rs_refract(_vec(i), _vec(n), n0, n1, theta_i, t)
    return theta_t, np.array(t[:])


def reflect(i, n):
    r = (C.c_double * 3)()
    lib().rs_reflect(_vec(i), _vec(n), r)
    return np.array(r[:])


def lightsheet_fit(center, thickness_center, length, thickness_edges):
    abc = (C.c_double * 3)()
    if lib().rs_lightsheet_fit(center, thickness_center, length, thickness_edges, abc) != 0:
        raise ValueError("Cannot not invert Delta-Matrix, failed to fit function")
    return tuple(abc[:])


def inject_info(sigma):
    size = (C.c_int32 * 3)()
    sw, npx = C.c_double(), C.c_int32()
    lib().rs_inject_info(_vec(sigma), size, C.byref(sw), C.byref(npx))
    return list(size), sw.value, npx.value


def inject(image, weight, sigma, xyz, intensity, normalized=False):
    """addGaussian / addNormalizedGaussian per point in list order, in place on contiguous float32 (Nz, Ny, Nx) arrays."""
    assert image.dtype == np.float32 and weight.dtype == np.float32 and image.flags.c_contiguous and weight.flags.c_contiguous
    pts = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    inten = np.ascontiguousarray(intensity, dtype=np.float64)
    assert len(inten) == len(pts)
    lib().rs_inject(_p(image, _f), _p(weight, _f), _dim(image), _vec(sigma), _p(pts, _d), _p(inten, _d), len(pts), int(normalized))


def normalize(image, weight):
    out = np.empty_like(image)
    lib().rs_normalize(_p(image, _f), _p(weight, _f), image.size, _p(out, _f))
    return out


def project(image, weight):
    out = np.empty(image.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        lib().rs_project(_p(image, _f), _p(weight, _f), _dim(image), _p(out, _f))
    return out


def refract3d_ray_starts(state, shape, illum, z, abc, n):
    s = C.c_uint64(state)
    dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
    pos, vec = np.zeros((n, 3)), np.zeros((n, 3))
    lib().rs_refract3d_ray_starts(C.byref(s), dim, int(illum), int(z), _vec(abc), n, _p(pos, _d), _p(vec, _d))
    return pos, vec, s.value


def camera_ray_starts(state, shape, rays_per_pixel):
    s = C.c_uint64(state)
    dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
    pos = np.zeros((shape[1] * shape[2] * rays_per_pixel, 3))
    lib().rs_camera_ray_starts(C.byref(s), dim, rays_per_pixel, _p(pos, _d))
    return pos, s.value


def refract3d(img, ri_img, illum, z, ls_middle, ls_edge, ri, num_rays, state=None, inject=True):
    """Returns a dict: image, weight, xyz (steps, 3), value (steps), moves (rays), decisions (rays: a hash of every branch the ray
    took and of Math.round of its positions), state (the generator afterwards)."""
    a, b = _vol(img), _vol(ri_img)
    assert a.shape == b.shape
    s = C.c_uint64(seed_state(2423) if state is None else state)
    cap = num_rays * a.shape[0]
    out = {"image": np.zeros(a.shape, np.float32), "weight": np.zeros(a.shape, np.float32), "xyz": np.zeros((cap, 3)),
           "value": np.zeros(cap, np.float32), "moves": np.zeros(num_rays, np.int32), "decisions": np.zeros(num_rays, np.uint64)}
    n = lib().rs_refract3d(_p(a, _f), _p(b, _f), _dim(a), int(illum), int(z), ls_middle, ls_edge, ri, num_rays, C.byref(s),
                           _p(out["image"], _f), _p(out["weight"], _f), _p(out["xyz"], _d), _p(out["value"], _f), _p(out["moves"], _i32),
                           _p(out["decisions"], _u64), int(inject))
    if n < 0:
        raise ValueError("light sheet fit failed")
    out["xyz"], out["value"], out["state"] = out["xyz"][:n], out["value"][:n], s.value
    return out


def project_to_camera(ri_img, refr, current_z, rays_per_pixel=500, state=None):
    a, b = _vol(ri_img), _vol(refr)
    assert a.shape == b.shape
    s = C.c_uint64(seed_state(464232194) if state is None else state)
    nrays = a.shape[1] * a.shape[2] * rays_per_pixel
    out = {"proj": np.zeros(a.shape[1:], np.float32), "moves": np.zeros(nrays, np.int32), "decisions": np.zeros(nrays, np.uint64)}
    lib().rs_project_to_camera(_p(a, _f), _p(b, _f), _dim(a), int(current_z), rays_per_pixel, C.byref(s), _p(out["proj"], _f),
                               _p(out["moves"], _i32), _p(out["decisions"], _u64))
    out["state"] = s.value
    return out


def smooth_blobs(shape, seed, count=6, sigma=(0.18, 0.3), lo=0.0, hi=1.0):
    """A smooth field in [lo, hi]: a sum of wide Gaussians (widths as fractions of the smallest dimension), range-normalised."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = np.zeros(shape, dtype=np.float64)
    for _ in range(count):
        c = rng.random(3) * np.array([nz, ny, nx])
        s = (sigma[0] + rng.random() * (sigma[1] - sigma[0])) * min(shape)
        f += rng.random() * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    f = (f - f.min()) / (f.max() - f.min())
    return np.ascontiguousarray(lo + (hi - lo) * f, dtype=np.float32)
