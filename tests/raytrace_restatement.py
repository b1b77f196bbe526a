"""Sequential restatement of the ray sandbox (raytracing/RayTracingTest.java, Raytrace.drawSimpleImage) and of the general tracer
under it: the yardstick of raytrace.hip.  The loops live in tests/raytrace_restatement.c, which includes aberr_restatement.c -- the
sampler, Hessian, bend_ray, injection and twin of refract3d's yardstick, unchanged.  Conventions as tests/aberrations_restatement.py;
``twin(True)`` here bends this library's libm results."""
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

KEEP, REFLECT = 0, 1


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="raytrace_restatement_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "raytrace_restatement.so")
        subprocess.check_call([shutil.which("gcc") or "gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                               "-shared", "-fPIC", os.path.join(HERE, "raytrace_restatement.c"), "-lm", "-o", so])
        L = C.CDLL(so)
        L.rs_trace_rays.restype = C.c_int64
        L.rs_trace_rays.argtypes = [_f, _f, _i64, _d, _d, _f, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int, C.c_int,
                                    C.c_double, _d, C.c_int, _f, _f, _d, _f, _i32, _u64, _d, _d, _i64, _i64, C.c_int]
        L.rs_sandbox_ray_starts.argtypes = [_u64, _i64, C.c_int, C.c_int, C.c_int64, _d, _d]
        L.rs_grid_ray_starts.restype = C.c_int64
        L.rs_grid_ray_starts.argtypes = [_i64, C.c_int, C.c_int, _d, _d]
        L.rs_draw_simple_image.argtypes = [_f, _i64, C.c_float, C.c_float]
        L.rs_inject.argtypes = [_f, _f, _i64, _d, _d, _d, C.c_int64, C.c_int]
        _lib = L
    return _lib


def twin(on):
    lib().rs_set_twin(1 if on else 0)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _shape_dim(shape):
    return (C.c_int64 * 3)(shape[2], shape[1], shape[0])


def default_max_moves(shape):
    return 4 * (shape[0] + shape[1] + shape[2])


def trace_rays(ri_img, pos3, dir3, img=None, intensity=None, n_a=0.0, n_b=1.0, ev_threshold=0.01, max_moves=None, total_reflection=KEEP,
               normalize_dirs=False, constant_value=1.0, sigma=(0.5, 0.5, 0.5), normalized=True, inject=True):
    """Returns a dict: image, weight (inject), xyz (steps, 3), value (steps), moves, decisions, end_pos, end_dir (rays), n_capped,
    n_reflected."""
    b = np.ascontiguousarray(ri_img, dtype=np.float32)
    a = None if img is None else np.ascontiguousarray(img, dtype=np.float32)
    assert b.ndim == 3 and (a is None or a.shape == b.shape)
    pos = np.ascontiguousarray(pos3, dtype=np.float64).reshape(-1, 3)
    vec = np.ascontiguousarray(dir3, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    assert len(vec) == n
    inten = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32)
    assert inten is None or len(inten) == n
    mm = default_max_moves(b.shape) if max_moves is None else int(max_moves)
    cap = max(1, n * mm)
    out = {"image": np.zeros(b.shape, np.float32), "weight": np.zeros(b.shape, np.float32), "xyz": np.zeros((cap, 3)),
           "value": np.zeros(cap, np.float32), "moves": np.zeros(n, np.int32), "decisions": np.zeros(n, np.uint64),
           "end_pos": np.zeros((n, 3)), "end_dir": np.zeros((n, 3))}
    capped, reflected = C.c_int64(0), C.c_int64(0)
    sg = (C.c_double * 3)(*[float(s) for s in sigma])
    k = lib().rs_trace_rays(_p(b, _f), _p(a, _f), _shape_dim(b.shape), _p(pos, _d), _p(vec, _d), _p(inten, _f), n, n_a, n_b, ev_threshold,
                            mm, int(total_reflection), int(bool(normalize_dirs)), constant_value, sg, int(bool(normalized)),
                            _p(out["image"], _f), _p(out["weight"], _f), _p(out["xyz"], _d), _p(out["value"], _f), _p(out["moves"], _i32),
                            _p(out["decisions"], _u64), _p(out["end_pos"], _d), _p(out["end_dir"], _d), C.byref(capped),
                            C.byref(reflected), int(bool(inject)))
    out["xyz"], out["value"] = out["xyz"][:k].copy(), out["value"][:k].copy()
    out["n_capped"], out["n_reflected"] = capped.value, reflected.value
    return out


def inject(image, weight, sigma, xyz, intensity, normalized=False):
    """addGaussian / addNormalizedGaussian per point in list order, in place (this library's copy of the injection)."""
    assert image.dtype == np.float32 and weight.dtype == np.float32 and image.flags.c_contiguous and weight.flags.c_contiguous
    pts = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    inten = np.ascontiguousarray(intensity, dtype=np.float64)
    assert len(inten) == len(pts)
    sg = (C.c_double * 3)(*[float(s) for s in sigma])
    lib().rs_inject(_p(image, _f), _p(weight, _f), _shape_dim(image.shape), sg, _p(pts, _d), _p(inten, _d), len(pts), int(normalized))


def sandbox_ray_starts(state, shape, x, z, n):
    s = C.c_uint64(state)
    pos, vec = np.zeros((n, 3)), np.zeros((n, 3))
    lib().rs_sandbox_ray_starts(C.byref(s), _shape_dim(shape), int(x), int(z), n, _p(pos, _d), _p(vec, _d))
    return pos, vec, s.value


def grid_ray_starts(shape, z, spacing):
    dim = _shape_dim(shape)
    n = lib().rs_grid_ray_starts(dim, int(z), int(spacing), None, None)
    pos, vec = np.zeros((n, 3)), np.zeros((n, 3))
    if n:
        lib().rs_grid_ray_starts(dim, int(z), int(spacing), _p(pos, _d), _p(vec, _d))
    return pos, vec


def draw_simple_image(shape, low, high):
    out = np.zeros(shape, np.float32)
    lib().rs_draw_simple_image(_p(out, _f), _shape_dim(shape), low, high)
    return out
