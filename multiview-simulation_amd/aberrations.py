"""Mirror of the reference's refraction simulator, ``net.preibisch.simulation.SimulateMultiViewAberrations``, and of the classes it
is made of (``Hessian``, ``raytracing.Raytrace``, ``raytracing.Lightsheet``, ``VolumeInjection``): names and argument order of the
Java methods.  The rays are traced and injected by the HIP kernels of aberrations.hip through the ``Context`` methods below; the
single-vector helpers of ``Raytrace`` and the light-sheet fit are a handful of fp64 operations and run on the host.

Volumes are ``(Nz, Ny, Nx)`` float32 arrays, positions ``(n, 3)`` float64 with x first.  Random numbers come from a ``JavaRandom``
that is advanced exactly as the reference advances its ``java.util.Random``.

The simulator's own phantom, ``simulate(rnd, dir)`` (:408-440), is ``simulatePhantom``: everything behind its ``Tools.open(dir +
"block4.tif")``.  The reference does not ship that file, so the caller passes the canvas of refractive indices (or a directory that
holds the file; ``synthetic.index_block`` is a stand-in).  ``multiSpheres`` uses the ranges the reference hard-codes; its
``min == max`` branches never run and are not offered.

The ray sandbox, ``raytracing.RayTracingTest``, sits on the general tracer of raytrace.hip (``Context.trace_rays``: the caller's
rays through the same move); ``RefractiveIndexMap`` is the linear map that tracer takes, ``ClearingMap`` the reference's stub.
``cluster/`` stays out of scope, as in the C ABI."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)


def _vol(a, name="image") -> np.ndarray:
    v = np.ascontiguousarray(a, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError(f"{name}: expected 3 dimensions, got {v.ndim}")
    return v


def _dim(v):
    nz, ny, nx = v.shape
    return (C.c_int64 * 3)(nx, ny, nz)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _vec3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _points(xyz) -> np.ndarray:
    return np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)


class _State:
    """The 48-bit state of a JavaRandom as the uint64 the C ABI advances; written back on exit."""

    def __init__(self, rnd, default_seed):
        from . import JavaRandom
        self.rnd = JavaRandom(default_seed) if rnd is None else rnd
        if not isinstance(self.rnd, JavaRandom):
            raise TypeError("rnd must be a JavaRandom (the generator is jumped ahead natively)")
        self.c = C.c_uint64(self.rnd._s)

    def commit(self):
        self.rnd._s = int(self.c.value)


class ContextAberrations:
    """The refraction simulator's entry points of a ``Context`` (aberrations.hip through include/mvsim.h)."""

    def hessian_at(self, img, xyz):
        """Hessian of the interpolated, mirrored image at real positions and its largest eigenpair:
        (matrix (n, 3, 3), eigenvector (n, 3), eigenvalue (n))."""
        v, pts = _vol(img), _points(xyz)
        n = len(pts)
        m, vec, val = np.empty((n, 3, 3)), np.empty((n, 3)), np.empty(n)
        _lib.check(self._L.mvsim_hessian_at(self._h, _p(v), _dim(v), _d(pts), n, _d(m), _d(vec), _d(val)))
        return m, vec, val

    def hessian_images(self, img):
        """Hessian.java:69-99 at every voxel: (eigenvalue image (Nz, Ny, Nx), eigenvector image (3, Nz, Ny, Nx))."""
        v = _vol(img)
        val = np.empty(v.shape, dtype=np.float32)
        vec = np.empty((3,) + v.shape, dtype=np.float32)
        _lib.check(self._L.mvsim_hessian_images(self._h, _p(v), _dim(v), _p(val), _p(vec)))
        return val, vec

    def refract3d_ray_starts(self, shape, illum, z, abc, n, rnd=None):
        """The starts of refract3d's first n rays for a (Nz, Ny, Nx) volume: (positions (n, 3), directions (n, 3)); rnd advances."""
        st = _State(rnd, 2423)
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        pos, vec = np.empty((n, 3)), np.empty((n, 3))
        _lib.check(self._L.mvsim_refract3d_ray_starts(self._h, C.byref(st.c), dim, int(bool(illum)), int(z), _vec3(abc), n, _d(pos), _d(vec)))
        st.commit()
        return pos, vec

    def camera_ray_starts(self, shape, rays_per_pixel=500, rnd=None):
        """The starts of projectToCamera's rays, pixel-major: (Ny * Nx * rays_per_pixel, 3); rnd advances."""
        st = _State(rnd, 464232194)
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        pos = np.empty((shape[1] * shape[2] * rays_per_pixel, 3))
        _lib.check(self._L.mvsim_camera_ray_starts(self._h, C.byref(st.c), dim, rays_per_pixel, _d(pos)))
        st.commit()
        return pos

    def refract3d(self, img, ri_img, illum, z, ls_middle, ls_edge, ri, num_rays=200000, rnd=None, steps=False, inject=True) -> dict:
        """SimulateMultiViewAberrations.refract3d (:261-401).  Returns {"image", "weight"} (inject) and, with steps=True,
        {"xyz" (steps, 3), "value" (steps), "moves" (rays)}: the step list in ray order, then move order."""
        a, b = _vol(img, "imgIn"), _vol(ri_img, "imgRi")
        if a.shape != b.shape:
            raise ValueError("imgIn and imgRi must have the same dimensions")
        st = _State(rnd, 2423)                                                                    # :305
        out = {}
        if inject:
            out["image"], out["weight"] = np.empty(a.shape, np.float32), np.empty(a.shape, np.float32)
        rs = None
        if steps:
            cap = max(1, int(num_rays)) * a.shape[0]
            xyz, val, mv = np.empty((cap, 3)), np.empty(cap, np.float32), np.empty(max(1, int(num_rays)), np.int32)
            rs = _lib.RaySteps(cap, 0, _d(xyz), val.ctypes.data_as(C.POINTER(C.c_float)), mv.ctypes.data_as(C.POINTER(C.c_int32)))
        _lib.check(self._L.mvsim_refract3d(self._h, _p(a), _p(b), _dim(a), int(bool(illum)), int(z), float(ls_middle), float(ls_edge),
                                           float(ri), int(num_rays), C.byref(st.c), _p(out.get("image")), _p(out.get("weight")),
                                           None if rs is None else C.byref(rs)))
        st.commit()
        if steps:
            out["xyz"], out["value"], out["moves"] = xyz[:rs.n].copy(), val[:rs.n].copy(), mv[:int(num_rays)]
        return out

    def volume_inject(self, image, weight, sigma, xyz, intensity, normalized=False) -> None:
        """VolumeInjection.addGaussian / addNormalizedGaussian for every point in list order, in place on float32 volumes."""
        for a, name in ((image, "image"), (weight, "weight")):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or not a.flags.writeable or a.ndim != 3:
                raise ValueError(f"{name}: in-place injection needs a writable C-contiguous 3-D float32 numpy array")
        if image.shape != weight.shape:
            raise ValueError("image and weight must have the same dimensions")
        pts = _points(xyz)
        inten = np.ascontiguousarray(intensity, dtype=np.float64).reshape(-1)
        if len(inten) != len(pts):
            raise ValueError("one intensity per point")
        _lib.check(self._L.mvsim_volume_inject(self._h, _p(image), _p(weight), _dim(image), _vec3(sigma), _d(pts), _d(inten), len(pts),
                                               int(bool(normalized))))

    def volume_normalize(self, image, weight) -> np.ndarray:
        a, w = _vol(image), _vol(weight, "weight")
        if a.shape != w.shape:
            raise ValueError("image and weight must have the same dimensions")
        out = np.empty_like(a)
        _lib.check(self._L.mvsim_volume_normalize(self._h, _p(a), _p(w), a.size, _p(out)))
        return out

    def volume_project(self, image, weight) -> np.ndarray:
        a, w = _vol(image), _vol(weight, "weight")
        if a.shape != w.shape:
            raise ValueError("image and weight must have the same dimensions")
        out = np.empty(a.shape[1:], dtype=np.float32)
        _lib.check(self._L.mvsim_volume_project(self._h, _p(a), _p(w), _dim(a), _p(out)))
        return out

    def project_to_camera(self, ri_img, refr, current_z, rays_per_pixel=500, rnd=None) -> np.ndarray:
        """SimulateMultiViewAberrations.projectToCamera (:89-254): the (Ny, Nx) camera image of plane current_z."""
        a, b = _vol(ri_img, "imgRi"), _vol(refr, "refr")
        if a.shape != b.shape:
            raise ValueError("imgRi and refr must have the same dimensions")
        st = _State(rnd, 464232194)
        out = np.empty(a.shape[1:], dtype=np.float32)
        _lib.check(self._L.mvsim_project_to_camera(self._h, _p(a), _p(b), _dim(a), int(current_z), int(rays_per_pixel), C.byref(st.c),
                                                   _p(out)))
        st.commit()
        return out


    # ---- the general tracer and the ray sandbox (raytrace.hip) ----
    def _trace_params(self, dim, n_a, n_b, ev_threshold, max_moves, total_reflection, normalize_dirs, constant_value, sigma, normalized):
        tp = _lib.TraceParams()
        _lib.check(self._L.mvsim_trace_params_default(dim, C.byref(tp)))
        tp.n_a, tp.n_b, tp.ev_threshold = float(n_a), float(n_b), float(ev_threshold)
        if max_moves is not None:
            tp.max_moves = int(max_moves)
        policies = {"keep": _lib.MVSIM_TRACE_KEEP, "reflect": _lib.MVSIM_TRACE_REFLECT}
        if total_reflection not in policies:
            raise ValueError("total_reflection must be 'keep' or 'reflect'")
        tp.total_reflection = policies[total_reflection]
        tp.normalize_dirs, tp.constant_value, tp.normalized = int(bool(normalize_dirs)), float(constant_value), int(bool(normalized))
        tp.sigma[0], tp.sigma[1], tp.sigma[2] = (float(x) for x in sigma)
        return tp

    def _trace_call(self, fn, ri_p, img_p, dim, pos3, dir3, intensity, tp, image_p, weight_p, steps, ends):
        pos, vec = _points(pos3), _points(dir3)
        n = len(pos)
        if len(vec) != n:
            raise ValueError("one direction per ray")
        inten = None
        if intensity is not None:
            inten = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
            if len(inten) != n:
                raise ValueError("one intensity per ray")
        out, rs = {}, None
        if steps:
            cap = max(1, n) * int(tp.max_moves)
            xyz, val, mv = np.empty((cap, 3)), np.empty(cap, np.float32), np.empty(max(1, n), np.int32)
            rs = _lib.RaySteps(cap, 0, _d(xyz), val.ctypes.data_as(C.POINTER(C.c_float)), mv.ctypes.data_as(C.POINTER(C.c_int32)))
        if ends:
            out["end_pos"], out["end_dir"] = np.empty((n, 3)), np.empty((n, 3))
        capped = C.c_int64(0)
        _lib.check(fn(self._h, ri_p, img_p, dim, _d(pos), _d(vec), None if inten is None else inten.ctypes.data_as(C.POINTER(C.c_float)), n,
                      C.byref(tp), image_p, weight_p, None if rs is None else C.byref(rs), _d(out.get("end_pos")), _d(out.get("end_dir")),
                      C.byref(capped)))
        if steps:
            out["xyz"], out["value"], out["moves"] = xyz[:rs.n].copy(), val[:rs.n].copy(), mv[:n]
        out["n_capped"] = int(capped.value)
        return out

    def trace_rays(self, ri_img, pos3, dir3, img=None, intensity=None, n_a=0.0, n_b=1.0, ev_threshold=0.01, max_moves=None,
                   total_reflection="keep", normalize_dirs=False, constant_value=1.0, sigma=(0.5, 0.5, 0.5), normalized=True, steps=False,
                   inject=True, ends=True) -> dict:
        """Caller-supplied rays through the move of refract3d (mvsim_trace_rays).  ri_img: the index volume, mapped by
        n = (n_b - n_a) * sample + n_a; the value a ray carries: the sample of ``img``, else ``intensity`` per ray, else
        ``constant_value``.  max_moves: 4 * (Nx + Ny + Nz) by default.  Returns {"image", "weight"} (inject), {"xyz", "value", "moves"}
        (steps=True), {"end_pos", "end_dir"} (ends) and "n_capped": the rays still inside after max_moves moves."""
        b = _vol(ri_img, "imgRi")
        a = None if img is None else _vol(img, "imgIn")
        if a is not None and a.shape != b.shape:
            raise ValueError("imgIn and imgRi must have the same dimensions")
        dim = _dim(b)
        tp = self._trace_params(dim, n_a, n_b, ev_threshold, max_moves, total_reflection, normalize_dirs, constant_value, sigma, normalized)
        image = np.empty(b.shape, np.float32) if inject else None
        weight = np.empty(b.shape, np.float32) if inject else None
        out = self._trace_call(self._L.mvsim_trace_rays, _p(b), _p(a), dim, pos3, dir3, intensity, tp, _p(image), _p(weight), steps, ends)
        if inject:
            out["image"], out["weight"] = image, weight
        return out

    def trace_rays_dev(self, ri_dev, shape, pos3, dir3, img_dev=None, intensity=None, image_dev=None, weight_dev=None, n_a=0.0, n_b=1.0,
                       ev_threshold=0.01, max_moves=None, total_reflection="keep", normalize_dirs=False, constant_value=1.0,
                       sigma=(0.5, 0.5, 0.5), normalized=True, steps=False, ends=True) -> dict:
        """trace_rays on DEVICE volumes of (Nz, Ny, Nx) floats (addresses as dev_alloc returns them); image_dev and weight_dev, given
        together or not at all, are ADDED to.  Ray lists and every returned list are host arrays."""
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        tp = self._trace_params(dim, n_a, n_b, ev_threshold, max_moves, total_reflection, normalize_dirs, constant_value, sigma, normalized)
        vp = lambda q: None if q is None else C.c_void_p(int(q))
        return self._trace_call(self._L.mvsim_trace_rays_dev, vp(ri_dev), vp(img_dev), dim, pos3, dir3, intensity, tp, vp(image_dev),
                                vp(weight_dev), steps, ends)

    def sandbox_ray_starts(self, shape, x, z, n, rnd=None):
        """RayTracingTest.drawMultipleRays' bundle (:110-123) for a (Nz, Ny, Nx) volume: (positions (n, 3), directions (n, 3)); rnd
        (new Random(234345) by default) advances."""
        st = _State(rnd, 234345)
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        pos, vec = np.empty((n, 3)), np.empty((n, 3))
        _lib.check(self._L.mvsim_sandbox_ray_starts(self._h, C.byref(st.c), dim, int(x), int(z), n, _d(pos), _d(vec)))
        st.commit()
        return pos, vec

    def grid_ray_starts(self, shape, z, spacing):
        """RayTracingTest.drawRays' grid (:334-344): (positions (Nx // spacing, 3), directions)."""
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        n = C.c_int64(0)
        _lib.check(self._L.mvsim_grid_ray_starts(self._h, dim, int(z), int(spacing), 0, None, None, C.byref(n)))
        pos, vec = np.empty((n.value, 3)), np.empty((n.value, 3))
        if n.value:
            _lib.check(self._L.mvsim_grid_ray_starts(self._h, dim, int(z), int(spacing), n.value, _d(pos), _d(vec), C.byref(n)))
        return pos, vec

    def draw_simple_image(self, shape, low, high) -> np.ndarray:
        """Raytrace.drawSimpleImage (:96-128): the wedge as a (Nz, Ny, Nx) volume."""
        out = np.empty(tuple(int(k) for k in shape), np.float32)
        _lib.check(self._L.mvsim_draw_simple_image(self._h, _p(out), _dim(out), float(low), float(high)))
        return out

    def hessian_plane(self, img, z, vectors=False):
        """Plane z of hessian_images at the cost of one plane: the eigenvalue plane (Ny, Nx), with vectors=True
        (eigenvalue plane, eigenvector planes (3, Ny, Nx))."""
        v = _vol(img)
        val = np.empty(v.shape[1:], np.float32)
        vec = np.empty((3,) + v.shape[1:], np.float32) if vectors else None
        _lib.check(self._L.mvsim_hessian_plane(self._h, _p(v), _dim(v), int(z), _p(val), _p(vec)))
        return (val, vec) if vectors else val


def _ctx():
    from . import default_context
    return default_context()


class Lightsheet:
    """raytracing/Lightsheet.java: the thickness a x x + b x + c fitted through centre and both edges."""

    def __init__(self, center, thicknessCenter=None, length=None, thickNessEdges=None):
        if thicknessCenter is not None and thickNessEdges is None:      # Lightsheet(a, b, c), :66-71
            self.a, self.b, self.c = float(center), float(thicknessCenter), float(length)
            return
        abc = (C.c_double * 3)()
        _lib.check(_lib.load().mvsim_lightsheet_fit(float(center), float(thicknessCenter), float(length), float(thickNessEdges), abc))
        self.a, self.b, self.c = abc[0], abc[1], abc[2]

    def getA(self):
        return self.a

    def getB(self):
        return self.b

    def getC(self):
        return self.c

    def predict(self, x: float) -> float:
        return self.a * x * x + self.b * x + self.c


class Raytrace:
    """raytracing/Raytrace.java :32-93 on single vectors (host fp64; the kernels hold the same operations)."""

    @staticmethod
    def reflect(i, n, r) -> None:
        dotP = i[0] * n[0] + i[1] * n[1] + i[2] * n[2]
        for d in range(3):
            r[d] = i[d] - 2 * dotP * n[d]

    @staticmethod
    def refract(i, n, n0, n1, thetaI, t) -> float:
        deltaN = n0 / n1
        s = deltaN * math.sin(thetaI)
        thetaT = math.asin(s) if -1.0 <= s <= 1.0 else float("nan")
        if math.isnan(thetaT):
            return thetaT
        cosThetaI = math.cos(thetaI)
        sinThetaT = math.sin(thetaT)
        for d in range(3):
            t[d] = deltaN * i[d] - n[d] * (deltaN * cosThetaI - math.sqrt(1 - sinThetaT * sinThetaT))
        return thetaT

    @staticmethod
    def length(v) -> float:
        return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])

    @staticmethod
    def norm(v) -> None:
        l = Raytrace.length(v)
        for d in range(3):
            v[d] /= l

    @staticmethod
    def drawSimpleImage(randomAccessible, low, high, ctx=None) -> None:
        """:96-128 -- the wedge, in place on a writable C-contiguous (Nz, Ny, Nx) float32 array."""
        a = randomAccessible
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 3 or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("drawSimpleImage needs a writable C-contiguous 3-D float32 numpy array")
        a[...] = (ctx or _ctx()).draw_simple_image(a.shape, low, high)

    @staticmethod
    def incidentAngle(i, n) -> float:
        """:75-93 -- flips n in place and SUBTRACTS pi / 2 when the angle is >= pi / 2 (the reference's quirk, kept)."""
        c = (n[0] * i[0] + n[1] * i[1] + n[2] * i[2]) / (math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) *
                                                           math.sqrt(i[0] * i[0] + i[1] * i[1] + i[2] * i[2]))
        thetaI = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")
        if thetaI >= math.pi / 2:
            for d in range(3):
                n[d] *= -1
            thetaI -= math.pi / 2
        return thetaI


class RefractiveIndexMap:
    """raytracing/RefractiveIndexMap.java, as the linear map the tracers apply: getRI(i) = (n_b - n_a) * i + n_a.  (1, ri) is
    refract3d's map, (0, 1) the sandbox's raw index image."""

    def __init__(self, n_a=0.0, n_b=1.0):
        self.n_a, self.n_b = float(n_a), float(n_b)

    def getRI(self, intensity: float) -> float:
        return (self.n_b - self.n_a) * intensity + self.n_a


class ClearingMap(RefractiveIndexMap):
    """raytracing/ClearingMap.java: the reference's stub, getRI returns 0."""

    def __init__(self):
        super().__init__(0.0, 0.0)

    def getRI(self, intensity: float) -> float:
        return 0


class Hessian:
    """Hessian.java on the GPU."""

    @staticmethod
    def largestEigenVector(img):
        """:46-102 without the Gauss3 blur (blur the image first to follow the reference to the letter): (eigenvalue image,
        eigenvector image (3, Nz, Ny, Nx))."""
        return _ctx().hessian_images(img)

    @staticmethod
    def computeHessianMatrix3D(img, position) -> np.ndarray:
        """:155-278 at one real position of the interpolated, mirrored image."""
        return _ctx().hessian_at(img, [position])[0][0]

    @staticmethod
    def computeLargestEigenVectorAndValue3d(img, position):
        """:110-147 of the Hessian at one real position: (eigenvalue, eigenvector)."""
        _, vec, val = _ctx().hessian_at(img, [position])
        return float(val[0]), vec[0]


class VolumeInjection:
    """VolumeInjection.java: Gaussians added to an image and a weight volume in call order."""

    def __init__(self, image, weight, sigma, ctx=None):
        self.image, self.weight, self.sigma = image, weight, [float(s) for s in sigma]
        self._ctx = ctx
        size = (C.c_int32 * 3)()
        sw, npx = C.c_double(), C.c_int32()
        _lib.check(_lib.load().mvsim_volume_inject_info(_vec3(self.sigma), size, C.byref(sw), C.byref(npx)))
        self.size, self.sumWeights, self.numPixels = list(size), sw.value, npx.value

    def _c(self):
        return self._ctx or _ctx()

    def getSize(self):
        return self.size

    def getImage(self):
        return self.image

    def getWeight(self):
        return self.weight

    def getSumWeights(self):
        return self.sumWeights

    def getNumPixels(self):
        return self.numPixels

    def addGaussian(self, intensity, location) -> None:
        self._c().volume_inject(self.image, self.weight, self.sigma, [location], [intensity], False)

    def addNormalizedGaussian(self, intensity, location) -> None:
        self._c().volume_inject(self.image, self.weight, self.sigma, [location], [intensity], True)

    def addGaussians(self, intensities, locations, normalized=False) -> None:
        """Many calls of addGaussian / addNormalizedGaussian in list order as one launch sequence."""
        self._c().volume_inject(self.image, self.weight, self.sigma, locations, intensities, normalized)

    def normalize(self) -> np.ndarray:
        return self._c().volume_normalize(self.image, self.weight)

    def project(self) -> np.ndarray:
        return self._c().volume_project(self.image, self.weight)


class SimulateMultiViewAberrations:
    """net.preibisch.simulation.SimulateMultiViewAberrations."""

    @staticmethod
    def _rnd():
        from . import JavaRandom
        if SimulateMultiViewAberrations.rnd is None:
            SimulateMultiViewAberrations.rnd = JavaRandom(464232194)                            # :78
        return SimulateMultiViewAberrations.rnd

    rnd = None

    @staticmethod
    def inside(rayPosition, interval) -> bool:
        """:80-87 -- interval: a (Nz, Ny, Nx) array or shape."""
        shape = getattr(interval, "shape", interval)
        return all(0 <= rayPosition[d] <= shape[2 - d] - 1 for d in range(len(rayPosition)))

    @staticmethod
    def refract3d(imgIn, imgRi, illum, z, lsMiddle, lsEdge, ri, numRays=200000, ctx=None) -> VolumeInjection:
        """:261-401 -- the reference's 200 000 rays from new Random(2423)."""
        c = ctx or _ctx()
        out = c.refract3d(imgIn, imgRi, illum, z, lsMiddle, lsEdge, ri, num_rays=numRays)
        return VolumeInjection(out["image"], out["weight"], [0.5, 0.5, 0.5], ctx=ctx)

    @staticmethod
    def projectToCamera(imgRi, refr, ri, currentzPlane, raysPerPixel=500, ctx=None) -> np.ndarray:
        """:89-254 -- draws from the class's generator; ``ri`` is accepted and unused, as in the reference (:117)."""
        c = ctx or _ctx()
        return c.project_to_camera(imgRi, refr, currentzPlane, raysPerPixel, SimulateMultiViewAberrations._rnd())

    @staticmethod
    def downSample2x(img) -> np.ndarray:
        """:442-472 -- the kernel of SimulateMultiViewDataset.downSample2x."""
        return _ctx().downsample2x(img)

    @staticmethod
    def multiSpheres(image, ri, scale, rnd, ctx=None) -> int:
        """:474-586, in place on two float32 volumes of one shape; returns the number of small spheres drawn."""
        return (ctx or _ctx()).multi_spheres(image, ri, scale, rnd)

    @staticmethod
    def simulatePhantom(rnd=None, ri=None, dir=None, scale=2, ctx=None):
        """simulate(rnd, dir) (:408-440): noise on the index canvas, multiSpheres on a zero image and the canvas, both down-sampled
        2x.  ``ri``: the (Nz, Ny, Nx) canvas the reference reads from block4.tif (580^3 there), or ``dir``: where that file is, opened
        through Tools.open.  ``rnd``: the class's generator by default.  Returns (img, ri)."""
        if ri is None:
            if dir is None:
                raise ValueError("simulatePhantom needs the index canvas (ri=) or the directory of block4.tif (dir=)")
            from . import Tools
            ri = Tools.open(str(dir) + "block4.tif")
        return (ctx or _ctx()).simulate_aberration_phantom(ri, SimulateMultiViewAberrations._rnd() if rnd is None else rnd, scale)

    @staticmethod
    def simulate(imgIn, imgRi, illum, lsMiddle, lsEdge, ri, z, numRays=200000, raysPerPixel=500, ctx=None) -> dict:
        """What simulate(illum, lsMiddle, lsEdge, ri, dir, service, z) computes for one z plane on a given image / index pair:
        {"refr_img", "refr_weight", "proj"}; the caller saves them."""
        c = ctx or _ctx()
        out = c.refract3d(imgIn, imgRi, illum, z, lsMiddle, lsEdge, ri, num_rays=numRays)
        proj = c.project_to_camera(imgRi, out["image"], z, raysPerPixel, SimulateMultiViewAberrations._rnd())
        return {"refr_img": out["image"], "refr_weight": out["weight"], "proj": proj}


class RayTracingTest:
    """net.preibisch.simulation.raytracing.RayTracingTest: the ray sandbox, on Context.trace_rays.  The reference's loops have no
    move cap; the mirror passes max_moves = 4 * (Nx + Ny + Nz) and raises if a ray is still inside after that many moves, because the
    result would not be the reference's.  An index map other than the sandbox's raw image is a ``RefractiveIndexMap``."""

    @staticmethod
    def _trace(imgIn, pos, vec, ctx, riMap, steps=False, inject=True):
        c = ctx or _ctx()
        m = riMap or RefractiveIndexMap(0.0, 1.0)
        v = _vol(imgIn, "imgIn")
        out = c.trace_rays(v, pos, vec, n_a=m.n_a, n_b=m.n_b, max_moves=4 * sum(v.shape), steps=steps, inject=inject, ends=False)
        if out["n_capped"] > 0:
            raise RuntimeError(f"{out['n_capped']} rays were still inside the image after {4 * sum(v.shape)} moves: the reference would "
                               "go on tracing them")
        return out

    @staticmethod
    def hessian(img, z, ctx=None) -> np.ndarray:
        """:55-84 -- a copy of img with plane z replaced by the largest eigenvalue of the Hessian."""
        out = np.array(_vol(img), dtype=np.float32, copy=True)
        out[int(z)] = (ctx or _ctx()).hessian_plane(img, z)
        return out

    @staticmethod
    def drawMultipleRays(imgIn, z, x, numRays, ctx=None, riMap=None) -> VolumeInjection:
        """:86-194 -- numRays rays from new Random(234345) around (x, Ny - 1, z), going down y."""
        c = ctx or _ctx()
        pos, vec = c.sandbox_ray_starts(np.shape(imgIn), x, z, int(numRays))
        out = RayTracingTest._trace(imgIn, pos, vec, c, riMap)
        return VolumeInjection(out["image"], out["weight"], [0.5, 0.5, 0.5], ctx=ctx)

    @staticmethod
    def drawRays(imgIn, z, spacing, ctx=None, riMap=None) -> VolumeInjection:
        """:308-415 -- one ray every ``spacing`` voxels of x from (x, Ny - 25, z), going down y."""
        c = ctx or _ctx()
        pos, vec = c.grid_ray_starts(np.shape(imgIn), z, spacing)
        out = RayTracingTest._trace(imgIn, pos, vec, c, riMap)
        return VolumeInjection(out["image"], out["weight"], [0.5, 0.5, 0.5], ctx=ctx)

    @staticmethod
    def drawSingleRay(imgIn, z, x, ctx=None, riMap=None) -> np.ndarray:
        """:196-306 -- the ray from (x, Ny - 25, z): the stack (moves, Ny, Nx) of the weight's plane z after each move, built from
        the step list by injecting step after step.  The text overlay is not restated."""
        c = ctx or _ctx()
        v = _vol(imgIn, "imgIn")
        out = RayTracingTest._trace(v, [[float(x), float(v.shape[1] - 25), float(z)]], [[0.0, -1.0, 0.0]], c, riMap, steps=True, inject=False)
        image, weight = np.zeros(v.shape, np.float32), np.zeros(v.shape, np.float32)
        frames = np.empty((len(out["xyz"]),) + v.shape[1:], np.float32)
        for k in range(len(out["xyz"])):
            c.volume_inject(image, weight, (0.5, 0.5, 0.5), out["xyz"][k:k + 1], out["value"][k:k + 1].astype(np.float64), True)
            frames[k] = RayTracingTest.getProcessor(weight, z)
        return frames

    @staticmethod
    def getProcessor(img, z) -> np.ndarray:
        """:417-437 -- a copy of plane z."""
        return np.array(np.asarray(img)[int(z)], dtype=np.float32, copy=True)

    @staticmethod
    def renderDifferentNAs(size=(300, 300, 10), naFrom=1.0, naTo=2.0, naStep=0.01, z=5, spacing=8, ctx=None) -> np.ndarray:
        """:439-463 -- for na = naFrom; na <= naTo; na += naStep: the wedge (1.0, (float)na) of ``size`` = (Nx, Ny, Nz),
        drawRays(wedge, z, spacing), plane z of its weight.  Returns the stack.  na is accumulated in fp64 as the reference's loop
        does: its defaults give 100 scenes, 1.0 .. 1.99, because the sum passes 2 before the 101st."""
        c = ctx or _ctx()
        shape = (int(size[2]), int(size[1]), int(size[0]))
        frames = []
        na = float(naFrom)
        while na <= naTo:
            wedge = c.draw_simple_image(shape, 1.0, np.float32(na))
            frames.append(RayTracingTest.getProcessor(RayTracingTest.drawRays(wedge, z, spacing, ctx=c).getWeight(), z))
            na += naStep
        return np.stack(frames) if frames else np.empty((0, shape[1], shape[2]), np.float32)
