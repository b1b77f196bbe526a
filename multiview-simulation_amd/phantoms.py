"""Mirror of the reference's procedural phantom, ``HypersphereCollectionRealRandomAccessible.main`` (:199-286): a Perlin field
(``PerlinNoiseRealRandomAccessible``), sets of spheres (``HypersphereCollectionRealRandomAccessible``), the two forms of
``SimpleCalculatedRealRandomAccessible`` that ``main`` uses, and ``PointRejectionSampling``.  Values, rasters and the sampler run in
the HIP kernels of procedural.hip through ``ContextPhantoms``; the draws replay ``java.util.Random``.

Positions are (x, y, z); ``dim`` and ``origin`` are (x, y, z) too; rasters are ``(Nz, Ny, Nx)`` float32 arrays.  The arithmetic
contract -- what equals a literal restatement bit for bit, and the one deliberate difference (``Math.pow`` as products) -- is
DESIGN.md section 12.

Third-party semantics restated from the published sources (not checked against a JVM here): ``Random.nextGaussian()`` (polar method
over ``StrictMath.log`` = fdlibm's ``__ieee754_log``), ``Collections.shuffle``, ImgLib2's ``Util.distance`` (squares summed in
dimension order, then ``Math.sqrt``), ``FloatType.setReal`` (a cast to float) and ``FinalInterval(dim)`` = [0, dim - 1].
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np

from . import _lib

_DP = C.POINTER(C.c_double)


# ---- StrictMath.log: fdlibm's __ieee754_log (e_log.c), for JavaRandom.nextGaussian() ---------------------------------------
def _from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


_LN2_HI, _LN2_LO = _from_bits(0x3fe62e42fee00000), _from_bits(0x3dea39ef35793c76)
_LG1, _LG2, _LG3, _LG4, _LG5, _LG6, _LG7 = (_from_bits(b) for b in (
    0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF, 0x3FC7466496CB03DE, 0x3FC39A09D078C69F,
    0x3FC2F112DF3E5244))


def strict_log(x: float) -> float:
    """StrictMath.log(x)."""
    x = float(x)
    if math.isnan(x) or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    if math.isinf(x):
        return x
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    hx, k = bits >> 32, 0
    if hx < 0x00100000:                                    # subnormal: scale up
        k -= 54
        x *= 18014398509481984.0
        bits = struct.unpack("<Q", struct.pack("<d", x))[0]
        hx = bits >> 32
    k += (hx >> 20) - 1023
    hx &= 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    x = _from_bits(((hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffff))      # normalise x or x / 2
    k += i >> 20
    f = x - 1.0
    dk = float(k)
    if (0x000fffff & (2 + hx)) < 3:                        # |f| < 2^-20
        if f == 0.0:
            return 0.0 if k == 0 else dk * _LN2_HI + dk * _LN2_LO
        R = f * f * (0.5 - 0.33333333333333333 * f)
        return f - R if k == 0 else dk * _LN2_HI - ((R - dk * _LN2_LO) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (_LG2 + w * (_LG4 + w * _LG6))
    t2 = z * (_LG1 + w * (_LG3 + w * (_LG5 + w * _LG7)))
    R = t2 + t1
    if ((hx - 0x6147a) | (0x6b851 - hx)) > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * _LN2_HI - ((hfsq - (s * (hfsq + R) + dk * _LN2_LO)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * _LN2_HI - ((s * (f - R) - dk * _LN2_LO) - f)


def _ctx():
    from . import default_context
    return default_context()


def _i3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def _points(points) -> np.ndarray:
    return np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)


class ContextPhantoms:
    """The procedural phantom's entry points of a Context (include/mvsim.h: mvsim_perlin_*, mvsim_spheres_*,
    mvsim_rejection_sample).  ``field`` is a _lib.Perlin, ``spheres`` a _lib.SphereSet (see the classes below for how they are made)."""

    def perlin_at(self, field, points) -> np.ndarray:
        pts = _points(points)
        out = np.empty(len(pts), dtype=np.float64)
        _lib.check(self._L.mvsim_perlin_at(self._h, C.byref(field), pts.ctypes.data, len(pts), out.ctypes.data))
        return out

    def perlin_raster(self, field, dim, origin=(0, 0, 0)) -> np.ndarray:
        out = np.empty((int(dim[2]), int(dim[1]), int(dim[0])), dtype=np.float32)
        _lib.check(self._L.mvsim_perlin_raster(self._h, C.byref(field), _i3(origin), _i3(dim), out.ctypes.data))
        return out

    def perlin_raster_dev(self, field, dim, origin, dptr: int) -> None:
        _lib.check(self._L.mvsim_perlin_raster_dev(self._h, C.byref(field), _i3(origin), _i3(dim), C.c_void_p(dptr)))

    def spheres_at(self, spheres, points) -> np.ndarray:
        pts = _points(points)
        out = np.empty(len(pts), dtype=np.float32)
        _lib.check(self._L.mvsim_spheres_at(self._h, C.byref(spheres), pts.ctypes.data, len(pts), out.ctypes.data))
        return out

    def spheres_raster(self, spheres, dim, origin=(0, 0, 0), out=None, combine: bool = False) -> np.ndarray:
        """combine: ``out = Math.max(out, value)`` over the volume given (in place); else the values are written."""
        shape = (int(dim[2]), int(dim[1]), int(dim[0]))
        if out is None:
            if combine:
                raise ValueError("combine needs the volume to combine with")
            out = np.empty(shape, dtype=np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != shape:
            raise ValueError("out: a contiguous float32 array of shape (Nz, Ny, Nx)")
        _lib.check(self._L.mvsim_spheres_raster(self._h, C.byref(spheres), _i3(origin), _i3(dim), int(bool(combine)), out.ctypes.data))
        return out

    def spheres_raster_dev(self, spheres, dim, origin, dptr: int, combine: bool = False) -> None:
        _lib.check(self._L.mvsim_spheres_raster_dev(self._h, C.byref(spheres), _i3(origin), _i3(dim), int(bool(combine)), C.c_void_p(dptr)))

    def rejection_sample(self, rmin, rmax, n_samples: int, density, rnd, max_trials: int = 1 << 40):
        """mvsim_rejection_sample against a _lib.Perlin or a _lib.SphereSet; ``rnd`` is a JavaRandom, advanced as the reference's
        loop advances it.  Returns (points (n, 3), trials)."""
        d = _lib.Density()
        if isinstance(density, _lib.Perlin):
            d.kind, d.perlin = 0, C.pointer(density)
        else:
            d.kind, d.spheres = 1, C.pointer(density)
        out = np.empty((int(n_samples), 3), dtype=np.float64)
        st, trials = C.c_uint64(rnd._s), C.c_int64(0)
        _lib.check(self._L.mvsim_rejection_sample(self._h, C.byref(st), (C.c_double * 3)(*[float(v) for v in rmin]),
                                                  (C.c_double * 3)(*[float(v) for v in rmax]), int(n_samples), C.byref(d), int(max_trials),
                                                  out.ctypes.data_as(_DP), C.byref(trials)))
        rnd._s = int(st.value)
        return out, int(trials.value)


class _Field:
    """What every accessible here offers: get(pos), at(points), raster(dim, origin)."""

    def get(self, pos) -> float:
        return float(self.at([pos])[0])

    def realRandomAccess(self):
        return self


class PerlinNoiseRealRandomAccessible(_Field):
    """PerlinNoiseRealRandomAccessible(type, scales, loopExtents, nVectors, rng) of a FloatType, three dimensions."""

    def __init__(self, scales, loopExtents, nVectors: int, rng):
        from . import JavaRandom
        self.scales = [float(s) for s in scales]
        self.loopExtents = [int(e) for e in loopExtents]
        self.nVectors = int(nVectors)
        if len(self.scales) != 3 or len(self.loopExtents) != 3:
            raise ValueError("three dimensions only")
        if self.nVectors < 1:
            raise ValueError("n_vectors must be >= 1")
        self.gradients = np.empty((self.nVectors, 3), dtype=np.float64)
        self.permutation = np.empty(self.nVectors, dtype=np.int32)
        if isinstance(rng, JavaRandom):                                # the constructor (:56-73), natively
            st = C.c_uint64(rng._s)
            pend = C.c_double(math.nan if rng._pending is None else rng._pending)
            _lib.check(_lib.load().mvsim_perlin_init(C.byref(st), self.nVectors, self.gradients.ctypes.data_as(_DP),
                                                     self.permutation.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(pend)))
            rng._s = int(st.value)
            rng._pending = None if math.isnan(pend.value) else float(pend.value)
        else:                                                          # any object with nextGaussian() and nextInt(bound)
            for i in range(self.nVectors):
                self.gradients[i] = self.randomUnitVector(3, rng)
            perm = list(range(self.nVectors))
            for i in range(self.nVectors, 1, -1):
                j = rng.nextInt(i)
                perm[i - 1], perm[j] = perm[j], perm[i - 1]
            self.permutation[:] = perm

    @staticmethod
    def randomUnitVector(nDim: int, rng) -> list:
        """:99-111."""
        res, s_sum = [0.0] * nDim, 0.0
        for d in range(nDim):
            res[d] = rng.nextGaussian()
            s_sum += res[d] * res[d]
        for d in range(nDim):
            res[d] /= math.sqrt(s_sum)
        return res

    def _struct(self, threshold=None) -> "_lib.Perlin":
        f = _lib.Perlin()
        f.scales[:] = self.scales
        f.loop_extents[:] = self.loopExtents
        f.n_vectors = self.nVectors
        f.gradients = self.gradients.ctypes.data_as(_DP)
        f.permutation = self.permutation.ctypes.data_as(C.POINTER(C.c_int32))
        f.threshold = math.nan if threshold is None else float(threshold)
        f._keep = self                                                 # the tables live as long as the struct
        return f

    def at(self, points, threshold=None) -> np.ndarray:
        """get() at (n, 3) positions -> n doubles (with a threshold: 1.0 / 0.0)."""
        return _ctx().perlin_at(self._struct(threshold), points)

    def raster(self, dim, origin=(0, 0, 0), threshold=None, device: bool = False):
        """Views.raster over [origin, origin + dim): (Nz, Ny, Nx) float32 -- or, with ``device``, a device buffer the caller frees
        with Context.dev_free."""
        ctx = _ctx()
        if not device:
            return ctx.perlin_raster(self._struct(threshold), dim, origin)
        dptr = ctx.dev_alloc(int(dim[0]) * int(dim[1]) * int(dim[2]) * 4)
        try:
            ctx.perlin_raster_dev(self._struct(threshold), dim, origin, dptr)
        except Exception:
            ctx.dev_free(dptr)
            raise
        return dptr


class HypersphereCollectionRealRandomAccessible(_Field):
    """HypersphereCollectionRealRandomAccessible(numDimensions, type) of a FloatType whose value is ``background``."""

    def __init__(self, numDimensions: int = 3, background: float = 0.0):
        if int(numDimensions) != 3:
            raise ValueError("three dimensions only")
        self.background = float(np.float32(background))
        self.sphereCenters, self.sphereRadii, self.sphereValues = [], [], []

    def addSphere(self, location, radius: float, value: float) -> None:
        loc = [float(v) for v in location]
        if len(loc) != 3:
            raise ValueError("three dimensions only")
        self.sphereCenters.append(loc)
        self.sphereRadii.append(float(radius))
        self.sphereValues.append(np.float32(value))

    def _struct(self) -> "_lib.SphereSet":
        s = _lib.SphereSet()
        c = np.ascontiguousarray(self.sphereCenters, dtype=np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(self.sphereRadii, dtype=np.float64)
        v = np.ascontiguousarray(self.sphereValues, dtype=np.float32)
        s.n = len(r)
        s.centres, s.radii, s.values = c.ctypes.data_as(_DP), r.ctypes.data_as(_DP), v.ctypes.data_as(C.POINTER(C.c_float))
        s.background = self.background
        s._keep = (c, r, v)
        return s

    def at(self, points) -> np.ndarray:
        return _ctx().spheres_at(self._struct(), points)

    def raster(self, dim, origin=(0, 0, 0), out=None, combine: bool = False) -> np.ndarray:
        return _ctx().spheres_raster(self._struct(), dim, origin, out=out, combine=combine)


class _Thresholded(_Field):
    def __init__(self, src: PerlinNoiseRealRandomAccessible, t: float):
        if not isinstance(src, PerlinNoiseRealRandomAccessible):
            raise TypeError("threshold: a PerlinNoiseRealRandomAccessible")
        self.src, self.t = src, float(t)

    def _struct(self):
        return self.src._struct(self.t)

    def at(self, points) -> np.ndarray:
        return self.src.at(points, threshold=self.t)

    def raster(self, dim, origin=(0, 0, 0), device: bool = False):
        return self.src.raster(dim, origin, threshold=self.t, device=device)


class _Maximum(_Field):
    def __init__(self, srcs):
        for s in srcs:
            if not isinstance(s, HypersphereCollectionRealRandomAccessible):
                raise TypeError("maximum: HypersphereCollectionRealRandomAccessible sources")
        self.srcs = list(srcs)

    def at(self, points) -> np.ndarray:
        res = np.zeros(len(_points(points)), dtype=np.float32)
        for s in self.srcs:
            res = np.maximum(res, s.at(points))
        return res

    def raster(self, dim, origin=(0, 0, 0)) -> np.ndarray:
        """res = 0; res = Math.max(res, t) per source, on a volume that stays on the device until it is complete."""
        ctx = _ctx()
        shape = (int(dim[2]), int(dim[1]), int(dim[0]))
        nbytes = shape[0] * shape[1] * shape[2] * 4
        dptr = ctx.dev_alloc(nbytes)
        try:
            _lib.check(ctx._L.mvsim_dev_memset(ctx._h, C.c_void_p(dptr), 0, nbytes))
            for s in self.srcs:
                ctx.spheres_raster_dev(s._struct(), dim, origin, dptr, combine=True)
            return ctx.download(dptr, shape)
        finally:
            ctx.dev_free(dptr)


class SimpleCalculatedRealRandomAccessible:
    """The two lambdas HypersphereCollectionRealRandomAccessible.main builds (generic ones have no device form)."""

    @staticmethod
    def threshold(src, t: float) -> _Thresholded:
        """(a, b) -> a.setReal(b.get() > t ? 1.0 : 0) (:221-223)."""
        return _Thresholded(src, t)

    @staticmethod
    def maximum(*srcs) -> _Maximum:
        """(a, b) -> res = 0; for t in b: res = Math.max(res, t) (:265-270)."""
        return _Maximum(srcs)


class PointRejectionSampling:
    @staticmethod
    def sampleRealPoints(interval, nSamples: int, density, rnd, max_trials: int = 1 << 40) -> np.ndarray:
        """:37-55 -- (nSamples, 3) doubles.  ``interval`` = ((min x, y, z), (max x, y, z)).  A Perlin field (raw or thresholded) or a
        sphere set sampled with a JavaRandom runs on the GPU; any other density with get(pos), or any other generator with
        nextDouble(), takes the reference's loop here."""
        from . import JavaRandom
        mn, mx = [float(v) for v in interval[0]], [float(v) for v in interval[1]]
        gpu = isinstance(density, (PerlinNoiseRealRandomAccessible, HypersphereCollectionRealRandomAccessible, _Thresholded))
        if gpu and isinstance(rnd, JavaRandom):
            return _ctx().rejection_sample(mn, mx, nSamples, density._struct(), rnd, max_trials)[0]
        out, trials = [], 0
        while len(out) < int(nSamples):
            if trials >= max_trials:
                raise ValueError("rejection sampling: max_trials exhausted")
            pos = [mn[d] + rnd.nextDouble() * (mx[d] - mn[d]) for d in range(3)]
            p = rnd.nextDouble()
            trials += 1
            if p < float(np.float32(density.get(pos))):                # the FloatType's value as a double
                out.append(pos)
        return np.array(out, dtype=np.float64).reshape(-1, 3)


def main(dim=(1024, 1024, 256), seed: int = 42, nBigSpheres: int = 400, nSmallSamples: int = 20000) -> np.ndarray:
    """HypersphereCollectionRealRandomAccessible.main (:201-280) with the reference's constants and order of draws; returns the volume
    (Nz, Ny, Nx) that the reference shows."""
    from . import JavaRandom
    f32 = np.float32
    rnd = JavaRandom(seed)
    dim = [int(d) for d in dim]
    minRadiusBig, maxRadiusBig, minValueBig, maxValueBig = f32(20), f32(40), f32(1.2), f32(2.4)
    minRadiusSmall, maxRadiusSmall, minValueSmall, maxValueSmall = f32(2), f32(4), f32(4.0), f32(6.0)
    interval = ((0, 0, 0), tuple(d - 1 for d in dim))                                          # new FinalInterval(dim)

    rrablePerlin = PerlinNoiseRealRandomAccessible((dim[0] // 4, dim[1] / 1.5, dim[2]), (15, 15, 15), 100, rnd)      # :220
    rrablePerlinThrd = SimpleCalculatedRealRandomAccessible.threshold(rrablePerlin, 0.1)
    bigSpherePositions = PointRejectionSampling.sampleRealPoints(interval, nBigSpheres, rrablePerlinThrd, rnd)      # :225
    rrableDensity = HypersphereCollectionRealRandomAccessible(3, 0.0)
    bigSphereRadii = []
    for i in range(nBigSpheres):                                                                                     # :227-235
        radius = float(minRadiusBig) + rnd.nextDouble() * float(maxRadiusBig - minRadiusBig)
        rrableDensity.addSphere(bigSpherePositions[i], radius, 1.0)
        bigSphereRadii.append(radius)
    rrableBigPoints = HypersphereCollectionRealRandomAccessible(3, 0.0)
    rrableSmallPoints = HypersphereCollectionRealRandomAccessible(3, 0.0)
    smallPoints = PointRejectionSampling.sampleRealPoints(interval, nSmallSamples, rrableDensity, rnd)               # :239
    for sp in smallPoints:                                                                                           # :241-247
        radius = float(minRadiusSmall) + rnd.nextDouble() * float(maxRadiusSmall - minRadiusSmall)
        value = f32(float(minValueSmall) + rnd.nextDouble() * float(maxValueSmall - minValueSmall))
        rrableSmallPoints.addSphere(sp, radius, value)
    for i in range(nBigSpheres):                                                                                     # :249-255
        value = f32(float(minValueBig) + rnd.nextDouble() * float(maxValueBig - minValueBig))
        rrableBigPoints.addSphere(bigSpherePositions[i], bigSphereRadii[i], value)
    rrableFinal = SimpleCalculatedRealRandomAccessible.maximum(rrableBigPoints, rrableSmallPoints)                   # :265-270
    return rrableFinal.raster(dim)


HypersphereCollectionRealRandomAccessible.main = staticmethod(main)
