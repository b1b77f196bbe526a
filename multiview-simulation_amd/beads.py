"""Mirror of the reference's bead simulators, ``net.preibisch.simulation.SimulateBeads`` and ``SimulateBeads2``: random bead
clouds rendered as Gaussians, one image per view.  The rendering (``renderPoints``) runs in the HIP kernels of beads.hip through
``Context.render_beads``; the point generation replays ``java.util.Random`` and the transforms are composed on the host.

Intervals are ``((min x, min y, min z), (max x, max y, max z))``; images are ``(Nz, Ny, Nx)`` arrays whose extent is
``max - min`` per axis, one voxel less than the interval, as the reference allocates them (SimulateBeads.java:105-106).

Third-party semantics restated from the published sources (not checked against a JVM here):
  - ImgLib2 ``Util.getSuggestedKernelDiameter(sigma)``: ``max(3, 2 * (int)(3 sigma + 0.5) + 1)`` for sigma > 0, else 3.
  - ImgLib2 ``AffineTransform3D``: ``rotate`` pre-concatenates the rotation ``R(axis, cos, sin)``; ``translate`` adds to the last
    column; ``inverse`` is the adjugate times 1 / det3x3 with translation ``-(inv row . t)``; ``preConcatenate(b)`` is ``b * this``;
    ``apply`` evaluates ``((x m00 + y m01) + z m02) + m03`` per row.
  - ``Math.toRadians(deg)`` on Java 11: ``deg * 0.017453292519943295``.
  - ``Math.round(double)`` / ``Math.round(float)``: half up (floor plus one when the fraction is >= 0.5); NaN -> 0; saturating.
  - ``UnsignedShortType.set(int)`` keeps the low 16 bits.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

DEGREES_TO_RADIANS = 0.017453292519943295


def to_radians(degrees: float) -> float:
    """Math.toRadians on Java 11."""
    return float(degrees) * DEGREES_TO_RADIANS


def kernel_diameter(sigma: float) -> int:
    """ImgLib2 Util.getSuggestedKernelDiameter."""
    if sigma > 0:
        return max(3, 2 * int(3 * sigma + 0.5) + 1)
    return 3


def java_round(x: float) -> int:
    """Math.round(double) -> long."""
    x = float(x)
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return (1 << 63) - 1 if x > 0 else -(1 << 63)
    f = math.floor(x)
    r = int(f) + (1 if x - f >= 0.5 else 0)
    return max(-(1 << 63), min((1 << 63) - 1, r))


def java_round_float(x) -> np.ndarray:
    """Math.round(float) -> int, element-wise over a float32 array (NaN -> 0, saturating at the int range)."""
    a = np.asarray(x, dtype=np.float32)
    f = np.floor(a)
    frac = (a - f).astype(np.float32)
    with np.errstate(invalid="ignore"):
        r = f.astype(np.float64) + np.where(frac >= np.float32(0.5), 1.0, 0.0)
        r = np.clip(np.nan_to_num(r, nan=0.0, posinf=2147483647.0, neginf=-2147483648.0), -2147483648.0, 2147483647.0)
    return r.astype(np.int64)


def to_unsigned_short(img) -> np.ndarray:
    """LegacySimulatedBeadsImgLoader.getImage: UnsignedShortType.set(Math.round(v)), the low 16 bits."""
    return (java_round_float(img) & 0xFFFF).astype(np.uint16)


def _interval(interval):
    mn, mx = interval
    return tuple(int(v) for v in mn), tuple(int(v) for v in mx)


class AffineTransform3D:
    """The part of ImgLib2's AffineTransform3D that SimulateBeads2 uses; ``m`` is the row-major 3x4 matrix."""

    def __init__(self, m=None):
        self.m = np.eye(3, 4, dtype=np.float64) if m is None else np.array(m, dtype=np.float64).reshape(3, 4)

    def copy(self) -> "AffineTransform3D":
        return AffineTransform3D(self.m)

    def preConcatenate(self, b: "AffineTransform3D") -> "AffineTransform3D":
        a, t = b.m, self.m
        r = np.empty((3, 4), dtype=np.float64)
        for i in range(3):
            for j in range(4):
                v = a[i, 0] * t[0, j] + a[i, 1] * t[1, j] + a[i, 2] * t[2, j]
                r[i, j] = v + a[i, 3] if j == 3 else v
        self.m = r
        return self

    def rotate(self, axis: int, angle: float) -> "AffineTransform3D":
        c, s = math.cos(angle), math.sin(angle)
        if axis == 0:
            r = [[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0]]
        elif axis == 1:
            r = [[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0]]
        else:
            r = [[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0]]
        return self.preConcatenate(AffineTransform3D(r))

    def translate(self, t) -> "AffineTransform3D":
        for d in range(3):
            self.m[d, 3] += float(t[d])
        return self

    def getTranslation(self):
        return [float(self.m[d, 3]) for d in range(3)]

    def inverse(self) -> "AffineTransform3D":
        (m00, m01, m02, m03), (m10, m11, m12, m13), (m20, m21, m22, m23) = [[float(v) for v in row] for row in self.m]
        det = (m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21
               - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22)
        idet = 1.0 / det
        i00 = (m11 * m22 - m12 * m21) * idet
        i01 = (m02 * m21 - m01 * m22) * idet
        i02 = (m01 * m12 - m02 * m11) * idet
        i10 = (m12 * m20 - m10 * m22) * idet
        i11 = (m00 * m22 - m02 * m20) * idet
        i12 = (m02 * m10 - m00 * m12) * idet
        i20 = (m10 * m21 - m11 * m20) * idet
        i21 = (m01 * m20 - m00 * m21) * idet
        i22 = (m00 * m11 - m01 * m10) * idet
        i03 = -i00 * m03 - i01 * m13 - i02 * m23
        i13 = -i10 * m03 - i11 * m13 - i12 * m23
        i23 = -i20 * m03 - i21 * m13 - i22 * m23
        return AffineTransform3D([[i00, i01, i02, i03], [i10, i11, i12, i13], [i20, i21, i22, i23]])

    def apply(self, points) -> np.ndarray:
        """((x m00 + y m01) + z m02) + m03 per row, for one point or an (n, 3) array."""
        return apply_affine(self.m, points)


def apply_affine(m, points) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + m[r, 3] for r in range(3)], axis=-1)


def _ctx():
    from . import default_context
    return default_context()


class SimulateBeads:
    """net.preibisch.simulation.SimulateBeads (SimulateBeads.java:59-225)."""

    def __init__(self, angles, axis: int, numPoints: int, rangeSimulation, intervalRender, sigma):
        from . import JavaRandom
        self.angles = [int(a) for a in angles]
        self.axis = int(axis)
        self.numPoints = int(numPoints)
        self.rangeSimulation = _interval(rangeSimulation)
        self.intervalRender = _interval(intervalRender)
        self.sigma = [float(s) for s in sigma]
        self.rnd = JavaRandom(535)                                  # :69
        self.imgs = None
        self.points = None                                          # drawn once, by getImgs or detect

    def matrices(self) -> np.ndarray:
        """axisRotation(rangeSimulation, axis, angle) of every angle (:138), (V, 3, 4)."""
        from . import SimulateMultiViewDataset
        mn, mx = self.rangeSimulation
        dims = [mx[d] - mn[d] + 1 for d in range(3)]
        return np.stack([SimulateMultiViewDataset.axisRotation(dims, self.axis, a) for a in self.angles])

    def getImgs(self) -> list:
        """:83-95 -- one float image per angle, rendered together (the transforms are applied on the GPU)."""
        if self.imgs is None:
            if self.points is None:
                self.points = self.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)
            self.imgs = _ctx().render_beads(self.points, self.intervalRender, self.sigma, matrices=self.matrices())["f32"]
        return self.imgs

    def getImage(self, view: int) -> np.ndarray:
        """LegacySimulatedBeadsImgLoader.getImage (:76-94): Math.round to unsigned short."""
        return to_unsigned_short(self.getImgs()[view])

    def getFloatImage(self, view: int, normalize: bool) -> np.ndarray:
        """LegacySimulatedBeadsImgLoader.getFloatImage (:97-108)."""
        img = self.getImgs()[view].copy()
        if normalize:
            _ctx().beads_normalize(img)
        return img

    def detect(self, view: int, detector=None, u16: bool = False):
        """Render view ``view`` on the device and detect its beads there, without a download of the image (the library's own
        consumer of the bead images; the reference has none).  Returns (peaks, n_found, truth): ``truth`` are the view's true
        bead positions in image coordinates.  The cloud is drawn once, as getImgs draws it."""
        from .detection import detect_rendered
        if self.points is None:
            self.points = self.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)
        return detect_rendered(_ctx(), self.points, self.matrices()[view], self.intervalRender, self.sigma, detector, u16)

    def register(self, view_a: int, view_b: int, detector=None, matcher=None, u16: bool = False):
        """Render views ``view_a`` and ``view_b`` on the device, detect their beads and register A -> B there; only the result is
        downloaded.  Returns (registration, candidates, mask, truth): ``truth`` is the true A -> B transform in image coordinates
        (3 x 4), q_B = M_B M_A^-1 (q_A + min) - min with min from intervalRender."""
        from .registration import register_rendered
        if self.points is None:
            self.points = self.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)
        m = self.matrices()
        return register_rendered(_ctx(), self.points, m[view_a], m[view_b], self.intervalRender, self.sigma, detector, matcher, u16)

    def fuse(self, views=None, reference: int = 0, detector=None, matcher=None, u16: bool = False, params=None):
        """Render ``views`` (default: all), detect their beads, register each against view ``reference`` (an index into ``views``) and
        fuse them into the reference's interval, all on the device.  Returns (fused, registrations, fused_with_true_matrices):
        ``registrations[v]`` is the record of view v -> reference, None at the reference itself."""
        from .fusion import fuse_rendered
        if self.points is None:
            self.points = self.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)
        m = self.matrices()
        picked = list(range(len(m))) if views is None else [int(v) for v in views]
        return fuse_rendered(_ctx(), self.points, [m[v] for v in picked], self.intervalRender, self.sigma, reference, detector, matcher, u16,
                             params)

    def extract_psf(self, view: int = 0, detector=None, u16: bool = False, params=None):
        """Render view ``view``, detect its beads and extract its PSF in the view's own frame, all on the device.  Returns
        (psf, record, analytic): ``analytic`` is the renderer's Gaussian under the same minimum subtraction and normalisation."""
        from .psf import psf_rendered
        if self.points is None:
            self.points = self.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)
        return psf_rendered(_ctx(), self.points, self.intervalRender, self.sigma, self.matrices()[view], detector, u16, params)

    @staticmethod
    def randomPoints(numPoints: int, range_, rnd) -> np.ndarray:
        """:151-166 -- (numPoints, 3) doubles.  A JavaRandom is replayed natively and advanced; any other object with
        java.util.Random's nextDouble() is drawn from here."""
        from . import JavaRandom
        mn, mx = _interval(range_)
        out = np.empty((int(numPoints), 3), dtype=np.float64)
        if isinstance(rnd, JavaRandom):
            st = C.c_uint64(rnd._s)
            _lib.check(_lib.load().mvsim_beads_random_points(C.byref(st), int(numPoints), (C.c_int64 * 3)(*mn), (C.c_int64 * 3)(*mx),
                                                             out.ctypes.data_as(C.POINTER(C.c_double))))
            rnd._s = int(st.value)
            return out
        for i in range(int(numPoints)):
            for d in range(3):
                out[i, d] = rnd.nextDouble() * float(mx[d] - mn[d]) + float(mn[d])
        return out

    @staticmethod
    def transformPoints(points, angles, axis: int, range_) -> list:
        """:132-149 -- one transformed copy of the points per angle (AffineModel3D.apply)."""
        from . import SimulateMultiViewDataset
        mn, mx = _interval(range_)
        dims = [mx[d] - mn[d] + 1 for d in range(3)]
        return [apply_affine(SimulateMultiViewDataset.axisRotation(dims, axis, int(a)), points) for a in angles]

    @staticmethod
    def isInsideAdjust(p, interval) -> bool:
        """:120-130 -- subtracts the interval's min from p in place, axis by axis, and stops at the first axis outside."""
        mn, mx = _interval(interval)
        for d in range(3):
            p[d] -= float(mn[d])
            if p[d] < 0 or p[d] > float(mx[d] - mn[d]):
                return False
        return True

    @staticmethod
    def renderPoints(lists, interval, sigma) -> list:
        """:97-118 -- one float image per list, on the GPU.  Like the reference, the points of the caller's lists are adjusted
        in place by isInsideAdjust (only (n, 3) numpy arrays and lists of mutable points can be)."""
        arrays = [np.array(lst, dtype=np.float64).reshape(-1, 3) for lst in lists]
        offs = np.zeros(len(arrays) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(a) for a in arrays])
        pts = np.concatenate(arrays) if arrays else np.zeros((0, 3))
        imgs = _ctx().render_beads(pts, interval, sigma, view_offsets=offs)["f32"]
        mn, mx = _interval(interval)
        for lst, arr in zip(lists, arrays):
            adjusted = _adjust(arr, mn, mx)
            if isinstance(lst, np.ndarray):
                lst[...] = adjusted.reshape(lst.shape)
            else:
                for p, q in zip(lst, adjusted):
                    for d in range(3):
                        p[d] = float(q[d])
        return imgs

    @staticmethod
    def addGaussian(image: np.ndarray, location, sigma) -> None:
        """:168-205 -- one bead added in place to a (Nz, Ny, Nx) float32 image (host arithmetic: one box of voxels)."""
        size = [kernel_diameter(s) * 2 for s in sigma]
        lo = [java_round(location[d]) - size[d] // 2 for d in range(3)]
        dims = (image.shape[2], image.shape[1], image.shape[0])
        a = [max(lo[d], 0) for d in range(3)]
        b = [min(lo[d] + size[d] - 1, dims[d] - 1) for d in range(3)]
        if any(a[d] > b[d] for d in range(3)):
            return
        f = []
        for d in range(3):
            x = float(location[d]) - np.arange(a[d], b[d] + 1, dtype=np.float64)
            f.append(np.exp(-(x * x) / (2 * float(sigma[d]) * float(sigma[d]))))
        value = (f[0][None, None, :] * f[1][None, :, None]) * f[2][:, None, None]
        win = image[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1]
        win[...] = win + value.astype(np.float32) * np.float32(1000.0)


def _adjust(arr, mn, mx) -> np.ndarray:
    """isInsideAdjust over an (n, 3) array: the adjusted copy (axes after the first failing one untouched)."""
    out = np.array(arr, dtype=np.float64)
    active = np.ones(len(out), dtype=bool)
    for d in range(3):
        out[active, d] -= float(mn[d])
        active &= (out[:, d] >= 0) & (out[:, d] <= float(mx[d] - mn[d]))
    return out


class SimulateBeads2:
    """net.preibisch.simulation.SimulateBeads2: one bead cloud seen per (time point, angle, channel, tile, illumination)."""

    def __init__(self, numPoints: int, sigma, rangeSimulation, intervalRender):
        from . import JavaRandom
        self.numPoints = int(numPoints)
        self.sigma = [float(s) for s in sigma]
        self.rangeSimulation = _interval(rangeSimulation)
        self.intervalRender = _interval(intervalRender)
        self.imgs = {}
        self.angleTransforms, self.channelTransforms, self.illumTransforms = {}, {}, {}
        self.tpTransforms, self.tileTransforms = {}, {}
        self.rnd = JavaRandom(535)                                                            # :58
        self.points = SimulateBeads.randomPoints(self.numPoints, self.rangeSimulation, self.rnd)  # :76

    def getTilesExtent(self):
        """:80-97 -- (mins, maxs) over the tiles."""
        mn, mx = self.intervalRender
        mins = [np.finfo(np.float64).max] * 3
        maxs = [-np.finfo(np.float64).max] * 3
        for tt in self.tileTransforms.values():
            t = tt.getTranslation()
            for d in range(3):
                mins[d] = min(mins[d], -t[d])
                maxs[d] = max(maxs[d], -t[d] + (mx[d] - mn[d] + 1))
        return mins, maxs

    def addAngle(self, id_: int, axis: int, degrees: float) -> None:
        self.angleTransforms[id_] = AffineTransform3D().rotate(axis, to_radians(degrees))

    def addChannel(self, id_: int, shift) -> None:
        self.channelTransforms[id_] = AffineTransform3D().translate(shift)

    def addIllumination(self, id_: int, shift) -> None:
        self.illumTransforms[id_] = AffineTransform3D().translate(shift)

    def addTimepoint(self, id_: int, shift) -> None:
        self.tpTransforms[id_] = AffineTransform3D().translate(shift)

    def addTile(self, id_: int, shift) -> None:
        self.tileTransforms[id_] = AffineTransform3D().translate(shift).inverse()

    def transform(self, tp: int, angle: int, channel: int, tile: int, illumination: int) -> AffineTransform3D:
        """:148-171 -- tp, angle, channel, illumination, tile, each pre-concatenated."""
        t = AffineTransform3D()
        for table, key in ((self.tpTransforms, tp), (self.angleTransforms, angle), (self.channelTransforms, channel),
                           (self.illumTransforms, illumination), (self.tileTransforms, tile)):
            if key in table:
                t.preConcatenate(table[key])
        return t

    def getImg(self, tp: int, angle: int, channel: int, tile: int, illumination: int) -> np.ndarray:
        """:99-111 -- rendered once per key, then cached."""
        key = (tp, angle, channel, tile, illumination)
        if key not in self.imgs:
            m = self.transform(*key).m
            self.imgs[key] = _ctx().render_beads(self.points, self.intervalRender, self.sigma, matrices=m[None])["f32"][0]
        return self.imgs[key]

    def detect(self, tp: int, angle: int, channel: int, tile: int, illumination: int, detector=None, u16: bool = False):
        """Render this view on the device and detect its beads there, without a download of the image.  Returns
        (peaks, n_found, truth) as SimulateBeads.detect does."""
        from .detection import detect_rendered
        m = self.transform(tp, angle, channel, tile, illumination).m
        return detect_rendered(_ctx(), self.points, m, self.intervalRender, self.sigma, detector, u16)

    def register(self, view_a, view_b, detector=None, matcher=None, u16: bool = False):
        """Two views, each a (tp, angle, channel, tile, illumination) key: rendered, detected and registered A -> B on the device.
        Returns (registration, candidates, mask, truth) as SimulateBeads.register does."""
        from .registration import register_rendered
        return register_rendered(_ctx(), self.points, self.transform(*view_a).m, self.transform(*view_b).m, self.intervalRender, self.sigma,
                                 detector, matcher, u16)

    def fuse(self, views, reference: int = 0, detector=None, matcher=None, u16: bool = False, params=None):
        """``views``: (tp, angle, channel, tile, illumination) keys.  Rendered, detected, registered against ``views[reference]`` and
        fused into its interval on the device.  Returns (fused, registrations, fused_with_true_matrices) as SimulateBeads.fuse does."""
        from .fusion import fuse_rendered
        return fuse_rendered(_ctx(), self.points, [self.transform(*v).m for v in views], self.intervalRender, self.sigma, reference, detector,
                             matcher, u16, params)

    def extract_psf(self, tp: int, angle: int, channel: int, tile: int, illumination: int, detector=None, u16: bool = False, params=None):
        """The PSF of one view from its rendered and detected beads, on the device: (psf, record, analytic) as SimulateBeads.extract_psf."""
        from .psf import psf_rendered
        return psf_rendered(_ctx(), self.points, self.intervalRender, self.sigma, self.transform(tp, angle, channel, tile, illumination).m,
                            detector, u16, params)

    def getImage(self, tp: int, angle: int, channel: int, tile: int, illumination: int) -> np.ndarray:
        """LegacySimulatedBeadsImgLoader2.getImage (:65-85): uint16, written by the kernel directly."""
        m = self.transform(tp, angle, channel, tile, illumination).m
        return _ctx().render_beads(self.points, self.intervalRender, self.sigma, matrices=m[None], f32=False, u16=True)["u16"][0]

    def getFloatImage(self, tp: int, angle: int, channel: int, tile: int, illumination: int, normalize: bool) -> np.ndarray:
        """LegacySimulatedBeadsImgLoader2.getFloatImage (:94-106): a copy, normalised on request."""
        img = self.getImg(tp, angle, channel, tile, illumination).copy()
        if normalize:
            _ctx().beads_normalize(img)
        return img
