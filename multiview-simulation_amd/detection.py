"""Bead detection: the consumer of the bead images that SimulateBeads / SimulateBeads2 render.  A difference-of-Gaussian volume
over a device-resident image, its strict local maxima above a threshold in index order, and a quadratic sub-voxel fit of every
maximum; include/mvsim.h states the recipe, DESIGN.md section 17 its kernels.  ``ContextDetection`` is the part of ``Context``
that binds the C ABI, ``DifferenceOfGaussian`` the class a user calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MVSIM_DOG_MAX_TAPS, MVSIM_SRC_F32, MVSIM_SRC_U16, DogParams, Peak

#: one detection: ``pos`` is (x, y, z) in voxels, ``voxel`` the linear index x + Nx (y + Ny z) of the final base voxel
PEAK_DTYPE = np.dtype([("pos", np.float64, (3,)), ("value", np.float32), ("flags", np.int32), ("voxel", np.int64)])
assert PEAK_DTYPE.itemsize == C.sizeof(Peak) == 40


def dog_params(**kw) -> DogParams:
    """``mvsim_dog_params`` with the library's defaults.  ``sigma1`` / ``sigma2``: a number for every axis, or (x, y, z)."""
    p = DogParams()
    _lib.load().mvsim_dog_params_default(C.byref(p))
    for k, v in kw.items():
        if k in ("sigma1", "sigma2"):
            vals = [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]
            if len(vals) != 3:
                raise ValueError(f"{k}: one number or three (x, y, z)")
            setattr(p, k, (C.c_double * 3)(*vals))
        elif k in ("threshold", "max_moves"):
            setattr(p, k, v)
        else:
            raise TypeError(f"unknown detection parameter {k!r}")
    return p


def dog_taps(sigma: float) -> np.ndarray:
    """The float taps of one sigma (step 1 of the recipe); host only."""
    t = (C.c_float * MVSIM_DOG_MAX_TAPS)()
    n = C.c_int(0)
    _lib.check(_lib.load().mvsim_dog_taps(float(sigma), t, C.byref(n)))
    return np.array(t[: n.value], dtype=np.float32)


def dog_geometry() -> dict:
    """The launch geometry of the detector's kernels; host only."""
    g = (C.c_int64 * 5)()
    _lib.check(_lib.load().mvsim_dog_geometry(g))
    return {"tile_x": int(g[0]), "tile_y": int(g[1]), "tile_z": int(g[2]), "max_radius": int(g[3]), "peak_block_voxels": int(g[4])}


def _src_type(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.float32:
        return MVSIM_SRC_F32
    if dt == np.uint16:
        return MVSIM_SRC_U16
    raise ValueError("detect: the image must be float32 or uint16")


def _dim3(dim_xyz):
    return (C.c_int64 * 3)(*[int(v) for v in dim_xyz])


class ContextDetection:
    """Detection entry points of ``Context`` (``self._h``: the context, ``self._L``: the library)."""

    def dog_dev(self, img_dptr: int, dtype, dim_xyz, dog_dptr: int, params: DogParams | None = None) -> None:
        """D = G(sigma1) - G(sigma2) of a device image (float32 or uint16, not written) into device floats.  Asynchronous."""
        p = params if params is not None else dog_params()
        _lib.check(self._L.mvsim_dog_dev(self._h, C.c_void_p(img_dptr), _src_type(dtype), _dim3(dim_xyz), C.byref(p), C.c_void_p(dog_dptr)))

    def find_peaks_dev(self, vol_dptr: int, dim_xyz, threshold: float, capacity: int, voxels_dptr: int, n_found_dptr: int) -> None:
        """The peaks of a device float volume: min(n_found, capacity) int64 indices in ascending order, the count in device memory."""
        _lib.check(self._L.mvsim_find_peaks_dev(self._h, C.c_void_p(vol_dptr), _dim3(dim_xyz), float(threshold), int(capacity),
                                                C.c_void_p(voxels_dptr), C.c_void_p(n_found_dptr)))

    def localise_peaks_dev(self, vol_dptr: int, dim_xyz, voxels_dptr: int, n_found_dptr: int, capacity: int, max_moves: int,
                           peaks_dptr: int) -> None:
        """The sub-voxel fit of the first min(n_found, capacity) listed voxels into ``mvsim_peak`` records (40 bytes each)."""
        _lib.check(self._L.mvsim_localise_peaks_dev(self._h, C.c_void_p(vol_dptr), _dim3(dim_xyz), C.c_void_p(voxels_dptr),
                                                    C.c_void_p(n_found_dptr), int(capacity), int(max_moves), C.c_void_p(peaks_dptr)))

    def detect_beads_dev(self, img_dptr: int, dtype, dim_xyz, capacity: int, peaks_dptr: int = 0, n_found_dptr: int = 0,
                         params: DogParams | None = None):
        """The whole recipe on a device image.  With ``peaks_dptr`` and ``n_found_dptr`` the call only enqueues and returns None;
        without them the outputs are allocated for the call, fetched and returned as (peaks, n_found)."""
        p = params if params is not None else dog_params()
        own = not (peaks_dptr and n_found_dptr)
        if own:
            peaks_dptr = self.dev_alloc(int(capacity) * PEAK_DTYPE.itemsize + 8)
            n_found_dptr = peaks_dptr + int(capacity) * PEAK_DTYPE.itemsize
        try:
            _lib.check(self._L.mvsim_detect_beads_dev(self._h, C.c_void_p(img_dptr), _src_type(dtype), _dim3(dim_xyz), C.byref(p),
                                                      int(capacity), C.c_void_p(peaks_dptr), C.c_void_p(n_found_dptr)))
            if not own:
                return None
            n = int(self.download(n_found_dptr, (1,), np.int64)[0])
            listed = min(n, int(capacity))
            peaks = self.download(peaks_dptr, (listed,), PEAK_DTYPE) if listed else np.zeros(0, PEAK_DTYPE)
            return peaks, n
        finally:
            if own:
                self.dev_free(peaks_dptr)

    def detect_beads(self, img, capacity: int = 1 << 16, params: DogParams | None = None):
        """A host image (Nz, Ny, Nx), float32 or uint16 (anything else is converted to float32).  Returns (peaks, n_found): a
        structured array of min(n_found, capacity) detections in ascending order of their peak voxels."""
        p = params if params is not None else dog_params()
        a = np.asarray(img)
        if a.dtype != np.uint16:
            a = a.astype(np.float32, copy=False)
        a = np.ascontiguousarray(a)
        if a.ndim != 3 or a.size == 0:
            raise ValueError("detect: expected 3 non-empty dimensions")
        peaks = np.zeros(max(1, int(capacity)), PEAK_DTYPE)
        n = C.c_int64(0)
        _lib.check(self._L.mvsim_detect_beads(self._h, C.c_void_p(a.ctypes.data), _src_type(a.dtype), _dim3(a.shape[::-1]), C.byref(p),
                                              int(capacity), C.c_void_p(peaks.ctypes.data), C.byref(n)))
        return peaks[: min(int(n.value), int(capacity))].copy(), int(n.value)


class DifferenceOfGaussian:
    """DoG interest points with sub-voxel localisation.

        det = DifferenceOfGaussian(sigma=1.8, threshold=0.008)
        peaks, n_found = det.detect(img)          # peaks["pos"]: (n, 3) x, y, z

    ``sigma`` is sigma1 (a number or (x, y, z)); ``sigma2`` defaults to sigma * 2^(1/4) per axis.  The default threshold is the
    usual proposal for images normalised to [0, 1]."""

    def __init__(self, sigma=1.8, threshold: float = 0.008, sigma2=None, max_moves: int = 4, capacity: int = 1 << 16, ctx=None):
        s1 = [float(sigma)] * 3 if np.isscalar(sigma) else [float(v) for v in sigma]
        s2 = [v * 2.0 ** 0.25 for v in s1] if sigma2 is None else sigma2
        self.params = dog_params(sigma1=s1, sigma2=s2, threshold=threshold, max_moves=max_moves)
        self.capacity = int(capacity)
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            from . import default_context
            self._ctx = default_context()
        return self._ctx

    def detect(self, img):
        return self._context().detect_beads(img, self.capacity, self.params)

    def detect_dev(self, img_dptr: int, dtype, dim_xyz):
        """The same on a device image; returns (peaks, n_found) and synchronises."""
        return self._context().detect_beads_dev(img_dptr, dtype, dim_xyz, self.capacity, params=self.params)


def detect_rendered(ctx, points, matrix, interval, sigma, detector: DifferenceOfGaussian | None = None, u16: bool = False):
    """Render one view of a bead cloud on the device and detect in it there, without a download of the image.  Returns
    (peaks, n_found, truth): ``truth`` are the view's true bead positions in image coordinates -- the matrix applied, the
    interval's min subtracted."""
    from .beads import apply_affine
    det = detector if detector is not None else DifferenceOfGaussian(ctx=ctx)
    mn, mx = interval
    dim = [int(mx[d]) - int(mn[d]) for d in range(3)]
    n = dim[0] * dim[1] * dim[2]
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 4)
    img = ctx.dev_alloc(n * (2 if u16 else 4))
    try:
        ctx.render_beads_dev(points, interval, sigma, f32_dptrs=None if u16 else [img], u16_dptrs=[img] if u16 else None, matrices=m[None])
        peaks, n_found = ctx.detect_beads_dev(img, np.uint16 if u16 else np.float32, dim, det.capacity, params=det.params)
    finally:
        ctx.dev_free(img)
    truth = apply_affine(m, np.asarray(points, dtype=np.float64).reshape(-1, 3)) - np.array([float(v) for v in mn])
    return peaks, n_found, truth
