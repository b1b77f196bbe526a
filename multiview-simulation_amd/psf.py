"""PSF extraction: the link between the bead detector / the bead registration and the deconvolution.  The beads of one view are
averaged into that view's PSF, sampled through the inverse of the view's registration so that the PSF comes out in the output frame
-- what ``deconvolve_dev`` takes as it is.  include/mvsim.h states the recipe, DESIGN.md section 20 its kernels.  ``ContextPsf`` is
the part of ``Context`` that binds the C ABI, ``PsfExtraction`` the class a user calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MVSIM_PSF_CHUNK, MVSIM_PSF_CROWDED, MVSIM_PSF_FLAT, MVSIM_PSF_MASKED, MVSIM_PSF_MAX_DIM, MVSIM_PSF_MAX_POINTS,  # noqa: F401
                   MVSIM_PSF_NO_BEADS, MVSIM_PSF_NONFINITE, MVSIM_PSF_OUTSIDE, MVSIM_PSF_SINGULAR, MVSIM_PSF_USED, MVSIM_SRC_F32,
                   MVSIM_SRC_U16, PsfParams, PsfResult)

assert C.sizeof(PsfParams) == 64 and C.sizeof(PsfResult) == 72

PSF_RESULT_DTYPE = np.dtype([("minimum", "<f8"), ("sum", "<f8"), ("n_listed", "<i8"), ("n_used", "<i8"), ("n_nonfinite", "<i8"),
                             ("n_masked", "<i8"), ("n_outside", "<i8"), ("n_crowded", "<i8"), ("flags", "<i4"), ("pad", "<i4")])
assert PSF_RESULT_DTYPE.itemsize == 72

_PARAM_NAMES = ("kdim", "min_separation", "src_type", "subtract_min", "normalize")


def psf_params(**kw) -> PsfParams:
    """``mvsim_psf_params`` with the library's defaults; ``kdim`` and ``min_separation`` are one number or three (x, y, z)."""
    p = PsfParams()
    _lib.load().mvsim_psf_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in _PARAM_NAMES:
            raise TypeError(f"unknown PSF extraction parameter {k!r}")
        if k == "kdim":
            b = np.broadcast_to(np.asarray(v, dtype=np.int64), (3,))
            p.kdim[0], p.kdim[1], p.kdim[2] = int(b[0]), int(b[1]), int(b[2])
        elif k == "min_separation":
            b = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
            p.min_separation[0], p.min_separation[1], p.min_separation[2] = float(b[0]), float(b[1]), float(b[2])
        else:
            setattr(p, k, int(v))
    return p


def psf_geometry() -> dict:
    """The chunk of the sums, the taps one block of the gather kernel owns, the beads the crowding kernel stages per tile and the
    most blocks a launch has; host only."""
    g = (C.c_int64 * 4)()
    _lib.check(_lib.load().mvsim_psf_geometry(g))
    return {"chunk": int(g[0]), "taps_per_block": int(g[1]), "select_tile": int(g[2]), "max_blocks": int(g[3])}


def _m12(m):
    if m is None:
        return None
    a = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    if a.size != 12:
        raise ValueError("a matrix is 3 x 4")
    return a


def _mp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _i3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def _opt(dptr):
    return C.c_void_p(dptr) if dptr else None


def psf_offsets(m, kdim_xyz):
    """Steps 1 and 2 of the recipe (host only): the offset of every tap, (Kz, Ky, Kx, 3) with (x, y, z) last, or None when the
    matrix's linear part is singular or not finite.  ``m`` None: the identity."""
    kd = [int(v) for v in kdim_xyz]
    out = np.zeros((kd[2], kd[1], kd[0], 3), np.float64)
    s = C.c_int(0)
    a = _m12(m)
    _lib.check(_lib.load().mvsim_psf_offsets(_mp(a), _i3(kd), C.c_void_p(out.ctypes.data), C.byref(s)))
    return None if s.value else out


def _positions(positions):
    """A host point list: a structured array whose first field is ``pos`` (the detector's records) keeps its stride."""
    a = np.asarray(positions)
    if a.dtype.names:
        a = np.ascontiguousarray(a)
        return a, a.dtype.itemsize, a.shape[0]
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    return a, 24, a.shape[0]


def psf_select(positions, dim_xyz, m=None, use=None, params: PsfParams | None = None):
    """Step 3 on the host: (status bytes, record)."""
    p = params if params is not None else psf_params()
    a, stride, n = _positions(positions)
    u = np.ascontiguousarray(use, dtype=np.uint8) if use is not None else None
    if u is not None and u.size != n:
        raise ValueError("use: one byte per point")
    st = np.zeros(max(1, n), np.uint8)
    res = PsfResult()
    mm = _m12(m)
    _lib.check(_lib.load().mvsim_psf_select(C.c_void_p(a.ctypes.data), stride, n, _mp(u), _mp(mm), _i3(dim_xyz), C.byref(p),
                                            C.c_void_p(st.ctypes.data), C.byref(res)))
    return st[:n], _record(res)


def psf_finish(totals, record, params: PsfParams | None = None):
    """Step 6 on the host over (Kz, Ky, Kx) totals and the record the selection left: (psf, record)."""
    p = params if params is not None else psf_params()
    t = np.ascontiguousarray(totals, dtype=np.float64)
    if t.size != p.kdim[0] * p.kdim[1] * p.kdim[2]:
        raise ValueError("totals: one double per tap")
    out = np.empty((p.kdim[2], p.kdim[1], p.kdim[0]), np.float32)
    res = PsfResult.from_buffer_copy(np.asarray(record, dtype=PSF_RESULT_DTYPE).tobytes())
    _lib.check(_lib.load().mvsim_psf_finish(C.c_void_p(t.ctypes.data), C.byref(p), C.c_void_p(out.ctypes.data), C.byref(res)))
    return out, _record(res)


def _record(res: PsfResult):
    return np.frombuffer(bytes(res), dtype=PSF_RESULT_DTYPE)[0].copy()


class ContextPsf:
    """PSF extraction entry points of ``Context`` (``self._h``: the context, ``self._L``: the library).  Every ``*_dev`` call only
    enqueues."""

    def psf_select_dev(self, pos_dptr: int, stride: int, n_dptr: int, capacity: int, dim_xyz, status_dptr: int, result_dptr: int,
                       use_dptr: int = 0, m=None, m_dptr: int = 0, params: PsfParams | None = None) -> None:
        p = params if params is not None else psf_params()
        mm = _m12(m)
        _lib.check(self._L.mvsim_psf_select_dev(self._h, C.c_void_p(pos_dptr), stride, C.c_void_p(n_dptr), capacity, _opt(use_dptr), _mp(mm),
                                                _opt(m_dptr), _i3(dim_xyz), C.byref(p), _opt(status_dptr), _opt(result_dptr)))

    def psf_gather_dev(self, img_dptr: int, dim_xyz, pos_dptr: int, stride: int, n_dptr: int, capacity: int, status_dptr: int,
                       totals_dptr: int, m=None, m_dptr: int = 0, params: PsfParams | None = None) -> None:
        p = params if params is not None else psf_params()
        mm = _m12(m)
        _lib.check(self._L.mvsim_psf_gather_dev(self._h, C.c_void_p(img_dptr), _i3(dim_xyz), C.c_void_p(pos_dptr), stride, C.c_void_p(n_dptr),
                                                capacity, _opt(status_dptr), _mp(mm), _opt(m_dptr), C.byref(p), _opt(totals_dptr)))

    def psf_finish_dev(self, totals_dptr: int, psf_dptr: int, result_dptr: int, params: PsfParams | None = None) -> None:
        p = params if params is not None else psf_params()
        _lib.check(self._L.mvsim_psf_finish_dev(self._h, C.c_void_p(totals_dptr), C.byref(p), C.c_void_p(psf_dptr), C.c_void_p(result_dptr)))

    def psf_use_from_matches_dev(self, candidates_dptr: int, n_candidates_dptr: int, capacity: int, mask_dptr: int, side: int,
                                 n_points_capacity: int, use_dptr: int) -> None:
        """The inliers of a registration (``mask_dptr`` 0: every candidate) as the use-mask of list A (``side`` 0) or B (1)."""
        _lib.check(self._L.mvsim_psf_use_from_matches_dev(self._h, C.c_void_p(candidates_dptr), C.c_void_p(n_candidates_dptr), capacity,
                                                          _opt(mask_dptr), side, n_points_capacity, C.c_void_p(use_dptr)))

    def extract_psf_dev(self, img_dptr: int, dim_xyz, pos_dptr: int, stride: int, n_dptr: int, capacity: int, psf_dptr: int, result_dptr: int,
                        status_dptr: int = 0, use_dptr: int = 0, m=None, m_dptr: int = 0, params: PsfParams | None = None) -> None:
        """The PSF of a device view from a device list into ``psf_dptr`` (prod(kdim) floats); ``m_dptr`` non-zero: the matrix is read
        from device memory (12 doubles, e.g. the head of a ``mvsim_registration``)."""
        p = params if params is not None else psf_params()
        mm = _m12(m)
        _lib.check(self._L.mvsim_extract_psf_dev(self._h, C.c_void_p(img_dptr), _i3(dim_xyz), C.c_void_p(pos_dptr), stride, C.c_void_p(n_dptr),
                                                 capacity, _opt(use_dptr), _mp(mm), _opt(m_dptr), C.byref(p), _opt(psf_dptr), _opt(result_dptr),
                                                 _opt(status_dptr)))

    def extract_psf(self, img, positions, m=None, use=None, params: PsfParams | None = None, status: bool = False):
        """A host view (Nz,Ny,Nx) and a host point list ((n, 3) doubles, x first, or the detector's records).  Returns (psf (Kz,Ky,Kx),
        record), and the status bytes where asked for."""
        p = params if params is not None else psf_params()
        v = np.ascontiguousarray(img, dtype=np.uint16 if p.src_type == MVSIM_SRC_U16 else np.float32)
        if v.ndim != 3 or v.size == 0:
            raise ValueError("img: expected 3 non-empty dimensions")
        a, stride, n = _positions(positions)
        u = np.ascontiguousarray(use, dtype=np.uint8) if use is not None else None
        if u is not None and u.size != n:
            raise ValueError("use: one byte per point")
        out = np.empty((p.kdim[2], p.kdim[1], p.kdim[0]), np.float32)
        st = np.zeros(max(1, n), np.uint8)
        res = PsfResult()
        mm = _m12(m)
        _lib.check(self._L.mvsim_extract_psf(self._h, C.c_void_p(v.ctypes.data), _i3((v.shape[2], v.shape[1], v.shape[0])),
                                             C.c_void_p(a.ctypes.data), stride, n, _mp(u), _mp(mm), C.byref(p), C.c_void_p(out.ctypes.data),
                                             C.byref(res), C.c_void_p(st.ctypes.data)))
        return (out, _record(res), st[:n]) if status else (out, _record(res))


class PsfExtraction:
    """Extracts a view's PSF from its beads.

        x = PsfExtraction(kdim=(15, 15, 21))
        psf, record = x.extract(view, peaks)                       # in the view's own frame
        psf, record = x.extract(view, peaks, m=registration["m"])  # in the frame the view was registered to

    ``peaks`` is what ``DifferenceOfGaussian`` returns or an (n, 3) array, x first; ``use`` one byte per point."""

    def __init__(self, ctx=None, **params):
        self.params = psf_params(**params)
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            from . import default_context
            self._ctx = default_context()
        return self._ctx

    def extract(self, img, positions, m=None, use=None, status: bool = False, ctx=None):
        return (ctx if ctx is not None else self._context()).extract_psf(img, positions, m, use, self.params, status)


def gaussian_psf(sigma_xyz, kdim_xyz, m=None, params: PsfParams | None = None) -> np.ndarray:
    """The analytic Gaussian of a rendered bead on the taps of the recipe, under the same minimum subtraction and normalisation:
    what an extraction converges to.  float64, (Kz, Ky, Kx)."""
    p = params if params is not None else psf_params(kdim=kdim_xyz)
    off = psf_offsets(m, kdim_xyz)
    if off is None:
        raise ValueError("gaussian_psf: the matrix is singular")
    s = np.asarray(sigma_xyz, dtype=np.float64)
    g = np.exp(-0.5 * ((off[..., 0] / s[0]) ** 2 + (off[..., 1] / s[1]) ** 2 + (off[..., 2] / s[2]) ** 2))
    if p.subtract_min:
        g = g - g.min()
    if p.normalize and g.sum() > 0:
        g = g / g.sum()
    return g


def psf_rendered(ctx, points, interval, sigma, matrix=None, detector=None, u16: bool = False, params: PsfParams | None = None):
    """Render one view of a bead cloud on the device, detect its beads and extract its PSF in the view's own frame -- all on the
    device; only the results are downloaded.  Returns (psf, record, analytic): ``analytic`` is ``gaussian_psf`` for the renderer's
    sigma under the same parameters."""
    from .detection import PEAK_DTYPE, DifferenceOfGaussian
    det = detector if detector is not None else DifferenceOfGaussian(ctx=ctx)
    p = PsfParams.from_buffer_copy(params) if params is not None else psf_params()
    p.src_type = MVSIM_SRC_U16 if u16 else MVSIM_SRC_F32
    mn, mx = interval
    dim = [int(mx[d]) - int(mn[d]) for d in range(3)]
    nvox = dim[0] * dim[1] * dim[2]
    cap = min(det.capacity, MVSIM_PSF_MAX_POINTS)
    item = PEAK_DTYPE.itemsize
    kd = (int(p.kdim[0]), int(p.kdim[1]), int(p.kdim[2]))
    taps = kd[0] * kd[1] * kd[2]
    img = ctx.dev_alloc(nvox * (2 if u16 else 4))
    lst = ctx.dev_alloc(cap * item + 8)
    out = ctx.dev_alloc(taps * 4 + 256)
    try:
        mats = None if matrix is None else np.asarray(matrix, dtype=np.float64).reshape(1, 3, 4)
        ctx.render_beads_dev(points, interval, sigma, f32_dptrs=None if u16 else [img], u16_dptrs=[img] if u16 else None, matrices=mats)
        ctx.detect_beads_dev(img, np.uint16 if u16 else np.float32, dim, cap, lst, lst + cap * item, params=det.params)
        rec = out + (taps * 4 + 7) // 8 * 8
        ctx.extract_psf_dev(img, dim, lst, item, lst + cap * item, cap, out, rec, params=p)
        psf = ctx.download(out, (kd[2], kd[1], kd[0]), np.float32)
        record = ctx.download(rec, (1,), PSF_RESULT_DTYPE)[0]
    finally:
        for ptr in (img, lst, out):
            ctx.dev_free(ptr)
    return psf, record, gaussian_psf(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)), kd, None, p)
