"""Multi-view deconvolution: the consumer of the dataset that SimulateMultiViewDataset writes (aligned views, their PSFs and
their normalised weights).  A weighted, sequential (OSEM) multi-view Richardson-Lucy on the GPU; include/mvsim.h states the
recipe, DESIGN.md section 16 its rounding points.  ``ContextDeconvolution`` is the part of ``Context`` that binds the C ABI,
``MultiViewDeconvolution`` the class a user calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeconParams, DeconStat


def decon_params(**kw) -> DeconParams:
    """``mvsim_decon_params`` with the library's defaults; ``lambda_`` (or ``tikhonov``) is the Tikhonov weight."""
    p = DeconParams()
    _lib.load().mvsim_decon_params_default(C.byref(p))
    for k, v in kw.items():
        k = {"lambda": "lambda_", "tikhonov": "lambda_"}.get(k, k)
        if not hasattr(p, k):
            raise TypeError(f"unknown deconvolution parameter {k!r}")
        setattr(p, k, v)
    return p


def decon_geometry():
    """(most blocks an elementwise kernel launches, voxels a block takes per trip of its grid-stride loop)."""
    g = (C.c_int64 * 2)()
    _lib.check(_lib.load().mvsim_decon_geometry(g))
    return int(g[0]), int(g[1])


def flip_psf(psf) -> np.ndarray:
    """The correlation kernel of a PSF (Kz,Ky,Kx): flipped on every axis behind one leading zero on every axis of even extent."""
    p = np.ascontiguousarray(psf, dtype=np.float32)
    if p.ndim != 3 or p.size == 0:
        raise ValueError("psf: expected 3 non-empty dimensions")
    kz, ky, kx = p.shape
    out = np.empty((kz | 1, ky | 1, kx | 1), dtype=np.float32)
    od = (C.c_int64 * 3)()
    _lib.check(_lib.load().mvsim_decon_flip_psf(C.c_void_p(p.ctypes.data), (C.c_int64 * 3)(kx, ky, kz), C.c_void_p(out.ctypes.data), od))
    assert (od[2], od[1], od[0]) == out.shape
    return out


def _psf_args(psfs):
    """PSFs as contiguous float32 copies (the library reads them, it never writes), their pointer table and extents."""
    keep = [np.ascontiguousarray(p, dtype=np.float32) for p in psfs]
    for p in keep:
        if p.ndim != 3 or p.size == 0:
            raise ValueError("psf: expected 3 non-empty dimensions")
    ptrs = (C.c_void_p * len(keep))(*[p.ctypes.data for p in keep])
    kd = (C.c_int64 * (3 * len(keep)))(*[e for p in keep for e in (p.shape[2], p.shape[1], p.shape[0])])
    return keep, ptrs, kd


def _stats_list(buf, iterations: int, n_views: int):
    return [[buf[i * n_views + v].as_dict() for v in range(n_views)] for i in range(iterations)]


class ContextDeconvolution:
    """Deconvolution entry points of ``Context`` (``self._h``: the context, ``self._L``: the library)."""

    def decon_ratio_dev(self, phi_dptr: int, blurred_dptr: int, n: int, eps: float, ratio_dptr: int) -> None:
        """ratio = phi / fmaxf(blurred, eps) on n device floats; ``ratio_dptr`` may be ``blurred_dptr``.  Asynchronous."""
        _lib.check(self._L.mvsim_decon_ratio_dev(self._h, C.c_void_p(phi_dptr), C.c_void_p(blurred_dptr), int(n), float(eps),
                                                 C.c_void_p(ratio_dptr)))

    def decon_update_dev(self, psi_dptr: int, corr_dptr: int, weight_dptr: int, n: int, min_value: float, lambda_: float = 0.0,
                         stats: bool = False):
        """The update step in place on ``psi``; ``weight_dptr`` 0: no weights.  With ``stats`` the call synchronises and returns
        {sum_psi, max_change, n_floored}."""
        st = DeconStat()
        _lib.check(self._L.mvsim_decon_update_dev(self._h, C.c_void_p(psi_dptr), C.c_void_p(corr_dptr), C.c_void_p(weight_dptr or None),
                                                  int(n), float(min_value), float(lambda_), C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def deconvolve_dev(self, view_dptrs, dim_xyz, psfs, psi_dptr: int, weight_dptrs=None, params: DeconParams | None = None,
                       stats: bool = False):
        """Device volumes of ``dim_xyz`` floats each; ``psfs``: host arrays (Kz,Ky,Kx), not written.  Asynchronous unless ``stats``
        (then: a list [iteration][view] of {sum_psi, max_change, n_floored})."""
        p = params if params is not None else decon_params()
        nv = len(view_dptrs)
        if len(psfs) != nv or (weight_dptrs is not None and len(weight_dptrs) != nv):
            raise ValueError("deconvolve: views, psfs and weights must have one entry per view")
        keep, pp, kd = _psf_args(psfs)
        va = (C.c_void_p * nv)(*view_dptrs)
        wa = (C.c_void_p * nv)(*weight_dptrs) if weight_dptrs is not None else None
        sb = (DeconStat * (max(1, int(p.iterations)) * max(1, nv)))() if stats else None
        _lib.check(self._L.mvsim_deconvolve_dev(self._h, va, wa, pp, kd, nv, (C.c_int64 * 3)(*dim_xyz), C.byref(p), C.c_void_p(psi_dptr), sb))
        del keep
        return _stats_list(sb, int(p.iterations), nv) if stats else None

    def deconvolve(self, views, psfs, weights=None, params: DeconParams | None = None, psi=None, stats: bool = False):
        """Host arrays (Nz,Ny,Nx) of one shape.  Returns the estimate, or (estimate, stats).  ``psi`` is the start estimate
        where ``params.init_from_psi`` is set (it is not written)."""
        p = params if params is not None else decon_params()
        vs = [np.ascontiguousarray(v, dtype=np.float32) for v in views]
        nv = len(vs)
        if nv and (vs[0].ndim != 3 or vs[0].size == 0):
            raise ValueError("views: expected 3 non-empty dimensions")
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights] if weights is not None else None
        if len(psfs) != nv or (ws is not None and len(ws) != nv):
            raise ValueError("deconvolve: views, psfs and weights must have one entry per view")
        if any(v.shape != vs[0].shape for v in vs) or (ws is not None and any(w.shape != vs[0].shape for w in ws)):
            raise ValueError("deconvolve: all views and weights must have the same shape")
        shape = vs[0].shape if nv else (1, 1, 1)
        if p.init_from_psi:
            if psi is None or np.shape(psi) != shape:
                raise ValueError("deconvolve: init_from_psi needs a start estimate of the views' shape")
            out = np.array(psi, dtype=np.float32, order="C")
        else:
            out = np.empty(shape, dtype=np.float32)
        keep, pp, kd = _psf_args(psfs)
        va = (C.c_void_p * max(1, nv))(*[v.ctypes.data for v in vs])
        wa = (C.c_void_p * max(1, nv))(*[w.ctypes.data for w in ws]) if ws is not None else None
        sb = (DeconStat * (max(1, int(p.iterations)) * max(1, nv)))() if stats else None
        dim = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        _lib.check(self._L.mvsim_deconvolve(self._h, va, wa, pp, kd, nv, dim, C.byref(p), C.c_void_p(out.ctypes.data), sb))
        del keep
        return (out, _stats_list(sb, int(p.iterations), nv)) if stats else out


class MultiViewDeconvolution:
    """Weighted OSEM multi-view Richardson-Lucy over the outputs of SimulateMultiViewDataset: ``aligned_view_<angle>``,
    ``aligned_view_psf_<angle>`` and ``aligned_view_weights<angle>`` (normalised with the same ``osem`` factor).

        d = MultiViewDeconvolution(iterations=10)
        psi = d.run(views, psfs, weights)
    """

    def __init__(self, ctx=None, **params):
        self._ctx = ctx
        self.params = decon_params(**params)

    def _context(self):
        if self._ctx is None:
            from . import default_context
            self._ctx = default_context()
        return self._ctx

    def run(self, views, psfs, weights=None, params: DeconParams | None = None, stats: bool = False, psi=None):
        return self._context().deconvolve(views, psfs, weights, params if params is not None else self.params, psi=psi, stats=stats)
