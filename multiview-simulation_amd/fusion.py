"""View fusion: the consumer of the transforms that ``BeadRegistration`` leaves.  Every view is resampled through its affine into one
output interval and either averaged under smooth border weights (the fused volume) or handed back aligned, with its weight volume --
what ``normalize_weights_dev`` and ``deconvolve_dev`` take as they are.  include/mvsim.h states the recipe, DESIGN.md section 19 its
kernel.  ``ContextFusion`` is the part of ``Context`` that binds the C ABI, ``ViewFusion`` the class a user calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MVSIM_FUSE_SINGULAR, MVSIM_MAX_VIEWS, MVSIM_SRC_F32, MVSIM_SRC_U16, FuseParams, FuseView  # noqa: F401

assert C.sizeof(FuseParams) == 32 and C.sizeof(FuseView) == 136

_PARAM_NAMES = ("blend", "background", "src_type")


def fuse_params(**kw) -> FuseParams:
    """``mvsim_fuse_params`` with the library's defaults; ``blend`` is one number or three (x, y, z)."""
    p = FuseParams()
    _lib.load().mvsim_fuse_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in _PARAM_NAMES:
            raise TypeError(f"unknown fusion parameter {k!r}")
        if k == "blend":
            b = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
            p.blend[0], p.blend[1], p.blend[2] = float(b[0]), float(b[1]), float(b[2])
        else:
            setattr(p, k, v)
    return p


def fusion_geometry() -> dict:
    """The brick of output one block owns (x, y, z) and the most blocks a launch has; host only."""
    g = (C.c_int64 * 4)()
    _lib.check(_lib.load().mvsim_fusion_geometry(g))
    return {"brick": (int(g[0]), int(g[1]), int(g[2])), "max_blocks": int(g[3])}


def _m12(m):
    a = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    if a.size != 12:
        raise ValueError("a matrix is 3 x 4")
    return a


def fuse_invert(m):
    """Step 1 of the recipe (host only): the 3 x 4 inverse of a 3 x 4 matrix, or None when it is singular or not finite."""
    a = _m12(m)
    inv = np.zeros(12, np.float64)
    s = C.c_int(0)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().mvsim_fuse_invert(a.ctypes.data_as(dp), inv.ctypes.data_as(dp), C.byref(s)))
    return None if s.value else inv.reshape(3, 4)


def fusion_bounds(matrices, dims_xyz, intersection: bool = False):
    """The output interval that holds every view, or with ``intersection`` the one every view covers: (out_min, out_dim), x first."""
    ms = np.ascontiguousarray([_m12(m) for m in matrices], dtype=np.float64)
    ds = np.ascontiguousarray(dims_xyz, dtype=np.int64).reshape(-1, 3)
    if len(ms) != len(ds):
        raise ValueError("fusion_bounds: one matrix and one size per view")
    mn, dm = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    _lib.check(_lib.load().mvsim_fusion_bounds(ms.ctypes.data_as(C.POINTER(C.c_double)), ds.ctypes.data_as(C.POINTER(C.c_int64)), len(ms),
                                               1 if intersection else 0, mn, dm))
    return tuple(int(v) for v in mn), tuple(int(v) for v in dm)


def psf_matrix(m, kdim_xyz, out_kdim_xyz) -> np.ndarray:
    """The matrix that brings a view's PSF of ``kdim_xyz`` into the output frame as a volume of ``out_kdim_xyz``: centre to centre."""
    a = _m12(m)
    out = np.zeros(12, np.float64)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().mvsim_fusion_psf_matrix(a.ctypes.data_as(dp), (C.c_int64 * 3)(*[int(v) for v in kdim_xyz]),
                                                   (C.c_int64 * 3)(*[int(v) for v in out_kdim_xyz]), out.ctypes.data_as(dp)))
    return out.reshape(3, 4)


def _views_table(srcs, dims_xyz, matrices, matrix_dptrs=None):
    """``mvsim_fuse_view`` records: ``srcs`` pointers, ``dims_xyz`` extents, ``matrices`` 3 x 4 each (or None where ``matrix_dptrs``
    names 12 doubles in device memory)."""
    n = len(srcs)
    if len(dims_xyz) != n or (matrices is not None and len(matrices) != n) or (matrix_dptrs is not None and len(matrix_dptrs) != n):
        raise ValueError("fusion: one size and one matrix per view")
    tab = (FuseView * max(1, n))()
    for v in range(n):
        tab[v].src = srcs[v]
        for d in range(3):
            tab[v].dim[d] = int(dims_xyz[v][d])
        dptr = matrix_dptrs[v] if matrix_dptrs is not None else 0
        tab[v].m_dev = dptr or None
        if not dptr:
            if matrices is None or matrices[v] is None:
                raise ValueError("fusion: a view has neither a matrix nor a device matrix")
            for k, val in enumerate(_m12(matrices[v])):
                tab[v].m[k] = float(val)
    return tab


def _ptr_table(ptrs, n):
    return (C.c_void_p * max(1, n))(*[p or None for p in ptrs])


def _i3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


class ContextFusion:
    """Fusion entry points of ``Context`` (``self._h``: the context, ``self._L``: the library).  Every ``*_dev`` call only enqueues."""

    def fuse_views_dev(self, src_dptrs, dims_xyz, matrices, out_min, out_dim, fused_dptr: int, sum_weights_dptr: int = 0, status_dptr: int = 0,
                       params: FuseParams | None = None, matrix_dptrs=None) -> None:
        """The blended average of device views into ``fused_dptr`` (prod(out_dim) floats); ``matrix_dptrs[v]`` non-zero: view v's
        matrix is read from device memory (12 doubles, e.g. the head of a ``mvsim_registration``)."""
        p = params if params is not None else fuse_params()
        tab = _views_table(src_dptrs, dims_xyz, matrices, matrix_dptrs)
        _lib.check(self._L.mvsim_fuse_views_dev(self._h, tab, len(src_dptrs), _i3(out_min), _i3(out_dim), C.byref(p), C.c_void_p(fused_dptr),
                                                C.c_void_p(sum_weights_dptr) if sum_weights_dptr else None,
                                                C.c_void_p(status_dptr) if status_dptr else None))

    def align_views_dev(self, src_dptrs, dims_xyz, matrices, out_min, out_dim, aligned_dptrs, weight_dptrs=None, status_dptr: int = 0,
                        params: FuseParams | None = None, matrix_dptrs=None) -> None:
        """One resampled volume and one weight volume per device view; entries of either list may be 0."""
        p = params if params is not None else fuse_params()
        n = len(src_dptrs)
        if len(aligned_dptrs) != n or (weight_dptrs is not None and len(weight_dptrs) != n):
            raise ValueError("fusion: one output entry per view")
        tab = _views_table(src_dptrs, dims_xyz, matrices, matrix_dptrs)
        _lib.check(self._L.mvsim_align_views_dev(self._h, tab, n, _i3(out_min), _i3(out_dim), C.byref(p), _ptr_table(aligned_dptrs, n),
                                                 _ptr_table(weight_dptrs, n) if weight_dptrs is not None else None,
                                                 C.c_void_p(status_dptr) if status_dptr else None))

    @staticmethod
    def _host_views(views, p):
        dt = np.uint16 if p.src_type == MVSIM_SRC_U16 else np.float32
        vs = [np.ascontiguousarray(v, dtype=dt) for v in views]
        for v in vs:
            if v.ndim != 3 or v.size == 0:
                raise ValueError("views: expected 3 non-empty dimensions")
        return vs, [v.ctypes.data for v in vs], [(v.shape[2], v.shape[1], v.shape[0]) for v in vs]

    def fuse_views(self, views, matrices, out_min, out_dim, params: FuseParams | None = None, sum_weights: bool = False, status: bool = False):
        """Host arrays (Nz,Ny,Nx), one matrix each.  Returns the fused volume (out_dim z, y, x), followed by the sum of weights
        and / or the status words where asked for."""
        p = params if params is not None else fuse_params()
        vs, ptrs, dims = self._host_views(views, p)
        shape = (int(out_dim[2]), int(out_dim[1]), int(out_dim[0]))
        out = np.empty(shape, np.float32)
        sw = np.empty(shape, np.float32) if sum_weights else None
        st = np.zeros(max(1, len(vs)), np.int32) if status else None
        tab = _views_table(ptrs, dims, matrices)
        _lib.check(self._L.mvsim_fuse_views(self._h, tab, len(vs), _i3(out_min), _i3(out_dim), C.byref(p), C.c_void_p(out.ctypes.data),
                                            C.c_void_p(sw.ctypes.data) if sum_weights else None, C.c_void_p(st.ctypes.data) if status else None))
        res = (out,) + ((sw,) if sum_weights else ()) + ((st[: len(vs)],) if status else ())
        return res[0] if len(res) == 1 else res

    def align_views(self, views, matrices, out_min, out_dim, params: FuseParams | None = None, weights: bool = True, status: bool = False):
        """Host arrays (Nz,Ny,Nx), one matrix each.  Returns (aligned list, weights list or None), and the status words where asked for."""
        p = params if params is not None else fuse_params()
        vs, ptrs, dims = self._host_views(views, p)
        n = len(vs)
        shape = (int(out_dim[2]), int(out_dim[1]), int(out_dim[0]))
        al = [np.empty(shape, np.float32) for _ in range(n)]
        wt = [np.empty(shape, np.float32) for _ in range(n)] if weights else None
        st = np.zeros(max(1, n), np.int32) if status else None
        tab = _views_table(ptrs, dims, matrices)
        _lib.check(self._L.mvsim_align_views(self._h, tab, n, _i3(out_min), _i3(out_dim), C.byref(p), _ptr_table([a.ctypes.data for a in al], n),
                                             _ptr_table([w.ctypes.data for w in wt], n) if weights else None,
                                             C.c_void_p(st.ctypes.data) if status else None))
        return (al, wt, st[:n]) if status else (al, wt)


def transform_psf(psf, m, out_shape=None, ctx=None) -> np.ndarray:
    """A view's PSF (Kz,Ky,Kx) in the output frame: resampled through the linear part of ``m`` about its centre into a volume of
    ``out_shape`` (default: the PSF's own), blend 0."""
    k = np.ascontiguousarray(psf, dtype=np.float32)
    if k.ndim != 3 or k.size == 0:
        raise ValueError("psf: expected 3 non-empty dimensions")
    shape = tuple(int(s) for s in (out_shape if out_shape is not None else k.shape))
    kd, od = (k.shape[2], k.shape[1], k.shape[0]), (shape[2], shape[1], shape[0])
    if ctx is None:
        from . import default_context
        ctx = default_context()
    al, _ = ctx.align_views([k], [psf_matrix(m, kd, od)], (0, 0, 0), od, fuse_params(blend=0.0), weights=False)
    return al[0]


class ViewFusion:
    """Fuses registered views.

        f = ViewFusion(blend=8.0)
        fused = f.fuse(views, matrices)                    # into view 0's own interval
        aligned, weights = f.align(views, matrices, interval=((x0, y0, z0), (nx, ny, nz)))

    ``matrices[v]`` is the 3 x 4 matrix view v -> output frame (``registration["m"]`` for a view registered against the reference, the
    identity for the reference itself); ``interval`` is (out_min, out_dim), x first."""

    def __init__(self, ctx=None, **params):
        self.params = fuse_params(**params)
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            from . import default_context
            self._ctx = default_context()
        return self._ctx

    @staticmethod
    def _interval(views, interval):
        if interval is not None:
            return tuple(interval[0]), tuple(interval[1])
        s = np.shape(views[0])
        return (0, 0, 0), (s[2], s[1], s[0])

    def fuse(self, views, matrices, interval=None, sum_weights: bool = False, status: bool = False):
        mn, dm = self._interval(views, interval)
        return self._context().fuse_views(views, matrices, mn, dm, self.params, sum_weights, status)

    def align(self, views, matrices, interval=None, weights: bool = True, status: bool = False):
        mn, dm = self._interval(views, interval)
        return self._context().align_views(views, matrices, mn, dm, self.params, weights, status)


def fuse_rendered(ctx, points, matrices, interval, sigma, reference: int = 0, detector=None, matcher=None, u16: bool = False,
                  params: FuseParams | None = None):
    """Render the views of a bead cloud on the device, detect in each, register every view against view ``reference`` and fuse them
    into the reference's interval -- all on the device: the fusion reads the registrations' matrices from device memory, and only
    the results are downloaded.  Returns (fused, registrations, fused_true): ``registrations[v]`` is the record of v -> reference
    (None at the reference), ``fused_true`` the same fusion with the true transforms."""
    from .detection import PEAK_DTYPE, DifferenceOfGaussian
    from .registration import REGISTRATION_DTYPE, BeadRegistration, MVSIM_REG_MAX_POINTS, true_transform
    det = detector if detector is not None else DifferenceOfGaussian(ctx=ctx)
    reg = matcher if matcher is not None else BeadRegistration(ctx=ctx)
    p = FuseParams.from_buffer_copy(params) if params is not None else fuse_params()
    p.src_type = MVSIM_SRC_U16 if u16 else MVSIM_SRC_F32
    mn, mx = interval
    dim = [int(mx[d]) - int(mn[d]) for d in range(3)]
    nvox = dim[0] * dim[1] * dim[2]
    mats = [np.asarray(m, dtype=np.float64).reshape(3, 4) for m in matrices]
    V = len(mats)
    cap = min(det.capacity, MVSIM_REG_MAX_POINTS)
    item = PEAK_DTYPE.itemsize
    img_bytes = (nvox * (2 if u16 else 4) + 255) // 256 * 256
    list_bytes = (cap * item + 8 + 255) // 256 * 256
    imgs = ctx.dev_alloc(V * img_bytes)
    lists = ctx.dev_alloc(V * list_bytes)
    recs = ctx.dev_alloc(V * 256)
    out = ctx.dev_alloc(nvox * 4)
    try:
        img = [imgs + v * img_bytes for v in range(V)]
        pk = [lists + v * list_bytes for v in range(V)]
        res = [recs + v * 256 for v in range(V)]
        for v in range(V):
            ctx.render_beads_dev(points, interval, sigma, f32_dptrs=None if u16 else [img[v]], u16_dptrs=[img[v]] if u16 else None,
                                 matrices=mats[v][None])
            ctx.detect_beads_dev(img[v], np.uint16 if u16 else np.float32, dim, cap, pk[v], pk[v] + cap * item, params=det.params)
        for v in range(V):
            if v != reference:
                ctx.register_beads_dev(pk[v], item, pk[v] + cap * item, cap, pk[reference], item, pk[reference] + cap * item, cap, res[v],
                                       params=reg.params)
        eye = np.hstack([np.eye(3), np.zeros((3, 1))])
        ctx.fuse_views_dev(img, [dim] * V, [eye if v == reference else None for v in range(V)], (0, 0, 0), dim, out, params=p,
                           matrix_dptrs=[0 if v == reference else res[v] for v in range(V)])
        shape = (dim[2], dim[1], dim[0])
        fused = ctx.download(out, shape, np.float32)
        regs = [None if v == reference else ctx.download(res[v], (1,), REGISTRATION_DTYPE)[0] for v in range(V)]
        true = [eye if v == reference else true_transform(mats[v], mats[reference], mn) for v in range(V)]
        ctx.fuse_views_dev(img, [dim] * V, true, (0, 0, 0), dim, out, params=p)
        fused_true = ctx.download(out, shape, np.float32)
    finally:
        for ptr in (imgs, lists, recs, out):
            ctx.dev_free(ptr)
    return fused, regs, fused_true
