"""Bead-based registration: the consumer of the detections that ``DifferenceOfGaussian`` leaves.  Nearest neighbours, geometric
descriptors, ratio-test matching A -> B, RANSAC over java.util.Random hypotheses and an affine refit, all on device-resident lists;
include/mvsim.h states the recipe, DESIGN.md section 18 its kernels.  ``ContextRegistration`` is the part of ``Context`` that binds
the C ABI, ``BeadRegistration`` the class a user calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MVSIM_REG_CAPPED, MVSIM_REG_FEW_CANDIDATES, MVSIM_REG_FEW_INLIERS, MVSIM_REG_MAX_POINTS, MVSIM_REG_NO_MODEL,  # noqa: F401
                   Match, MatchParams, Registration)

#: one candidate correspondence: point ``a`` of list A, point ``b`` of list B, the best and the second-best descriptor distance
MATCH_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("v_best", np.float64), ("v_second", np.float64)])
#: the result record: ``m`` is the 3 x 4 row-major matrix A -> B
REGISTRATION_DTYPE = np.dtype([("m", np.float64, (12,)), ("mean_error", np.float64), ("max_error", np.float64), ("n_a", np.int64),
                               ("n_b", np.int64), ("n_candidates", np.int64), ("n_inliers", np.int64), ("best_hypothesis", np.int64),
                               ("refits", np.int32), ("flags", np.int32)])
assert MATCH_DTYPE.itemsize == C.sizeof(Match) == 24 and REGISTRATION_DTYPE.itemsize == C.sizeof(Registration) == 160

_PARAM_NAMES = ("ratio", "max_epsilon", "min_inlier_ratio", "seed", "redundancy", "hypotheses", "max_refits", "min_inliers")


def match_params(**kw) -> MatchParams:
    """``mvsim_match_params`` with the library's defaults."""
    p = MatchParams()
    _lib.load().mvsim_match_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in _PARAM_NAMES:
            raise TypeError(f"unknown registration parameter {k!r}")
        setattr(p, k, v)
    return p


def descriptor_subsets(redundancy: int = 1) -> np.ndarray:
    """The rank triples of the descriptors, (S, 3); host only."""
    t = (C.c_int32 * 30)()
    n = C.c_int(0)
    _lib.check(_lib.load().mvsim_descriptor_subsets(int(redundancy), t, C.byref(n)))
    return np.array(t[: 3 * n.value], dtype=np.int32).reshape(n.value, 3)


def match_geometry(capacity_a: int, capacity_b: int | None = None, redundancy: int = 1) -> dict:
    """The launch geometry of the two all-pairs kernels for lists of these capacities; host only."""
    g = (C.c_int64 * 8)()
    _lib.check(_lib.load().mvsim_match_geometry(int(capacity_a), int(capacity_a if capacity_b is None else capacity_b), int(redundancy), g))
    names = ("queries", "knn_tile", "knn_splits", "knn_tiles_per_split", "match_tile", "match_splits", "match_tiles_per_split", "ransac_tile")
    return {k: int(v) for k, v in zip(names, g)}


def fit_affine(p, q, mask=None):
    """The affine fit of the recipe over pairs p[i] -> q[i] (host only): the 3 x 4 matrix, or None when there is no model."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    if len(p) != len(q):
        raise ValueError("fit_affine: as many p as q")
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if mk is not None and len(mk) != len(p):
        raise ValueError("fit_affine: one mask byte per pair")
    m = (C.c_double * 12)()
    has = C.c_int(0)
    _lib.check(_lib.load().mvsim_fit_affine(C.c_void_p(p.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(mk.ctypes.data) if mk is not None else None,
                                            len(p), m, C.byref(has)))
    return np.array(m, dtype=np.float64).reshape(3, 4) if has.value else None


def _positions(pos):
    """(array kept alive, pointer, stride, n) of a host list: an (n, 3) float64 array, or the structured detections of the detector."""
    a = np.asarray(pos)
    if a.dtype.names and "pos" in a.dtype.names:
        a = np.ascontiguousarray(a)
        return a, a.ctypes.data + a.dtype.fields["pos"][1], a.dtype.itemsize, len(a)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    return a, a.ctypes.data, 24, len(a)


class ContextRegistration:
    """Registration entry points of ``Context`` (``self._h``: the context, ``self._L``: the library).  Every ``*_dev`` call only
    enqueues; counts live in device memory (one int64 each)."""

    def knn_dev(self, pos_dptr: int, stride: int, n_dptr: int, capacity: int, redundancy: int, idx_dptr: int, d2_dptr: int) -> None:
        """The K = 3 + redundancy nearest other points of every point: K int32 indices and K float64 d2 per point."""
        _lib.check(self._L.mvsim_knn_dev(self._h, C.c_void_p(pos_dptr), int(stride), C.c_void_p(n_dptr), int(capacity), int(redundancy),
                                         C.c_void_p(idx_dptr), C.c_void_p(d2_dptr)))

    def bead_descriptors_dev(self, pos_dptr: int, stride: int, n_dptr: int, capacity: int, redundancy: int, idx_dptr: int, desc_dptr: int,
                             n_described_dptr: int) -> None:
        """6 S float64 per point from the neighbour indices of ``knn_dev``; the number of described points in device memory."""
        _lib.check(self._L.mvsim_bead_descriptors_dev(self._h, C.c_void_p(pos_dptr), int(stride), C.c_void_p(n_dptr), int(capacity),
                                                      int(redundancy), C.c_void_p(idx_dptr), C.c_void_p(desc_dptr), C.c_void_p(n_described_dptr)))

    def match_descriptors_dev(self, desc_a_dptr: int, n_a_dptr: int, capacity_a: int, desc_b_dptr: int, n_b_dptr: int, capacity_b: int,
                              redundancy: int, ratio: float, capacity: int, candidates_dptr: int, n_candidates_dptr: int) -> None:
        """The ratio-test candidates A -> B in ascending a: min(n_candidates, capacity) ``mvsim_match`` records (24 bytes each)."""
        _lib.check(self._L.mvsim_match_descriptors_dev(self._h, C.c_void_p(desc_a_dptr), C.c_void_p(n_a_dptr), int(capacity_a),
                                                       C.c_void_p(desc_b_dptr), C.c_void_p(n_b_dptr), int(capacity_b), int(redundancy),
                                                       float(ratio), int(capacity), C.c_void_p(candidates_dptr), C.c_void_p(n_candidates_dptr)))

    def ransac_affine_dev(self, pos_a_dptr: int, stride_a: int, n_a_dptr: int, capacity_a: int, pos_b_dptr: int, stride_b: int, n_b_dptr: int,
                          capacity_b: int, candidates_dptr: int, n_candidates_dptr: int, capacity: int, result_dptr: int, mask_dptr: int = 0,
                          params: MatchParams | None = None) -> None:
        """RANSAC and refit over any candidate list into one ``mvsim_registration`` (160 bytes) and, on request, the inlier mask."""
        p = params if params is not None else match_params()
        _lib.check(self._L.mvsim_ransac_affine_dev(self._h, C.c_void_p(pos_a_dptr), int(stride_a), C.c_void_p(n_a_dptr), int(capacity_a),
                                                   C.c_void_p(pos_b_dptr), int(stride_b), C.c_void_p(n_b_dptr), int(capacity_b),
                                                   C.c_void_p(candidates_dptr), C.c_void_p(n_candidates_dptr), int(capacity), C.byref(p),
                                                   C.c_void_p(result_dptr), C.c_void_p(mask_dptr) if mask_dptr else None))

    def register_beads_dev(self, pos_a_dptr: int, stride_a: int, n_a_dptr: int, capacity_a: int, pos_b_dptr: int, stride_b: int, n_b_dptr: int,
                           capacity_b: int, result_dptr: int = 0, candidates_dptr: int = 0, mask_dptr: int = 0, params: MatchParams | None = None):
        """The whole recipe on two device lists.  With ``result_dptr`` the call only enqueues and returns None; without it the outputs
        are allocated for the call, fetched and returned as (registration, candidates, mask)."""
        p = params if params is not None else match_params()
        own = not result_dptr
        cap = int(capacity_a)
        if own:
            result_dptr = self.dev_alloc(256 + 24 * cap + cap)
            candidates_dptr, mask_dptr = result_dptr + 256, result_dptr + 256 + 24 * cap
        try:
            _lib.check(self._L.mvsim_register_beads_dev(self._h, C.c_void_p(pos_a_dptr), int(stride_a), C.c_void_p(n_a_dptr), cap,
                                                        C.c_void_p(pos_b_dptr), int(stride_b), C.c_void_p(n_b_dptr), int(capacity_b), C.byref(p),
                                                        C.c_void_p(result_dptr), C.c_void_p(candidates_dptr) if candidates_dptr else None,
                                                        C.c_void_p(mask_dptr) if mask_dptr else None))
            if not own:
                return None
            res = self.download(result_dptr, (1,), REGISTRATION_DTYPE)[0]
            listed = min(max(int(res["n_candidates"]), 0), cap)
            cand = self.download(candidates_dptr, (listed,), MATCH_DTYPE) if listed else np.zeros(0, MATCH_DTYPE)
            mask = self.download(mask_dptr, (listed,), np.uint8) if listed else np.zeros(0, np.uint8)
            return res, cand, mask
        finally:
            if own:
                self.dev_free(result_dptr)

    def register_beads(self, pos_a, pos_b, params: MatchParams | None = None):
        """Two host lists -- (n, 3) float64 arrays or the detector's structured detections.  Returns (registration, candidates,
        mask): the record, the candidate list and one byte per candidate (1 = inlier)."""
        p = params if params is not None else match_params()
        a, pa, sa, na = _positions(pos_a)
        b, pb, sb, nb = _positions(pos_b)
        res = np.zeros(1, REGISTRATION_DTYPE)
        cand = np.zeros(max(na, 1), MATCH_DTYPE)
        mask = np.zeros(max(na, 1), np.uint8)
        spare = np.zeros(5, np.float64)                    # an empty list still needs a pointer
        _lib.check(self._L.mvsim_register_beads(self._h, C.c_void_p(pa if na else spare.ctypes.data), sa, na,
                                                C.c_void_p(pb if nb else spare.ctypes.data), sb, nb, C.byref(p), C.c_void_p(res.ctypes.data),
                                                C.c_void_p(cand.ctypes.data), C.c_void_p(mask.ctypes.data)))
        listed = min(max(int(res[0]["n_candidates"]), 0), max(na, 1))
        return res[0], cand[:listed].copy(), mask[:listed].copy()


class BeadRegistration:
    """Registers bead views from their detections alone.

        reg = BeadRegistration(redundancy=1, ratio=3.0, max_epsilon=5.0)
        result, candidates, mask = reg.register(peaks_a["pos"], peaks_b["pos"])
        matrix = result["m"].reshape(3, 4)                 # A -> B

    ``result["flags"]`` holds MVSIM_REG_* bits; the matrix is reported whenever a model was found."""

    def __init__(self, ctx=None, capacity: int = MVSIM_REG_MAX_POINTS, **params):
        self.params = match_params(**params)
        self.capacity = int(capacity)
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            from . import default_context
            self._ctx = default_context()
        return self._ctx

    def register(self, pos_a, pos_b):
        return self._context().register_beads(pos_a, pos_b, self.params)

    def register_dev(self, pos_a_dptr: int, stride_a: int, n_a_dptr: int, capacity_a: int, pos_b_dptr: int, stride_b: int, n_b_dptr: int,
                     capacity_b: int):
        """The same on two device lists whose counts live in device memory; returns (registration, candidates, mask), synchronises."""
        return self._context().register_beads_dev(pos_a_dptr, stride_a, n_a_dptr, capacity_a, pos_b_dptr, stride_b, n_b_dptr, capacity_b,
                                                  params=self.params)

    def register_views(self, list_of_positions, fixed: int = 0):
        """Every view against view ``fixed``: a list of (registration, candidates, mask), view -> fixed; None at ``fixed`` itself."""
        views = list(list_of_positions)
        return [None if v == fixed else self.register(views[v], views[fixed]) for v in range(len(views))]


def register_rendered(ctx, points, matrix_a, matrix_b, interval, sigma, detector=None, matcher: BeadRegistration | None = None, u16: bool = False):
    """Render two views of a bead cloud on the device, detect in both and register A -> B there; only the result is downloaded.
    Returns (registration, candidates, mask, truth): ``truth`` is the true A -> B transform in image coordinates, 3 x 4,
    q_B = M_B M_A^-1 (q_A + min) - min."""
    from .detection import PEAK_DTYPE, DifferenceOfGaussian
    det = detector if detector is not None else DifferenceOfGaussian(ctx=ctx)
    reg = matcher if matcher is not None else BeadRegistration(ctx=ctx)
    mn, mx = interval
    dim = [int(mx[d]) - int(mn[d]) for d in range(3)]
    nvox = dim[0] * dim[1] * dim[2]
    cap = min(det.capacity, MVSIM_REG_MAX_POINTS)
    item = PEAK_DTYPE.itemsize
    mats = [np.asarray(m, dtype=np.float64).reshape(3, 4) for m in (matrix_a, matrix_b)]
    img = ctx.dev_alloc(nvox * (2 if u16 else 4))
    lists = ctx.dev_alloc(2 * (cap * item + 8))
    try:
        peaks = [lists, lists + cap * item + 8]
        for m, pk in zip(mats, peaks):
            ctx.render_beads_dev(points, interval, sigma, f32_dptrs=None if u16 else [img], u16_dptrs=[img] if u16 else None, matrices=m[None])
            ctx.detect_beads_dev(img, np.uint16 if u16 else np.float32, dim, cap, pk, pk + cap * item, params=det.params)
        res, cand, mask = ctx.register_beads_dev(peaks[0], item, peaks[0] + cap * item, cap, peaks[1], item, peaks[1] + cap * item, cap,
                                                 params=reg.params)
    finally:
        ctx.dev_free(img)
        ctx.dev_free(lists)
    return res, cand, mask, true_transform(mats[0], mats[1], mn)


def true_transform(matrix_a, matrix_b, interval_min) -> np.ndarray:
    """M_B M_A^-1 between two views' image coordinates (each view's image holds M p - min): 3 x 4."""
    def h(m):
        return np.vstack([np.asarray(m, dtype=np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    shift = np.eye(4)
    shift[:3, 3] = [float(v) for v in interval_min]
    back = np.eye(4)
    back[:3, 3] = -shift[:3, 3]
    return (back @ h(matrix_b) @ np.linalg.inv(h(matrix_a)) @ shift)[:3]
