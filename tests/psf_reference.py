"""The PSF extraction of include/mvsim.h restated in numpy float64, operation for operation: numpy's float64 + - * / and floor are the
IEEE operations, nothing is fused, every expression below is parenthesised as the header writes it, float32 appears exactly where the
recipe rounds, and the chunked sums are explicit loops in the stated order.  It reads nothing from the library.  Arrays are
(Nz, Ny, Nx); extents and positions are x first, as in the C ABI."""
import numpy as np

from .fuse_reference import invert as fuse_invert
from .fuse_reference import same_bits  # noqa: F401

F64 = np.float64
CHUNK = 256
MAX_DIM, MAX_POINTS = 63, 65536
USED, NONFINITE, MASKED, OUTSIDE, CROWDED = 0, 1, 2, 3, 4
SINGULAR, NO_BEADS, FLAT = 1, 2, 4
RESULT_DTYPE = np.dtype([("minimum", "<f8"), ("sum", "<f8"), ("n_listed", "<i8"), ("n_used", "<i8"), ("n_nonfinite", "<i8"),
                         ("n_masked", "<i8"), ("n_outside", "<i8"), ("n_crowded", "<i8"), ("flags", "<i4"), ("pad", "<i4")])
DEFAULTS = {"kdim": (15, 15, 15), "min_separation": (15.0, 15.0, 15.0), "subtract_min": 1, "normalize": 1}


def record(n_listed=0, flags=0):
    r = np.zeros((), RESULT_DTYPE)
    r["n_listed"], r["flags"] = n_listed, flags
    return r


def invert(m):
    """Step 1: the nine i_rc as a 3 x 3 array, from [A | 0]; None: singular.  m None: the identity through the same arithmetic."""
    a = np.zeros((3, 4), F64)
    a[:, :3] = np.eye(3) if m is None else np.asarray(m, F64).reshape(3, 4)[:, :3]
    inv = fuse_invert(a)
    return None if inv is None else inv.reshape(3, 4)[:, :3].copy()


def taps_j(kdim):
    """j_d = (double)(k_d - c_d) for every tap, three (Kz, Ky, Kx) arrays (x, y, z)."""
    kx, ky, kz = (int(k) for k in kdim)
    jz, jy, jx = np.meshgrid((np.arange(kz) - kz // 2).astype(F64), (np.arange(ky) - ky // 2).astype(F64),
                             (np.arange(kx) - kx // 2).astype(F64), indexing="ij")
    return jx, jy, jz


def offsets(m, kdim):
    """Step 2: (Kz, Ky, Kx, 3) with (delta_x, delta_y, delta_z) last, or None."""
    inv = invert(m)
    if inv is None:
        return None
    jx, jy, jz = taps_j(kdim)
    with np.errstate(all="ignore"):
        return np.stack([((inv[r, 2] * jz) + inv[r, 1] * jy) + inv[r, 0] * jx for r in range(3)], axis=-1)


def select(pos, dim, m=None, use=None, kdim=DEFAULTS["kdim"], min_separation=DEFAULTS["min_separation"]):
    """Step 3: (status bytes, record with the counts); singular: (None, record)."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    n = len(pos)
    off = offsets(m, kdim)
    if off is None:
        return None, record(n, SINGULAR)
    sep = [F64(s) for s in min_separation]
    crowding = any(s != 0.0 for s in sep)
    finite = np.isfinite(pos).all(axis=1)
    corners = [off[kz, ky, kx] for kz in (0, -1) for ky in (0, -1) for kx in (0, -1)]
    status = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not finite[i]:
                status[i] = NONFINITE
                continue
            if use is not None and use[i] == 0:
                status[i] = MASKED
                continue
            outside = False
            for c in corners:
                for d in range(3):
                    p = pos[i, d] + c[d]
                    if not (0.0 <= p and p <= F64(int(dim[d]) - 1)):
                        outside = True
            if outside:
                status[i] = OUTSIDE
                continue
            if crowding:
                near = finite.copy()
                near[i] = False
                for d in range(3):
                    near &= np.fabs(pos[:, d] - pos[i, d]) < sep[d]
                if near.any():
                    status[i] = CROWDED
    r = record(n)
    for name, code in (("n_used", USED), ("n_nonfinite", NONFINITE), ("n_masked", MASKED), ("n_outside", OUTSIDE), ("n_crowded", CROWDED)):
        r[name] = int((status == code).sum())
    return status, r


def sample(vol64, pos, off):
    """Step 4 for one bead at every tap: float32 (Kz, Ky, Kx).  vol64: the image widened to float32 and then to float64."""
    Nz, Ny, Nx = vol64.shape
    top = [F64(Nx - 1), F64(Ny - 1), F64(Nz - 1)]
    with np.errstate(all="ignore"):
        q = []
        for d in range(3):
            p = pos[d] + off[..., d]
            p = np.where(p > 0.0, p, 0.0)
            q.append(np.where(p < top[d], p, top[d]))
        f = [np.floor(v) for v in q]
        u = [q[d] - f[d] for d in range(3)]
        lo = [v.astype(np.int64) for v in f]
        hi = [np.minimum(lo[0] + 1, Nx - 1), np.minimum(lo[1] + 1, Ny - 1), np.minimum(lo[2] + 1, Nz - 1)]

        def at(a, b, c):
            return vol64[(hi[2] if c else lo[2]), (hi[1] if b else lo[1]), (hi[0] if a else lo[0])]

        cx = {(b, c): at(0, b, c) + u[0] * (at(1, b, c) - at(0, b, c)) for b in (0, 1) for c in (0, 1)}
        cy = {c: cx[(0, c)] + u[1] * (cx[(1, c)] - cx[(0, c)]) for c in (0, 1)}
        s = cy[0] + u[2] * (cy[1] - cy[0])
        return s.astype(np.float32)


def gather(img, pos, status, m=None, kdim=DEFAULTS["kdim"]):
    """Steps 4 and 5: the per-tap totals, float64 (Kz, Ky, Kx); all +0.0 when the matrix is singular."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    shape = (int(kdim[2]), int(kdim[1]), int(kdim[0]))
    off = offsets(m, kdim)
    total = np.zeros(shape, F64)
    if off is None:
        return total
    vol64 = np.asarray(img).astype(np.float32).astype(F64)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(pos), CHUNK):
            chunk = np.zeros(shape, F64)
            for i in range(c0, min(c0 + CHUNK, len(pos))):
                if status[i] != USED:
                    continue
                chunk = chunk + sample(vol64, pos[i], off).astype(F64)
            total = total + chunk
    return total


def finish(totals, rec, subtract_min=1, normalize=1):
    """Step 6: (psf float32 of the totals' shape, the completed record)."""
    totals = np.asarray(totals, F64)
    r = rec.copy()
    if (int(r["flags"]) & SINGULAR) or int(r["n_used"]) <= 0:
        r["minimum"], r["sum"] = 0.0, 0.0
        if not int(r["flags"]) & SINGULAR:
            r["flags"] = int(r["flags"]) | NO_BEADS
        return np.zeros(totals.shape, np.float32), r
    flat = totals.reshape(-1)
    with np.errstate(all="ignore"):
        mean = flat / F64(int(r["n_used"]))
        b = F64(np.inf)
        for v in mean:
            if v < b:
                b = v
        v = mean - b if subtract_min else mean
        S = F64(0.0)
        for t0 in range(0, len(v), CHUNK):
            s = F64(0.0)
            for x in v[t0:t0 + CHUNK]:
                s = s + x
            S = S + s
        scale = bool(normalize) and bool(S > 0.0) and bool(np.isfinite(S))
        psf = (v / S).astype(np.float32) if scale else v.astype(np.float32)
    r["minimum"], r["sum"] = b, S
    if normalize and not scale:
        r["flags"] = int(r["flags"]) | FLAT
    return psf.reshape(totals.shape), r


def extract(img, pos, m=None, use=None, kdim=DEFAULTS["kdim"], min_separation=DEFAULTS["min_separation"], subtract_min=1, normalize=1):
    """The whole recipe: (psf, record, status bytes or None when singular, totals)."""
    dim = np.asarray(img).shape[::-1]
    status, rec = select(pos, dim, m, use, kdim, min_separation)
    totals = gather(img, pos, status, m, kdim) if status is not None else np.zeros((int(kdim[2]), int(kdim[1]), int(kdim[0])), F64)
    psf, rec = finish(totals, rec, subtract_min, normalize)
    return psf, rec, status, totals


def use_from_matches(candidates_ab, n_candidates, capacity, mask, side, n_points):
    """mvsim_psf_use_from_matches_dev as a numpy scatter."""
    use = np.zeros(n_points, np.uint8)
    n = min(max(int(n_candidates), 0), int(capacity))
    for i in range(n):
        if mask is not None and mask[i] != 1:
            continue
        at = int(candidates_ab[i][side])
        if 0 <= at < n_points:
            use[at] = 1
    return use


# ---- what the tests share ---------------------------------------------------------------------------------------------------------------------
def rms_range(a, b):
    """The RMS error of a against b, normalised by b's range."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (b.max() - b.min()))


def gaussian(sigma, kdim, m=None, subtract_min=1, normalize=1):
    """The analytic bead on the taps, under the recipe's minimum subtraction and normalisation (float64)."""
    off = offsets(m, kdim)
    g = np.exp(-0.5 * ((off[..., 0] / sigma[0]) ** 2 + (off[..., 1] / sigma[1]) ** 2 + (off[..., 2] / sigma[2]) ** 2))
    if subtract_min:
        g = g - g.min()
    return g / g.sum() if normalize else g
