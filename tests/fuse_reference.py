"""The view fusion of include/mvsim.h restated in numpy float64, operation for operation: numpy's float64 + - * / and floor are the
IEEE operations, nothing is fused, and every expression below is parenthesised as the header writes it.  It reads nothing from the
library.  Arrays are (Nz, Ny, Nx); intervals and extents are x first, as in the C ABI."""
import numpy as np

F64 = np.float64
SINGULAR = 1
MAX_VIEWS = 32
DEFAULTS = {"blend": (8.0, 8.0, 8.0), "background": 0.0}


def same_bits(a, b):
    """Equal bit for bit, NaNs compared as NaNs (any payload), +0 and -0 told apart."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def invert(m):
    """Step 1: the 12 doubles [i | it] row-major, or None (non-finite entry, det zero or non-finite)."""
    m = np.asarray(m, F64).reshape(12)
    if not np.all(np.isfinite(m)):
        return None
    m00, m01, m02, tx, m10, m11, m12, ty, m20, m21, m22, tz = [F64(v) for v in m]
    with np.errstate(all="ignore"):
        det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22
        if det == 0.0 or not np.isfinite(det):
            return None
        idet = F64(1.0) / det
        i = [[(m11 * m22 - m12 * m21) * idet, (m02 * m21 - m01 * m22) * idet, (m01 * m12 - m02 * m11) * idet],
             [(m12 * m20 - m10 * m22) * idet, (m00 * m22 - m02 * m20) * idet, (m02 * m10 - m00 * m12) * idet],
             [(m10 * m21 - m11 * m20) * idet, (m01 * m20 - m00 * m21) * idet, (m00 * m11 - m01 * m10) * idet]]
        out = []
        for r in range(3):
            out += [i[r][0], i[r][1], i[r][2], -((i[r][0] * tx + i[r][1] * ty) + i[r][2] * tz)]
    return np.array(out, F64)


def _ramp(p, top, blend):
    g = top - p
    e = np.where(p < g, p, g)
    if not blend > 0.0:                                    # e >= 0 inside: e < 0 never holds
        return np.ones_like(p)
    q = e / F64(blend)
    return np.where(e < blend, (q * q) * (3.0 - 2.0 * q), 1.0)


def resample(src, m, out_min, out_dim, blend):
    """Steps 1-5 and 7 for one view: (s_f float32, w float64, inside bool) over the output interval, and the status word."""
    nx, ny, nz = (int(v) for v in out_dim)
    shape = (nz, ny, nx)
    inv = invert(m)
    if inv is None:
        return np.zeros(shape, np.float32), np.zeros(shape, F64), np.zeros(shape, bool), SINGULAR
    src = np.asarray(src)
    Nz, Ny, Nx = src.shape
    vol = src.astype(np.float32).astype(F64)
    oz = (np.arange(nz, dtype=np.int64) + int(out_min[2])).astype(F64)[:, None, None]
    oy = (np.arange(ny, dtype=np.int64) + int(out_min[1])).astype(F64)[None, :, None]
    ox = (np.arange(nx, dtype=np.int64) + int(out_min[0])).astype(F64)[None, None, :]
    with np.errstate(all="ignore"):
        p = [np.broadcast_to(((inv[4 * r + 3] + inv[4 * r + 2] * oz) + inv[4 * r + 1] * oy) + inv[4 * r] * ox, shape) for r in range(3)]
        top = [F64(Nx - 1), F64(Ny - 1), F64(Nz - 1)]
        inside = np.ones(shape, bool)
        for d in range(3):
            inside &= (0.0 <= p[d]) & (p[d] <= top[d])
        q = [np.where(inside, p[d], 0.0) for d in range(3)]           # outside: any valid position, masked out below
        f = [np.floor(v) for v in q]
        u = [q[d] - f[d] for d in range(3)]
        lo = [v.astype(np.int64) for v in f]
        hi = [np.minimum(lo[0] + 1, Nx - 1), np.minimum(lo[1] + 1, Ny - 1), np.minimum(lo[2] + 1, Nz - 1)]

        def at(a, b, c):
            return vol[(hi[2] if c else lo[2]), (hi[1] if b else lo[1]), (hi[0] if a else lo[0])]

        cx = {(b, c): at(0, b, c) + u[0] * (at(1, b, c) - at(0, b, c)) for b in (0, 1) for c in (0, 1)}
        cy = {c: cx[(0, c)] + u[1] * (cx[(1, c)] - cx[(0, c)]) for c in (0, 1)}
        s = cy[0] + u[2] * (cy[1] - cy[0])
        s_f = np.where(inside, s.astype(np.float32), np.float32(0.0)).astype(np.float32)
        r = [_ramp(q[d], top[d], float(blend[d])) for d in range(3)]
        w = np.where(inside, (r[0] * r[1]) * r[2], 0.0)
    return s_f, w, inside, 0


def fuse(views, matrices, out_min, out_dim, blend=DEFAULTS["blend"], background=DEFAULTS["background"]):
    """Step 6: (fused float32, sum of weights float32, status int32 per view)."""
    shape = (int(out_dim[2]), int(out_dim[1]), int(out_dim[0]))
    num, den = np.zeros(shape, F64), np.zeros(shape, F64)
    status = np.zeros(len(views), np.int32)
    with np.errstate(all="ignore"):
        for v, (src, m) in enumerate(zip(views, matrices)):
            s_f, w, inside, status[v] = resample(src, m, out_min, out_dim, blend)
            num = np.where(inside, num + w * s_f.astype(F64), num)
            den = np.where(inside, den + w, den)
        safe = np.where(den > 0.0, den, 1.0)
        out = np.where(den > 0.0, (num / safe).astype(np.float32), np.float32(background)).astype(np.float32)
    return out, den.astype(np.float32), status


def align(views, matrices, out_min, out_dim, blend=DEFAULTS["blend"]):
    """Step 7: ([aligned float32], [weight float32], status)."""
    al, wt = [], []
    status = np.zeros(len(views), np.int32)
    for v, (src, m) in enumerate(zip(views, matrices)):
        s_f, w, _, status[v] = resample(src, m, out_min, out_dim, blend)
        al.append(s_f)
        wt.append(w.astype(np.float32))
    return al, wt, status


def bounds(matrices, dims_xyz, intersection=False):
    """mvsim_fusion_bounds: (out_min, out_dim) or None (empty intersection, non-finite corner)."""
    lo = hi = None
    for m, N in zip(matrices, dims_xyz):
        m = np.asarray(m, F64).reshape(3, 4)
        cs = []
        for c in range(8):
            x, y, z = F64(N[0] - 1 if c & 1 else 0), F64(N[1] - 1 if c & 2 else 0), F64(N[2] - 1 if c & 4 else 0)
            with np.errstate(all="ignore"):
                cs.append([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)])
        cs = np.array(cs, F64)
        if not np.all(np.isfinite(cs)):
            return None
        f, c = np.floor(cs.min(axis=0)), np.ceil(cs.max(axis=0))
        if lo is None:
            lo, hi = f, c
        elif intersection:
            lo, hi = np.maximum(lo, f), np.minimum(hi, c)
        else:
            lo, hi = np.minimum(lo, f), np.maximum(hi, c)
    if np.any(lo > hi):
        return None
    return tuple(int(v) for v in lo), tuple(int(h - l) + 1 for l, h in zip(lo, hi))


def psf_matrix(m, kdim, out_kdim):
    m = np.asarray(m, F64).reshape(3, 4)
    out = m.copy()
    c = [F64(int(k) // 2) for k in kdim]
    for r in range(3):
        out[r, 3] = F64(int(out_kdim[r]) // 2) - ((m[r, 0] * c[0] + m[r, 1] * c[1]) + m[r, 2] * c[2])
    return out


# ---- matrices the tests share -------------------------------------------------------------------------------------------------------------
def identity():
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def translation(t):
    return np.hstack([np.eye(3), np.asarray(t, F64).reshape(3, 1)])


def rotation(axis, degrees, centre):
    """Rotation about an axis through `centre` (x, y, z), 3 x 4."""
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    centre = np.asarray(centre, F64)
    return np.hstack([R, (centre - R @ centre).reshape(3, 1)])
