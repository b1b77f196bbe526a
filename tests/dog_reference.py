"""The bead detector's recipe (include/mvsim.h) restated literally in numpy: taps with math.exp, float32 passes
with a separate multiply and add per tap in ascending order, the peak rule, the fp64 fit with the header's operation order.  The
GPU tests compare against this bit for bit; the host tests run the recipe on its own through it."""
import math

import numpy as np

F32 = np.float32
SINGULAR, FROZEN, CAPPED, OUTSIDE = 1, 2, 4, 8
MAX_TAPS = 63
PEAK_DTYPE = np.dtype([("pos", np.float64, (3,)), ("value", np.float32), ("flags", np.int32), ("voxel", np.int64)])
DEFAULT_SIGMA1 = (1.8,) * 3
DEFAULT_SIGMA2 = (1.8 * math.pow(2.0, 0.25),) * 3


def same_bits(a, b) -> bool:
    """Equal bit for bit, except that every NaN equals every NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.names:
        return all(same_bits(a[n], b[n]) for n in a.dtype.names)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a) & np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all(nan | (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u))))


def diameter(sigma: float) -> int:
    return max(3, 2 * int(3 * sigma + 0.5) + 1)


def taps(sigma: float) -> np.ndarray:
    d = diameter(sigma)
    if d > MAX_TAPS:
        raise ValueError("diameter above 63")
    r = d // 2
    e = [math.exp(-((j - r) * (j - r)) / (2 * sigma * sigma)) for j in range(d)]
    s = 0.0
    for v in e:
        s += v
    return np.array([F32(v / s) for v in e], dtype=F32)


def fold(i, n: int):
    """mirror-single: period 2 n - 2, folded as often as needed."""
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def blur_axis(v: np.ndarray, t: np.ndarray, axis: int) -> np.ndarray:
    """One pass: acc = t[0] v_0, then acc = acc + t[j] v_j, float32 throughout."""
    assert v.dtype == F32 and t.dtype == F32
    n, r = v.shape[axis], len(t) // 2
    i = np.arange(n)
    with np.errstate(all="ignore"):
        acc = t[0] * np.take(v, fold(i - r, n), axis=axis)
        for j in range(1, len(t)):
            acc = acc + t[j] * np.take(v, fold(i + j - r, n), axis=axis)
    assert acc.dtype == F32
    return acc


def blur(v: np.ndarray, taps_xyz) -> np.ndarray:
    """x then y then z over a (Nz, Ny, Nx) volume; taps_xyz: the three tap arrays, x first."""
    for axis, t in zip((2, 1, 0), taps_xyz):
        v = blur_axis(v, t, axis)
    return v


def dog(img: np.ndarray, taps1, taps2) -> np.ndarray:
    """D = G1 - G2; img float32 or uint16 (one conversion on load)."""
    v = np.asarray(img).astype(F32)
    with np.errstate(all="ignore"):
        return blur(v, taps1) - blur(v, taps2)


def dog_sigmas(img, sigma1=DEFAULT_SIGMA1, sigma2=DEFAULT_SIGMA2, taps_of=taps) -> np.ndarray:
    return dog(img, [taps_of(s) for s in sigma1], [taps_of(s) for s in sigma2])


def find_peaks(D: np.ndarray, threshold) -> np.ndarray:
    """Linear indices of the peaks in ascending order."""
    nz, ny, nx = D.shape
    if min(nz, ny, nx) < 3:
        return np.zeros(0, np.int64)
    c = D[1:-1, 1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        ok = c > F32(threshold)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    off = dx + nx * (dy + ny * dz)
                    if off == 0:
                        continue
                    nb = D[1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]
                    ok &= (c > nb) if off < 0 else (c >= nb)
    z, y, x = np.nonzero(ok)
    return np.sort((x + 1) + nx * ((y + 1) + ny * (z + 1))).astype(np.int64)


def _fit(D, x, y, z):
    """The fit at base (x, y, z): (g, o, c, singular), every operation in the header's order, in Python floats (IEEE doubles)."""
    def at(dx=0, dy=0, dz=0):
        return float(D[z + dz, y + dy, x + dx])

    def off(d, s, e=None, t=0):
        k = [0, 0, 0]
        k[d] += s
        if e is not None:
            k[e] += t
        return at(*k)
    c = at()
    g, h = [0.0] * 3, [[0.0] * 3 for _ in range(3)]
    for d in range(3):
        p, m = off(d, 1), off(d, -1)
        g[d] = (p - m) / 2.0
        h[d][d] = (p - 2.0 * c) + m
    for d in range(3):
        for e in range(d + 1, 3):
            pp, mp, pm, mm = off(d, 1, e, 1), off(d, -1, e, 1), off(d, 1, e, -1), off(d, -1, e, -1)
            h[d][e] = h[e][d] = (((pp - mp) - pm) + mm) / 4.0
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = h
    det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22
    if det == 0.0 or not math.isfinite(det):
        return g, [0.0] * 3, c, True
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
    o = [-((i00 * g[0] + i01 * g[1]) + i02 * g[2]), -((i10 * g[0] + i11 * g[1]) + i12 * g[2]), -((i20 * g[0] + i21 * g[1]) + i22 * g[2])]
    if not all(math.isfinite(v) for v in o):
        return g, [0.0] * 3, c, True
    return g, o, c, False


def localise_one(D: np.ndarray, voxel: int, max_moves: int):
    """One mvsim_peak as a tuple (pos, value, flags, voxel)."""
    nz, ny, nx = D.shape
    N = (nx, ny, nz)
    inside = 0 <= voxel < nx * ny * nz
    b = [0, 0, 0]
    if inside:
        b = [voxel % nx, (voxel // nx) % ny, voxel // (nx * ny)]
        inside = all(1 <= b[d] <= N[d] - 2 for d in range(3))
    if not inside:
        return tuple(float(v) for v in b), F32(0), OUTSIDE, voxel
    moved, moves = [0, 0, 0], 0
    with np.errstate(all="ignore"):
        while True:
            g, o, c, singular = _fit(D, *b)
            flags = SINGULAR if singular else 0
            step = [0, 0, 0]
            for d in range(3):
                if not abs(o[d]) > 0.5:
                    continue
                dr = 1 if o[d] > 0.0 else -1
                if not 1 <= b[d] + dr <= N[d] - 2:
                    continue
                if moved[d] == -dr:
                    flags |= FROZEN
                    continue
                step[d] = dr
            if not any(step):
                break
            if moves >= max_moves:
                flags |= CAPPED
                break
            for d in range(3):
                if step[d]:
                    b[d] += step[d]
                    moved[d] = step[d]
            moves += 1
        value = F32(np.float64(c + 0.5 * ((g[0] * o[0] + g[1] * o[1]) + g[2] * o[2])))
    return (b[0] + o[0], b[1] + o[1], b[2] + o[2]), value, flags, b[0] + nx * (b[1] + ny * b[2])


def localise(D: np.ndarray, voxels, max_moves: int = 4) -> np.ndarray:
    out = np.zeros(len(voxels), PEAK_DTYPE)
    for i, v in enumerate(voxels):
        pos, value, flags, voxel = localise_one(D, int(v), max_moves)
        out[i] = (pos, value, flags, voxel)
    return out


def localise_plain(D: np.ndarray, voxel: int, max_moves: int = 4):
    """The plain rule the recipe does NOT use, as ImgLib2's SubpixelLocalization loops (restated from its published source, not
    checked against a JVM): up to max_moves rounds of fit-then-move, a move whenever |o| > 0.5 and the interior allows it; when the
    rounds run out, the base has moved once more and the offset of the previous base is added to it.  Returns the position."""
    nz, ny, nx = D.shape
    N = (nx, ny, nz)
    b = [voxel % nx, (voxel // nx) % ny, voxel // (nx * ny)]
    o = [0.0] * 3
    for _ in range(max_moves):
        _, o, _, _ = _fit(D, *b)
        stable = True
        for d in range(3):
            if abs(o[d]) > 0.5:
                dr = 1 if o[d] > 0.0 else -1
                if 1 <= b[d] + dr <= N[d] - 2:
                    b[d] += dr
                    stable = False
        if stable:
            break
    return (b[0] + o[0], b[1] + o[1], b[2] + o[2])


def detect(img, sigma1=DEFAULT_SIGMA1, sigma2=DEFAULT_SIGMA2, threshold=0.008, max_moves=4, taps_of=taps):
    """The whole recipe: (peaks, D)."""
    D = dog_sigmas(img, sigma1, sigma2, taps_of)
    return localise(D, find_peaks(D, threshold), max_moves), D


# ---- bead volumes for the tests ------------------------------------------------------------------------------------------------------
BEAD_SIGMA = (1.0, 1.0, 3.0)
BEAD_AMPLITUDE = 1000.0


def draw_positions(shape_zyx, n, rng, min_dist=12.0, margin=8.0, accept=None) -> np.ndarray:
    """n positions (x, y, z), at least min_dist apart (Euclidean) and margin from every face; accept(p): a further condition."""
    nz, ny, nx = shape_zyx
    hi = np.array([nx - 1, ny - 1, nz - 1], dtype=np.float64) - margin
    pts = []
    for _ in range(200000):
        if len(pts) == n:
            break
        p = margin + rng.random(3) * (hi - margin)
        if all(np.linalg.norm(p - q) >= min_dist for q in pts) and (accept is None or accept(p)):
            pts.append(p)
    assert len(pts) == n, "the volume does not hold that many beads at this distance"
    return np.array(pts)


def render_beads(shape_zyx, pts, sigma=BEAD_SIGMA, amplitude=BEAD_AMPLITUDE) -> np.ndarray:
    """Gaussians of the given sigma at pts, summed in fp64 (separable per bead, cut at 6 sigma), returned as float32."""
    nz, ny, nx = shape_zyx
    img = np.zeros(shape_zyx, np.float64)
    for p in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
        sl, f = [], []
        for d, n in enumerate((nx, ny, nz)):
            a, b = max(0, int(math.floor(p[d] - 6 * sigma[d]))), min(n - 1, int(math.ceil(p[d] + 6 * sigma[d])))
            x = np.arange(a, b + 1, dtype=np.float64) - p[d]
            sl.append(slice(a, b + 1))
            f.append(np.exp(-(x * x) / (2 * sigma[d] * sigma[d])))
        img[sl[2], sl[1], sl[0]] += amplitude * f[2][:, None, None] * f[1][None, :, None] * f[0][None, None, :]
    return img.astype(F32)


def add_poisson(img, rng, background=10.0) -> np.ndarray:
    return rng.poisson(np.asarray(img, np.float64) + background).astype(F32)


def nearest(truth, found):
    """For every true position the distance to its nearest detection (inf without detections)."""
    truth, found = np.asarray(truth, np.float64).reshape(-1, 3), np.asarray(found, np.float64).reshape(-1, 3)
    if len(found) == 0:
        return np.full(len(truth), np.inf)
    return np.array([np.min(np.linalg.norm(found - p, axis=1)) for p in truth])
